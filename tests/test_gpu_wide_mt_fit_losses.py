"""GCV and CV in the device-resident fit of multitask / derivative-informed GPs on wide inputs (9 <= d <= 64, the same n
in every task): fgp_wide_mt_fit_desc.loss_metric through multitask.WideMtEngine, FastGP.fit under FGP_WIDE_FIT_DEVICE=1.

1. The reference's 6-iteration GCV / CV trajectories (tests/golden/wide_mt_loss/*.npz, the REAL reference) with the
   bounds of tests/test_gpu_wide_mt_fit.py (loss 2e-7, parameter and task-kernel histories 1e-10, post_mean 1e-7); the fit
   goes through fgp_wide_mt_fit_run.
2. Device fit = generic fit in one run, the same bounds; the generic run calls fgp_wide_mt_k1_bwd, not the device loop.
3. Two engine runs of 4 iterations: bit-identical raw history, loss history and gradient; the parameters move.
4. The new stage against the extended-precision restatement (tests/wide_mt_loss_reference.py), see
   test_loss_stage_against_the_extended_precision_restatement.
5. A frozen task factor keeps its bits under GCV.  6. Routing outside the domain.  7. Early stopping and the best iterate.
"""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import wide_fit_cases as C
from tests import wide_fit_reference as R
from tests import wide_mt_loss_reference as LR
from tests.gpu_fixtures import DEV, rel_err
from tests.gpu_fixtures import same_bits as _same
from tests.gpu_fixtures import to_np as _np
from tests.test_gpu_wide_mt import _recorded, product_mt
from tests.test_gpu_wide_mt_fit_exact import BLOCKS, FORWARD, K1, LAMS, PROLOGUE, DeviceMt
from tests.test_wide_mt_cpu import load_wide_mt

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

LOSS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_mt_loss")
CASES = ("mt_lattice_d12_a2_T3_n64", "mt_net_d9_a2_T2_n512_b2", "deriv_lattice_d12_a2_n64")
METRICS = ("GCV", "CV")
HISTS = ("loss_hist", "scale_hist", "lengthscales_hist", "task_kernel_hist")


@pytest.fixture(autouse=True)
def device_switch(monkeypatch):
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    monkeypatch.delenv("FGP_ALT_LOSS_DEVICE", raising=False)


def _load(case, metric):
    with np.load(os.path.join(LOSS_DIR, "%s_%s.npz" % (case, metric.lower())), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    assert str(g["metric"]) == metric
    return g


def _gp(g, **kw):
    """product_mt with the constructor arguments the fixture was generated with (`ctor_<name>`: the net case's noise)."""
    ctor = {k[5:]: float(g[k]) for k in g if k.startswith("ctor_")}
    ctor.update(kw)
    return product_mt(g, **ctor)


def _fit_kw(g, **kw):
    out = dict(loss_metric=str(g["metric"]), store_hists=True, verbose=0)
    if str(g["metric"]) == "CV":
        out["cv_weights"] = float(g["cv_weight"])
    out.update(kw)
    return out


def test_the_six_fixtures_exist():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(LOSS_DIR, "*.npz")))
    assert have == sorted("%s_%s" % (c, m.lower()) for c in CASES for m in METRICS)


# ---------------------------------------------------------------------------------------------- 1. reference
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", CASES)
def test_device_fit_follows_the_reference(case, metric, monkeypatch):
    g = _load(case, metric)
    its = int(g["fit_iterations"])
    assert its == 6 and len(set(int(v) for v in g["ns"])) == 1
    gp = _gp(g)
    calls = _recorded(monkeypatch)
    data = gp.fit(**_fit_kw(g, iterations=its, stop_crit_wait_iterations=its + 5))
    assert "fgp_wide_mt_fit_run" in calls and "fgp_wide_mt_k1_bwd" not in calls
    assert data["iterations"] == its
    errs = {k: rel_err(data[k], g["fit_" + k]) for k in HISTS}
    errs["pmean"] = rel_err(gp.post_mean(torch.from_numpy(g["x_test"]).to(DEV)), g["fit_pmean"])
    print("trajectory", case, metric, errs)
    assert errs["loss_hist"] < 2e-7
    assert errs["lengthscales_hist"] < 1e-10 and errs["scale_hist"] < 1e-10 and errs["task_kernel_hist"] < 1e-10
    assert errs["pmean"] < 1e-7


# ---------------------------------------------------------------------------------------------- 2. device = generic
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", CASES)
def test_device_fit_equals_generic_fit(case, metric, monkeypatch):
    g = _load(case, metric)
    kw = _fit_kw(g, iterations=3, stop_crit_wait_iterations=8)
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", switch)
        calls = _recorded(monkeypatch)
        out[switch] = _gp(g).fit(**kw)
        assert ("fgp_wide_mt_fit_run" in calls) == (switch == "1")
        assert ("fgp_wide_mt_k1_bwd" in calls) == (switch == "0")
    for k in ("scale_hist", "lengthscales_hist", "noise_hist", "task_kernel_hist"):
        assert rel_err(out["1"][k], out["0"][k]) < 1e-10, k
    assert rel_err(out["1"]["loss_hist"], out["0"]["loss_hist"]) < 2e-7


# ---------------------------------------------------------------------------------------------- 3. repeatability
@pytest.mark.parametrize("metric", METRICS)
def test_engine_runs_repeat_bit_for_bit(metric):
    g = _load("mt_net_d9_a2_T2_n512_b2", metric)
    hists = []
    for _ in range(2):
        eng = _gp(g)._fused_engine(3, 0.1, loss_metric=metric, cv_weight=float(g["cv_weight"]))
        assert type(eng).__name__ == "WideMtEngine" and eng.loss_metric == metric
        eng.run(0, 4, final_no_update=True)
        hists.append((eng.raw_hist[:4].clone(), eng.loss_hist[:4].clone(), eng.grad.clone()))
    assert all(_same(a, b) for a, b in zip(*hists))
    assert not torch.equal(hists[0][0][0], hists[0][0][3])
    rows = hists[0][1].reshape(4, 3)                                    # (loss, N, D) or (loss, NaN, NaN)
    assert bool(torch.isfinite(rows[:, 0]).all()) and bool(torch.isfinite(hists[0][2]).all())
    if metric == "CV":
        assert bool(torch.isnan(rows[:, 1:]).all())
    else:
        assert bool(torch.isfinite(rows).all()) and rel_err(rows[:, 1] / rows[:, 2], rows[:, 0]) < 1e-15


# ---------------------------------------------------------------------------------------------- 4. the stage, pinned
def _stage_case(tag, fam):
    if tag == "T2n4":        # one partly filled wave; derivative-style pairs (P = 3), one lengthscale, a rank-1 task factor
        return C._mt("loss-" + tag, fam, [4, 4], d=9, dl=1, B=1, rank=1, vexp=0, P=3, conj=(0, 1, 0))
    return C._mt("loss-" + tag, fam, [64, 64, 64], d=12, B=2, rank=2, conj=(0, 1, 0, 0, 1, 0))


def _stage_inputs(c):
    """wide_fit_cases.mt_inputs' recipe for a case of this file: dominant first elements (positive, well separated
    eigenvalues), couplings smaller by 4 T (strictly diagonally dominant class blocks), real data for nets."""
    g = np.random.default_rng([41, c.fam, len(c.ns), c.ns[0], c.d, c.B, c.P])
    T = len(c.ns)
    pairs = []
    for k in range(T):
        for l in range(k, T):
            n = c.ns[k]
            parts = g.uniform(-1.0, 1.0, (c.P, c.d, n)) / math.sqrt(n)
            parts[..., 0] = g.uniform(1.0, 2.0, (c.P, c.d))
            ind = np.ones((c.P, c.d), dtype=np.int32)
            if c.P > 1:
                ind[1:] = g.integers(0, 2, (c.P - 1, c.d))
                ind[1:, 0] = 1
            cc = np.ones(c.P) if c.P == 1 else g.uniform(0.5, 1.0, c.P) / c.P
            if k != l:
                parts /= 4.0 * T * c.P
                cc = cc / (4.0 * T)
            pairs.append((np.ascontiguousarray(parts), ind, cc))
    rn = sum(c.ns)
    y = g.uniform(-1, 1, (c.B, rn)) + (0 if c.fam == C.NET else 1j) * g.uniform(-1, 1, (c.B, rn))
    sp = C.mt_spec(c)
    raw = g.uniform(-0.3, 0.3, sp.n_params)
    raw[1:1 + c.dl] = np.log(g.uniform(0.1, 0.3, c.dl))
    raw[sp.noise_off] = g.uniform(-2.0, -1.0)
    raw[sp.v_off:] = g.uniform(0.0, 0.3, c.T_all) if c.vexp else g.uniform(1.0, 1.4, c.T_all)
    return dict(pairs=pairs, y=y.astype(np.complex128), raw=raw)


class DeviceMtLoss(DeviceMt):
    """DeviceMt with the descriptor's loss_metric / cv_weight set: the larger work buffer (0xFF-filled) and the view of
    the partials (fgp_wide_mt_fit_loss_layout)."""

    def __init__(self, c, inp, loss, cv_weight):
        super().__init__(c, inp)
        mll_bytes = self.work.numel()
        self.desc.loss_metric, self.desc.cv_weight = loss, cv_weight
        nb, o15, o2 = ctypes.c_int64(0), (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 2)()
        N.call("fgp_wide_mt_fit_work", self.desc, ctypes.byref(nb))
        N.call("fgp_wide_mt_fit_work_layout", self.desc, o15)
        N.call("fgp_wide_mt_fit_loss_layout", self.desc, o2)
        assert list(o15) == [self.off[k] for k in self.off] and o2[0] == mll_bytes and nb.value > mll_bytes
        self.work = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
        self.work.fill_(255)
        self.desc.work = self.work.data_ptr()
        self.off["pl"] = o2[0]
        self.shape["pl"] = (torch.float64, o2[1] // 8)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("fam", [C.LAT, C.NET], ids=["lattice", "net"])
@pytest.mark.parametrize("tag", ["T2n4", "T3n64"])
def test_loss_stage_against_the_extended_precision_restatement(tag, fam, metric):
    """Stages 0 - 4 through fgp_wide_mt_fit_stage at T = 2, n = 4 and T = 3, n = 64 (B = 2), both families, both metrics;
    lams, z, zinv, the partials and glp read back from `work`.

    The stage's inputs are what the three block calls leave: they are fgp_mt_factor / _solve / _selinv on the device's own
    lams and y BIT FOR BIT (asserted here; those entry points have their own 80-bit pins, tests/test_gpu_mt_exact.py), so
    the restatement is evaluated on the device's own zinv and z -- the device's lams and y carried through the pinned
    calls -- and no conditioning of the blocks enters the bound of the two new kernels.

    Bound: |device - restatement| <= (u / (1 - C u) + 2^-63) e, u = 2^-53, e the first-order twin B_q of the output (one
    |intermediate| per rounding, carried through the absolute values of what it then meets), C the longest chain, counted
    from the kernels (tests/wide_mt_loss_reference.py):
        partials   2 B T fmas + T additions + block_sum's 10                       C_sums = 2 B T + T + 10
        glp        second level ceil(nbx / 256) + 10, the coefficients 5, per task of the inner sum 3 B (cmulc and an
                   addition per data vector) + 9 (three products, an addition, two fmas)
                                                                                   C_grad = ceil(nbx / 256) + 15 + T (3 B + 9)
    Nothing is fitted to the device's figures.  The seeded defect -- the restatement with the -2 N / (D Tr) dTr term
    (c2) dropped -- must exceed the bound; every bound must be non-vacuous (wide_fit_reference.vacuity)."""
    c = _stage_case(tag, fam)
    inp = _stage_inputs(c)
    cv = metric == "CV"
    w = C.CV_WEIGHT
    dm = DeviceMtLoss(c, inp, N.LOSS_CV if cv else N.LOSS_GCV, w)
    sp = dm.sp
    T, n, B = sp.T, sp.ns[0], c.B
    dm.issue(0, PROLOGUE, 1)
    for stage in (K1, FORWARD, LAMS):
        dm.issue(0, stage)
    want = dm.blocks_direct()
    dm.issue_twice(0, BLOCKS)
    for k in ("fac", "logdet", "z", "zinv"):
        assert _same(dm.v(k), want[k]), (c.name, k, "the block calls are not the stand-alone entry points'")
    assert int(dm.v("info")[0]) == 0
    zinv, z = _np(dm.v("zinv")), _np(dm.v("z"))
    if fam == C.NET:
        assert (zinv.imag == 0).all() and (z.imag == 0).all()
    nt = T if cv else 1
    pl = _np(dm.v("pl")).reshape(nt, 2, sp.nbx)
    glp = _np(dm.v("glp"))
    assert np.isfinite(pl).all() and np.isfinite(glp.view(np.float64)).all()
    # nothing of the MLL's gradient rows or of the contraction's partials is written by this stage
    assert bool((dm.v("part").view(torch.uint8) == 255).all())
    Cn = LR.counts(T, n, B)
    tp = LR.loss_sums_ref(T, n, B, zinv, z, cv)
    gx, gy = LR.loss_grad_ref(T, n, B, zinv, z, pl, cv, w)
    worst = {}
    for what, t, got, Cq in (("partials", tp, pl, Cn["sums"]), ("glp re", gx, glp.real, Cn["grad"]),
                             ("glp im", gy, glp.imag, Cn["grad"])):
        r = R.rel(got, t, Cq)
        vac, fin = R.vacuity(t, Cq)
        worst[what] = r
        print("%-14s %-4s %-9s err / bound = %.3f   ||u e|| / cap = %.3g" % (c.name, metric, what, r, vac))
        assert fin and vac <= 1.0, (c.name, metric, what, "vacuous bound", vac)
        assert r <= 1.0, (c.name, metric, what, r)
    bx, by = LR.loss_grad_ref(T, n, B, zinv, z, pl, cv, w, mutate="noc2")
    bad = max(R.rel(glp.real, bx, Cn["grad"]), R.rel(glp.imag, by, Cn["grad"]))
    print("%-14s %-4s seeded defect err / bound = %.3g" % (c.name, metric, bad))
    assert bad > 1.0
    # the diagonal of a Hermitian block: no imaginary part
    diag = np.concatenate([np.arange(o, o + n) for o in LR.offk(T, n)])
    assert (glp.imag[diag] == 0).all()


# ---------------------------------------------------------------------------------------------- 5. frozen blocks
def test_frozen_task_factor_keeps_its_bits_under_gcv(monkeypatch):
    g = _load("mt_lattice_d12_a2_T3_n64", "GCV")
    gp = _gp(g, requires_grad_factor_task_kernel=False)
    blocks = ("raw_scale", "raw_lengthscales", "raw_factor_task_kernel", "raw_noise_task_kernel")
    before = {nm: getattr(gp, nm).detach().clone() for nm in blocks}
    calls = _recorded(monkeypatch)
    gp.fit(loss_metric="GCV", iterations=3, verbose=0, stop_crit_wait_iterations=8)
    assert "fgp_wide_mt_fit_run" in calls
    for nm in blocks:
        now = getattr(gp, nm).detach()
        if nm == "raw_factor_task_kernel":
            assert torch.equal(now, before[nm]) and not gp.raw_factor_task_kernel.requires_grad
        else:
            assert bool((now != before[nm]).all()), nm


# ---------------------------------------------------------------------------------------------- 6. routing
def _equal(case, metric="GCV"):
    return lambda: _load(case, metric)


_OUTSIDE = {
    "unequal_n": (lambda: load_wide_mt("mt_lattice_d12_a2_T3"), {}, lambda gp: dict(loss_metric="GCV"), None),
    "cv_per_point_weights": (_equal("mt_lattice_d12_a2_T3_n64", "CV"), {},
                             lambda gp: dict(loss_metric="CV", cv_weights=torch.linspace(0.5, 1.5, 192, device=DEV)), None),
    "masks": (_equal("mt_net_d9_a2_T2_n512_b2"), {}, lambda gp: dict(loss_metric="GCV", masks=torch.tensor([1])), None),
    "optimizer": (_equal("mt_lattice_d12_a2_T3_n64"), {},
                  lambda gp: dict(loss_metric="GCV", optimizer=torch.optim.Rprop(gp.parameters(), lr=0.1)), None),
    "adaptive_nugget": (_equal("mt_lattice_d12_a2_T3_n64"), dict(adaptive_nugget=True), lambda gp: dict(loss_metric="GCV"), None),
    "alt_loss_switch_off": (_equal("mt_lattice_d12_a2_T3_n64"), {}, lambda gp: dict(loss_metric="GCV"), "0"),
}


@pytest.mark.parametrize("case", sorted(_OUTSIDE))
def test_fits_outside_the_domain_take_the_generic_loop(case, monkeypatch):
    """(No cap on T below FGP_MT_MAX_TASKS was introduced: the gradient kernel re-reads the inverse from global memory.)"""
    load, ctor_kw, fit_kw, alt = _OUTSIDE[case]
    if alt is not None:
        monkeypatch.setenv("FGP_ALT_LOSS_DEVICE", alt)
    out = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", switch)
        g = load()
        gp = _gp(g, **ctor_kw)
        calls = _recorded(monkeypatch)
        out[switch] = gp.fit(iterations=2, store_hists=True, verbose=0, stop_crit_wait_iterations=7, **fit_kw(gp))
        assert "fgp_wide_mt_fit_run" not in calls, case
    for k in HISTS:
        assert rel_err(out["1"][k], out["0"][k]) < 1e-12, (case, k)


# ---------------------------------------------------------------------------------------------- 7. early stopping
@pytest.mark.parametrize("metric", METRICS)
def test_early_stop_and_best_iterate_restore_as_the_generic_loop(metric, monkeypatch):
    """stop_crit_improvement_threshold = 1e30 (log(1 + 1e30) ~ 69 exceeds this fixture's improvements of 3 - 31 per
    iteration): the rule counts two iterations without a sufficient improvement and ends the fit inside the device
    loop's first chunk, whose later iterations are discarded."""
    g = _load("mt_net_d9_a2_T2_n512_b2", metric)
    kw = _fit_kw(g, iterations=6, stop_crit_wait_iterations=2, stop_crit_improvement_threshold=1e30)
    out, gps = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", switch)
        gps[switch] = _gp(g)
        calls = _recorded(monkeypatch)
        out[switch] = gps[switch].fit(**kw)
        assert ("fgp_wide_mt_fit_run" in calls) == (switch == "1")
    assert out["1"]["iterations"] == out["0"]["iterations"] < 6
    for k in ("scale_hist", "lengthscales_hist", "task_kernel_hist"):
        assert out["1"][k].shape == out["0"][k].shape and rel_err(out["1"][k], out["0"][k]) < 1e-10, k
    for nm in ("raw_scale", "raw_lengthscales", "raw_factor_task_kernel", "raw_noise_task_kernel", "raw_noise"):
        assert rel_err(getattr(gps["1"], nm), getattr(gps["0"], nm)) < 1e-10, nm
    best = int(torch.argmin(out["0"]["loss_hist"]))                      # (the history holds the loss itself)
    assert rel_err(gps["1"].lengthscales, out["0"]["lengthscales_hist"][best]) < 1e-10
