"""Predictions of multitask and derivative-informed GPs at d <= 8 through the fused task-pair kernel (fgp_mt_rows) and the
matrix-free posterior mean (fgp_mt_post_mean), csrc/fgp_mt_pred.hip:

  * the fused route against FGP_MT_FUSED_ROWS=0 (fgp_mt_parts + the torch formulation) on small GPs -- a lattice with
    d = 3, T = 3, n = [256, 64, 256]; a derivative-informed net with d = 2, (f, d1 f, d2 f), n = 128 each; a parameter
    batch shape_batch = [2, 3] at d = 6 -- for post_mean (rows and matrix-free), post_var (both FGP_MT_POST_VAR_QF
    settings), post_cov, post_ci and the n = projection, at the tolerances tests/test_gpu_multitask.py has for the same
    quantities (post_mean 1e-7 relative; post_var 1e-8 kxx, post_cov 1e-7 kxx absolute, kxx = 10 max(1, max post_var);
    the projection 2e-7 max K_tt(x, x) with derivatives, else 1e-8 kxx);
  * the same methods against the REAL-reference multitask fixtures under tests/golden/, under the default route, which
    is asserted to be the fused one;
  * routing, by the recorded N.call names: a d = 3 prediction calls fgp_mt_rows and no fgp_mt_parts; a post_mean past
    the byte threshold calls fgp_mt_post_mean and no fgp_mt_rows; FGP_MT_FUSED_ROWS=0, eval=False with gradients, a
    pair with more than 16 multi-index pairs, integer net inputs and the public kernel() call neither; an empty task is
    skipped;
  * memory: post_mean of 2048 points over n = [4096, 1024, 4096] at d = 3 peaks below one eighth of its rows array
    (8 N sum n T' = 453 MB for the three requested tasks, 151 MB per requested task).
"""
import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from tests.golden_util import load_golden
from tests.gpu_fixtures import DEV, abs_err, rel_err
from tests.test_oracle_multitask import MT_NAMES, REF_INVERSE_ERROR, pred_tol

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

ROWS, MEAN, PARTS = "fgp_mt_rows", "fgp_mt_post_mean", "fgp_mt_parts"


def _recorded(monkeypatch):
    calls = []
    real = N.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, "call", call)
    return calls


def _f(x):
    return torch.exp(-((x - 0.3) ** 2).sum(1)) + torch.sin(3 * x).sum(1)


def _lattice_t3(ns=(256, 64, 256), d=3):
    gp = F.FastGPLattice([F.Lattice(d, seed=11 + l) for l in range(3)], num_tasks=3, alpha=2, device=DEV)
    xs = gp.get_x_next(n=list(ns))
    gp.add_y_next([_f(x) + 0.1 * l * x[:, 0] if x.shape[0] else x[:, 0] for l, x in enumerate(xs)])
    return gp


def _deriv_net(n=128, d=2):
    derivs = [torch.zeros((1, d), dtype=torch.int64)] + [e[None] for e in torch.eye(d, dtype=torch.int64)]
    gp = F.FastGPDigitalNetB2([F.DigitalNetB2(d, seed=7, randomize="DS") for _ in range(d + 1)], derivatives=derivs, alpha=4,
                              num_tasks=d + 1, device=DEV)
    xs = gp.get_x_next(n * torch.ones(d + 1, dtype=torch.int64))
    ys = []
    for l in range(d + 1):
        x = xs[l].clone().requires_grad_()
        y = _f(x)
        ys.append(y.detach() if l == 0 else torch.autograd.grad(y.sum(), x)[0][:, l - 1].detach())
    gp.add_y_next(ys)
    return gp


def _param_batch(d=6, ns=(64, 32, 64)):
    sb = [2, 3]
    gp = F.FastGPLattice([F.Lattice(d, seed=3 + l) for l in range(3)], num_tasks=3, alpha=2, device=DEV, shape_batch=sb,
                         shape_scale=sb + [1], shape_lengthscales=sb[1:] + [d])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gp.raw_scale.copy_((0.5 * torch.randn(gp.raw_scale.shape, generator=g)).to(DEV))
        gp.raw_lengthscales.copy_((-1.0 + 0.5 * torch.randn(gp.raw_lengthscales.shape, generator=g)).to(DEV))
    xs = gp.get_x_next(n=list(ns))
    gp.add_y_next([(_f(x) + 0.1 * l).expand(2, 3, -1).contiguous() for l, x in enumerate(xs)])
    return gp


def _same_sums(gp, x, a, b, tasks=None):
    """a and b are two fp64 summations of the same terms Kt K_i c_i over the sum n training points (the rows and an
    einsum; the matrix-free chunks): each lies within (sum n + 8) 2^-53 sum_i |Kt K_i c_i| of the exact sum, the worst
    case of any order (8: the task weight, the scale and the accumulation over the tasks), so they differ by at most
    twice that."""
    tasks = list(range(gp.num_tasks)) if tasks is None else tasks
    with torch.no_grad():
        mag = (gp._kmat_rows(x, tasks, gp._ns).abs() * gp.coeffs.abs()[..., None, None, :]).sum(-1)
    bound = 2 * (sum(gp._ns) + 8) * 2.0 ** -53 * mag
    return a.shape == b.shape == bound.shape and bool(((a - b).abs() <= bound).all())


MAKERS = {"lattice_d3_T3": _lattice_t3, "deriv_net_d2": _deriv_net, "batch_2x3_d6": _param_batch}


def _predict(gp, x, n_new, qf):
    """Everything the comparison needs of one route."""
    out = dict(pmean=gp.post_mean(x), pcov=gp.post_cov(x[:4], x[4:9]), ci=gp.post_ci(x, confidence=0.95),
               pvar_new=gp.post_var(x, n=torch.tensor(n_new)), pmean_task=gp.post_mean(x, task=1))
    for v in ("0", "1"):
        qf(v)
        out["pvar" + v] = gp.post_var(x)
    qf(None)
    with torch.no_grad():
        out["kdiag"] = max(float(gp._kmat_block(x, x, t, t, zip_pairs=True).abs().max()) for t in range(gp.num_tasks))
    return out


@pytest.mark.parametrize("which", sorted(MAKERS))
def test_fused_rows_against_the_parts_and_torch_formulation(which, monkeypatch):
    def qf(v):
        if v is None:
            monkeypatch.delenv("FGP_MT_POST_VAR_QF", raising=False)
        else:
            monkeypatch.setenv("FGP_MT_POST_VAR_QF", v)

    d = {"lattice_d3_T3": 3, "deriv_net_d2": 2, "batch_2x3_d6": 6}[which]
    x = torch.rand((24, d), generator=torch.Generator().manual_seed(1)).to(DEV)
    res = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("FGP_MT_FUSED_ROWS", fused)
        gp = MAKERS[which]()
        n_new = [2 * int(v) for v in gp.n.tolist()]
        calls = _recorded(monkeypatch)
        res[fused] = _predict(gp, x, n_new, qf)
        assert (ROWS in calls) == (fused == "1")
        if fused == "1":
            # the matrix-free mean, forced at this small size
            monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "1")
            del calls[:]
            mf = gp.post_mean(x)
            assert MEAN in calls and ROWS not in calls and PARTS not in calls
            monkeypatch.delenv("FGP_WIDE_MT_POST_MEAN")
            assert abs_err(gp.post_mean(x[3:4]), res["1"]["pmean"][..., 3:4]) == 0.0   # a point alone: the same bits
    a, b = res["1"], res["0"]
    kxx = 10 * max(1.0, float(b["pvar0"].abs().max()))
    assert a["pmean"].shape == b["pmean"].shape and rel_err(a["pmean"], b["pmean"]) < 1e-7
    assert rel_err(mf, b["pmean"]) < 1e-7
    assert abs_err(a["pmean_task"], a["pmean"][..., 1, :]) == 0.0
    for v in ("0", "1"):
        assert abs_err(a["pvar" + v], b["pvar" + v]) <= 1e-8 * kxx
    assert abs_err(a["pvar1"], b["pvar0"]) <= 1e-8 * kxx
    assert abs_err(a["pcov"], b["pcov"]) <= 1e-7 * kxx
    tol_new = 2e-7 * b["kdiag"] if which == "deriv_net_d2" else 1e-8 * kxx
    assert abs_err(a["pvar_new"], b["pvar_new"]) <= tol_new
    assert abs(a["kdiag"] - b["kdiag"]) <= 1e-12 * b["kdiag"]
    (m1, v1, q1, lo1, hi1), (m0, v0, q0, lo0, hi0) = a["ci"], b["ci"]
    assert q1 == q0 and rel_err(m1, m0) < 1e-7 and abs_err(v1, v0) <= 1e-8 * kxx
    # post_ci returns pmean -+ q perror with perror = q sqrt(pvar) of post_error (the reference scales by q twice,
    # abstract_gp.py:497-498, 523-525, kept for parity): lo = m - q^2 sqrt(v).  With |m1 - m0| <= 1e-7 max |m0| and
    # |v1 - v0| <= 1e-8 kxx from above, and |sqrt(v1) - sqrt(v0)| <= sqrt(|v1 - v0|):
    tol_ci = 1e-7 * float(m0.abs().max()) + q0 * q0 * (1e-8 * kxx) ** 0.5
    assert abs_err(lo1, lo0) <= tol_ci and abs_err(hi1, hi0) <= tol_ci


@pytest.mark.parametrize("name", [nm for nm in MT_NAMES if nm not in REF_INVERSE_ERROR and pred_tol(nm, "predictions", True)])
def test_reference_fixtures_under_the_default_route(name, monkeypatch):
    """tests/test_gpu_multitask.py::test_multitask_predictions' comparisons with the reference's own values, with the
    route recorded: every fixture has d <= 8 and at most 16 multi-index pairs per task pair, so all rows are fused."""
    from tests.test_gpu_multitask import kxx_scale, product_mt
    for k in ("FGP_MT_FUSED_ROWS", "FGP_WIDE_MT_POST_MEAN", "FGP_MT_POST_VAR_QF"):
        monkeypatch.delenv(k, raising=False)
    g = load_golden(name)
    assert int(g["d"]) <= N.MAX_D
    gp = product_mt(g)
    xd = torch.from_numpy(g["x_test"]).to(DEV)
    kxx = kxx_scale(g)
    gp.coeffs
    calls = _recorded(monkeypatch)
    pm, pv, pc = gp.post_mean(xd), gp.post_var(xd), gp.post_cov(xd[:4], xd[4:9])
    assert ROWS in calls and PARTS not in calls
    assert rel_err(pm, g["pmean"]) < pred_tol(name, "pmean", 1e-7)
    assert abs_err(pv, g["pvar"]) <= pred_tol(name, "pvar", 1e-8) * kxx
    assert abs_err(pc, g["pcov"]) <= pred_tol(name, "pcov", 1e-7) * kxx
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "1")
    del calls[:]
    assert rel_err(gp.post_mean(xd), g["pmean"]) < pred_tol(name, "pmean", 1e-7) and MEAN in calls and ROWS not in calls
    monkeypatch.delenv("FGP_WIDE_MT_POST_MEAN")
    if pred_tol(name, "pvar_new", 0.0) is not None:
        pv_new = gp.post_var(xd, n=torch.tensor([int(v) for v in g["n_new"]]))
        tol_ref = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
        assert abs_err(pv_new, g["pvar_new"]) <= tol_ref


def test_routing_at_d3(monkeypatch):
    for k in ("FGP_MT_FUSED_ROWS", "FGP_WIDE_MT_POST_MEAN", "FGP_MT_POST_VAR_QF"):
        monkeypatch.delenv(k, raising=False)
    gp = _lattice_t3()
    T, d = 3, 3
    x = torch.rand((16, d), generator=torch.Generator().manual_seed(2)).to(DEV)
    ref = gp.post_mean(x)                                                # (warms the caches: lam, the factor, coeffs)
    gp.post_var(x)
    calls = _recorded(monkeypatch)
    pm, pv, pc = gp.post_mean(x), gp.post_var(x), gp.post_cov(x[:4], x[4:9])
    assert PARTS not in calls and MEAN not in calls
    # post_mean T T blocks; post_var T T blocks and T zipped priors; post_cov 2 T T rows blocks and T T of kmat_new
    assert calls.count(ROWS) == T * T + (T * T + T) + (2 * T * T + T * T)
    assert abs_err(pm, ref) == 0.0
    # a post_mean past the byte threshold: 8 T N sum n > 2^22
    Nt = 512
    assert 8 * T * Nt * sum(gp._ns) > ops.MT_WIDE_POST_MEAN_BYTES
    xl = torch.rand((Nt, d), generator=torch.Generator().manual_seed(3)).to(DEV)
    del calls[:]
    big = gp.post_mean(xl)
    assert calls.count(MEAN) == T * T and ROWS not in calls and PARTS not in calls
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "0")
    del calls[:]
    rows = gp.post_mean(xl)
    assert calls.count(ROWS) == T * T and MEAN not in calls and _same_sums(gp, xl, big, rows)
    monkeypatch.delenv("FGP_WIDE_MT_POST_MEAN")
    # the fall-backs call neither
    del calls[:]
    g1 = gp.post_mean(x, eval=False)                                     # an autograd graph
    assert g1.requires_grad and ROWS not in calls and MEAN not in calls and PARTS in calls and rel_err(g1, ref) < 1e-9
    del calls[:]
    k = gp.kernel(x[:4, None, :], x[None, 4:9, :], torch.zeros((1, d), dtype=torch.int64, device=DEV),
                  torch.zeros((1, d), dtype=torch.int64, device=DEV))    # the public kernel
    assert ROWS not in calls and PARTS in calls and tuple(k.shape[-2:]) == (4, 5)
    monkeypatch.setenv("FGP_MT_FUSED_ROWS", "0")
    del calls[:]
    p0 = gp.post_mean(xl)
    assert ROWS not in calls and MEAN not in calls and PARTS in calls and rel_err(p0, big) < 1e-9


def test_routing_of_pairs_past_16_multi_indices_and_integer_inputs(monkeypatch):
    for k in ("FGP_MT_FUSED_ROWS", "FGP_WIDE_MT_POST_MEAN"):
        monkeypatch.delenv(k, raising=False)
    d = 5
    derivs = [torch.zeros((1, d), dtype=torch.int64), torch.eye(d, dtype=torch.int64)[:5]]
    dcoeffs = [torch.ones(1), torch.tensor([1.0, -0.5, 0.25, 2.0, -1.5])]
    gp25 = F.FastGPLattice([F.Lattice(d, seed=5 + l) for l in range(2)], num_tasks=2, alpha=3, device=DEV,
                           derivatives=derivs, derivatives_coeffs=[c.to(DEV) for c in dcoeffs])
    xs = gp25.get_x_next(n=[32, 32])
    gp25.add_y_next([torch.sin(3 * x).mean(1) + 0.1 * l for l, x in enumerate(xs)])
    assert gp25._fused_pair_spec(0, 1).P == 5 and gp25._fused_pair_spec(1, 1) is None       # 25 pairs
    x = torch.rand((8, d), generator=torch.Generator().manual_seed(4)).to(DEV)
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "1")
    both = gp25.post_mean(x)
    calls = _recorded(monkeypatch)
    both = gp25.post_mean(x)                                             # task 1 has an unfused pair: the rows route,
    assert MEAN not in calls and calls.count(ROWS) == 3 and calls.count(PARTS) == 1         # three blocks of it fused
    del calls[:]
    only0 = gp25.post_mean(x, task=0)                                    # (0, 0) and (0, 1) are fused: matrix-free
    assert calls.count(MEAN) == 2 and ROWS not in calls and _same_sums(gp25, x, only0[None], both[..., :1, :], tasks=[0])
    monkeypatch.delenv("FGP_WIDE_MT_POST_MEAN")
    # integer (already binary) net inputs
    net = F.FastGPDigitalNetB2([F.DigitalNetB2(2, seed=7, randomize="DS") for _ in range(2)], num_tasks=2, alpha=2, device=DEV)
    xn = net.get_x_next(n=[64, 32])
    net.add_y_next([_f(v) + 0.1 * l for l, v in enumerate(xn)])
    xf = torch.rand((8, 2), generator=torch.Generator().manual_seed(6)).to(DEV)
    xi = torch.floor(xf * 2.0 ** net.t).to(torch.int64)
    want = net.post_mean(xf)
    del calls[:]
    got = net.post_mean(xi)
    assert ROWS not in calls and MEAN not in calls and PARTS in calls and rel_err(got, want) < 1e-12


def test_a_task_without_points_is_skipped(monkeypatch):
    monkeypatch.delenv("FGP_MT_FUSED_ROWS", raising=False)
    gp = _lattice_t3(ns=(64, 0, 32))
    x = torch.rand((8, 3), generator=torch.Generator().manual_seed(8)).to(DEV)
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "0")
    calls = _recorded(monkeypatch)
    rows = gp.post_mean(x)
    assert calls.count(ROWS) == 3 * 2                                    # every requested task against tasks 0 and 2
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "1")
    del calls[:]
    pm = gp.post_mean(x)
    assert calls.count(MEAN) == 3 * 2 and ROWS not in calls
    assert _same_sums(gp, x, pm, rows)
    monkeypatch.setenv("FGP_MT_FUSED_ROWS", "0")
    assert rel_err(gp.post_mean(x), rows) < 1e-9


def test_post_mean_stores_no_kernel_rows(monkeypatch):
    for k in ("FGP_MT_FUSED_ROWS", "FGP_WIDE_MT_POST_MEAN"):
        monkeypatch.delenv(k, raising=False)
    T, d, ns, Nt = 3, 3, [4096, 1024, 4096], 2048
    gp = _lattice_t3(ns=ns)
    x = torch.rand((Nt, d), generator=torch.Generator().manual_seed(5)).to(DEV)
    rows_bytes = 8 * Nt * sum(ns)                                        # one requested task's rows: 151 MB
    assert rows_bytes == 150994944
    with torch.no_grad():
        gp.coeffs                                                        # the resident state: the solve, the points
        for l in range(T):
            gp._xb_dm(l, ns[l])
    calls = _recorded(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pm = gp.post_mean(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak bytes above the resident state: %d (one requested task's rows %d, all three %d)" % (peak, rows_bytes, T * rows_bytes))
    assert calls.count(MEAN) == T * T and ROWS not in calls and PARTS not in calls
    assert tuple(pm.shape) == (T, Nt) and bool(torch.isfinite(pm).all())
    assert peak < rows_bytes // 8, peak
    # the same numbers as the rows route on a slice that route can hold
    monkeypatch.setenv("FGP_WIDE_MT_POST_MEAN", "0")
    assert _same_sums(gp, x[:64], pm[:, :64], gp.post_mean(x[:64]))
