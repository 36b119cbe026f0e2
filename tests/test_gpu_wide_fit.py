"""The device-resident fit of wide GPs (9 <= d <= 64): fgp_wide_fit_run through wide_fit.WideMLL, FastGP.fit under
FGP_WIDE_FIT_DEVICE=1, fit_batched and GPBatch.

1. The reference's 3-iteration trajectories (tests/golden/wide/*.npz, the REAL reference) under the switch, with the
   bounds of tests/test_gpu_wide.py; the masked fit; the per-output fixture keeps the generic loop.
2. Loss and raw-parameter gradient of one evaluation against _loss_generic + autograd on the same device, 2e-7 (the
   bound the wide tests use between formulations; the gradient relative to max |g|).
3. Batched fits = individual fits = fit() under the switch, bit for bit (shared and stacked parts).
4. Frozen parameters keep their bits.  5. Early stopping and the best-iterate restore per GP.
6. GPBatch coeffs / post_mean / post_var against each GP's own.  7. Routing.
"""
import math

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native, batch
from oracle.fgp_oracle import f_ackley
from tests.gpu_fixtures import DEV, abs_err, rel_err
from tests.test_gpu_wide import _ackley_gp, load_wide, net_matrices, wide_gp

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

SINGLE = ["lattice_m6_d9_a3_b0", "lattice_m7_d64_a2_b0", "lattice_m8_d12_a2_b0", "net_m6_d64_a1_b0", "net_m7_d13_a2_b0",
          "net_m8_d12_a1_b0", "net_m8_d12_a1_b3"]


@pytest.fixture
def device_fit(monkeypatch):
    """FGP_WIDE_FIT_DEVICE=1 and a spy on _native.call."""
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    return _spy(monkeypatch)


def _spy(monkeypatch):
    names = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    return names


# ---------------------------------------------------------------------------------------------- 1. reference
def _check_trajectory(g, gp):
    its = int(g["fit_iterations"])
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5)
    assert data["iterations"] == its
    errs = (rel_err(data["loss_hist"], g["fit_loss_hist"]), rel_err(data["scale_hist"], g["fit_scale_hist"]),
            rel_err(data["lengthscales_hist"], g["fit_lengthscales_hist"]), rel_err(gp.raw_scale, g["fit_raw_scale"]),
            rel_err(gp.raw_lengthscales, g["fit_raw_lengthscales"]))
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    pm = rel_err(gp.post_mean(xt), g["fit_pmean"])
    print("trajectory errors (loss, scale, ls, raw scale, raw ls, pmean)", errs, pm)
    assert errs[0] <= 2e-7
    assert max(errs[1:]) <= 1e-10
    assert pm <= 1e-7


def _check_masked(g, gp):
    its = len(g["mask_loss_hist"]) - 1
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=8,
                  masks=torch.from_numpy(g["mask"]))
    assert rel_err(data["loss_hist"], g["mask_loss_hist"]) <= 2e-7
    assert rel_err(data["lengthscales_hist"], g["mask_lengthscales_hist"]) <= 1e-10
    assert rel_err(gp.raw_lengthscales, g["mask_raw_lengthscales"]) <= 1e-10
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xt), g["mask_pmean"]) <= 1e-7


@pytest.mark.parametrize("name", SINGLE)
def test_device_fit_trajectory_matches_reference(name, device_fit):
    g = load_wide(name)
    _check_trajectory(g, wide_gp(g))
    assert "fgp_wide_fit_run" in device_fit and "fgp_wide_k1_bwd" not in device_fit


def test_device_masked_fit_matches_reference(device_fit):
    g = load_wide("net_m8_d12_a1_b3")
    _check_masked(g, wide_gp(g))
    assert "fgp_wide_fit_run" in device_fit and "fgp_wide_k1_bwd" not in device_fit


def test_per_output_hyperparameters_keep_the_generic_loop(device_fit):
    g = load_wide("lattice_m8_d12_a2_b3_po")
    _check_trajectory(g, wide_gp(g))
    _check_masked(g, wide_gp(g))
    assert "fgp_wide_fit_run" not in device_fit and "fgp_wide_k1_bwd" in device_fit


def test_default_fit_stays_generic(monkeypatch):
    monkeypatch.delenv("FGP_WIDE_FIT_DEVICE", raising=False)
    names = _spy(monkeypatch)
    g = load_wide("net_m8_d12_a1_b0")
    _check_trajectory(g, wide_gp(g))
    assert "fgp_wide_fit_run" not in names and "fgp_wide_k1_bwd" in names


# ---------------------------------------------------------------------------------------------- 2. one evaluation
def _eval_case(family, d, n, dl):
    gen = torch.Generator().manual_seed(7 * d + dl)
    kw = dict(requires_grad_noise=True, scale=0.5 + float(torch.rand((), generator=gen)))
    if dl == 1:
        kw.update(lengthscales=0.07, shape_lengthscales=[1])
    else:
        kw.update(lengthscales=0.02 + 0.18 * torch.rand((d,), generator=gen))
    gp = _ackley_gp(family, d, n, **kw)
    assert gp.raw_lengthscales.shape[-1] == dl and gp._wide_fit_ok()
    eng = gp._wide_engine(0, 0.1)
    eng.run(0, 1, final_no_update=True)
    loss, t1, t2, _ = gp._loss_generic("MLL", None, 1, 1)
    gs, gl, gn = torch.autograd.grad(loss, [gp.raw_scale, gp.raw_lengthscales, gp.raw_noise])
    gref = torch.cat([gs.reshape(-1), gl.reshape(-1), gn.reshape(-1)])
    row = eng.loss_hist[0, 0]
    el = rel_err(row, torch.stack([loss.detach(), t1.detach(), t2.detach()]))
    eg = float((eng.grad - gref).abs().max()) / float(gref.abs().max())
    # final_no_update: the parameters are unstepped, and the history row holds them
    raw0 = torch.cat([gp.raw_scale.detach().reshape(-1), gp.raw_lengthscales.detach().reshape(-1),
                      gp.raw_noise.detach().reshape(-1)])
    assert torch.equal(eng.raw, raw0) and torch.equal(eng.raw_hist[0], raw0)
    print("one evaluation", family, d, n, dl, "loss row rel err", el, "gradient rel err", eg)
    return el, eg


@pytest.mark.parametrize("n", [16, 2 ** 8, 2 ** 13])
@pytest.mark.parametrize("d", [9, 13, 64])
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_loss_and_gradient_against_autograd(family, d, n):
    """n = 2^13: the first two-pass transform and more than one block of partials per sum."""
    for dl in (1, d):
        el, eg = _eval_case(family, d, n, dl)
        assert el <= 2e-7 and eg <= 2e-7, (dl, el, eg)


def test_loss_and_gradient_at_the_first_half_length_size():
    el, eg = _eval_case("lattice", 9, 2 ** 17, 9)
    assert el <= 2e-7 and eg <= 2e-7, (el, eg)


# ---------------------------------------------------------------------------------------------- 3 - 5. batches
def _lattice_z(d, k):
    """Generating vector k: seqs.Lattice's default (k = 0), else its components shifted by 2 k (odd, < 2^20)."""
    z = [int(v) for v in F.Lattice(d).z]
    return z if k == 0 else [z[0]] + [v + 2 * k for v in z[1:]]


def _replica(family, d, n, p, own_generator=False, **kw):
    """Shifted replica p (its own shift and data) of one lattice / net, or with a generator of its own."""
    if family == "lattice":
        seq = F.Lattice(d, seed=20 + p, generating_vector=_lattice_z(d, p if own_generator else 0))
        gp = F.FastGPLattice(seq, device=DEV, **kw)
    else:
        seq = F.DigitalNetB2(d, seed=20 + p, generating_matrices=net_matrices(d, 3 + (p if own_generator else 0)))
        gp = F.FastGPDigitalNetB2(seq, alpha=1, device=DEV, **kw)
    x = gp.get_x_next(n)
    gp.add_y_next(f_ackley(x) * (1 + 0.1 * p) + 0.05 * p * x[:, 0])
    return gp


def _raw(gp):
    return torch.cat([gp.raw_scale.detach().reshape(-1), gp.raw_lengthscales.detach().reshape(-1),
                      gp.raw_noise.detach().reshape(-1)])


@pytest.mark.parametrize("family,own", [("lattice", False), ("lattice", True), ("net", False)])
def test_batched_fits_are_the_individual_fits_bit_for_bit(family, own, monkeypatch):
    """P = 5 crosses fgp_wide_k1's four rows per workgroup; own = True: different generating vectors, the stacked
    parts.  Every GP: fit_batched(all) == fit_batched([gp]) == gp.fit() under the switch."""
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    d, n, P, its = 12, 2 ** 8, 5, 6
    engs = []
    orig = batch.batched_engine
    monkeypatch.setattr(batch, "batched_engine", lambda *a, **k: (engs.append(orig(*a, **k)), engs[-1])[1])
    together = [_replica(family, d, n, p, own) for p in range(P)]
    dt = F.fit_batched(together, iterations=its, store_hists=True)
    assert engs[0].G == P and engs[0].parts.dim() == (3 if own else 2)
    for p in range(P):
        alone = _replica(family, d, n, p, own)
        da = F.fit_batched([alone], iterations=its, store_hists=True)[0]
        solo = _replica(family, d, n, p, own)
        ds = solo.fit(iterations=its, store_hists=True, verbose=0)
        assert dt[p]["iterations"] == da["iterations"] == ds["iterations"] == its
        assert torch.equal(dt[p]["loss_hist"], da["loss_hist"]) and torch.equal(dt[p]["loss_hist"], ds["loss_hist"])
        assert torch.equal(_raw(together[p]), _raw(alone)) and torch.equal(_raw(together[p]), _raw(solo))
        # (different problems: Rprop's sign steps may coincide, the losses do not)
        assert not torch.equal(dt[p]["loss_hist"], dt[(p + 1) % P]["loss_hist"])


@pytest.mark.parametrize("frozen", ["noise", "scale"])
def test_frozen_parameters_keep_their_bits(frozen, monkeypatch):
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    kw = dict(requires_grad_scale=False) if frozen == "scale" else {}
    gps = [_replica("lattice", 12, 2 ** 8, p, scale=0.8, lengthscales=0.1, **kw) for p in range(2)]
    solo = _replica("lattice", 12, 2 ** 8, 2, scale=0.8, lengthscales=0.1, **kw)
    before = [_raw(gp).clone() for gp in gps + [solo]]
    F.fit_batched(gps, iterations=5)
    solo.fit(iterations=5, verbose=0)
    for gp, b in zip(gps + [solo], before):
        a = _raw(gp)
        keep = torch.zeros(a.numel(), dtype=torch.bool)
        keep[-1] = True                                        # the noise (requires_grad_noise = False, the default)
        if frozen == "scale":
            keep[0] = True
        keep = keep.to(DEV)
        assert torch.equal(a[keep], b[keep])
        assert bool((a[~keep] != b[~keep]).all())


def test_early_stopping_and_restore_per_gp(monkeypatch):
    d, n, P = 12, 2 ** 8, 3
    engs = []
    orig = batch.batched_engine
    monkeypatch.setattr(batch, "batched_engine", lambda *a, **k: (engs.append(orig(*a, **k)), engs[-1])[1])
    gps = [_replica("lattice", d, n, p) for p in range(P)]
    # from the default parameters 40 iterations all still improve (no GP stops); the checked fit starts from the
    # restored best iterate of a longer one, where Rprop's fresh 0.1 steps first overshoot and the rule has to act
    F.fit_batched(gps, iterations=300)
    datas = F.fit_batched(gps, iterations=40, store_hists=True)
    eng = engs[1]
    logtol, wait_max = math.log(1 + 5e-2), 10
    for p, (gp, data) in enumerate(zip(gps, datas)):
        losses = (-data["loss_hist"]).tolist()
        # the reference's rule (abstract_gp.py:241-289) on this GP's own history
        best, save, waited, best_i, stop = math.inf, math.inf, 0, 0, None
        for i, lv in enumerate(losses):
            if lv < best:
                best, best_i = lv, i
            if (save - lv) > logtol:
                waited, save = 0, best
            else:
                waited += 1
            if i == 40 or waited == wait_max:
                stop = i
                break
        print("GP", p, "stopped at", data["iterations"], "best iterate", best_i)
        assert stop == data["iterations"] == len(losses) - 1
        assert torch.equal(eng.loss_hist[:stop + 1, p, 0].cpu(), torch.tensor(losses))
        first_min = int(np.argmin(np.asarray(losses)))
        assert first_min == best_i
        row = eng.raw_hist[first_min]
        dl = gp.raw_lengthscales.shape[-1]
        want = torch.cat([row[p:p + 1], row[P + p * dl:P + (p + 1) * dl], row[P + P * dl + p:P + P * dl + p + 1]])
        assert torch.equal(_raw(gp), want)
    assert any(data["iterations"] < 40 for data in datas), "no GP stopped early: the rule was not exercised"


# ---------------------------------------------------------------------------------------------- 6. GPBatch
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_gpbatch_predictions_match_each_gp(family, monkeypatch):
    names = _spy(monkeypatch)
    d, n, P = 12, 2 ** 13, 3
    gps = [_replica(family, d, n, p, lengthscales=0.1) for p in range(P)]
    b = F.GPBatch(gps)
    b.set_data(torch.stack([gp._y[0] for gp in gps]).clone())
    datas = b.fit(iterations=4)
    assert [dd["iterations"] for dd in datas] == [4] * P
    c = b.coeffs()
    gen = torch.Generator().manual_seed(5)
    xt = torch.rand((7, d), generator=gen).to(DEV)
    xs = torch.rand((P, 5, d), generator=gen).to(DEV)
    pm, pms, pv = b.post_mean(xt), b.post_mean(xs), b.post_var(xt)
    assert pm.shape == (P, 7) and pms.shape == (P, 5) and pv.shape == (P, 7)
    assert "fgp_wide_fit_run" in names
    bad = [nm for nm in names if nm.startswith("fgp_fit_run") or nm in ("fgp_post_mean_batched", "fgp_post_var_batched",
                                                                     "fgp_nll_lam", "fgp_nll_fwd")]
    assert not bad, bad
    for p, gp in enumerate(gps):
        with torch.no_grad():
            kxx = float(gp._kdiag(xt).abs().max())
            errs = (rel_err(c[p], gp.coeffs), rel_err(pm[p], gp.post_mean(xt)), rel_err(pms[p], gp.post_mean(xs[p])),
                    abs_err(pv[p], gp.post_var(xt)) / kxx)
        print("GPBatch", family, p, "coeffs / mean / mean (own points) / var errors", errs)
        assert max(errs[:3]) <= 1e-10 and errs[3] <= 1e-8


# ---------------------------------------------------------------------------------------------- 7. routing
def test_narrow_batches_never_reach_the_wide_fit(monkeypatch):
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    names = _spy(monkeypatch)
    gps = [_ackley_gp("lattice", 3, 2 ** 8) for _ in range(2)]
    F.fit_batched(gps, iterations=2)
    gps[0].fit(iterations=2, verbose=0)
    assert names and not [nm for nm in names if nm.startswith("fgp_wide_")], names


def test_wide_batches_never_reach_the_narrow_fit(monkeypatch):
    names = _spy(monkeypatch)
    gps = [_replica("net", 9, 2 ** 8, p) for p in range(2)]
    F.fit_batched(gps, iterations=2)
    b = F.GPBatch(gps)
    b.fit(iterations=2)
    b.post_mean(torch.rand((3, 9), generator=torch.Generator().manual_seed(1)).to(DEV))
    assert "fgp_wide_fit_run" in names and "fgp_wide_post_mean" in names
    bad = [nm for nm in names if nm.startswith("fgp_fit_run") or nm == "fgp_post_mean_batched"]
    assert not bad, bad


def test_batches_refuse_per_output_hyperparameters():
    g = load_wide("lattice_m8_d12_a2_b3_po")
    with pytest.raises(AssertionError, match="fused MLL path"):
        F.fit_batched([wide_gp(g)], iterations=1)
