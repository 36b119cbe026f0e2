"""The GCV and CV losses of the device-resident fit of wide GPs (9 <= d <= 64): fgp_wide_fit_desc.loss_metric through
wide_fit.WideMLL, FastGP.fit(loss_metric=) under FGP_WIDE_FIT_DEVICE=1, fit_batched and GPBatch.fit(loss_metric=).

1. The reference's 4-iteration GCV / CV trajectories -- net_m8_d12_a1_b0's gcv_* / cv_* keys and the fixtures of
   tests/golden/make_golden_wide_losses.py (the REAL reference, noise 1e-2 trained, cv_weights 0.5) -- under the switch,
   with the bounds of test_wide_alternative_losses_match_reference: loss 2e-7, parameter histories and final raw
   parameters 1e-10, post_mean 1e-8.  The new fixtures also through the default generic loop.
   (Lattices: the reference's GCV / CV raise TypeError, tests/golden/make_golden_losses.py; they are held to the generic
   loop in 2.)
2. Loss and raw-parameter gradient of one evaluation against _loss_generic + autograd on the same device, 5e-7 (the
   project's device-against-generic bound for these losses; the gradient relative to max |g|).
3. Batched fits = fit() under the switch, bit for bit (shared and stacked parts, n = 2^13: a two-pass transform and four
   partials per sum).
4. History rows.  5. Frozen parameters keep their bits.  6. Early stopping and the best-iterate restore per GP.
7. Routing.
"""
import glob
import os

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from tests.gpu_fixtures import DEV, product_gp, rel_err
from tests.test_gpu_wide import _ackley_gp, load_wide, wide_gp
from tests.test_gpu_wide_fit import _raw, _replica, _spy

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

LOSS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_losses")
NEW = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(LOSS_DIR, "*.npz")))
_LOADED = {}
METRICS = ["GCV", "CV"]
CV_W = 0.5
NOISY = dict(noise=1e-2, requires_grad_noise=True)


def load_loss(name):
    if name not in _LOADED:
        with np.load(os.path.join(LOSS_DIR, name + ".npz"), allow_pickle=False) as f:
            _LOADED[name] = {k: f[k] for k in f.files}
    return _LOADED[name]


def _fit_kw(metric, w=CV_W):
    return dict(loss_metric=metric, cv_weights=w) if metric == "CV" else dict(loss_metric=metric)


@pytest.fixture
def device_fit(monkeypatch):
    """FGP_WIDE_FIT_DEVICE=1 and a spy on _native.call."""
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    monkeypatch.delenv("FGP_ALT_LOSS_DEVICE", raising=False)
    return _spy(monkeypatch)


def _on_device(names):
    return "fgp_wide_fit_run" in names and "fgp_wide_k1_bwd" not in names


def _generic(names):
    return "fgp_wide_fit_run" not in names and "fgp_wide_k1_bwd" in names


# ---------------------------------------------------------------------------------------------- 1. reference
def test_new_fixtures_present():
    assert NEW == ["net_m4_d9_a1_b0", "net_m6_d64_a1_b3", "net_m7_d13_a2_b0"]


def _check_d12(metric):
    """What test_wide_alternative_losses_match_reference checks.  The scale is left out as there: at this fixture's
    1e-16 nugget both losses are invariant to the scale (N1 and D, or I^2, carry the same scale^-2), dL/dscale is exactly
    zero and what any formulation computes for it is rounding whose sign Rprop follows."""
    g = load_wide("net_m8_d12_a1_b0")
    key = metric.lower()
    gp = wide_gp(g)
    its = len(g[key + "_loss_hist"]) - 1
    data = gp.fit(loss_metric=metric, iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5)
    errs = (rel_err(data["loss_hist"], g[key + "_loss_hist"]),
            rel_err(data["lengthscales_hist"], g[key + "_lengthscales_hist"]),
            rel_err(gp.raw_lengthscales, g[key + "_raw_lengthscales"]))
    pm = rel_err(gp.post_mean(torch.from_numpy(g["x_test"]).to(DEV)), g[key + "_pmean"])
    print("d12", metric, "errors (loss, ls history, raw ls, pmean)", errs, pm)
    assert data["iterations"] == its
    assert errs[0] <= 2e-7 and max(errs[1:]) <= 1e-10 and pm <= 1e-8


def _check_new(name, metric):
    g = load_loss(name)
    key = metric.lower()
    gp = product_gp(g, lengthscales=torch.from_numpy(g["lengthscales"]).to(DEV), noise=float(g["noise"]),
                    requires_grad_noise=True)
    its = len(g[key + "_loss_hist"]) - 1
    assert its == 4
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=9,
                  **_fit_kw(metric, float(g["cv_weight"])))
    hist = [rel_err(data[k + "_hist"], g[key + "_" + k + "_hist"]) for k in ("scale", "lengthscales", "noise")]
    raw = [rel_err(getattr(gp, "raw_" + k), g[key + "_raw_" + k]) for k in ("scale", "lengthscales", "noise")]
    el = rel_err(data["loss_hist"], g[key + "_loss_hist"])
    pm = rel_err(gp.post_mean(torch.from_numpy(g["x_test"]).to(DEV)), g[key + "_pmean"])
    print(name, metric, "errors: loss", el, "histories (scale, ls, noise)", hist, "raw", raw, "pmean", pm)
    assert data["iterations"] == its
    assert el <= 2e-7 and max(hist + raw) <= 1e-10 and pm <= 1e-8


@pytest.mark.parametrize("metric", METRICS)
def test_d12_trajectory_on_the_device_matches_reference(metric, device_fit):
    _check_d12(metric)
    assert _on_device(device_fit), sorted(set(device_fit))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NEW)
def test_trained_noise_trajectory_on_the_device_matches_reference(name, metric, device_fit):
    _check_new(name, metric)
    assert _on_device(device_fit), sorted(set(device_fit))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NEW)
def test_trained_noise_trajectory_in_the_generic_loop_matches_reference(name, metric, monkeypatch):
    monkeypatch.delenv("FGP_WIDE_FIT_DEVICE", raising=False)
    names = _spy(monkeypatch)
    _check_new(name, metric)
    assert _generic(names), sorted(set(names))


# ---------------------------------------------------------------------------------------------- 2. one evaluation
def _eval_case(family, d, n, dl, metric):
    gen = torch.Generator().manual_seed(7 * d + dl)
    kw = dict(scale=0.5 + float(torch.rand((), generator=gen)), **NOISY)
    if dl == 1:
        kw.update(lengthscales=0.07, shape_lengthscales=[1])
    else:
        kw.update(lengthscales=0.02 + 0.18 * torch.rand((d,), generator=gen))
    gp = _ackley_gp(family, d, n, **kw)
    assert gp.raw_lengthscales.shape[-1] == dl and gp._wide_fit_ok()
    eng = gp._wide_engine(0, 0.1, loss_metric=metric, cv_weight=CV_W)
    eng.run(0, 1, final_no_update=True)
    loss, t1, t2, _ = gp._loss_generic(metric, None, CV_W, 1)
    gs, gl, gn = torch.autograd.grad(loss, [gp.raw_scale, gp.raw_lengthscales, gp.raw_noise])
    gref = torch.cat([gs.reshape(-1), gl.reshape(-1), gn.reshape(-1)])
    row = eng.loss_hist[0, 0]
    el = rel_err(row[0], loss.detach())
    if metric == "GCV":                                        # (loss, numer, denom)
        et = max(rel_err(row[1], t1.detach()), rel_err(row[2], t2.detach()))
    else:
        et = 0.0
        assert bool(torch.isnan(row[1:]).all())
    eg = float((eng.grad - gref).abs().max()) / float(gref.abs().max())
    raw0 = _raw(gp)
    assert torch.equal(eng.raw, raw0) and torch.equal(eng.raw_hist[0], raw0)
    assert bool(torch.isfinite(eng.grad).all()) and float(gref[-1].abs()) > 0.0
    print("one evaluation", metric, family, d, n, dl, "loss rel err", el, "terms", et, "gradient rel err", eg)
    return max(el, et), eg


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [16, 2 ** 8, 2 ** 13])
@pytest.mark.parametrize("d", [9, 13, 64])
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_loss_and_gradient_against_autograd(family, d, n, metric):
    for dl in (1, d):
        el, eg = _eval_case(family, d, n, dl, metric)
        assert el <= 5e-7 and eg <= 5e-7, (dl, el, eg)


@pytest.mark.parametrize("metric", METRICS)
def test_loss_and_gradient_at_the_first_half_length_size(metric):
    el, eg = _eval_case("lattice", 9, 2 ** 17, 9, metric)
    assert el <= 5e-7 and eg <= 5e-7, (el, eg)


# ---------------------------------------------------------------------------------------------- 3. batches
def _noisy_replica(family, d, n, p, own=False, **kw):
    args = dict(lengthscales=0.1, **NOISY)
    args.update(kw)
    return _replica(family, d, n, p, own, **args)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family,own", [("lattice", False), ("lattice", True), ("net", False), ("net", True)])
def test_batched_fits_are_the_individual_fits_bit_for_bit(family, own, metric, monkeypatch):
    """own = True: a generator per GP, the stacked parts.  No environment switch for the batch; fit() under it."""
    monkeypatch.delenv("FGP_WIDE_FIT_DEVICE", raising=False)
    d, n, P, its = 12, 2 ** 13, 3, 5
    names = _spy(monkeypatch)
    together = [_noisy_replica(family, d, n, p, own) for p in range(P)]
    dt = F.fit_batched(together, iterations=its, store_hists=True, **_fit_kw(metric))
    assert _on_device(names), sorted(set(names))
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    for p in range(P):
        solo = _noisy_replica(family, d, n, p, own)
        start = _raw(solo).clone()
        ds = solo.fit(iterations=its, store_hists=True, verbose=0, **_fit_kw(metric))
        assert dt[p]["iterations"] == ds["iterations"] == its
        assert torch.equal(dt[p]["loss_hist"], ds["loss_hist"]), (dt[p]["loss_hist"], ds["loss_hist"])
        assert torch.equal(_raw(together[p]), _raw(solo))
        assert bool((_raw(solo) != start).all()), "a parameter did not move"
        assert not torch.equal(dt[p]["loss_hist"], dt[(p + 1) % P]["loss_hist"])
        assert bool((dt[p]["loss_hist"] > 0).all())
    assert "fgp_wide_k1_bwd" not in names


# ---------------------------------------------------------------------------------------------- 4. history rows
@pytest.mark.parametrize("metric", METRICS)
def test_history_rows(metric, device_fit, monkeypatch):
    its = 4
    gp = _noisy_replica("net", 12, 2 ** 8, 0)
    engs = []
    orig = gp._wide_engine
    monkeypatch.setattr(gp, "_wide_engine", lambda *a, **k: (engs.append(orig(*a, **k)), engs[-1])[1])
    data = gp.fit(iterations=its, store_hists=True, verbose=0, **_fit_kw(metric))
    assert _on_device(device_fit) and len(engs) == 1
    rows = engs[0].loss_hist[:its + 1, 0].cpu()
    assert bool(torch.isfinite(rows[:, 0]).all()) and bool((rows[:, 0] > 0).all())
    assert torch.equal(data["loss_hist"], rows[:, 0])
    if metric == "GCV":
        quot = rows[:, 1] / rows[:, 2]
        assert bool(((rows[:, 0] - quot).abs() <= 2.0 ** -52 * rows[:, 0].abs()).all()), (rows, quot)
        assert bool((rows[:, 1:] > 0).all())
    else:
        assert bool(torch.isnan(rows[:, 1:]).all())


# ---------------------------------------------------------------------------------------------- 5. frozen parameters
@pytest.mark.parametrize("metric", METRICS)
def test_frozen_noise_keeps_its_bits(metric, device_fit):
    gps = [_noisy_replica("lattice", 12, 2 ** 8, p, requires_grad_noise=False) for p in range(3)]
    before = [_raw(gp).clone() for gp in gps]
    F.fit_batched(gps[:2], iterations=5, **_fit_kw(metric))
    gps[2].fit(iterations=5, verbose=0, **_fit_kw(metric))
    assert _on_device(device_fit)
    for gp, b in zip(gps, before):
        a = _raw(gp)
        assert torch.equal(a[-1:], b[-1:])
        assert bool((a[:-1] != b[:-1]).all())


@pytest.mark.parametrize("metric", METRICS)
def test_only_the_noise_moves_when_the_rest_is_frozen(metric, device_fit):
    kw = dict(requires_grad_scale=False, requires_grad_lengthscales=False)
    gps = [_noisy_replica("net", 12, 2 ** 8, p, **kw) for p in range(3)]
    before = [_raw(gp).clone() for gp in gps]
    F.fit_batched(gps[:2], iterations=5, **_fit_kw(metric))
    gps[2].fit(iterations=5, verbose=0, **_fit_kw(metric))
    assert _on_device(device_fit)
    for gp, b in zip(gps, before):
        a = _raw(gp)
        assert torch.equal(a[:-1], b[:-1])
        assert bool((a[-1:] != b[-1:]).all())


# ---------------------------------------------------------------------------------------------- 6. early stopping
def test_early_stopping_and_restore_per_gp_in_a_gcv_batch(device_fit):
    """A batch of three against each GP fitted alone by fit() under the switch, from the same state: the restored best
    iterate of a longer fit, where Rprop's fresh 0.1 steps first overshoot and the stopping rule has to act."""
    d, n, P = 12, 2 ** 8, 3
    gps = [_noisy_replica("lattice", d, n, p) for p in range(P)]
    solos = [_noisy_replica("lattice", d, n, p) for p in range(P)]
    F.fit_batched(gps, iterations=300, loss_metric="GCV")
    datas = F.fit_batched(gps, iterations=40, store_hists=True, loss_metric="GCV")
    for p, (gp, solo, data) in enumerate(zip(gps, solos, datas)):
        solo.fit(loss_metric="GCV", iterations=300, verbose=0)
        ds = solo.fit(loss_metric="GCV", iterations=40, store_hists=True, verbose=0)
        losses = data["loss_hist"]
        print("GP", p, "stopped at", data["iterations"], "best iterate", int(torch.argmin(losses)))
        assert data["iterations"] == ds["iterations"] == len(losses) - 1
        assert torch.equal(losses, ds["loss_hist"])
        assert torch.equal(_raw(gp), _raw(solo))
    assert _on_device(device_fit)
    assert any(data["iterations"] < 40 for data in datas), "no GP stopped early: the rule was not exercised"
    assert any(int(torch.argmin(data["loss_hist"])) < data["iterations"] for data in datas), \
        "every best iterate is the last one: the restore was not exercised"


# ---------------------------------------------------------------------------------------------- 7. routing
def test_without_the_switch_the_fit_stays_generic(monkeypatch):
    monkeypatch.delenv("FGP_WIDE_FIT_DEVICE", raising=False)
    names = _spy(monkeypatch)
    _ackley_gp("net", 12, 2 ** 8, lengthscales=0.1, **NOISY).fit(loss_metric="GCV", iterations=2, verbose=0)
    assert _generic(names), sorted(set(names))


@pytest.mark.parametrize("why", ["masks", "cv_weights tensor", "FGP_ALT_LOSS_DEVICE=0"])
def test_under_the_switch_these_stay_generic(why, device_fit, monkeypatch):
    if why == "masks":
        gp = wide_gp(load_wide("net_m8_d12_a1_b3"))
        gp.fit(loss_metric="GCV", iterations=2, verbose=0, masks=torch.tensor([[0, 2]]))
    elif why == "cv_weights tensor":
        gp = _ackley_gp("net", 12, 2 ** 8, lengthscales=0.1, **NOISY)
        w = torch.linspace(0.5, 1.5, 2 ** 8).to(DEV)
        gp.fit(loss_metric="CV", iterations=2, verbose=0, cv_weights=w)
    else:
        monkeypatch.setenv("FGP_ALT_LOSS_DEVICE", "0")
        gp = _ackley_gp("net", 12, 2 ** 8, lengthscales=0.1, **NOISY)
        gp.fit(loss_metric="GCV", iterations=2, verbose=0)
    assert _generic(device_fit), sorted(set(device_fit))


def test_a_one_element_cv_weights_tensor_goes_to_the_device(device_fit):
    gp = _ackley_gp("net", 12, 2 ** 8, lengthscales=0.1, **NOISY)
    gp.fit(loss_metric="CV", iterations=2, verbose=0, cv_weights=torch.tensor([0.5]))
    assert _on_device(device_fit)


def test_narrow_batches_refuse_the_alternative_losses():
    gps = [_ackley_gp("lattice", 3, 2 ** 8) for _ in range(2)]
    with pytest.raises(AssertionError, match="narrow batch"):
        F.fit_batched(gps, iterations=2, loss_metric="GCV")
    with pytest.raises(AssertionError, match="narrow batch"):
        F.GPBatch(gps).fit(iterations=2, loss_metric="CV")
    F.fit_batched(gps, iterations=2, loss_metric="MLL")


@pytest.mark.parametrize("family", ["lattice", "net"])
def test_gpbatch_cv_fit_then_post_mean_matches_each_gp(family, monkeypatch):
    names = _spy(monkeypatch)
    d, n, P = 12, 2 ** 8, 3
    gps = [_noisy_replica(family, d, n, p) for p in range(P)]
    before = [_raw(gp).clone() for gp in gps]
    b = F.GPBatch(gps)
    b.set_data(torch.stack([gp._y[0] for gp in gps]).clone())
    datas = b.fit(iterations=4, store_hists=True, loss_metric="CV", cv_weights=CV_W)
    assert [dd["iterations"] for dd in datas] == [4] * P and _on_device(names)
    xt = torch.rand((7, d), generator=torch.Generator().manual_seed(5)).to(DEV)
    pm = b.post_mean(xt)
    for p, gp in enumerate(gps):
        assert bool((_raw(gp) != before[p]).all()) and bool((datas[p]["loss_hist"] > 0).all())
        assert datas[p]["loss_hist"][-1] < datas[p]["loss_hist"][0]
        with torch.no_grad():
            assert rel_err(pm[p], gp.post_mean(xt)) <= 1e-10
