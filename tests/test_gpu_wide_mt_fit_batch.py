"""Parameter batches in the device-resident fit of multitask GPs on wide inputs (9 <= d <= 64): fgp_wide_mt_fit_batch_run
over G = d_out problems through multitask.WideMtEngine, FastGP.fit under FGP_WIDE_MT_FIT_BATCH=1.

1. Routing: under the switch a parameter-batched wide GP's fit() goes through fgp_wide_mt_fit_batch_run and Python never calls
   fgp_wide_mt_k1_bwd; without the switch, or with GCV, masks or an optimizer, it takes the generic loop; the two routes'
   histories agree at the bounds of 2.
2. The reference's 4-iteration trajectories (tests/golden/wide_batch_mt/*.npz, the REAL reference), the bounds of
   tests/test_gpu_multitask_batch.py: loss history 2e-7 relative, every fitted raw parameter 1e-9, post_mean 1e-8.
3. The summed loss row and every raw gradient of one evaluation against _norm_logdet() + autograd on the same GP, 2e-7
   (the gradient relative to max |g|, as tests/test_gpu_wide_mt_fit.py::_eval_case), d = 9, n = [8192, 4096], G = 4.
4. A frozen block keeps its bits; a block shared by all G ends at the generic loop's value.  5. Early stopping and the
   best-iterate restore as the generic loop.  6. The fit repeats bit for bit.
"""
import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from oracle.fgp_oracle import f_ackley
from tests.gpu_fixtures import DEV, rel_err
from tests.test_gpu_wide import net_matrices
from tests.test_gpu_wide_mt import _recorded
from tests.wide_mt_batch_cases import GOLDEN, PNAMES, golden_gp, load_golden_batch

pytestmark = pytest.mark.gpu
RUN = "fgp_wide_mt_fit_batch_run"          # the batch descriptor's counterpart of fgp_wide_mt_fit_run
torch.set_default_dtype(torch.float64)


@pytest.fixture(autouse=True)
def batch_switch(monkeypatch):
    monkeypatch.setenv("FGP_WIDE_MT_FIT_BATCH", "1")


def test_the_two_fixtures_exist():
    assert GOLDEN == ["lattice_d12_a2_T3_b2x3", "net_d9_a2_T3_b2x3"]


# ---------------------------------------------------------------------------------------------- 1. routing
def _fit(gp, its=2, **kw):
    return gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5, **kw)


def _raws(gp):
    return {nm: getattr(gp, nm).detach().clone() for nm in PNAMES}


def test_switch_routes_a_parameter_batch_to_the_device_loop(monkeypatch):
    g = load_golden_batch(GOLDEN[0])
    gp = golden_gp(g)
    assert gp._mt_wide_batch_ok() and not gp._mt_wide_ok() and gp._mt_param_rows() is not None
    calls = _recorded(monkeypatch)
    dev = _fit(gp)
    assert RUN in calls and "fgp_wide_mt_k1_bwd" not in calls
    monkeypatch.setenv("FGP_WIDE_MT_FIT_BATCH", "0")
    gp0 = golden_gp(g)
    calls = _recorded(monkeypatch)
    gen = _fit(gp0)
    assert RUN not in calls and "fgp_wide_mt_fit_run" not in calls and "fgp_wide_mt_k1_bwd" in calls
    assert rel_err(dev["loss_hist"], gen["loss_hist"]) <= 2e-7
    a, b = _raws(gp), _raws(gp0)
    for nm in PNAMES:
        assert float((a[nm] - b[nm]).abs().max()) <= 1e-9, nm


@pytest.mark.parametrize("case", ["unset", "gcv", "masks", "optimizer"])
def test_outside_the_route_the_generic_loop_runs(case, monkeypatch):
    g = load_golden_batch(GOLDEN[1])
    gp = golden_gp(g)
    kw = {}
    if case == "unset":
        monkeypatch.delenv("FGP_WIDE_MT_FIT_BATCH")
    elif case == "gcv":
        kw = dict(loss_metric="GCV")
    elif case == "masks":
        kw = dict(masks=torch.tensor([1]))
    else:
        kw = dict(optimizer=torch.optim.Rprop(gp.parameters(), lr=0.1))
    calls = _recorded(monkeypatch)
    _fit(gp, **kw)
    assert RUN not in calls and "fgp_wide_mt_fit_run" not in calls, case


def test_the_wide_fit_switch_alone_does_not_route_a_batch(monkeypatch):
    monkeypatch.delenv("FGP_WIDE_MT_FIT_BATCH")
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    gp = golden_gp(load_golden_batch(GOLDEN[1]))
    calls = _recorded(monkeypatch)
    _fit(gp)
    assert RUN not in calls and "fgp_wide_mt_fit_run" not in calls


# ---------------------------------------------------------------------------------------------- 2. reference
@pytest.mark.parametrize("name", GOLDEN)
def test_device_fit_follows_the_reference(name, monkeypatch):
    g = load_golden_batch(name)
    gp = golden_gp(g)
    its = len(g["fit_loss_hist"]) - 1
    calls = _recorded(monkeypatch)
    data = _fit(gp, its)
    assert RUN in calls and "fgp_wide_mt_k1_bwd" not in calls
    el = rel_err(data["loss_hist"], g["fit_loss_hist"])
    ep = {nm: float((getattr(gp, nm).detach().cpu() - torch.from_numpy(g["fit_" + nm])).abs().max()) for nm in PNAMES}
    em = rel_err(gp.post_mean(torch.from_numpy(g["x_test"]).to(DEV)), g["fit_pmean"])
    print("trajectory", name, "loss", el, "params", ep, "post_mean", em)
    assert el <= 2e-7, (data["loss_hist"], g["fit_loss_hist"])
    for nm in PNAMES:
        assert ep[nm] <= 1e-9, nm
    assert em <= 1e-8


# ---------------------------------------------------------------------------------------------- 3. one evaluation
def _eval_gp(family, d, ns, dl):
    T, sb = len(ns), [2, 2]
    kw = dict(num_tasks=T, alpha=2, device=DEV, requires_grad_noise=True, shape_batch=sb, shape_scale=sb + [1],
              shape_lengthscales=sb[1:] + [dl], shape_noise=[1], shape_factor_task_kernel=sb + [T, T],
              shape_noise_task_kernel=sb[1:] + [T])
    if family == "lattice":
        gp = F.FastGPLattice([F.Lattice(d, seed=3 + l) for l in range(T)], **kw)
    else:
        C = net_matrices(d, 3)
        gp = F.FastGPDigitalNetB2([F.DigitalNetB2(d, seed=3 + l, generating_matrices=C) for l in range(T)], **kw)
    gen = torch.Generator().manual_seed(7 * d + dl)
    with torch.no_grad():
        ls = torch.full((dl,), 0.07) if dl == 1 else 0.02 + 0.18 * torch.rand((d,), generator=gen)
        gp.raw_lengthscales.copy_(torch.log(ls).to(DEV).expand_as(gp.raw_lengthscales))
        for nm in PNAMES:
            p = getattr(gp, nm)
            p.add_((0.2 * (torch.rand(p.shape, generator=gen) - 0.5)).to(DEV))
    xs = gp.get_x_next(n=list(ns))
    amp = torch.tensor([[1.0, 1.3], [0.8, 1.1]], device=DEV)[..., None]
    gp.add_y_next([amp * (f_ackley(x) * (1 + 0.2 * l) + 0.1 * l) for l, x in enumerate(xs)])
    return gp


@pytest.mark.parametrize("dl", [1, 9])
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_loss_and_gradient_against_autograd(family, dl):
    d, ns = 9, [8192, 4096]
    gp = _eval_gp(family, d, ns, dl)
    assert gp.raw_lengthscales.shape[-1] == dl and gp._mt_wide_batch_ok()
    eng = gp._fused_engine(0, 0.1)
    assert type(eng).__name__ == "WideMtEngine" and eng.G == 4 and eng.B == 1
    raw0 = eng.raw.clone()
    eng.run(0, 1, final_no_update=True)
    norm, logdet = gp._norm_logdet()
    d_out = 4
    t1, t2 = norm.sum(), d_out / logdet.numel() * logdet.sum()
    loss = 0.5 * (t1 + t2 + d_out * sum(ns) * np.log(2 * np.pi))
    params = [getattr(gp, nm) for nm in PNAMES]
    assert all(p.requires_grad for p in params)
    gref = torch.cat([v.reshape(-1) for v in torch.autograd.grad(loss, params)])
    assert gref.numel() == eng.n_params == sum(eng.sizes)
    el = rel_err(eng.loss_hist[0, 0], torch.stack([loss.detach(), t1.detach(), t2.detach()]))
    eg = float((eng.grad - gref).abs().max()) / float(gref.abs().max())
    assert torch.equal(eng.raw, raw0) and torch.equal(eng.raw_hist[0], raw0)
    print("one evaluation", family, d, ns, dl, "loss row rel err", el, "gradient rel err", eg)
    assert el <= 2e-7 and eg <= 2e-7, (el, eg)


# ---------------------------------------------------------------------------------------------- 4. frozen, shared
def test_frozen_block_keeps_its_bits_and_shared_block_follows_the_generic_loop(monkeypatch):
    g = load_golden_batch(GOLDEN[0])
    kw = dict(requires_grad_lengthscales=False, requires_grad_noise=True)
    gp = golden_gp(g, **kw)
    assert tuple(gp.raw_noise.shape) == (1,)                   # no batch dimensions: one row, shared by all G
    before = _raws(gp)
    calls = _recorded(monkeypatch)
    _fit(gp, 3)
    assert RUN in calls
    after = _raws(gp)
    assert torch.equal(after["raw_lengthscales"], before["raw_lengthscales"]) and not gp.raw_lengthscales.requires_grad
    for nm in PNAMES:
        if nm != "raw_lengthscales":
            assert bool((after[nm] != before[nm]).all()), nm
    monkeypatch.setenv("FGP_WIDE_MT_FIT_BATCH", "0")
    gp0 = golden_gp(g, **kw)
    _fit(gp0, 3)
    ref = _raws(gp0)
    assert float((after["raw_noise"] - ref["raw_noise"]).abs().max()) <= 1e-10
    for nm in PNAMES:
        assert float((after[nm] - ref[nm]).abs().max()) <= 1e-10, nm


# ---------------------------------------------------------------------------------------------- 5. early stopping
def test_early_stop_and_best_iterate_restore_as_the_generic_loop(monkeypatch):
    """As tests/test_gpu_wide_mt_fit.py: an improvement threshold no iteration reaches, so the rule ends the fit after two
    iterations without a sufficient improvement, inside the device loop's first chunk."""
    g = load_golden_batch(GOLDEN[1])
    kw = dict(iterations=12, store_hists=True, verbose=0, stop_crit_wait_iterations=2, stop_crit_improvement_threshold=1e30)
    out, gps = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("FGP_WIDE_MT_FIT_BATCH", switch)
        gps[switch] = golden_gp(g)
        calls = _recorded(monkeypatch)
        out[switch] = gps[switch].fit(**kw)
        assert (RUN in calls) == (switch == "1") and "fgp_wide_mt_fit_run" not in calls
    assert out["1"]["iterations"] == out["0"]["iterations"] < 12
    assert rel_err(out["1"]["loss_hist"], out["0"]["loss_hist"]) <= 2e-7
    for nm in PNAMES:
        assert float((getattr(gps["1"], nm).detach() - getattr(gps["0"], nm).detach()).abs().max()) <= 1e-10, nm


# ---------------------------------------------------------------------------------------------- 6. repeatability
def test_fit_repeats_bit_for_bit():
    g = load_golden_batch(GOLDEN[0])
    hists = []
    for _ in range(2):
        eng = golden_gp(g)._fused_engine(3, 0.1)
        assert eng.G == 6
        eng.run(0, 4, final_no_update=True)
        hists.append((eng.raw_hist[:4].clone(), eng.loss_hist[:4].clone(), eng.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*hists))
    assert not torch.equal(hists[0][0][0], hists[0][0][3])
