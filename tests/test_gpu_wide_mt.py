"""Multitask and derivative-informed fast GPs on wide inputs (9 <= d <= 64) on the device: the public classes on the
five fixtures of the REAL reference (tests/golden/make_golden_wide_mt.py) and against the dense oracle
(oracle/fgp_oracle_mt.py) on the same inputs -- construction, caches, the block inverse, the MLL and its gradients, every
posterior, the n_new projections and the 3-iteration fit trajectory -- once with the default (the fused
fgp_wide_mt_* first column and kernel rows) and once with FGP_WIDE_FUSED=0 (the torch formulation over
fgp_wide_mt_parts).  Tolerances are those of the corresponding tests of tests/test_gpu_multitask.py; no d > 8 case
needed a wider one.

Routing: with the default switch a d = 17 get_lam and post_mean call fgp_wide_mt_k1 / fgp_wide_mt_rows, never
fgp_mt_parts (which refuses d > 8) nor fgp_wide_mt_parts beyond the cached first-column parts, and allocate no
[N, M, P, d] temporary (torch.cuda.max_memory_allocated against the FGP_WIDE_FUSED=0 run of the same case); a task pair
with more than 16 derivative multi-index pairs takes the torch path and still matches the oracle.
"""
import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native as N
from tests.gpu_fixtures import DEV, abs_err, rel_err
from oracle.fgp_oracle_mt import OracleMultiTaskFastGP
from tests.test_wide_mt_cpu import NAMES, fixture_derivatives, kxx_scale, load_wide_mt, make_oracle

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

SWITCHES = ["fused", "torch"]


def _switch(monkeypatch, path):
    monkeypatch.setenv("FGP_WIDE_FUSED", "1" if path == "fused" else "0")


def product_mt(g, **kw):
    fam, d = str(g["family"]), int(g["d"])
    ns = [int(v) for v in g["ns"]]
    T, B = len(ns), int(g["B"])
    extra = dict(lengthscales=torch.from_numpy(g["lengthscales"]).clone(), **kw)
    if B > 0:
        extra["shape_batch"] = [B]
    derivs, dcoeffs = fixture_derivatives(g)
    if derivs is not None:
        extra["derivatives"], extra["derivatives_coeffs"] = derivs, [c.to(DEV) for c in dcoeffs]
    if fam == "lattice":
        seqs = [F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shifts"][l]) for l in range(T)]
        gp = F.FastGPLattice(seqs, num_tasks=T, alpha=int(g["alpha"]), device=DEV, **extra)
    else:
        seqs = [F.DigitalNetB2(d, randomize="DS", generating_matrices=g["C"].astype(np.uint64), t=int(g["t"]),
                               shift=g["shifts"][l].astype(np.uint64)) for l in range(T)]
        gp = F.FastGPDigitalNetB2(seqs, num_tasks=T, alpha=int(g["alpha"]), device=DEV, **extra)
    xs = gp.get_x_next(n=ns)
    for l in range(T):
        assert np.array_equal(xs[l].cpu().numpy(), g["x_%d" % l])
    gp.add_y_next([torch.from_numpy(g["y_%d" % l]).to(DEV) for l in range(T)])
    return gp


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_construction_and_caches(name, path, monkeypatch):
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    assert type(gp).__name__.startswith("MultiTask") and gp.d > 8
    assert not (gp._mt_fused_ok() or gp._mt_learn_ok() or gp._mt_general_ok())
    T = len(g["ns"])
    for a in range(T):
        for b in range(a, T):
            n = max(int(g["ns"][a]), int(g["ns"][b]))
            assert (gp._wide_pair_spec(a, b) is not None) == (path == "fused")
            assert rel_err(gp.get_k1parts(a, b, n), g["k1parts_%d%d" % (a, b)]) < 1e-12
            assert rel_err(gp.get_lam(a, b, n), g["lam_%d%d" % (a, b)]) < 1e-11
        assert rel_err(gp.get_ytilde(a), g["ytilde_%d" % a]) < 1e-12
    assert abs_err(gp.gram_matrix_tasks, g["gram_matrix_tasks"]) == 0.0


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_lam_doubling(name, path, monkeypatch):
    """get_lam at n from the cached lam at n / 2 (one DIT stage over the first column of the new half) equals the
    direct transform."""
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    n = int(g["ns"][0])
    with torch.no_grad():
        half = gp.get_lam(0, 0, n // 2)
        doubled = gp.get_lam(0, 0, n)
    assert ("lam", (0, 0, n // 2), True, False) in gp._cache and half.shape[-1] == n // 2
    assert rel_err(doubled, g["lam_00"]) < 1e-11


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_block_inverse(name, path, monkeypatch):
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    o = make_oracle(g)
    with torch.no_grad():
        inv, logdet = gp.get_inv_log_det()
        A, ld_o, _, _, _ = o.inv_logdet()
    Ao = A if np.iscomplexobj(g["inv"]) else A.real
    assert tuple(inv.shape) == tuple(g["inv"].shape)
    assert rel_err(inv, Ao) < 1e-7
    assert abs_err(logdet.reshape(-1), ld_o.reshape(-1)) <= 1e-10 * float(ld_o.abs().max()) + 1e-9
    assert rel_err(inv, g["inv"]) < 1e-6
    assert abs_err(logdet.reshape(-1), g["logdet"].reshape(-1)) <= 1e-8 * float(np.abs(g["logdet"]).max())


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_mll_and_gradients(name, path, monkeypatch):
    """loss and autograd gradients (fgp_wide_mt_k1_bwd under the default switch, then the transforms and
    fgp_mt_mll_grad) against the oracle's dense autograd and the reference's values."""
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    o = make_oracle(g)
    norm, logdet = gp._norm_logdet()
    d_out = int(torch.tensor(gp.shape_batch).prod())
    loss = 0.5 * (norm.sum() + d_out / torch.tensor(logdet.shape).prod() * logdet.sum()
                  + d_out * sum(int(v) for v in g["ns"]) * np.log(2 * np.pi))
    lo = o.mll_loss()
    assert abs(loss.item() - lo.item()) <= 1e-9 * abs(lo.item())
    names = [str(s) for s in g["grad_names"]]
    gr = torch.autograd.grad(loss, [getattr(gp, nm) for nm in names])
    go = torch.autograd.grad(lo, [getattr(o, nm) for nm in names])
    for nm, a, b in zip(names, gr, go):
        assert rel_err(a, b) < 1e-7, nm
    assert abs(loss.item() - float(g["loss"])) <= 2e-7 * abs(float(g["loss"]))
    for nm, a in zip(names, gr):
        assert rel_err(a, g["grad_" + nm]) < 2e-6, nm


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_predictions(name, path, monkeypatch):
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    o = make_oracle(g)
    xt = torch.from_numpy(g["x_test"])
    xd = xt.to(DEV)
    kxx = kxx_scale(g)
    ns_new = [int(v) for v in g["n_new"]]
    assert rel_err(gp.coeffs, o.coeffs().detach()) < 1e-6
    assert rel_err(gp.post_mean(xd), o.post_mean(xt)) < 1e-7
    assert abs_err(gp.post_var(xd), o.post_var(xt)) <= 1e-8 * kxx
    assert abs_err(gp.post_cov(xd[:4], xd[4:9]), o.post_cov(xt[:4], xt[4:9])) <= 1e-7 * kxx
    assert rel_err(gp.post_cubature_mean(), o.post_cubature_mean()) < 1e-7
    assert abs_err(gp.post_cubature_var(), o.post_cubature_var()) <= 1e-8 * kxx
    assert abs_err(gp.post_cubature_cov(), o.post_cubature_cov()) <= 1e-8 * kxx
    pv_new = gp.post_var(xd, n=torch.tensor(ns_new))
    kdiag = max(float(o.kernel(xt, xt, t, t).abs().max()) for t in range(o.T))
    tol_new = 2e-7 * kdiag if str(g["kind"]) == "deriv" else 1e-8 * kxx
    assert abs_err(pv_new, o.post_var(xt, ns_new)) <= tol_new
    assert abs_err(gp.post_cubature_var(n=torch.tensor(ns_new)), o.post_cubature_var(ns_new)) <= 1e-8 * kxx
    # against the reference's own values
    assert rel_err(gp.coeffs, g["coeffs"]) < 1e-5
    assert rel_err(gp.post_mean(xd), g["pmean"]) < 1e-7
    assert abs_err(gp.post_var(xd), g["pvar"]) <= 1e-8 * kxx
    assert abs_err(gp.post_cov(xd[:4], xd[4:9]), g["pcov"]) <= 1e-7 * kxx
    assert rel_err(gp.post_cubature_mean(), g["pcmean"]) < 1e-8
    assert abs_err(gp.post_cubature_var(), g["pcvar"]) <= 1e-8 * kxx
    assert abs_err(gp.post_cubature_cov(), g["pccov"]) <= 1e-8 * kxx
    tol_ref = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
    assert abs_err(pv_new, g["pvar_new"]) <= tol_ref
    assert abs_err(gp.post_cubature_var(n=torch.tensor(ns_new)), g["pcvar_new"]) <= 1e-8 * kxx
    # post_cov's diagonal is post_var; one task, and the public kernel() (the torch formulation at either switch)
    pc = gp.post_cov(xd, xd)
    T = pc.size(-4)
    r0, r1 = torch.arange(T), torch.arange(pc.size(-1))
    assert torch.allclose(pc[..., r0, r0, :, :][..., r1, r1], gp.post_var(xd)) and (gp.post_var(xd) >= 0).all()
    assert abs_err(gp.post_mean(xd, task=1), gp.post_mean(xd)[..., 1, :]) == 0.0
    kk = gp.kernel(xd[:, None, :], xd[None, :5, :], gp.derivatives[T - 1], gp.derivatives[0], gp.derivatives_coeffs[T - 1],
                   gp.derivatives_coeffs[0])
    assert abs_err(kk, o.kernel(xt[:, None, :], xt[None, :5, :], T - 1, 0).detach()) <= 1e-12 * kdiag


@pytest.mark.parametrize("path", SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_fit_trajectory(name, path, monkeypatch):
    """fit(store_hists) through the generic autograd loop (no device-resident multitask engine takes d > 6)."""
    _switch(monkeypatch, path)
    g = load_wide_mt(name)
    gp = product_mt(g)
    its = int(g["fit_iterations"])
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5)
    assert data["iterations"] == its
    assert rel_err(data["loss_hist"], g["fit_loss_hist"]) < 2e-7
    assert rel_err(data["lengthscales_hist"], g["fit_lengthscales_hist"]) < 1e-10
    assert rel_err(data["scale_hist"], g["fit_scale_hist"]) < 1e-10
    assert rel_err(data["task_kernel_hist"], g["fit_task_kernel_hist"]) < 1e-10
    xd = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xd), g["fit_pmean"]) < 1e-7


# ------------------------------------------------------------------------------------------------ routing
def _recorded(monkeypatch):
    calls = []
    real = N.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, "call", call)
    return calls


def _big_gp(g, n):
    """The fixture's derivative-informed lattice GP grown to n points per task (data: a smooth function of x)."""
    d, T = int(g["d"]), len(g["ns"])
    derivs, dcoeffs = fixture_derivatives(g)
    seqs = [F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shifts"][l]) for l in range(T)]
    gp = F.FastGPLattice(seqs, num_tasks=T, alpha=int(g["alpha"]), device=DEV, derivatives=derivs,
                         derivatives_coeffs=[c.to(DEV) for c in dcoeffs], lengthscales=torch.from_numpy(g["lengthscales"]).clone())
    xs = gp.get_x_next(n=[n] * T)
    gp.add_y_next([torch.sin(3 * x).mean(1) + 0.1 * l for l, x in enumerate(xs)])
    return gp


def test_wide_multitask_routing_and_peak_memory(monkeypatch):
    """d = 17, task 1 with two multi-indices: the pair (1, 1) has P = 4, so one [N, n, P, d] parts array of the torch
    formulation is 68 kernel-row blocks [N, n].  The torch run holds that array and at least one temporary of its size
    ((ind + l parts) before the product); the fused run's whole peak -- kernel rows of 2 blocks, their scaled copies and
    concatenations -- stays below a quarter of one such array."""
    g = load_wide_mt("deriv_lattice_d17_a3_c2")
    n, Nt, d, P11 = 4096, 60, 17, 4                          # (60 test points: one chunk of _kmat_block's torch loop)
    xd = torch.rand((Nt, d), generator=torch.Generator().manual_seed(3)).to(DEV)
    peak, out = {}, {}
    for path in SWITCHES:
        _switch(monkeypatch, path)
        gp = _big_gp(g, n)
        with torch.no_grad():
            gp.coeffs                                        # (the solve is the same work on both paths)
            gp.get_k1parts(0, 1)
        for key in [k for k in gp._cache if k[0] == "lam"]:
            del gp._cache[key]
        calls = _recorded(monkeypatch)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            lam = gp.get_lam(0, 1)
        pm = gp.post_mean(xd, task=1)
        torch.cuda.synchronize()
        peak[path] = torch.cuda.max_memory_allocated() - base
        out[path] = (lam, pm)
        monkeypatch.undo()
        assert "fgp_mt_parts" not in calls
        if path == "fused":
            assert "fgp_wide_mt_k1" in calls and calls.count("fgp_wide_mt_rows") == 2       # the blocks (1, 0), (1, 1)
            assert "fgp_wide_mt_parts" not in calls          # (the first-column parts are cached)
        else:
            assert "fgp_wide_mt_k1" not in calls and "fgp_wide_mt_rows" not in calls
            assert calls.count("fgp_wide_mt_parts") == 2
    assert rel_err(out["fused"][0], out["torch"][0]) < 1e-12 and rel_err(out["fused"][1], out["torch"][1]) < 1e-9
    temp = Nt * n * P11 * d * 8
    assert peak["torch"] >= 2 * temp, peak
    assert peak["fused"] <= temp // 4, peak


def test_predictions_with_an_autograd_graph_take_the_torch_path(monkeypatch):
    """eval=False with gradients enabled: the kernel rows carry a graph, so they come from the torch formulation over
    fgp_wide_mt_parts (no fgp_wide_mt_rows call), equal the eval=True values and are differentiable in the
    lengthscales."""
    g = load_wide_mt("deriv_lattice_d12_a2")
    gp = product_mt(g)
    xd = torch.from_numpy(g["x_test"]).to(DEV)
    ref = gp.post_mean(xd)
    calls = _recorded(monkeypatch)
    pm = gp.post_mean(xd, eval=False)
    assert pm.requires_grad and "fgp_wide_mt_rows" not in calls and "fgp_wide_mt_parts" in calls
    assert "fgp_wide_mt_k1" in calls                         # (the first columns stay fused: their adjoint is native)
    assert rel_err(pm, ref) < 1e-9
    gl, = torch.autograd.grad(pm.sum(), [gp.raw_lengthscales])
    assert gl.shape == gp.raw_lengthscales.shape and torch.isfinite(gl).all() and float(gl.abs().max()) > 0


def test_more_than_16_multi_index_pairs_take_the_torch_path(monkeypatch):
    """Task 1 is a sum of 5 first derivatives: the pair (1, 1) has 25 multi-index pairs, past the fused entry points'
    16 -- the torch formulation over fgp_wide_mt_parts (16 pairs a call) -- while (0, 0) and (0, 1) stay fused."""
    g = load_wide_mt("deriv_lattice_d12_a2")
    d, ns = 12, [32, 32]
    derivs = [torch.zeros((1, d), dtype=torch.int64), torch.eye(d, dtype=torch.int64)[:5]]
    dcoeffs = [torch.ones(1), torch.tensor([1.0, -0.5, 0.25, 2.0, -1.5])]
    seqs = [F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shifts"][l]) for l in range(2)]
    gp = F.FastGPLattice(seqs, num_tasks=2, alpha=3, device=DEV, derivatives=derivs,
                         derivatives_coeffs=[c.to(DEV) for c in dcoeffs], lengthscales=torch.from_numpy(g["lengthscales"]).clone())
    xs = gp.get_x_next(n=ns)
    ys = [torch.sin(3 * x).mean(1) + 0.1 * l for l, x in enumerate(xs)]
    gp.add_y_next(ys)
    o = OracleMultiTaskFastGP("lattice", g["z"], g["shifts"][:2], [y.cpu() for y in ys], alpha=3, derivatives=derivs,
                              derivatives_coeffs=dcoeffs)
    with torch.no_grad():
        o.raw_lengthscales.copy_(torch.log(torch.from_numpy(g["lengthscales"])))
    assert gp._wide_pair_spec(0, 0) is not None and gp._wide_pair_spec(0, 1) is not None and gp._wide_pair_spec(1, 1) is None
    calls = _recorded(monkeypatch)
    with torch.no_grad():
        lam11 = gp.get_lam(1, 1)
    assert "fgp_wide_mt_k1" not in calls and calls.count("fgp_wide_mt_parts") == 2            # 16 + 9 pairs
    assert rel_err(lam11, o.lam(1, 1, 32).detach()) < 1e-11
    xt = torch.from_numpy(g["x_test"])
    xd = xt.to(DEV)
    assert rel_err(gp.coeffs, o.coeffs().detach()) < 1e-6
    assert rel_err(gp.post_mean(xd), o.post_mean(xt)) < 1e-7
    kdiag = max(float(o.kernel(xt, xt, t, t).abs().max()) for t in range(2))
    assert abs_err(gp.post_var(xd), o.post_var(xt)) <= 1e-8 * 10 * kdiag
    with pytest.raises(RuntimeError, match="P=25"):
        N.call("fgp_wide_mt_k1_bwd_work", 32, d, 25, 1, None)
