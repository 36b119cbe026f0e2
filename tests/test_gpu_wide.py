"""Wide inputs (9 <= d <= 64 dimensions) on the GPU: the fgp_wide_* kernels and the FastGPLattice / FastGPDigitalNetB2
paths over them.

1. Per fixture (tests/golden/make_golden_wide.py -> tests/golden/wide/*.npz, the REAL reference), with the bounds of
   tests/test_gpu_gp.py: points array-equal, k1 parts 1e-14, lambda / ytilde 1e-12, MLL loss / norm term / gradients
   2e-7, coeffs 1e-6, post_mean 1e-8, post_var / post_cov 1e-8 K(x,x), cubature mean 1e-9 and variance 1e-8 scale, the
   3-iteration fit (loss history 2e-7, parameter histories 1e-10, post_mean afterwards 1e-7).
   (net_m7_d13_a2: Walsh order 2, parity unpinned at the qmcpy boundary as for every net fixture of order 2-4.)
2. Kernel corners against the torch formulation on the same device in fp64 (bounds derived where stated).
3. Routing: FGP_WIDE_FUSED=0 (the torch formulation over wide parts) passes the same loss / gradient / fit checks; the
   default goes through ops.wide_k1; d <= 8 GPs never reach a fgp_wide_* entry point.
4. fit(loss_metric="GCV" / "CV"), a user optimizer (Adam) and masks at d = 12 against the reference.
"""
import glob
import os

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native, ops
from tests.gpu_fixtures import DEV, abs_err, product_gp, rel_err

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

WIDE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WIDE_DIR, "*.npz")))
_LOADED = {}


def load_wide(name):
    if name not in _LOADED:
        with np.load(os.path.join(WIDE_DIR, name + ".npz"), allow_pickle=False) as f:
            _LOADED[name] = {k: f[k] for k in f.files}
    return _LOADED[name]


def wide_gp(g, **kw):
    """The product GP of a wide fixture: its explicit point set, its lengthscales (product_gp checks the points)."""
    return product_gp(g, lengthscales=torch.from_numpy(g["lengthscales"]).to(DEV), **kw)


def net_matrices(d, seed, t=32, mcols=32):
    """Unit-upper-triangular generating matrices (column k: bit t-1-k plus random more significant bits)."""
    rng = np.random.default_rng(seed)
    C = np.zeros((d, mcols), dtype=np.uint64)
    for j in range(d):
        for k in range(mcols):
            hi = int(rng.integers(0, 1 << k)) if k > 0 else 0
            C[j, k] = np.uint64((1 << (t - 1 - k)) | (hi << (t - k)))
    return C


# ---------------------------------------------------------------------------------------------- 1. fixtures
def test_fixtures_present():
    assert len(NAMES) == 8


@pytest.mark.parametrize("name", NAMES)
def test_wide_caches_match_reference(name):
    g = load_wide(name)
    gp = wide_gp(g)                                   # (points: array-equal to the fixture, asserted by product_gp)
    assert np.array_equal(gp.get_x(0).cpu().numpy(), g["x"])
    assert rel_err(gp.get_k1parts(), g["k1parts"]) <= 1e-14
    with torch.no_grad():
        assert rel_err(gp.get_lam(0, 0), g["lam"]) <= 1e-12
        assert rel_err(gp.get_ytilde(0), g["ytilde"]) <= 1e-12


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_wide_mll_and_gradient(name, fused, monkeypatch):
    """_loss_generic: torch autograd through ops.wide_k1 (fgp_wide_k1 / fgp_wide_k1_bwd) and the HIP transforms;
    fused = 0: the torch formulation of k1 over the wide parts."""
    monkeypatch.setenv("FGP_WIDE_FUSED", fused)
    g = load_wide(name)
    gp = wide_gp(g)
    d_out = int(torch.tensor(gp.shape_batch).prod())
    loss, t1, t2, _ = gp._loss_generic("MLL", None, 1, d_out)
    gs, gl = torch.autograd.grad(loss, [gp.raw_scale, gp.raw_lengthscales])
    print(name, fused, rel_err(loss, g["loss"]), rel_err(t1, g["norm_term"].sum()), rel_err(gs, g["grad_raw_scale"]),
          rel_err(gl, g["grad_raw_lengthscales"]))
    assert rel_err(loss, g["loss"]) <= 2e-7
    assert rel_err(t1, g["norm_term"].sum()) <= 2e-7
    assert rel_err(gs, g["grad_raw_scale"]) <= 2e-7
    assert rel_err(gl, g["grad_raw_lengthscales"]) <= 2e-7


@pytest.mark.parametrize("name", NAMES)
def test_wide_posteriors_match_reference(name):
    g = load_wide(name)
    gp = wide_gp(g)
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    kxx = float(gp._kdiag(xt).detach().abs().max())
    assert rel_err(gp.coeffs, g["coeffs"]) <= 1e-6
    assert rel_err(gp.post_mean(xt), g["pmean"]) <= 1e-8
    assert abs_err(gp.post_var(xt), g["pvar"]) <= 1e-8 * kxx
    assert abs_err(gp.post_cov(xt[:4], xt[4:9]), g["pcov"]) <= 1e-8 * kxx
    assert rel_err(gp.post_cubature_mean(), g["pcmean"]) <= 1e-9
    assert abs_err(gp.post_cubature_var(), g["pcvar"]) <= 1e-8 * float(gp.scale.max())
    n = 2 ** int(g["m"])
    assert abs_err(gp.post_var(xt, n=2 * n), g["pvar_2n"]) <= 1e-8 * kxx
    assert abs_err(gp.post_cubature_var(n=2 * n), g["pcvar_2n"]) <= 1e-8 * float(gp.scale.max())


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_wide_fit_trajectory_matches_reference(name, fused, monkeypatch):
    monkeypatch.setenv("FGP_WIDE_FUSED", fused)
    g = load_wide(name)
    gp = wide_gp(g)
    its = int(g["fit_iterations"])
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5)
    assert data["iterations"] == its
    assert rel_err(data["loss_hist"], g["fit_loss_hist"]) <= 2e-7
    assert rel_err(data["scale_hist"], g["fit_scale_hist"]) <= 1e-10
    assert rel_err(data["lengthscales_hist"], g["fit_lengthscales_hist"]) <= 1e-10
    assert rel_err(gp.raw_scale, g["fit_raw_scale"]) <= 1e-10
    assert rel_err(gp.raw_lengthscales, g["fit_raw_lengthscales"]) <= 1e-10
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xt), g["fit_pmean"]) <= 1e-7


# ---------------------------------------------------------------------------------------------- 2. kernel corners
def _k1_case(d, G, n, seed, big_ls=False):
    gen = torch.Generator().manual_seed(seed)
    parts = (torch.rand((d, n), generator=gen) * 1.2 - 0.6).to(DEV)          # parts of either sign, |p| <= 0.6
    scale = (0.5 + torch.rand((G,), generator=gen)).to(DEV)
    ls = (0.05 + 0.3 * torch.rand((G, d), generator=gen)).to(DEV)
    if big_ls:
        ls[:, ::3] = 4.0                                                      # 1 + 4 p < 0 wherever p < -0.25
    u = torch.randn((G, n), generator=gen).to(DEV)
    return parts, scale, ls, u


@pytest.mark.parametrize("n", [1, 16, 2 ** 13])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("d", [9, 13, 64])
def test_wide_k1_forward_backward_against_torch(d, G, n):
    """ops.wide_k1 against scale * (1 + ls * parts).prod(-2) with autograd and a random real u.  Bound 1e-12, relative
    to max |k1| (forward) and to sum_i |u_i dk1_i/dtheta| (backward): at most ~(2 d + log2 n + 8) roundings, ~2e-14
    at d = 64, n = 2^13, with a 50x margin for the summation / product order differing from torch's."""
    _check_k1(*_k1_case(d, G, n, 100 * d + 10 * G + (n % 7)))


def test_wide_k1_negative_factors():
    """Lengthscales large enough that factors 1 + l p are negative (and some close to zero): the leave-one-out
    products come from prefix / suffix products, never from k1 / factor."""
    parts, scale, ls, u = _k1_case(13, 3, 2 ** 13, 5, big_ls=True)
    parts[0, :8] = -0.25                                                       # factor exactly 0 in dimension 0
    assert bool(((1 + ls[:, :, None] * parts) < 0).any()) and bool(((1 + ls[:, :, None] * parts) == 0).any())
    _check_k1(parts, scale, ls, u)


def _check_k1(parts, scale, ls, u):
    s1, l1 = scale.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    k1 = ops.wide_k1(ops.LATTICE, parts, s1, l1)
    (k1 * u).sum().backward()
    s2, l2 = scale.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    fac = 1 + l2[:, :, None] * parts
    ref = s2[:, None] * fac.prod(-2)
    (ref * u).sum().backward()
    assert float((k1 - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    with torch.no_grad():
        # sum_i |u_i dk1_i / dtheta|: dk1/ds = prod f, dk1/dl_j = s p_j prod_{j' != j} f_j' (leave-one-out by masking)
        f = fac.detach()
        bs = (u * f.prod(-2)).abs().sum(-1)
        d = parts.shape[0]
        bl = torch.empty_like(ls)
        for j in range(d):
            fj = f.clone()
            fj[:, j] = 1.0
            bl[:, j] = (u * scale[:, None] * parts[j] * fj.prod(-2)).abs().sum(-1)
    es = (s1.grad - s2.grad).abs() / bs
    el = (l1.grad - l2.grad).abs() / bl
    print("k1 fwd/bwd rel err", float((k1 - ref).abs().max()) / float(ref.abs().max()), float(es.max()), float(el.max()))
    assert float(es.max()) <= 1e-12 and float(el.max()) <= 1e-12
    # bit-identical on a second call
    s3, l3 = scale.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    k3 = ops.wide_k1(ops.LATTICE, parts, s3, l3)
    (k3 * u).sum().backward()
    assert torch.equal(k3, k1) and torch.equal(s3.grad, s1.grad) and torch.equal(l3.grad, l1.grad)


def _corner_gp(family, d, alpha, Gk, seed):
    gen = torch.Generator().manual_seed(seed)
    kw = {}
    if Gk > 1:
        kw = dict(shape_batch=[Gk], shape_scale=[Gk, 1], scale=0.5 + torch.rand((Gk, 1), generator=gen),
                  lengthscales=0.02 + 0.18 * torch.rand((Gk, d), generator=gen))
    else:
        kw = dict(scale=0.5 + torch.rand((1,), generator=gen), lengthscales=0.02 + 0.18 * torch.rand((d,), generator=gen))
    if family == "lattice":
        return F.FastGPLattice(F.Lattice(d, seed=seed), alpha=alpha, device=DEV, **kw)
    seq = F.DigitalNetB2(d, seed=seed, generating_matrices=net_matrices(d, seed))
    return F.FastGPDigitalNetB2(seq, alpha=alpha, device=DEV, **kw)


def _train_points(gp, d, n, gen):
    if gp._FAMILY == ops.LATTICE:
        z = torch.rand((n, d), generator=gen).to(DEV)
    else:
        z = torch.randint(0, 2 ** gp.t, (n, d), generator=gen).to(DEV)
    return z, z.T.contiguous()


@pytest.mark.parametrize("family,d,alpha", [("lattice", 9, 3), ("lattice", 64, 2), ("net", 9, 2), ("net", 64, 1)])
def test_wide_kernel_rows_and_post_mean_against_torch(family, d, alpha):
    """Wide kernel_rows / post_mean_matfree against gp._kernel_torch: N in {1, 257} (crosses a 256-thread
    workgroup), n in {1, 2^8, 2^11}, B in {1, 3, 5, 8} outputs with shared and with per-output hyper-parameters
    (B = 5 crosses the 4-output block, B = 8 shared takes the GEMM path).  Rows 1e-13 relative; mean 1e-12 relative to
    sum_i |K_i c_i|."""
    gen = torch.Generator().manual_seed(d + alpha)
    worst_rows = worst_mean = 0.0
    for Gk in (1, 3, 5, 8):
        gp = _corner_gp(family, d, alpha, Gk, seed=11 + Gk)
        hyp = gp._hyp_rows(Gk > 1)
        assert hyp.shape == (Gk, 1 + d)
        for N in (1, 257):
            xt = torch.rand((N, d), generator=gen).to(DEV)
            for n in (1, 2 ** 8, 2 ** 11):
                z, z_dn = _train_points(gp, d, n, gen)
                with torch.no_grad():
                    ref = gp._kernel_torch(xt[:, None, :], z[None, :, :]).reshape(Gk, N, n)
                rows = ops.kernel_rows(gp._FAMILY, xt, z_dn, hyp, alphas=gp._alphas, tbits=gp._tbits())
                er = float((rows - ref).abs().max()) / float(ref.abs().max())
                worst_rows = max(worst_rows, er)
                assert er <= 1e-13, (Gk, N, n, er)
                # per-output hyper-parameters: B = Gk outputs; shared (Gk = 1): B in {1, 3, 5, 8}
                for B in ((Gk,) if Gk > 1 else (1, 3, 5, 8)):
                    c = torch.randn((B, n), generator=gen).to(DEV)
                    pm = ops.post_mean_matfree(gp._FAMILY, xt, z_dn, hyp, c, alphas=gp._alphas, tbits=gp._tbits())
                    kr = ref if Gk > 1 else ref.expand(B, N, n)
                    want = (kr * c[:, None, :]).sum(-1)
                    bound = (kr.abs() * c[:, None, :].abs()).sum(-1)
                    em = float(((pm - want).abs() / bound).max())
                    worst_mean = max(worst_mean, em)
                    assert em <= 1e-12, (Gk, B, N, n, em)
    print("worst rows / mean rel err", family, d, worst_rows, worst_mean)


def test_wide_post_mean_B8_shared_takes_gemm_path(monkeypatch):
    calls = []
    orig = ops.post_mean_gemm
    monkeypatch.setattr(ops, "post_mean_gemm", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    gp = _corner_gp("lattice", 9, 2, 1, seed=3)
    gen = torch.Generator().manual_seed(1)
    xt = torch.rand((5, 9), generator=gen).to(DEV)
    z, z_dn = _train_points(gp, 9, 64, gen)
    ops.post_mean_matfree(gp._FAMILY, xt, z_dn, gp._hyp_rows(False), torch.randn((8, 64), generator=gen).to(DEV),
                          alphas=gp._alphas)
    assert calls == [1]


@pytest.mark.parametrize("n_min,n_max", [(0, 1), (0, 256), (256, 512)])
def test_wide_lattice_points_bit_identical_to_host(n_min, n_max):
    d = 64
    seq = F.Lattice(d, seed=5)
    x = ops.lattice_points([int(v) for v in seq.z], seq.shift, n_min, n_max, device=DEV)
    assert np.array_equal(x.cpu().numpy(), seq(n_min, n_max))


# ---------------------------------------------------------------------------------------------- 3. routing
def _ackley_gp(family, d, n, **kw):
    from oracle.fgp_oracle import f_ackley
    if family == "lattice":
        gp = F.FastGPLattice(F.Lattice(d, seed=3), device=DEV, **kw)
    else:
        C = net_matrices(d, 3) if d > 8 else None
        gp = F.FastGPDigitalNetB2(F.DigitalNetB2(d, seed=3, generating_matrices=C), alpha=1, device=DEV, **kw)
    gp.add_y_next(f_ackley(gp.get_x_next(n)))
    return gp


def test_loss_generic_goes_through_wide_k1(monkeypatch):
    fwd, bwd = [], []
    of, ob = ops.wide_k1, ops.wide_k1_bwd_raw
    monkeypatch.setattr(ops, "wide_k1", lambda *a, **k: (fwd.append(1), of(*a, **k))[1])
    monkeypatch.setattr(ops, "wide_k1_bwd_raw", lambda *a, **k: (bwd.append(1), ob(*a, **k))[1])
    gp = _ackley_gp("lattice", 12, 2 ** 13, lengthscales=0.1)
    loss, _, _, _ = gp._loss_generic("MLL", None, 1, 1)
    assert fwd == [1] and bwd == []
    loss.backward()
    assert bwd == [1]
    assert torch.isfinite(gp.raw_lengthscales.grad).all() and gp.raw_lengthscales.grad.shape == (12,)
    # the torch formulation gives the same loss and gradient (loss / gradient bound of the fixture tests)
    monkeypatch.setenv("FGP_WIDE_FUSED", "0")
    gp2 = _ackley_gp("lattice", 12, 2 ** 13, lengthscales=0.1)
    loss2, _, _, _ = gp2._loss_generic("MLL", None, 1, 1)
    loss2.backward()
    assert fwd == [1] and bwd == [1]
    assert rel_err(loss, loss2.detach().cpu().numpy()) <= 2e-7
    assert rel_err(gp.raw_lengthscales.grad, gp2.raw_lengthscales.grad.cpu().numpy()) <= 2e-7


@pytest.mark.parametrize("family,d", [("lattice", 8), ("lattice", 3), ("net", 8), ("net", 3)])
def test_narrow_gps_never_call_wide_entry_points(family, d, monkeypatch):
    names = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    gp = _ackley_gp(family, d, 2 ** 8)
    xt = torch.rand((7, d), generator=torch.Generator().manual_seed(2)).to(DEV)
    gp.fit(iterations=2, verbose=0)
    opt = torch.optim.Rprop(gp.parameters(), lr=0.1)
    gp.fit(iterations=1, optimizer=opt, verbose=0)           # the generic autograd loop
    gp.post_mean(xt), gp.post_var(xt), gp.post_cov(xt[:2], xt[2:5]), gp.post_cubature_var()
    assert names and not [n for n in names if n.startswith("fgp_wide_")], names


def test_wide_gp_reaches_the_wide_entry_points(monkeypatch):
    names = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    gp = _ackley_gp("lattice", 12, 2 ** 8, lengthscales=0.1)
    xt = torch.rand((7, 12), generator=torch.Generator().manual_seed(2)).to(DEV)
    gp.fit(iterations=2, verbose=0)
    gp.post_mean(xt), gp.post_var(xt)
    assert {"fgp_wide_lattice_points", "fgp_wide_lattice_parts", "fgp_wide_k1", "fgp_wide_k1_bwd", "fgp_wide_post_mean",
            "fgp_wide_kernel_rows"} <= set(names)
    narrow = {"fgp_lattice_points", "fgp_lattice_parts", "fgp_net_parts", "fgp_kernel_rows", "fgp_post_mean",
              "fgp_nll_fwd", "fgp_nll_lam", "fgp_fit_run", "fgp_post_var_qf"}
    assert not narrow & set(names), narrow & set(names)


# ---------------------------------------------------------------------------------------------- 4. interface at d = 12
@pytest.mark.parametrize("metric", ["GCV", "CV"])
def test_wide_alternative_losses_match_reference(metric):
    """fit(loss_metric="GCV" / "CV") on the d = 12 net (the reference's lattice GCV raises, tests/test_gpu_losses.py)
    against the reference's 4-iteration trajectory, with that file's bounds."""
    g = load_wide("net_m8_d12_a1_b0")
    key = metric.lower()
    gp = wide_gp(g)
    its = len(g[key + "_loss_hist"]) - 1
    data = gp.fit(loss_metric=metric, iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=its + 5)
    assert rel_err(data["loss_hist"], g[key + "_loss_hist"]) <= 2e-7
    assert rel_err(gp.raw_lengthscales, g[key + "_raw_lengthscales"]) <= 1e-10
    assert rel_err(data["lengthscales_hist"], g[key + "_lengthscales_hist"]) <= 1e-10
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xt), g[key + "_pmean"]) <= 1e-8


def test_wide_user_optimizer_adam_matches_reference():
    """fit(optimizer=torch.optim.Adam(lr=0.05), iterations=3) on the d = 12 lattice against the reference.  Loss history:
    the MLL bound 2e-7.  Parameters: Adam's step lr m^ / (sqrt(v^) + eps) is a smooth function of the gradient ratios
    with |d step / d g_j| <= ~2 lr / |g_j|; the gradient is held to 2e-7 max|g| (above), so after 3 updates
    |delta raw_j| <= 3 x 2 lr x 2e-7 max|g| / min|g| with max / min |g| taken from the reference's own initial gradient
    (~7 here: ~4e-7 absolute)."""
    g = load_wide("lattice_m8_d12_a2_b0")
    gp = wide_gp(g)
    lr, its = 0.05, len(g["adam_loss_hist"]) - 1
    data = gp.fit(optimizer=torch.optim.Adam(gp.parameters(), lr=lr), iterations=its, store_hists=True, verbose=0,
                  stop_crit_wait_iterations=8)
    gall = np.abs(np.concatenate([g["grad_raw_scale"].reshape(-1), g["grad_raw_lengthscales"].reshape(-1)]))
    bound = its * 2 * lr * 2e-7 * gall.max() / gall.min()
    assert bound <= 1e-6
    assert rel_err(data["loss_hist"], g["adam_loss_hist"]) <= 2e-7
    assert abs_err(gp.raw_lengthscales, g["adam_raw_lengthscales"]) <= bound
    assert abs_err(gp.raw_scale, g["adam_raw_scale"]) <= bound
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xt), g["adam_pmean"]) <= 1e-7


@pytest.mark.parametrize("name", ["net_m8_d12_a1_b3", "lattice_m8_d12_a2_b3_po"])
def test_wide_masked_fit_matches_reference(name):
    """fit(masks=[[0, 2]]) on the B = 3 fixtures (shared and per-output hyper-parameters) against the reference, bounds
    of tests/test_gpu_masks.py."""
    g = load_wide(name)
    gp = wide_gp(g)
    its = len(g["mask_loss_hist"]) - 1
    data = gp.fit(iterations=its, store_hists=True, verbose=0, stop_crit_wait_iterations=8,
                  masks=torch.from_numpy(g["mask"]))
    assert rel_err(data["loss_hist"], g["mask_loss_hist"]) <= 2e-7
    assert rel_err(data["lengthscales_hist"], g["mask_lengthscales_hist"]) <= 1e-10
    assert rel_err(gp.raw_lengthscales, g["mask_raw_lengthscales"]) <= 1e-10
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    assert rel_err(gp.post_mean(xt), g["mask_pmean"]) <= 1e-7
