"""The extended-precision reference of the wide kernels (9 <= d <= 64; tests/predict_reference.py, cases of
tests/wide_cases.py), pinned without a GPU:

  * the first-column functions added for the wide path (lattice_parts, net_parts, k1, k1_bwd) and kernel_rows at
    d in {9, 64} equal the oracle (oracle/fgp_oracle.py, generic in d) to its fp64 accuracy;
  * the non-vacuity caps of every case of the GPU matrix, on the arrays the GPU test uses;
  * per group, an fp64 numpy evaluation in the kernel's order (product over j ascending, scale last) stays within the
    derived C, and the same evaluation with one factor 2^-40 off does not: the tolerance sees an error of that size;
  * an fp64 emulation of k_wide_post_mean's folded form gives inf / NaN in the fold-range cases and a result inside
    the bound at 1e-6, and the range W <= 960 (wide_cases.fold_log2) separates the two.
"""
import numpy as np
import pytest
import torch

from oracle import fgp_oracle as O
from tests import predict_cases as PC
from tests import predict_reference as PR
from tests import wide_cases as WC

torch.set_default_dtype(torch.float64)
U = float(PR.EPS53)
OFF = 2.0 ** -40


def _ratio(dev, ref, bnd):
    return PR.to_f64(abs(PR._x(np.asarray(dev)) - ref) / (PR.EPS53 * bnd))


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("d", [9, 64])
def test_first_column_reference_equals_the_oracle(d):
    g = np.random.default_rng(d)
    n, G, t = 300, 2, 40
    alphas = WC._mixed(d)
    # lattice parts: x [n, d] against the point z
    x, z = g.random((n, d)), g.random(d)
    P, B = PR.lattice_parts(x, z, [2 * a for a in alphas], [PC.lattice_coef(a) for a in alphas])
    po = O.lattice_kernel_parts(torch.from_numpy(x), torch.from_numpy(z)[None], alphas).numpy().T
    # (the oracle's Horner form in x cancels up to 190-fold at order 8)
    assert np.abs(PR.to_f64(P) - po).max() <= 1e-12 * np.abs(po).max()
    assert (PR.to_f64(B) >= np.abs(po) * (1 - 1e-12)).all()
    # net parts
    xb, zb = g.integers(0, 2 ** t, (n, d), dtype=np.int64), g.integers(0, 2 ** t, d, dtype=np.int64)
    xb[5] = zb
    Pn, Bn = PR.net_parts(xb, zb, alphas, t)
    with np.errstate(divide="ignore"):
        pn = O.net_kernel_parts(torch.from_numpy(xb), torch.from_numpy(zb)[None], t, alphas).numpy().T
    assert np.abs(PR.to_f64(Pn) - pn).max() <= 1e-14 and (PR.to_f64(Bn) >= np.abs(pn) * (1 - 1e-12)).all()
    assert (PR.to_f64(Pn)[[j for j in range(d) if alphas[j] == 1], 5] == 1).all()
    # k1 and its adjoint: the oracle's formula and autograd through it
    parts = PR.to_f64(P)
    scale = torch.from_numpy(0.5 + g.random(G)).requires_grad_(True)
    ls = torch.from_numpy(0.02 + 2.0 * g.random((G, d))).requires_grad_(True)
    u = g.standard_normal((G, n))
    pt = torch.from_numpy(parts.T.copy())
    ko = torch.stack([O.kernel_from_parts(pt, scale[gi:gi + 1], ls[gi]) for gi in range(G)])          # [G, n]
    (ko * torch.from_numpy(u)).sum().backward()
    sc, l = scale.detach().numpy(), ls.detach().numpy()
    k, Bk = PR.k1(parts, sc, l)
    ds, Bs, dl, Bl = PR.k1_bwd(parts, sc, l, u)
    assert _ratio(ko.detach().numpy(), k, Bk).max() <= 4 + d           # torch's product order: d roundings at most
    assert _ratio(scale.grad.numpy(), ds, Bs).max() <= 4 * d + 2 * np.log2(n)
    assert _ratio(ls.grad.numpy(), dl, Bl).max() <= 4 * d + 2 * np.log2(n)
    assert (PR.to_f64(Bk) >= np.abs(PR.to_f64(k))).all() and (PR.to_f64(Bl) >= np.abs(PR.to_f64(dl))).all()


@pytest.mark.parametrize("fam,d", [(PC.LAT, 9), (PC.LAT, 64), (PC.NET, 9), (PC.NET, 64)])
def test_wide_rows_equal_the_oracle_kernel(fam, d):
    n, Nt, t = 100, 6, 40
    g = np.random.default_rng(3 + d)
    alphas = WC._mixed(d)
    xt, z = PC._points(g, fam, d, n, Nt, t)
    hyp = PC._hyp(g, 1, d, "regular")
    order, coef = PC.pred_args(fam, alphas)
    K, BK = PR.kernel_rows(fam, xt, z, hyp, order, coef, t)
    kw = dict(alpha=alphas, scale=float(hyp[0, 0]), lengthscales=torch.from_numpy(hyp[0, 1:]))
    zt = torch.from_numpy(z.T.copy())
    if fam == PC.LAT:
        o = O.OracleFastGP("lattice", zt, None, torch.zeros(n), **kw)
    else:
        o = O.OracleFastGP("net", torch.from_numpy(xt), zt, torch.zeros(n), t=t, **kw)
    ko = o.kernel(torch.from_numpy(xt)[:, None, :], zt[None]).detach().numpy()
    assert np.abs(PR.to_f64(K[0]) - ko).max() <= 1e-12 * np.abs(ko).max()
    assert (PR.to_f64(BK[0]) >= d * np.abs(ko) * (1 - 1e-12)).all()   # B_K >= d |K|: what the caps' factor 10 rests on


# ------------------------------------------------------------------------------------------------ caps
def _cap(kind, d, C, q, B, what, cap=WC.CAP):
    q, B = np.abs(PR.to_f64(q)), PR.to_f64(B)
    assert np.isfinite(q).all() and np.isfinite(B).all() and (B >= q * (1 - 1e-12)).all(), what
    if kind == "regular":
        worst = float((C * U * B / q).max())
        assert worst <= cap, (what, worst, C)
    else:
        assert B.max() <= 4 * d * q.max(), (what, B.max() / q.max() / d)


@pytest.mark.parametrize("name", [c.name for c in WC.RM_CASES])
def test_rows_and_mean_cases_are_not_vacuous(name):
    case = WC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = WC.rm_reference(name)
    assert K.shape == (case.Gk, case.N, case.n) and mean.shape == (case.B, case.N)
    assert inp["coeffs"].strides[0] == 8 * (case.n + case.pad)
    _cap(case.kind, case.d, WC.c_rows(case), K, BK, "rows")
    _cap(case.kind, case.d, WC.c_mean(case), mean, Bm, "mean")
    if case.N > 2 and case.n > 5 and case.fam == PC.LAT:
        assert (inp["xt"][2] == inp["z"][:, 5]).all() and not inp["xt"][0].any() and (inp["xt"][1] == 1).all()
    if case.ls == "2000":                               # the values the issue names: about 1e200 .. 1e233
        assert 1e150 < np.abs(PR.to_f64(K)).max() < 1e300


@pytest.mark.parametrize("name", [c.name for c in WC.QF_CASES])
def test_quadratic_form_cases_are_not_vacuous(name):
    case = WC.QF_BY_NAME[name]
    inp, runs = WC.qf_reference(name)
    ev = inp["ev"]
    assert ev.min() > 0 and 10 <= ev.max() / ev.min() <= 1e4
    C = WC.c_quadform(case)
    n = 1 << case.m
    for run in WC.QF_RUNS:
        rows, Br, power = runs[run]
        for kind in WC.WA_KINDS:
            wa = inp["wa"][kind]
            assert np.array_equal(wa[1], 2 * wa[0])
            if case.fam == PC.LAT and kind != "gp":
                assert np.array_equal(wa[0][n // 2 + 1:], wa[0][1:n // 2][::-1])
            for p in range(WC.QF_P):
                q, B = PR.quadform(case.fam, rows[p], Br[p], wa[p], power=power[p])
                _cap("regular", case.d, C, q, B, (run, kind, p), cap=WC.CAP_QF)


@pytest.mark.parametrize("name", [c.name for c in WC.K1_CASES])
def test_first_column_cases_are_not_vacuous(name):
    case = WC.K1_BY_NAME[name]
    inp, k, Bk, ds, Bs, dl, Bl = WC.k1_reference(name)
    assert k.shape == (case.G, case.n) and ds.shape == (case.G,) and dl.shape == (case.G, case.d)
    _cap(case.kind, case.d, WC.c_k1(case), k, Bk, "k1")
    _cap(case.kind, case.d, WC.c_k1_bwd_scale(case), ds, Bs, "dscale")
    _cap(case.kind, case.d, WC.c_k1_bwd_ls(case), dl, Bl, "dls")
    if case.kind == "signed":
        f = 1 + inp["ls"][:, :, None] * inp["parts"][None]
        assert (f < 0).any() and (f == 0).any()


@pytest.mark.parametrize("name", [c.name for c in WC.PT_CASES])
def test_parts_cases_are_not_vacuous(name):
    case = WC.PT_BY_NAME[name]
    inp, P, B = WC.parts_reference(name)
    assert P.shape == (case.d, case.n) and inp["x"].strides[0] == 8 * (case.d + 3)
    assert np.isfinite(PR.to_f64(P)).all() and WC.parts_cap_ok(WC.c_parts(case), P, B).all()
    assert (inp["x"][5] == inp["z"]).all()
    if case.fam == PC.LAT:
        assert (inp["x"] < inp["z"]).any() and (inp["x"] > inp["z"]).any()


# ------------------------------------------------------------------------------------------------ sensitivity
def _lat_factor64(al, t, a):
    u = t * t - t
    if al == 1:
        return a * u + (1.0 + a * (1.0 / 6.0))
    if al == 2:
        return (a * u) * u + (1.0 - a * (1.0 / 30.0))
    if al == 3:
        return (a * u * u) * (u - 0.5) + (1.0 + a * (1.0 / 42.0))
    return (a * u * u) * (u * (u - 4.0 / 3.0) + 2.0 / 3.0) + (1.0 - a * (1.0 / 30.0))


def _rows64(xt, z, hyp, alphas, coef, off=0.0):
    """The lattice rows [G, N, n] in fp64, product over j ascending from 1.0, scale last (numpy: no fma); off: the
    relative error put on the factor of dimension 1."""
    K = np.empty((hyp.shape[0], xt.shape[0], z.shape[1]))
    for gi in range(hyp.shape[0]):
        p = np.ones((xt.shape[0], z.shape[1]))
        for j, al in enumerate(alphas):
            f = _lat_factor64(al, np.abs(xt[:, j, None] - z[j][None, :]), hyp[gi, 1 + j] * coef[j])
            p = p * (f * (1 + off) if j == 1 else f)
        K[gi] = hyp[gi, 0] * p
    return K


def test_rows_and_mean_bound_admits_fp64_and_sees_a_factor_2pm40_off():
    name = "var-lat-d9-n257-N5-B3-G3-c32-amix"
    case = WC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = WC.rm_reference(name)
    for off, inside in ((0.0, True), (OFF, False)):
        k64 = _rows64(inp["xt"], inp["z"], inp["hyp"], case.alphas, inp["coef"], off)
        m64 = np.stack([(k64[b % case.Gk] * inp["coeffs"][b][None, :]).sum(-1) for b in range(case.B)])
        for r, C in ((_ratio(k64, K, BK), WC.c_rows(case)), (_ratio(m64, mean, Bm), WC.c_mean(case))):
            assert (r.max() <= C) if inside else (r.max() > C), (off, r.max(), C)


def _bitrev(m):
    i = np.arange(1 << m)
    r = np.zeros_like(i)
    for b in range(m):
        r |= ((i >> b) & 1) << (m - 1 - b)
    return r


def test_quadratic_form_bound_admits_fp64_and_sees_a_factor_2pm40_off():
    name = "qf-lat-m13-d9-amix"
    case = WC.QF_BY_NAME[name]
    inp, runs = WC.qf_reference(name)
    rows, Br, power = runs["stacked"]
    C = WC.c_quadform(case)
    n = 1 << case.m
    for off, inside in ((0.0, True), (OFF, False)):
        k64 = _rows64(inp["xt"][0], inp["z"][0], inp["hyp"][:1], case.alphas, inp["coef"], off)[0]
        p64 = np.abs(np.fft.fft(k64[:, _bitrev(case.m)], axis=-1)) ** 2 / n
        worst = 0.0
        for kind in WC.WA_KINDS:
            q, B = PR.quadform(case.fam, rows[0], Br[0], inp["wa"][kind][0], power=power[0])
            worst = max(worst, _ratio((inp["wa"][kind][0] * p64).sum(-1), q, B).max())
        assert (worst <= C) if inside else (worst > C), (off, worst, C)


def _k1_64(inp, off=0.0):
    """(k1, dscale, dls) in fp64: factors 1 + l p, products over j ascending, the leave-one-out product from prefix
    and suffix products; off: the relative error put on the factor of dimension 1."""
    parts, scale, ls, u = inp["parts"], inp["scale"], inp["ls"], inp["u"]
    d = parts.shape[0]
    f = 1 + ls[:, :, None] * parts[None]
    f[:, 1] *= 1 + off
    pre = np.ones_like(f)
    suf = np.ones_like(f)
    for j in range(1, d):
        pre[:, j] = pre[:, j - 1] * f[:, j - 1]
    for j in range(d - 2, -1, -1):
        suf[:, j] = suf[:, j + 1] * f[:, j + 1]
    prod = pre[:, d - 1] * f[:, d - 1]
    dl = ((u * scale[:, None])[:, None, :] * parts[None] * (pre * suf)).sum(-1)
    return scale[:, None] * prod, (u * prod).sum(-1), dl


def test_first_column_bound_admits_fp64_and_sees_a_factor_2pm40_off():
    name = "k1-d9-G3-n257"
    case = WC.K1_BY_NAME[name]
    inp, k, Bk, ds, Bs, dl, Bl = WC.k1_reference(name)
    for off, inside in ((0.0, True), (OFF, False)):
        k64, ds64, dl64 = _k1_64(inp, off)
        for r, C in ((_ratio(k64, k, Bk), WC.c_k1(case)), (_ratio(ds64, ds, Bs), WC.c_k1_bwd_scale(case)),
                     (_ratio(dl64, dl, Bl), WC.c_k1_bwd_ls(case))):
            assert (r.max() <= C) if inside else (r.max() > C), (off, r.max(), C)


def test_parts_bound_admits_fp64_and_sees_a_value_2pm40_off():
    name = "parts-lat-d9-omix"
    case = WC.PT_BY_NAME[name]
    inp, P, B = WC.parts_reference(name)
    dl = np.remainder(inp["x"] - inp["z"][None, :], 1.0)
    u = dl * dl - dl
    bern = {2: lambda v: v + 1 / 6, 4: lambda v: v * v - 1 / 30, 6: lambda v: (v * v) * (v - 0.5) + 1 / 42,
            8: lambda v: (v * v) * (v * (v - 4 / 3) + 2 / 3) - 1 / 30}                # B_2a in u, as the kernel
    p64 = np.stack([inp["coef"][j] * bern[o](u[:, j]) for j, o in enumerate(case.orders)])
    C = WC.c_parts(case)
    assert _ratio(p64, P, B).max() <= C
    assert _ratio(p64 * (1 + OFF), P, B).max() > C


# ------------------------------------------------------------------------------------------------ the fold
def _folded_mean64(case, inp):
    """k_wide_post_mean's folded form in fp64 numpy: per point prod_j (u^2 + c'_j) over j ascending, c' = (1 - a / 30)
    / a; the sum over the points; the scale times the a_j one after the other, last."""
    xt, z, hyp, coef = inp["xt"], inp["z"], inp["hyp"], inp["coef"]
    out = np.empty((case.B, case.N))
    with np.errstate(all="ignore"):
        for b in range(case.B):
            h = hyp[b % case.Gk]
            pr = np.ones((case.N, case.n))
            sc = h[0]
            for j in range(case.d):
                a = h[1 + j] * coef[j]
                t = np.abs(xt[:, j, None] - z[j][None, :])
                u = t * t - t
                pr = pr * (u * u + (1.0 - a * (1.0 / 30.0)) / a)
            for j in range(case.d):
                sc = sc * (h[1 + j] * coef[j])
            out[b] = sc * (pr * inp["coeffs"][b][None, :]).sum(-1)
    return out


@pytest.mark.parametrize("name", [c.name for c in WC.RM_CASES if c.ls is not None])
def test_folded_form_fails_exactly_outside_the_fold_range(name):
    case = WC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = WC.rm_reference(name)
    m64 = _folded_mean64(case, inp)
    W = WC.fold_log2(case, inp["hyp"], inp["coef"])
    if case.ls == "1e-6":
        assert np.isfinite(m64).all() and _ratio(m64, mean, Bm).max() <= WC.c_mean(case)
        assert (W <= WC.FOLD_LOG2).all()                # inside the range
    else:
        assert not np.isfinite(m64).all()               # inf or NaN for a mean that fp64 holds
        assert np.isfinite(PR.to_f64(mean)).all() and (W > WC.FOLD_LOG2).all()


def test_fold_range_keeps_every_regular_case_folded():
    """W of every alpha = 2 case outside the fold group is inside the range by 2^64 at least (a kernel that folds by
    this range computes those cases as it does now), and a zero lengthscale is outside."""
    for case in WC.RM_CASES:
        if case.fam == PC.LAT and set(case.alphas) == {2} and case.ls is None:
            inp = WC.rm_inputs(case)
            W = WC.fold_log2(case, inp["hyp"], inp["coef"])
            assert np.isinf(W).all() if case.zero_ls else (W <= WC.FOLD_LOG2 - 64).all(), (case.name, W)
