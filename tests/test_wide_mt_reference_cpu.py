"""The extended-precision reference of the wide multitask kernels (tests/wide_mt_reference.py) and the case matrix of
tests/wide_mt_cases.py, without a device:

  * the reference against the REAL reference's fixtures (tests/golden/wide_mt): the pair parts k1parts_<a><b> from the
    stored points and the product's own spec tables (_pair_spec_eval), and lam_<a><b> = ft(k1) with the first column
    combined in 80-bit arithmetic and transformed by tests/transform_reference.ft -- no inverse transform in between;
  * the non-vacuity caps on the very arrays the GPU tests use (tests/test_gpu_wide_mt_exact.py): regular cases
    C 2^-53 B_q <= wide_cases.CAP |q|, cases with cancellation over p  max B_q <= 4 d max |q| (the signed cap of
    tests/test_gpu_wide_exact.py::_check), parts wide_cases.parts_cap_ok;
  * the reference's own consistency: the rows are the first column of the parts it forms from the same points, the
    adjoint is the derivative of the first column, and one pair without derivatives is predict_reference's kernel.
"""
import types

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import ops
from fastgaussianprocesses_amd.fast_gp import AbstractFastGP
from tests import predict_cases as PC
from tests import predict_reference as PR
from tests import transform_reference as TR
from tests import wide_cases as WC
from tests import wide_mt_cases as MC
from tests import wide_mt_reference as MR
from tests.test_wide_mt_cpu import NAMES, fixture_derivatives, load_wide_mt, make_oracle

torch.set_default_dtype(torch.float64)
U = PR.EPS53


def pair_tables(g, a, b):
    """(order, coef, add, ind, cc) of the fixture's task pair (a, b), from the product's _pair_spec_eval."""
    d, T = int(g["d"]), len(g["ns"])
    derivs, dcoeffs = fixture_derivatives(g)
    if derivs is None:
        derivs = [torch.zeros((1, d), dtype=torch.int64)] * T
        dcoeffs = [torch.ones(1)] * T
    fam = ops.LATTICE if str(g["family"]) == "lattice" else ops.NET
    stand_in = types.SimpleNamespace(_alphas=[int(g["alpha"])] * d, _FAMILY=fam, d=d)
    order, coef, add = AbstractFastGP._pair_spec_eval(stand_in, derivs[a], derivs[b])
    ind = ((derivs[a][:, None, :] + derivs[b][None, :, :]) == 0).to(torch.int64).reshape(-1, d).tolist()
    cc = (dcoeffs[a][:, None] * dcoeffs[b][None, :]).reshape(-1).tolist()
    return fam, order, coef, add, ind, cc


def _rel(a, ref):
    return float(np.max(np.abs(PR.to_f64(a) - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_the_fixtures_parts_and_lam(name):
    g = load_wide_mt(name)
    d, T = int(g["d"]), len(g["ns"])
    tb = int(g["t"]) if "t" in g else 0
    o = make_oracle(g)
    for a in range(T):
        for b in range(a, T):
            fam, order, coef, add, ind, cc = pair_tables(g, a, b)
            n = max(int(g["ns"][a]), int(g["ns"][b]))
            kp = g["k1parts_%d%d" % (a, b)]                             # [n, p0, p1, d]
            xa = o.points(a, n)[1].numpy()                              # (n may exceed task a's stored data)
            parts, _ = MR.mt_parts(fam, xa, o.points(b, 1)[1].numpy(), order, coef, add, tb)
            ref = kp.reshape(n, -1, d).transpose(1, 2, 0)
            assert _rel(parts, ref) < 1e-13
            k1, _ = MR.combine(parts, None, ind, cc, [1.0], g["lengthscales"][None, :])
            re, im = TR.ft(fam, k1)
            lam = g["lam_%d%d" % (a, b)].reshape(-1, n)[:1]
            got = PR.to_f64(re) + (1j * PR.to_f64(im) if np.iscomplexobj(lam) else 0)
            assert np.max(np.abs(got - lam)) <= 1e-12 * np.max(np.abs(lam))


# ------------------------------------------------------------------------------------------------ caps
def _cap(name, what, ref, bnd, C, kind, d):
    q, B = np.abs(PR.to_f64(ref)), PR.to_f64(bnd)
    assert np.isfinite(q).all() and np.isfinite(B).all() and (B >= 0).all()
    if kind == "regular":
        assert (C * U * B <= MC.CAP * q).all(), (name, what, float((C * U * B / np.maximum(q, 1e-300)).max()))
    else:
        assert B.max() <= 4 * d * q.max(), (name, what, float(B.max() / q.max()))


@pytest.mark.parametrize("name", [c.name for c in MC.K1_CASES])
def test_first_column_cases_stay_inside_their_caps(name):
    case = MC.K1_BY_NAME[name]
    inp, k, Bk, ds, Bs, dl, Bl = MC.k1_reference(name)
    _cap(name, "k1", k, Bk, MC.c_k1(case), case.kind, case.d)
    _cap(name, "dscale", ds, Bs, MC.c_k1_bwd_scale(case), case.kind, case.d)
    _cap(name, "dls", dl, Bl, MC.c_k1_bwd_ls(case), case.kind, case.d)
    if case.kind == "signed":                                # the exact zeros are there, and factors of either sign
        ind0 = [j for j in range(case.d) if inp["ind"][0][j] == 0]
        j = ind0[0] if ind0 else 0
        f = (0 if ind0 else 1) + inp["ls"][0, j] * inp["parts"][0, j, :8]
        assert (f == 0).all()
        assert ((1 + inp["ls"][:, None, :, None] * inp["parts"][None]) < 0).any()


@pytest.mark.parametrize("name", [c.name for c in MC.RW_CASES])
def test_rows_cases_stay_inside_their_caps(name):
    case = MC.RW_BY_NAME[name]
    inp, K, B = MC.rows_reference(name)
    _cap(name, "rows", K, B, MC.c_rows(case), case.kind, case.d)
    assert K.shape == ((case.Gk, case.N) if case.zip else (case.Gk, case.N, case.n))


@pytest.mark.parametrize("name", [c.name for c in MC.PT_CASES])
def test_parts_cases_stay_inside_their_caps(name):
    case = MC.PT_BY_NAME[name]
    inp, P, B, C = MC.parts_reference(name)
    E = case.N if case.zip else case.N * case.M
    assert P.shape == (case.P, case.d, E)
    assert WC.parts_cap_ok(C, P, B).all()
    pin = MC.pinned_pair(case)
    if pin is not None:                                                  # the pair at distance 0 is there
        assert (inp["x"][pin[0]] == inp["z"][pin[1]]).all()
    assert inp["x_full"].strides[0] == (case.d + 3) * 8


def test_the_matrix_covers_what_the_kernels_branch_on():
    k1 = MC.K1_CASES
    assert {c.d for c in k1} >= set(MC.DIMS) and {(c.d + 7) // 8 for c in k1} == set(range(2, 9))
    assert {c.n for c in k1} >= {1, 255, 257, 8225, 66048} and {c.P for c in k1} == {1, 3, 16}
    assert {c.G for c in k1} == {1, 4, 5, 8} and {c.pattern for c in k1} == {"ones", "mixed", "allbut1"}
    rw = MC.RW_CASES
    for fam in (MC.LAT, MC.NET):
        sub = [c for c in rw if c.fam == fam]
        assert {c.d for c in sub} >= set(MC.DIMS) and {c.P for c in sub} == {1, 3, 16} and {c.Gk for c in sub} == {1, 4, 5, 8}
        assert {c.n for c in sub} >= {1, 255, 257, 8225} and {c.N for c in sub if c.zip} == {1, 255, 257}
        assert {c.kind for c in sub} == {"regular", "signed"}
    assert {c.tbits for c in rw if c.fam == MC.NET} == {32, 63}
    assert {o for c in MC.PT_CASES if c.fam == MC.LAT for o in c.orders} == set(range(1, 9))
    assert {(o, c.tbits) for c in MC.PT_CASES if c.fam == MC.NET for o in c.orders} == {(o, t) for o in (1, 2, 3, 4) for t in (32, 63)}
    mixed = MC.ind_rows(9, 3, "mixed")
    assert [r.count(0) for r in mixed] == [0, 1, 3] and [r.count(1) for r in MC.ind_rows(9, 2, "allbut1")] == [1, 1]


# ------------------------------------------------------------------------------------------------ consistency
def test_rows_are_the_first_column_of_the_parts_of_the_same_points():
    case = MC.RW_BY_NAME[[c.name for c in MC.RW_CASES if c.fam == MC.LAT and c.kind == "signed"][0]]
    inp, K, B = MC.rows_reference(case.name)
    parts, _ = MR.mt_parts(case.fam, inp["xt"], inp["z"].T, inp["order"], inp["coef"], inp["add"])
    k1, _ = MR.mt_k1(PR.to_f64(parts), inp["ind"], inp["cc"], inp["hyp"][:, 0], inp["hyp"][:, 1:])
    # (the parts rounded to fp64 in between: 2^-53 per factor)
    assert np.max(np.abs(PR.to_f64(k1.reshape(K.shape) - K))) <= 4 * case.d * U * PR.to_f64(B).max()


def test_one_pair_without_derivatives_is_the_single_task_kernel():
    fam, d, n, N = MC.LAT, 9, 33, 3
    g = PC._rng(77)
    xt, z = PC._points(g, fam, d, n, N, 0)
    hyp = PC._hyp(g, 2, d, "regular")
    order, coef = PC.pred_args(fam, [2] * d)
    K0, _ = PR.kernel_rows(fam, xt, z, hyp, order, coef, 0)
    K1, _ = MR.mt_rows(fam, xt, z, hyp, [order], [coef], [[0.0] * d], [[1] * d], [1.0])
    assert np.max(np.abs(PR.to_f64(K1 - K0))) <= 1e-17 * np.max(np.abs(PR.to_f64(K0)))


def test_adjoint_is_the_derivative_of_the_first_column():
    case = MC.K1_BY_NAME[[c.name for c in MC.K1_CASES if c.kind == "signed" and c.d == 13][0]]
    inp, k, Bk, ds, Bs, dl, Bl = MC.k1_reference(case.name)
    u = PR._x(inp["u"])
    assert np.max(np.abs(PR.to_f64((u * k).sum(-1) / PR._x(inp["scale"]) - ds))) <= 1e-16 * PR.to_f64(Bs).max()
    h = 2.0 ** -20
    for j in (0, 5, case.d - 1):
        lp, lm = inp["ls"].copy(), inp["ls"].copy()
        lp[:, j] += h
        lm[:, j] -= h
        kp, _ = MR.mt_k1(inp["parts"], inp["ind"], inp["cc"], inp["scale"], lp)
        km, _ = MR.mt_k1(inp["parts"], inp["ind"], inp["cc"], inp["scale"], lm)
        fd = (u * (kp - km)).sum(-1) / (2 * h)
        assert np.max(np.abs(PR.to_f64(fd - dl[:, j]))) <= 1e-9 * PR.to_f64(Bl[:, j]).max()
