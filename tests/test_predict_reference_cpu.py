"""The extended-precision reference of the prediction kernels (tests/predict_reference.py), pinned without a GPU:

  * its kernel rows equal OracleFastGP.kernel and its transforms equal the oracle's fftbr / fwht, to fp64 rounding;
  * its Walsh parts of order 2..4 equal the truncated defining series (the helper of tests/test_oracle_golden.py);
  * an fp64 evaluation of the rows in the kernels' own form stays inside the derived tolerance C 2^-53 B, and the same
    evaluation 2e-11 off does not: the bound is neither too tight for a correct kernel nor vacuous;
  * the non-vacuity caps of every case of the GPU matrix (tests/predict_cases.py): C 2^-53 B_q <= 1e-11 |q| for every
    output of a 'regular' case, max B_q <= 100 max |q| for a 'signed' one;
  * fgp_post_mean accepts N == 0 for every B it otherwise accepts, before any HIP call.
"""
import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from oracle import fgp_oracle as O
from tests import predict_cases as PC
from tests import predict_reference as PR
from tests.test_oracle_golden import _walsh_series

torch.set_default_dtype(torch.float64)
U = PR.EPS53
CAP = 1e-11


def test_extended_precision_is_extended():
    assert PR.MP or np.finfo(np.longdouble).eps < 2e-19


@pytest.mark.parametrize("fam,alphas", [(PC.LAT, [1, 2, 3, 4]), (PC.LAT, [2, 2, 2]), (PC.NET, [1, 1]), (PC.NET, [1, 2, 3, 4])])
def test_rows_equal_the_oracle_kernel(fam, alphas):
    d, n, Nt, t = len(alphas), 300, 6, 40
    g = np.random.default_rng(3)
    xt, z = PC._points(g, fam, d, n, Nt, t)
    hyp = PC._hyp(g, 2, d, "signed")
    order, coef = PC.pred_args(fam, alphas)
    K, BK = PR.kernel_rows(fam, xt, z, hyp, order, coef, t)
    for gi in range(2):
        kw = dict(alpha=alphas, scale=float(hyp[gi, 0]), lengthscales=torch.from_numpy(hyp[gi, 1:]))
        if fam == PC.LAT:
            o = O.OracleFastGP("lattice", torch.from_numpy(z.T.copy()), None, torch.zeros(n), **kw)
            ko = o.kernel(torch.from_numpy(xt)[:, None, :], torch.from_numpy(z.T.copy())[None])
        else:
            zb = torch.from_numpy(z.T.copy())
            o = O.OracleFastGP("net", torch.from_numpy(xt), zb, torch.zeros(n), t=t, **kw)
            ko = o.kernel(torch.from_numpy(xt)[:, None, :], zb[None])
        ko = ko.detach().numpy()
        # the oracle's Horner form in x cancels up to 190-fold at order 8: 1e-12 of the largest value
        assert np.abs(PR.to_f64(K[gi]) - ko).max() <= 1e-12 * np.abs(ko).max()
        assert (PR.to_f64(BK[gi]) >= np.abs(ko) * (1 - 1e-12)).all()


def test_transforms_equal_the_oracle():
    g = np.random.default_rng(4)
    for m in (1, 4, 11):
        r = g.standard_normal((3, 1 << m))
        re, im = PR.ft(PC.LAT, PR._x(r))
        y = O.fftbr(torch.from_numpy(r)).numpy()
        assert np.abs(PR.to_f64(re) - y.real).max() <= 1e-14 * (1 + m) and np.abs(PR.to_f64(im) - y.imag).max() <= 1e-14 * (1 + m)
        re, im = PR.ft(PC.NET, PR._x(r))
        assert np.abs(PR.to_f64(re) - O.fwht(torch.from_numpy(r)).numpy()).max() <= 1e-14 * (1 + m)
        assert not PR.to_f64(im).any()
    # Parseval with unit weights
    r = PR._x(g.standard_normal((2, 256)))
    for fam in (PC.LAT, PC.NET):
        q, B = PR.quadform(fam, r, r * 0, np.ones(256))
        assert np.abs(PR.to_f64(q - (r * r).sum(-1))).max() <= 1e-16 * 256 and (PR.to_f64(B) >= PR.to_f64(q)).all()


@pytest.mark.parametrize("order", [2, 3, 4])
def test_walsh_orders_equal_the_truncated_series(order):
    t = 5
    delta = np.arange(2 ** t)
    om = PR.to_f64(PR.walsh_omega(order, delta.astype(np.uint64), t))
    e1 = np.max(np.abs(_walsh_series(order, delta, t, t + 6) - om))
    e2 = np.max(np.abs(_walsh_series(order, delta, t, t + 9) - om))
    assert e2 <= 2.0 ** -9 and e2 < e1 / 4
    assert om[0] == pytest.approx(float(PR.WALSH_W[order]), abs=1e-15)
    # and the oracle's fp64 recursion at t = 10 and t = 63
    for tt in (10, 63):
        dl = np.random.default_rng(order).integers(0, 2 ** tt, 500, dtype=np.int64)
        a = PR.to_f64(PR.walsh_omega(order, dl.astype(np.uint64), tt))
        assert np.abs(a - O.walsh_omega(order, torch.from_numpy(dl), tt).numpy()).max() <= 1e-14


def _rows_fp64_u_form(xt, z, hyp, alphas, coef):
    """The lattice rows in fp64 as polynomials in u = t (t - 1) of t = |x - z| (numpy: no fma)."""
    K = np.empty((hyp.shape[0], xt.shape[0], z.shape[1]))
    for gi in range(hyp.shape[0]):
        p = np.ones((xt.shape[0], z.shape[1]))
        for j, al in enumerate(alphas):
            t = np.abs(xt[:, j, None] - z[j][None, :])
            u = t * t - t
            a = hyp[gi, 1 + j] * coef[j]
            if al == 1:
                f = a * u + (1.0 + a * (1.0 / 6.0))
            elif al == 2:
                f = (a * u) * u + (1.0 - a * (1.0 / 30.0))
            elif al == 3:
                f = (a * u * u) * (u - 0.5) + (1.0 + a * (1.0 / 42.0))
            else:
                f = (a * u * u) * (u * (u - 4.0 / 3.0) + 2.0 / 3.0) + (1.0 - a * (1.0 / 30.0))
            p = p * f
        K[gi] = hyp[gi, 0] * p
    return K


@pytest.mark.parametrize("name", ["var-lat-d8-n257-N5-B3-G3-c32-a12341234", "sgn-lat-d8-n33-N5-B3-G3-c32-a12341234-signed"])
def test_bound_admits_an_fp64_evaluation_and_rejects_a_wrong_one(name):
    case = PC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = PC.rm_reference(name)
    k64 = _rows_fp64_u_form(inp["xt"], inp["z"], inp["hyp"], case.alphas, inp["coef"])
    C = PC.c_rows(case)
    ratio = PR.to_f64(abs(PR._x(k64) - K) / (U * BK))
    assert ratio.max() <= C, ratio.max()
    m64 = np.stack([(k64[b % case.Gk] * inp["coeffs"][b][None, :]).sum(-1) for b in range(case.B)])
    assert PR.to_f64(abs(PR._x(m64) - mean) / (U * Bm)).max() <= PC.c_mean(case)
    if case.kind == "regular":                          # the cap makes 2e-11 relative visible at every output
        wrong = PR.to_f64(abs(PR._x(k64 * (1 + 2e-11)) - K) / (U * BK))
        assert wrong.min() > C
        wrong = PR.to_f64(abs(PR._x(m64 * (1 + 2e-11)) - mean) / (U * Bm))
        assert wrong.min() > PC.c_mean(case)


def _cap(kind, C, q, B, what):
    q, B = np.abs(PR.to_f64(q)), PR.to_f64(B)
    assert np.isfinite(q).all() and np.isfinite(B).all() and (B >= q * (1 - 1e-12)).all(), what
    if kind == "regular":
        worst = float((C * U * B / q).max())
        assert worst <= CAP, (what, worst, C)
    else:
        assert B.max() <= 100 * q.max(), (what, B.max() / q.max())


@pytest.mark.parametrize("name", [c.name for c in PC.RM_CASES])
def test_rows_and_mean_cases_are_not_vacuous(name):
    case = PC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = PC.rm_reference(name)
    assert K.shape == (case.Gk, case.N, case.n) and mean.shape == (case.B, case.N)
    assert inp["coeffs"].strides[0] == 8 * (case.n + case.pad)
    _cap(case.kind, PC.c_rows(case), K, BK, "rows")
    _cap(case.kind, PC.c_mean(case), mean, Bm, "mean")
    if case.N > 2 and case.n > 5 and case.fam == PC.LAT:
        assert (inp["xt"][2] == inp["z"][:, 5]).all() and not inp["xt"][0].any() and (inp["xt"][1] == 1).all()


@pytest.mark.parametrize("name", [c.name for c in PC.BT_CASES])
def test_batched_mean_cases_are_not_vacuous(name):
    case = PC.BT_BY_NAME[name]
    inp, mean, Bm = PC.bt_reference(name)
    assert mean.shape == (case.P, case.N)
    _cap("regular", PC.c_batched(case), mean, Bm, "batched mean")


def _qf_caps(case, inp, regenerated):
    rows, Br, power = PC.qf_reference(case, inp, regenerated)
    C = PC.c_quadform(case)
    for kind in PC.WA_KINDS:
        wa = inp["wa"][kind]
        if case.fam == PC.LAT:
            n = wa.shape[0]
            assert np.array_equal(wa[n // 2 + 1:], wa[1:n // 2][::-1]) or kind == "gp"
        for p in range(PC.QF_P):
            q, B = PR.quadform(case.fam, rows[p], Br[p], wa, power=power[p])
            _cap("regular", C, q, B, (kind, p))
    wa = inp["wa"]["gp"]
    assert wa.min() > 0 and wa.max() <= 1.0001 / PC.GP_NOISE and wa.max() / wa.min() <= 1e3


@pytest.mark.parametrize("name", [c.name for c in PC.QF_CASES])
def test_quadratic_form_cases_are_not_vacuous(name):
    case = PC.QF_BY_NAME[name]
    _qf_caps(case, PC.qf_inputs(case), False)


@pytest.mark.parametrize("name", [c.name for c in PC.QF_CASES if c.fam == PC.LAT and c.r2c is None and c.m != 16])
def test_regenerated_lattice_cases_are_not_vacuous(name):
    case = PC.QF_BY_NAME[name]
    _qf_caps(case, PC.qf_inputs(case, PC.qf_gen_points_cpu(case)), True)


def test_post_mean_accepts_no_test_points_for_every_output_count():
    """fgp_post_mean(N = 0) returns FGP_OK for every (B, Gk) it accepts at N > 0 -- B <= 4, or B > 4 with Gk == B
    (the block launch) -- and refuses what it refuses at N > 0, before following a pointer or making a HIP call."""
    L = N.lib()
    order, coef = N.int_array([4, 4]), N.double_array([1.0, 1.0])

    def rc(Nt, B, Gk, n=16, d=2):
        return L.fgp_post_mean(PC.LAT, None, Nt, None, n, d, 0, order, coef, None, Gk, None, n, B, None, Nt, None, 32, None)

    for B, Gk in ((1, 1), (3, 1), (4, 4), (4, 2), (10, 10), (5, 5), (512, 512)):
        assert rc(0, B, Gk) == 0, (B, Gk, L.fgp_last_error())
    assert rc(0, 10, 1) != 0 and rc(0, 10, 10, n=0) != 0 and rc(-1, 10, 10) != 0 and rc(0, 10, 10, d=9) != 0
    assert rc(5, 10, 10) != 0 and rc(5, 2, 2) != 0            # null pointers at N > 0
