"""The d <= 8 prediction kernels against the extended-precision reference (tests/predict_reference.py).

The entry points are called directly on synthetic inputs (tests/predict_cases.py: chosen conditioning, no fitted GP
and no nugget between input and output) and every output is compared with the operation's definition evaluated in
80-bit arithmetic from the very arrays the kernel read:

  * fgp_kernel_rows (k_kernel_rows) and fgp_post_mean (k_post_mean + k_sum_chunks; the kernel rows + GEMM form of
    ops.post_mean_matfree for >= 8 outputs of one kernel): every D, the folded B4 instance and its two fall-backs
    (a == 0, |a| outside [2^-120, 2^120]), ORD = 0 with uniform and mixed orders, net orders 1..4 at t = 32 and 63,
    B = 1..4 with dead lanes, g = b mod Gk, the block launch of B > 4, n and N off the slab and tile sizes, both chunk
    sizes, a coefficient stride larger than n, test points at 0, at 1 and on a training point;
  * fgp_post_mean_batched: 3 problems, shared and own test points;
  * fgp_post_var_qf and fgp_post_var_batched (k_qf_rows / k_qf_cols, k_qf_rows_r2c / k_qf_cols_r2c, k_qf_finish):
    full length (m = 13, 16; m = 17 with FGP_R2C=0), half length (m = 17), nets, unit / uniform / 1/ev weights,
    regenerated lattice points, the variance clamped and not.

Tolerance, derived and not measured: |device - reference| <= C 2^-53 B_q per output, B_q the reference's first-order
bound, C the count of the kernel's roundings (predict_cases: c_rows, c_mean, c_batched, c_quadform, c_var).  The caps
that keep this from being vacuous (1e-11 |q| per output of a regular case) are asserted on the arrays used, here and in
tests/test_predict_reference_cpu.py.  Every call is made twice and must repeat bit for bit.  The worst observed
|device - reference| / (2^-53 B_q) per variant is printed (-s) and tabulated in DESIGN.md section 3.3.
"""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from tests import predict_cases as PC
from tests import predict_reference as PR
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

U = PR.EPS53
WORST = {}          # variant -> (worst err / (2^-53 B_q), C)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(variant, name, what, dev, ref, bnd, C, kind="regular"):
    dev = np.asarray(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    assert np.isfinite(dev).all(), (name, what, "not finite")
    q, B = np.abs(PR.to_f64(ref)), PR.to_f64(bnd)
    if kind == "regular":                               # the non-vacuity caps, on the arrays used
        assert (C * U * B <= 1e-11 * q).all(), (name, what, "cap")
    elif kind == "signed":
        assert B.max() <= 100 * q.max(), (name, what, "cap")
    ratio = float(PR.to_f64(abs(PR._x(dev) - ref) / (U * bnd)).max())
    w = WORST.get(variant, (0.0, 0))
    WORST[variant] = (max(w[0], ratio), max(w[1], C))
    print("%-58s %-12s err / (2^-53 B) = %8.2f   C = %d" % (name, what, ratio, C))
    assert ratio <= C, (name, what, ratio, C)


def _rm_variant(case):
    if case.fam == PC.LAT:
        if case.tiny or case.zero_ls:
            v = "lattice alpha 2, fold refused"
        elif set(case.alphas) == {2}:
            v = "lattice alpha 2 (folded B4)"
        else:
            v = "lattice ORD = 0"
    else:
        v = "net order 1" if set(case.alphas) == {1} else "net orders 1..4"
        if case.tbits == 63:
            v += ", t = 63"
    if case.kind == "signed":
        v += ", signed"
    return v


def _post_mean_direct(case, inp, xt, z, hyp):
    cf = _dev(inp["coeffs_full"])
    c = cf[:, :case.n]
    nchunks = (case.n + case.chunk - 1) // case.chunk
    work = torch.empty(nchunks * case.B * case.N, dtype=torch.float64, device=DEV)
    out = torch.full((case.B, case.N), float("nan"), dtype=torch.float64, device=DEV)
    N.call("fgp_post_mean", case.fam, N.ptr(xt), case.N, N.ptr(z), case.n, case.d, case.tbits, N.int_array(inp["order"]),
           N.double_array(inp["coef"]), N.ptr(hyp), case.Gk, N.ptr(c), cf.stride(0), case.B, N.ptr(out), case.N,
           N.ptr(work), case.chunk, N.stream_ptr(torch.device(DEV, torch.cuda.current_device())))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in PC.RM_CASES])
def test_rows_and_mean_match_extended_precision_reference(name):
    case = PC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = PC.rm_reference(name)
    xt, z, hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
    alphas = list(case.alphas)
    v = _rm_variant(case)

    def rows():
        return ops.kernel_rows(case.fam, xt, z, hyp, alphas=alphas, tbits=case.tbits).cpu().numpy()

    def pmean():
        if case.path == "ops":
            return ops.post_mean_matfree(case.fam, xt, z, hyp, _dev(inp["coeffs"]), alphas=alphas, tbits=case.tbits,
                                         chunk=case.chunk).cpu().numpy()
        return _post_mean_direct(case, inp, xt, z, hyp)

    r1 = rows()
    _check("k_kernel_rows, " + v, name, "rows", r1, K, BK, PC.c_rows(case), case.kind)
    assert np.array_equal(rows(), r1)
    m1 = pmean()
    gemm = case.path == "ops" and case.Gk == 1 and case.B >= 8
    _check(("kernel rows + GEMM, " if gemm else "k_post_mean, ") + v, name, "mean", m1, mean, Bm, PC.c_mean(case), case.kind)
    assert np.array_equal(pmean(), m1)


@pytest.mark.parametrize("name", [c.name for c in PC.BT_CASES])
def test_batched_mean_matches_extended_precision_reference(name):
    case = PC.BT_BY_NAME[name]
    inp, mean, Bm = PC.bt_reference(name)
    xt, z, hyp, co = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"]), _dev(inp["coeffs"])
    desc = N.PredDesc(family=case.fam, d=case.d, tbits=inp["tbits"], P=case.P, n=case.n, z=z.data_ptr(),
                      z_stride=case.d * case.n, hyp=hyp.data_ptr(), hyp_stride=hyp.stride(0), coeffs=co.data_ptr(),
                      coeff_stride=co.stride(0))
    for j in range(case.d):
        desc.order[j] = inp["order"][j]
        desc.coef[j] = inp["coef"][j]
    wl = ctypes.c_int64(0)
    N.call("fgp_post_mean_batched_work", desc, case.N, ctypes.byref(wl))

    def run():
        work = torch.empty(wl.value, dtype=torch.float64, device=DEV)
        out = torch.full((case.P, case.N), float("nan"), dtype=torch.float64, device=DEV)
        N.call("fgp_post_mean_batched", desc, N.ptr(xt), case.N * case.d if case.own_xt else 0, case.N, N.ptr(out),
               N.ptr(work), N.stream_ptr(torch.device(DEV, torch.cuda.current_device())))
        return out.cpu().numpy()

    o1 = run()
    fam = "lattice alpha 2 (folded B4)" if case.fam == PC.LAT else "net order 1"
    _check("fgp_post_mean_batched, " + fam, name, "mean", o1, mean, Bm, PC.c_batched(case))
    assert np.array_equal(run(), o1)


def _qf_variant(case, r2c):
    if case.fam == PC.NET:
        return "k_qf_rows / k_qf_cols, net " + ("order 1" if set(case.alphas) == {1} else "orders 1..4")
    if r2c:
        return "k_qf_rows_r2c / k_qf_cols_r2c, ORD = %d" % (4 if set(case.alphas) == {2} else 0)
    return "k_qf_rows / k_qf_cols, lattice"


def _var_batched(case, inp, wa2, z, gen):
    """fgp_post_var_batched of the QF_P problems: [P, N]."""
    n = 1 << case.m
    xt, hyp, wa = _dev(inp["xt"]), _dev(inp["hyp"]), _dev(wa2)
    desc = N.PredDesc(family=case.fam, d=case.d, tbits=case.tbits, P=PC.QF_P, n=n, z=z.data_ptr() if z is not None else 0,
                      z_stride=0, hyp=hyp.data_ptr(), hyp_stride=hyp.stride(0), wa=wa.data_ptr(), wa_stride=wa.stride(0))
    for j in range(case.d):
        desc.order[j] = inp["order"][j]
        desc.coef[j] = inp["coef"][j]
    keep = None
    if gen is not None:
        zg, sh = gen
        keep = _dev(sh)
        desc.points_gen = N.PARTS_LATTICE
        for j in range(case.d):
            desc.gen_z[j] = zg[j]
        desc.gen_shift = keep.data_ptr()
        desc.gen_shift_stride = case.d
    cdt = torch.complex128 if case.fam == PC.LAT else torch.float64
    work = torch.empty((PC.QF_P, PC.QF_N, n), dtype=cdt, device=DEV)
    partial = torch.empty((PC.QF_P, PC.QF_N, n >> 12), dtype=torch.float64, device=DEV)
    out = torch.full((PC.QF_P, PC.QF_N), float("nan"), dtype=torch.float64, device=DEV)
    N.call("fgp_post_var_batched", desc, N.ptr(xt), 0, PC.QF_N, N.double_array(inp["part0"]), N.ptr(out), N.ptr(work),
           N.ptr(partial), N.stream_ptr(torch.device(DEV, torch.cuda.current_device())))
    return out.cpu().numpy()


def _check_var(case, name, variant, inp, rows, Br, power, z, gen, what):
    """Problem 0 with the 1/ev weights scaled so that no variance is clamped, problem 1 with the uniform weights
    scaled so that every one is (a test point on a training point among them)."""
    k0 = PR.kxx(inp["hyp"], inp["part0"])
    wa2, ref, bnd = [], [], []
    for p, (kind, clamp) in enumerate((("gp", False), ("unif", True))):
        q, _ = PR.quadform(case.fam, rows[p], Br[p], inp["wa"][kind], power=power[p])
        w = inp["wa"][kind] * PC.var_weights(k0[p], q, clamp)
        q, Bq = PR.quadform(case.fam, rows[p], Br[p], w, power=power[p])
        v, Bv = PR.post_var(k0[p], q, Bq)
        assert (PR.to_f64(v) == 0).all() if clamp else (PR.to_f64(v) > 0.2 * float(k0[p])).all()
        wa2.append(w)
        ref.append(v)
        bnd.append(Bv)
    wa2 = np.stack(wa2)
    o1 = _var_batched(case, inp, wa2, z, gen)
    _check("k_qf_finish after " + variant, name, what, o1, np.stack(ref), np.stack(bnd), PC.c_var(case), kind=None)
    assert (o1[1] == 0).all() and (o1[0] > 0).all()
    assert np.array_equal(_var_batched(case, inp, wa2, z, gen), o1)


@pytest.mark.parametrize("name", [c.name for c in PC.QF_CASES])
def test_quadratic_form_and_variance_match_extended_precision_reference(name, monkeypatch):
    case = PC.QF_BY_NAME[name]
    if case.r2c is None:
        monkeypatch.delenv("FGP_R2C", raising=False)
    else:
        monkeypatch.setenv("FGP_R2C", case.r2c)
    r2c = case.fam == PC.LAT and case.m >= 17 and case.r2c is None
    variant = _qf_variant(case, r2c)
    inp = PC.qf_inputs(case)
    rows, Br, power = PC.qf_reference(case, inp)
    xt, z, hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
    alphas = list(case.alphas)
    C = PC.c_quadform(case)
    for kind in PC.WA_KINDS:
        wa = _dev(inp["wa"][kind])
        q, Bq = PR.quadform(case.fam, rows[0], Br[0], inp["wa"][kind], power=power[0])
        o1 = ops.post_var_quadform(case.fam, xt, z, hyp[0], wa, alphas=alphas, tbits=case.tbits).cpu().numpy()
        _check(variant, name, "qf wa=" + kind, o1, q, Bq, C)
        o2 = ops.post_var_quadform(case.fam, xt, z, hyp[0], wa, alphas=alphas, tbits=case.tbits).cpu().numpy()
        assert np.array_equal(o1, o2)
        if kind == "one":                                # Parseval: ||r||^2
            r2 = (rows[0] * rows[0]).sum(-1)
            assert PR.to_f64(abs(q - r2) / r2).max() <= 1e-17
    _check_var(case, name, variant, inp, rows, Br, power, z, None, "var")


@pytest.mark.parametrize("name", [c.name for c in PC.QF_CASES if c.fam == PC.LAT and c.r2c is None and c.m != 16])
def test_variance_with_regenerated_lattice_points(name, monkeypatch):
    """fgp_post_var_batched with points_gen = FGP_PARTS_LATTICE and z = NULL against the reference at the points
    ops.lattice_points materialises (each problem its own shift)."""
    monkeypatch.delenv("FGP_R2C", raising=False)
    case = PC.QF_BY_NAME[name]
    n = 1 << case.m
    zg, sh = PC.qf_gen(case)
    pts = np.stack([ops.lattice_points(zg, torch.from_numpy(sh[p]).to(DEV), 0, n).cpu().numpy() for p in range(PC.QF_P)])
    assert np.array_equal(pts, PC.qf_gen_points_cpu(case))
    inp = PC.qf_inputs(case, pts)
    rows, Br, power = PC.qf_reference(case, inp, regenerated=True)
    variant = _qf_variant(case, case.m >= 17) + ", regenerated points"
    _check_var(case, name, variant, inp, rows, Br, power, None, (zg, sh), "var gen")


def test_zz_worst_ratio_per_variant():
    """The table of DESIGN.md section 3.3: worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %d | %.2f |" % (v, WORST[v][1], WORST[v][0]))
