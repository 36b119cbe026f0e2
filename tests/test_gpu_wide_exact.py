"""The wide kernels (9 <= d <= 64: csrc/fgp_wide.hip and k_wide_qf_rows of csrc/fgp_predict.hip) against the
extended-precision reference (tests/predict_reference.py), as tests/test_gpu_predict_exact.py has the d <= 8 ones.

The entry points are called directly on the synthetic inputs of tests/wide_cases.py and every output is compared with
the operation's definition evaluated in 80-bit arithmetic from the very arrays the kernel read:

  * fgp_wide_kernel_rows (k_wide_rows<FAM, 1 | 4>; and the kernel rows + GEMM mean of ops.post_mean_matfree for 8
    outputs of one kernel): d in {9, 16, 17, 33, 63, 64}, every alpha, mixed orders, a == 0, nets of order 1 and 1..4 at
    t = 32 and 63, n from 1 to 8225, N about the 256-thread tile, Gk in {1..5, 8, 10} (dead rows, several row blocks),
    signed factors, and lengthscales from 1e-60 to 2000 (kernel values of 1e200 at d = 64);
  * fgp_wide_post_var_qf (k_wide_qf_rows<9..12, T, 0 | 4> + k_qf_cols): 2 problems, stacked and with z and xt shared,
    m = 13..17, unit / uniform / 1/ev weights;
  * fgp_wide_k1 (k_wide_k1<1 | 4>) and fgp_wide_k1_bwd (k_wide_k1_bwd<2..8> + k_wide_k1_bwd_sum, 258 blocks for its
    second level), fgp_wide_lattice_parts and fgp_wide_net_parts.

Tolerance, derived and not measured: |device - reference| <= C 2^-53 B_q per output (wide_cases: c_rows, c_mean,
c_quadform, c_parts, c_k1, c_k1_bwd_scale, c_k1_bwd_ls).  The caps that keep it from being vacuous are asserted on the
arrays used, here and in tests/test_wide_reference_cpu.py.  Outputs are pre-filled with NaN and must come back finite;
every call is made twice and must repeat bit for bit.  The worst observed |device - reference| / (2^-53 B_q) per variant is
printed (-s) and tabulated in DESIGN.md section 3.5.

Not compared here: fgp_wide_post_mean (k_wide_post_mean + k_wide_sum).  Its cases, reference, count c_mean and caps
are in tests/wide_cases.py and are asserted without a device by tests/test_wide_reference_cpu.py; DESIGN.md section 8
says what is open there.
"""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from tests import predict_cases as PC
from tests import predict_reference as PR
from tests import wide_cases as WC
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

U = PR.EPS53
WORST = {}          # variant -> (worst err / (2^-53 B_q), C)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return N.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _check(variant, name, what, dev, ref, bnd, C, kind="regular", d=0, cap=WC.CAP):
    dev = np.asarray(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    assert np.isfinite(dev).all(), (name, what, "not finite")
    q, B = np.abs(PR.to_f64(ref)), PR.to_f64(bnd)
    if kind == "regular":                               # the non-vacuity caps, on the arrays used
        assert (C * U * B <= cap * q).all(), (name, what, "cap")
    elif kind == "signed":
        assert B.max() <= 4 * d * q.max(), (name, what, "cap")
    elif kind == "parts":
        assert WC.parts_cap_ok(C, ref, bnd).all(), (name, what, "cap")
    ratio = float(PR.to_f64(abs(PR._x(dev) - ref) / (U * bnd)).max())
    w = WORST.get(variant, (0.0, 0))
    WORST[variant] = (max(w[0], ratio), max(w[1], C))
    print("%-58s %-12s err / (2^-53 B) = %8.2f   C = %d" % (name, what, ratio, C))
    assert ratio <= C, (name, what, ratio, C)


def _rm_variant(case):
    if case.fam == PC.LAT:
        if case.ls is not None:
            v = "lattice alpha 2, lengthscales " + case.ls
        elif case.zero_ls:
            v = "lattice alpha 2, fold refused (a = 0)"
        elif set(case.alphas) == {2}:
            v = "lattice alpha 2 (folded B4)"
        else:
            v = "lattice ORD = 0"
    else:
        v = "net order 1" if set(case.alphas) == {1} else "net orders 1..4"
        if case.tbits == 63:
            v += ", t = 63"
    if case.kind == "signed" and case.ls is None:
        v += ", signed"
    return v


def _rows_direct(case, inp, xt, z, hyp):
    rows = _nan(case.Gk, case.N, case.n)
    N.call("fgp_wide_kernel_rows", case.fam, N.ptr(xt), case.N, N.ptr(z), case.n, case.d, case.tbits,
           N.int_array(inp["order"]), N.double_array(inp["coef"]), N.ptr(hyp), case.Gk, N.ptr(rows), _stream())
    return rows.cpu().numpy()


def _rows_cases():
    """The cases of the rows-and-mean matrix whose rows differ (chunk, B and the coefficients belong to the mean)."""
    seen, out = set(), []
    for c in WC.RM_CASES:
        key = (c.fam, c.d, c.n, c.N, c.Gk, c.alphas, c.tbits, c.kind, c.zero_ls, c.ls, c.path)
        if key not in seen:
            seen.add(key)
            out.append(c.name)
    return out


@pytest.mark.parametrize("name", _rows_cases())
def test_wide_rows_match_extended_precision_reference(name):
    case = WC.RM_BY_NAME[name]
    inp, K, BK, mean, Bm = WC.rm_reference(name)
    xt, z, hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
    v = _rm_variant(case)
    r1 = _rows_direct(case, inp, xt, z, hyp)
    _check("k_wide_rows, " + v, name, "rows", r1, K, BK, WC.c_rows(case), case.kind, case.d)
    assert np.array_equal(_rows_direct(case, inp, xt, z, hyp), r1)
    if case.path == "ops":                               # 8 outputs of one kernel: kernel rows + GEMM
        assert case.Gk == 1 and case.B >= ops.GEMM_MIN_OUTPUTS

        def pmean():
            return ops.post_mean_matfree(case.fam, xt, z, hyp, _dev(inp["coeffs"]), alphas=list(case.alphas),
                                         tbits=case.tbits, chunk=case.chunk).cpu().numpy()

        m1 = pmean()
        _check("wide kernel rows + GEMM, " + v, name, "mean", m1, mean, Bm, WC.c_mean(case), case.kind, case.d)
        assert np.array_equal(pmean(), m1)


def _qf_variant(case):
    if case.fam == PC.NET:
        return "k_wide_qf_rows / k_qf_cols, net " + ("order 1" if set(case.alphas) == {1} else "orders 1..4")
    return "k_wide_qf_rows / k_qf_cols, lattice ORD = %d" % (4 if set(case.alphas) == {2} else 0)


def _qf_direct(case, inp, xt, z, hyp, wa):
    """fgp_wide_post_var_qf of QF_P problems: [P, N]; xt [P, N, d] or [N, d], z [P, d, n] or [d, n] (shared)."""
    n = 1 << case.m
    P, Nt, d = WC.QF_P, WC.QF_N, case.d
    cdt = torch.complex128 if case.fam == PC.LAT else torch.float64
    work = torch.empty((P, Nt, n), dtype=cdt, device=DEV)
    partial = torch.empty((P, Nt, n >> 12), dtype=torch.float64, device=DEV)
    out = _nan(P, Nt)
    N.call("fgp_wide_post_var_qf", case.fam, N.ptr(xt), Nt * d if xt.dim() == 3 else 0, Nt, N.ptr(z),
           d * n if z.dim() == 3 else 0, case.m, d, case.tbits, N.int_array(inp["order"]), N.double_array(inp["coef"]),
           N.ptr(hyp), 1 + d, N.ptr(wa), n, P, N.ptr(work), N.ptr(partial), N.ptr(out), _stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in WC.QF_CASES])
def test_wide_quadratic_form_matches_extended_precision_reference(name):
    case = WC.QF_BY_NAME[name]
    inp, runs = WC.qf_reference(name)
    variant = _qf_variant(case)
    C = WC.c_quadform(case)
    hyp = _dev(inp["hyp"])
    xt_all, z_all = _dev(inp["xt"]), _dev(inp["z"])
    for run in WC.QF_RUNS:
        rows, Br, power = runs[run]
        xt, z = (xt_all, z_all) if run == "stacked" else (xt_all[0].contiguous(), z_all[0].contiguous())
        for kind in WC.WA_KINDS:
            wa = _dev(inp["wa"][kind])
            ref = [PR.quadform(case.fam, rows[p], Br[p], inp["wa"][kind][p], power=power[p]) for p in range(WC.QF_P)]
            q, Bq = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
            o1 = _qf_direct(case, inp, xt, z, hyp, wa)
            _check(variant, name, "qf %s wa=%s" % (run, kind), o1, q, Bq, C, cap=WC.CAP_QF)
            assert np.array_equal(_qf_direct(case, inp, xt, z, hyp, wa), o1)
            if kind == "one":                            # Parseval: ||r||^2 (problem 1: twice)
                r2 = (rows[0] * rows[0]).sum(-1)
                assert PR.to_f64(abs(q[0] - r2) / r2).max() <= 1e-17


def _k1_direct(case, parts, scale, ls):
    k1 = _nan(case.G, case.n)
    N.call("fgp_wide_k1", N.ptr(parts), case.n, case.d, N.ptr(scale), N.ptr(ls), case.G, N.ptr(k1), _stream())
    return k1.cpu().numpy()


def _k1_bwd_direct(case, parts, scale, ls, u):
    wlen = ctypes.c_int64(0)
    N.call("fgp_wide_k1_bwd_work", case.n, case.d, case.G, ctypes.byref(wlen))
    assert wlen.value == case.G * (1 + case.d) * ((case.n + 255) // 256)
    work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
    ds, dl = _nan(case.G), _nan(case.G, case.d)
    N.call("fgp_wide_k1_bwd", N.ptr(parts), case.n, case.d, N.ptr(scale), N.ptr(ls), case.G, N.ptr(u), N.ptr(ds), N.ptr(dl),
           N.ptr(work), _stream())
    return ds.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in WC.K1_CASES])
def test_wide_first_column_matches_extended_precision_reference(name):
    case = WC.K1_BY_NAME[name]
    inp, k, Bk, ds, Bs, dl, Bl = WC.k1_reference(name)
    parts, scale, ls, u = (_dev(inp[key]) for key in ("parts", "scale", "ls", "u"))
    sg = ", signed" if case.kind == "signed" else ""
    k1 = _k1_direct(case, parts, scale, ls)
    _check("k_wide_k1<%d>%s" % (1 if case.G == 1 else 4, sg), name, "k1", k1, k, Bk, WC.c_k1(case), case.kind, case.d)
    assert np.array_equal(_k1_direct(case, parts, scale, ls), k1)
    s1, l1 = _k1_bwd_direct(case, parts, scale, ls, u)
    v = "k_wide_k1_bwd<%d>%s" % ((case.d + 7) // 8, sg)
    _check(v + ", dscale", name, "dscale", s1, ds, Bs, WC.c_k1_bwd_scale(case), case.kind, case.d)
    _check(v + ", dls", name, "dls", l1, dl, Bl, WC.c_k1_bwd_ls(case), case.kind, case.d)
    s2, l2 = _k1_bwd_direct(case, parts, scale, ls, u)
    assert np.array_equal(s2, s1) and np.array_equal(l2, l1)


@pytest.mark.parametrize("name", [c.name for c in WC.PT_CASES])
def test_wide_parts_match_extended_precision_reference(name):
    case = WC.PT_BY_NAME[name]
    inp, P, B = WC.parts_reference(name)
    full, z = _dev(inp["x_full"]), _dev(inp["z"])
    assert full.stride(0) == case.d + 3

    def run():
        out = _nan(case.d, case.n)
        if case.fam == PC.LAT:
            N.call("fgp_wide_lattice_parts", N.ptr(full), full.stride(0), N.ptr(z), case.n, case.d, N.int_array(inp["order"]),
                   N.double_array(inp["coef"]), N.ptr(out), _stream())
        else:
            N.call("fgp_wide_net_parts", N.ptr(full), full.stride(0), N.ptr(z), case.n, case.d, case.tbits,
                   N.int_array(inp["order"]), N.ptr(out), _stream())
        return out.cpu().numpy()

    o1 = run()
    if case.fam == PC.LAT:
        v = "k_wide_lattice_parts"
    else:
        v = "k_wide_net_parts, " + ("order %d" % case.orders[0] if len(set(case.orders)) == 1 else "orders 1..4") + \
            (", t = 63" if case.tbits == 63 else "")
    _check(v, name, "parts", o1, P, B, WC.c_parts(case), "parts")
    assert np.array_equal(run(), o1)


def test_zz_worst_ratio_per_variant():
    """The table of DESIGN.md section 3.5: worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %d | %.2f |" % (v, WORST[v][1], WORST[v][0]))
