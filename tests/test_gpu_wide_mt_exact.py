"""The wide multitask kernels (csrc/fgp_wide_mt.hip) against the extended-precision reference
(tests/wide_mt_reference.py), as tests/test_gpu_wide_exact.py has the single-task wide ones.

The four entry points are called directly on the synthetic inputs of tests/wide_mt_cases.py and every output is
compared with the operation's definition evaluated in 80-bit arithmetic from the very arrays the kernel read:

  * fgp_wide_mt_k1 (k_wmt_k1<1 | 4>) and fgp_wide_mt_k1_bwd (k_wmt_k1_bwd<2..8> + k_wmt_k1_bwd_sum; 258 blocks for
    its second level): d in {9, 16, 17, 24, 25, 33, 41, 49, 57, 63, 64}, n in {1, 255, 257, 8225, 66048}, P in {1, 3, 16},
    G in {1, 4, 5, 8}, ind = 0 in one, several and all-but-one dimensions, factors exactly 0 and negative factors;
  * fgp_wide_mt_rows (k_wmt_rows / k_wmt_rows_zip<FAM, 1 | 4>): both families, Bernoulli orders 1..8, Walsh orders
    1..4 at t = 32 and 63, zipped pairs with N about the 256-thread tile;
  * fgp_wide_mt_parts (k_wmt_parts): all pairs, one z, zipped pairs; rows of x with a stride.

Tolerance, derived and not measured: |device - reference| <= C 2^-53 B_q per output (wide_mt_cases: c_k1,
c_k1_bwd_scale, c_k1_bwd_ls, c_rows, c_parts).  The caps that keep it from being vacuous are asserted on the arrays
used, here and in tests/test_wide_mt_reference_cpu.py.  Outputs are pre-filled with NaN and must come back finite; every
call is made twice and must repeat bit for bit.  The worst observed |device - reference| / (2^-53 B_q) per variant is printed
(-s) and tabulated in DESIGN.md section 3.5.
"""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import predict_reference as PR
from tests import wide_cases as WC
from tests import wide_mt_cases as MC
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


def _flat_i(t):
    return N.int_array([v for r in t for v in r])


def _flat_d(t):
    return N.double_array([v for r in t for v in r])


def _check(variant, name, what, dev, ref, bnd, C, kind="regular", d=0):
    dev = np.asarray(dev)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    assert np.isfinite(dev).all(), (name, what, "not finite")
    q, B = np.abs(PR.to_f64(ref)), PR.to_f64(bnd)
    if kind == "regular":                               # the non-vacuity caps, on the arrays used
        assert (C * U * B <= MC.CAP * q).all(), (name, what, "cap")
    elif kind == "signed":
        assert B.max() <= 4 * d * q.max(), (name, what, "cap")
    elif kind == "parts":
        assert WC.parts_cap_ok(C, ref, bnd).all(), (name, what, "cap")
    err = abs(PR._x(dev) - ref)
    ratio = float(PR.to_f64(np.where(bnd > 0, err / np.where(bnd > 0, U * bnd, 1), np.where(err > 0, np.inf, 0))).max())
    w = WORST.get(variant, (0.0, 0))
    WORST[variant] = (max(w[0], ratio), max(w[1], C))
    print("%-58s %-8s err / (2^-53 B) = %8.2f   C = %d" % (name, what, ratio, C))
    assert ratio <= C, (name, what, ratio, C)


@pytest.mark.parametrize("name", [c.name for c in MC.K1_CASES])
def test_wide_mt_first_column_matches_extended_precision_reference(name):
    case = MC.K1_BY_NAME[name]
    inp, k, Bk, ds, Bs, dl, Bl = MC.k1_reference(name)
    parts, scale, ls, u = (_dev(inp[key]) for key in ("parts", "scale", "ls", "u"))
    ind, cc = _flat_i(inp["ind"]), N.double_array(inp["cc"])
    sg = ", signed" if case.kind == "signed" else ""

    def fwd():
        k1 = _nan(case.G, case.n)
        N.call("fgp_wide_mt_k1", N.ptr(parts), case.n, case.d, case.P, ind, cc, N.ptr(scale), N.ptr(ls), case.G, N.ptr(k1),
               _stream())
        return k1.cpu().numpy()

    def bwd():
        wlen = ctypes.c_int64(0)
        N.call("fgp_wide_mt_k1_bwd_work", case.n, case.d, case.P, case.G, ctypes.byref(wlen))
        assert wlen.value == case.G * (1 + case.d) * ((case.n + 255) // 256)
        work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
        s, l = _nan(case.G), _nan(case.G, case.d)
        N.call("fgp_wide_mt_k1_bwd", N.ptr(parts), case.n, case.d, case.P, ind, cc, N.ptr(scale), N.ptr(ls), case.G, N.ptr(u),
               N.ptr(s), N.ptr(l), N.ptr(work), _stream())
        return s.cpu().numpy(), l.cpu().numpy()

    k1 = fwd()
    _check("k_wmt_k1<%d>%s" % (1 if case.G == 1 else 4, sg), name, "k1", k1, k, Bk, MC.c_k1(case), case.kind, case.d)
    assert np.array_equal(fwd(), k1)
    s1, l1 = bwd()
    v = "k_wmt_k1_bwd<%d>%s" % ((case.d + 7) // 8, sg)
    _check(v + ", dscale", name, "dscale", s1, ds, Bs, MC.c_k1_bwd_scale(case), case.kind, case.d)
    _check(v + ", dls", name, "dls", l1, dl, Bl, MC.c_k1_bwd_ls(case), case.kind, case.d)
    s2, l2 = bwd()
    assert np.array_equal(s2, s1) and np.array_equal(l2, l1)


def _fam_tag(case):
    if case.fam == MC.LAT:
        return "lattice"
    return "net, t = %d" % case.tbits


@pytest.mark.parametrize("name", [c.name for c in MC.RW_CASES])
def test_wide_mt_rows_match_extended_precision_reference(name):
    case = MC.RW_BY_NAME[name]
    inp, K, B = MC.rows_reference(name)
    xt, z, hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
    order, coef, add, ind = _flat_i(inp["order"]), _flat_d(inp["coef"]), _flat_d(inp["add"]), _flat_i(inp["ind"])
    cc = N.double_array(inp["cc"])

    def run():
        rows = _nan(case.Gk, case.N) if case.zip else _nan(case.Gk, case.N, case.n)
        N.call("fgp_wide_mt_rows", case.fam, N.ptr(xt), case.N, N.ptr(z), case.n, int(case.zip), case.d, case.P, order, coef,
               add, ind, cc, case.tbits, N.ptr(hyp), case.Gk, N.ptr(rows), _stream())
        return rows.cpu().numpy()

    r1 = run()
    v = "k_wmt_rows%s<%d>, %s%s" % ("_zip" if case.zip else "", 1 if case.Gk == 1 else 4, _fam_tag(case),
                                    ", signed" if case.kind == "signed" else "")
    _check(v, name, "rows", r1, K, B, MC.c_rows(case), case.kind, case.d)
    assert np.array_equal(run(), r1)


@pytest.mark.parametrize("name", [c.name for c in MC.PT_CASES])
def test_wide_mt_parts_match_extended_precision_reference(name):
    case = MC.PT_BY_NAME[name]
    inp, P, B, C = MC.parts_reference(name)
    full, z = _dev(inp["x_full"]), _dev(inp["z"])
    assert full.stride(0) == case.d + 3
    order, coef, add = _flat_i(inp["order"]), _flat_d(inp["coef"]), _flat_d(inp["add"])
    E = case.N if case.zip else case.N * case.M

    def run():
        out = _nan(case.P, case.d, E)
        N.call("fgp_wide_mt_parts", case.fam, N.ptr(full), full.stride(0), case.N, N.ptr(z), case.d, case.M, int(case.zip),
               case.d, case.P, order, coef, add, case.tbits, N.ptr(out), _stream())
        return out.cpu().numpy()

    o1 = run()
    _check("k_wmt_parts, " + _fam_tag(case), name, "parts", o1, P, B, C, "parts")
    assert np.array_equal(run(), o1)


def test_zz_worst_ratio_per_variant():
    """The table of DESIGN.md section 3.5: worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %d | %.2f |" % (v, WORST[v][1], WORST[v][0]))
