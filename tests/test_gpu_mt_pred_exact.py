"""fgp_mt_rows (k_mt_rows / k_mt_rows_zip<FAM, D, 1 | 4>) and fgp_mt_post_mean (k_mt_post_mean<FAM, D, 1 | 4, 1 | 4> +
k_mt_post_mean_sum; csrc/fgp_mt_pred.hip) against the extended-precision references of the wide kernels, which are
d-agnostic (tests/wide_mt_reference.mt_rows, tests/wide_mt_mean_reference.mt_post_mean), as
tests/test_gpu_wide_mt_exact.py and tests/test_gpu_wide_mt_mean_exact.py have the 9 <= d <= 64 entry points.

The entry points are called directly on the synthetic inputs of tests/mt_pred_cases.py and every output is compared
with the definition evaluated in 80-bit arithmetic from the very arrays the kernel read:

  |device - reference| <= C 2^-53 B_q,   C = mt_pred_cases.c_rows / c_mean (derived for d <= 8, not measured),

with the non-vacuity caps asserted on the arrays used.  Rows: every D in 1..8 for both families, with P = 3 and with the
P == 1 instance; Bernoulli orders 1..8 and Walsh orders 1..4 at t = 32 and 63 one by one; n in {1, 255, 257, 8225} with
N = 3; Gk in {1, 4, 5, 8}; P in {1, 3, 16}; ind all ones, mixed and all but one; the signed kind; zipped pairs with N in
{1, 255, 257}; test points on a training point (point 5), at the origin and at 1 (training point 7).  Mean: every D, n
in {1, 1023, 1025}, 258 chunks of 256 (the second level of the chunk sum), B in {1, 3, 4, 5} with Gk in {1, B}, beta 0
and 1 onto a non-zero out, w NULL and signed, padded and tight strides, N = 0.  Outputs of calls that do not accumulate
are pre-filled with NaN and must come back finite.  Beyond the bound:

  * a second run of the same call repeats bit for bit;
  * every test point predicted alone (N = 1) carries the bits it has among the others, rows and mean;
  * the mean's kernel values are the rows' bits: the mean with one-hot coefficients returns the rows' entries exactly.

The worst observed |device - reference| / (2^-53 B_q) per variant is printed (-s).
"""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import mt_pred_cases as NC
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

WORST = {}          # variant -> (worst err / (2^-53 B_q), C)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return N.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _tables(inp):
    flat = lambda t: [v for r in t for v in r]
    return (N.int_array(flat(inp["order"])), N.double_array(flat(inp["coef"])), N.double_array(flat(inp["add"])),
            N.int_array(flat(inp["ind"])), N.double_array(inp["cc"]))


def _note(variant, name, ratio, C):
    w = WORST.get(variant, (0.0, 0))
    WORST[variant] = (max(w[0], ratio), max(w[1], C))
    print("%-72s err / (2^-53 B) = %8.2f   C = %d" % (name, ratio, C))


def _fam(case):
    return "lattice" if case.fam == NC.LAT else "net, t = %d" % case.tbits


# ------------------------------------------------------------------------------------------------ rows
class _Rows(object):
    def __init__(self, case, inp):
        self.case = case
        self.xt, self.z, self.hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
        self.tables = _tables(inp)

    def run(self, t0=0, t1=None):
        """Rows of test points t0 .. t1 - 1 -> [Gk, t1 - t0, n] (numpy); zip: all pairs -> [Gk, N]."""
        case = self.case
        order, coef, add, ind, cc = self.tables
        if case.zip:
            out = _nan(case.Gk, case.N)
            N.call("fgp_mt_rows", case.fam, N.ptr(self.xt), case.N, N.ptr(self.z), case.n, 1, case.d, case.P, order, coef,
                   add, ind, cc, case.tbits, N.ptr(self.hyp), case.Gk, N.ptr(out), _stream())
            return out.cpu().numpy()
        t1 = case.N if t1 is None else t1
        out = _nan(case.Gk, t1 - t0, case.n)
        N.call("fgp_mt_rows", case.fam, N.ptr(self.xt[t0:t1]), t1 - t0, N.ptr(self.z), case.n, 0, case.d, case.P, order,
               coef, add, ind, cc, case.tbits, N.ptr(self.hyp), case.Gk, N.ptr(out), _stream())
        return out.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in NC.RW_CASES])
def test_rows_match_extended_precision_reference(name):
    case = NC.RW_BY_NAME[name]
    inp, K, B = NC.rows_reference(name)
    C = NC.c_rows(case)
    assert NC.cap_ok(case.kind, C, K, B), (name, "cap")
    call = _Rows(case, inp)
    dev = call.run()
    assert dev.shape == K.shape and np.isfinite(dev).all(), (name, "not finite")
    r = NC.ratio(dev, K, B)
    _note("k_mt_rows%s<%d%s>, %s%s" % ("_zip" if case.zip else "", 1 if case.Gk == 1 else 4,
                                       ", P == 1" if case.P == 1 and not case.zip else "", _fam(case),
                                       ", signed" if case.kind == "signed" else ""), name, r, C)
    assert r <= C, (name, r, C)
    assert np.array_equal(call.run(), dev), "a second run of the same call"
    if not case.zip:
        for t in range(case.N):                               # a test point alone carries the bits it has among the others
            assert np.array_equal(call.run(t, t + 1), dev[:, t:t + 1]), (name, "alone", t)


def test_no_test_points_launch_nothing():
    """N = 0 is FGP_OK and writes nothing, rows and mean (the pointers are those of the N = 3 call: an empty tensor's
    is null, which the validation refuses first)."""
    case = NC.RW_CASES[0]
    call = _Rows(case, NC.rows_reference(case.name)[0])
    order, coef, add, ind, cc = call.tables
    out = _nan(case.Gk, case.N, case.n)
    N.call("fgp_mt_rows", case.fam, N.ptr(call.xt), 0, N.ptr(call.z), case.n, 0, case.d, case.P, order, coef, add, ind, cc,
           case.tbits, N.ptr(call.hyp), case.Gk, N.ptr(out), _stream())
    assert torch.isnan(out).all()
    case = NC.PM_CASES[0]
    call = _Mean(case, NC.mean_reference(case.name)[0])
    order, coef, add, ind, cc = call.tables
    out, work = _nan(case.B, case.N), _nan(8)
    N.call("fgp_mt_post_mean", case.fam, N.ptr(call.xt), 0, N.ptr(call.z), case.n, case.d, case.P, order, coef, add, ind,
           cc, case.tbits, N.ptr(call.hyp), case.Gk, N.ptr(call.full), call.full.stride(0), case.B, N.ptr(call.w), 1,
           N.ptr(out), case.N, N.ptr(work), case.chunk, _stream())
    assert torch.isnan(out).all() and torch.isnan(work).all()


# ------------------------------------------------------------------------------------------------ mean
class _Mean(object):
    """One case's device arrays and the call on them."""

    def __init__(self, case, inp):
        self.case = case
        self.xt, self.z, self.hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
        self.full = _dev(inp["coeffs_full"])
        assert self.full.stride(0) == case.n + case.pad
        self.w = _dev(inp["w"]) if inp["w"] is not None else None
        self.out0 = _dev(inp["out0"]) if inp["out0"] is not None else None
        self.tables = _tables(inp)

    def run(self, t0=0, t1=None, beta=None, coeffs_full=None, w="case", opad=0):
        """The call on test points t0 .. t1 - 1 -> [B, t1 - t0] (numpy); opad: extra elements per output row."""
        case = self.case
        t1 = case.N if t1 is None else t1
        Nt = t1 - t0
        beta = case.beta if beta is None else beta
        full = self.full if coeffs_full is None else coeffs_full
        w = self.w if isinstance(w, str) else w
        buf = _nan(case.B, Nt + opad)
        out = buf[:, :Nt]
        if beta:
            out.copy_(self.out0[:, t0:t1])
        wlen = ctypes.c_int64(0)
        N.call("fgp_mt_post_mean_work", Nt, case.n, case.B, case.chunk, ctypes.byref(wlen))
        work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
        order, coef, add, ind, cc = self.tables
        N.call("fgp_mt_post_mean", case.fam, N.ptr(self.xt[t0:t1]), Nt, N.ptr(self.z), case.n, case.d, case.P, order, coef,
               add, ind, cc, case.tbits, N.ptr(self.hyp), case.Gk, N.ptr(full), full.stride(0), case.B, N.ptr(w), beta,
               N.ptr(buf), Nt + opad, N.ptr(work), case.chunk, _stream())
        if opad:
            assert torch.isnan(buf[:, Nt:]).all(), "the padding of the output rows is not written"
        return out.cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in NC.PM_CASES])
def test_post_mean_matches_extended_precision_reference(name):
    case = NC.PM_BY_NAME[name]
    inp, q, Bq, K, BK = NC.mean_reference(name)
    C = NC.c_mean(case)
    assert NC.cap_ok(case.kind, C, q, Bq), (name, "cap")
    call = _Mean(case, inp)
    dev = call.run()
    assert dev.shape == q.shape and np.isfinite(dev).all(), (name, "not finite")
    r = NC.ratio(dev, q, Bq)
    _note("k_mt_post_mean<%d, %d%s>, %s%s" % (1 if case.Gk == 1 else 4, 1 if case.B == 1 else 4,
                                              ", P == 1" if case.P == 1 else "", _fam(case),
                                              ", signed" if case.kind == "signed" else ""), name, r, C)
    assert r <= C, (name, r, C)
    assert np.array_equal(call.run(), dev), "a second run of the same call"
    assert np.array_equal(call.run(opad=5), dev), "a padded out_stride"
    for t in range(case.N):                                   # a test point alone carries the bits it has among the others
        assert np.array_equal(call.run(t, t + 1), dev[:, t:t + 1]), (name, "alone", t)


@pytest.mark.parametrize("name", [c.name for c in NC.RW_CASES if not c.zip and c.n <= 257 and
                                  (c.kind == "signed" or c.P == 16 or c.Gk in (1, 5) or c.d in (1, 8))])
def test_the_mean_sums_the_bits_the_rows_write(name):
    """With coefficients that are 1 at training point i and 0 elsewhere, w NULL and beta = 0, the mean of row b is
    fma(K_i, 1, 0) plus zeros: rows[g(b)][t][i] bit for bit.  Both Gk == B (a kernel row per output row) and Gk == 1."""
    case = NC.RW_BY_NAME[name]
    inp = NC.rows_reference(name)[0]
    rows = _Rows(case, inp).run()                             # [Gk, N, n]
    pts = sorted({0, 5 % case.n, 7 % case.n, case.n // 2, case.n - 1})
    order, coef, add, ind, cc = _tables(inp)
    xt, z = _dev(inp["xt"]), _dev(inp["z"])
    for Gk in sorted({1, case.Gk}):
        B = case.Gk
        hyp = _dev(inp["hyp"][:Gk])
        for i in pts:
            coeffs = torch.zeros((B, case.n), device=DEV)
            coeffs[:, i] = 1.0
            out = _nan(B, case.N)
            wlen = ctypes.c_int64(0)
            N.call("fgp_mt_post_mean_work", case.N, case.n, B, 0, ctypes.byref(wlen))
            work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
            N.call("fgp_mt_post_mean", case.fam, N.ptr(xt), case.N, N.ptr(z), case.n, case.d, case.P, order, coef, add, ind,
                   cc, case.tbits, N.ptr(hyp), Gk, N.ptr(coeffs), case.n, B, None, 0, N.ptr(out), case.N, N.ptr(work), 0,
                   _stream())
            want = rows[:, :, i] if Gk == B else np.broadcast_to(rows[0, :, i], (B, case.N))
            got = out.cpu().numpy()
            assert np.array_equal(got == 0, want == 0) and np.array_equal(np.abs(got), np.abs(want)) and \
                np.array_equal(got[want != 0], want[want != 0]), (name, Gk, i)


def test_zz_worst_ratio_per_variant():
    """Worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %d | %.2f |" % (v, WORST[v][1], WORST[v][0]))
