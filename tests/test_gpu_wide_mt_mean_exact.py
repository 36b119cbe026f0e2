"""fgp_mt_wide_post_mean (k_wmt_post_mean<FAM, 1 | 4, 1 | 4> + k_wmt_post_mean_sum, csrc/fgp_wide_mt.hip) against the
extended-precision reference (tests/wide_mt_mean_reference.py), as tests/test_gpu_wide_mt_exact.py has the kernel rows.

The entry point is called directly on the synthetic inputs of tests/wide_mt_mean_cases.py and every output is compared
with sum_i K_i c_i w (+ out0) evaluated in 80-bit arithmetic from the very arrays the kernel read:

  |device - reference| <= C 2^-53 B_q,   C = wide_mt_mean_cases.c_mean (derived from the summation order, not measured),

with the non-vacuity caps asserted on the arrays used.  d in {9, 13, 17, 64}, P in {1, 3, 16}, both families (Bernoulli
orders 1..8, Walsh orders 1..4 at t = 32 and 63), n in {1, 33, 65, 255, 257, 600, 1025, 65793 (258 chunks of 256)}, N in
{1, 3, 257}, B in {1, 3, 5} with Gk in {1, B}, w NULL and signed, beta 0 and 1 onto a non-zero out, a padded
coeff_stride, an all-zero coefficient row, a test point on a training point, the signed kind.  Outputs of beta = 0 calls
are pre-filled with NaN and must come back finite.  Beyond the bound:

  * a second run of the same call repeats bit for bit;
  * every test point predicted alone (N = 1) carries the bits it has among the others;
  * beta = 1 twice equals, within one rounding, the sum of two beta = 0 calls.

The worst observed |device - reference| / (2^-53 B_q) per variant is printed (-s) and tabulated in DESIGN.md section 3.5.
"""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import predict_reference as PR
from tests import wide_mt_mean_cases as MM
from tests.gpu_fixtures import DEV
from tests.test_wide_mt_mean_cpu import _ratio, cap_ok

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

U = PR.EPS53
WORST = {}          # variant -> (worst err / (2^-53 B_q), C)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return N.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _flat_i(t):
    return N.int_array([v for r in t for v in r])


def _flat_d(t):
    return N.double_array([v for r in t for v in r])


class _Call(object):
    """One case's device arrays and the call on them."""

    def __init__(self, case, inp):
        self.case = case
        self.xt, self.z, self.hyp = _dev(inp["xt"]), _dev(inp["z"]), _dev(inp["hyp"])
        self.full = _dev(inp["coeffs_full"])
        assert self.full.stride(0) == case.n + case.pad
        self.w = _dev(inp["w"]) if inp["w"] is not None else None
        self.out0 = _dev(inp["out0"]) if inp["out0"] is not None else None
        self.tables = (_flat_i(inp["order"]), _flat_d(inp["coef"]), _flat_d(inp["add"]), _flat_i(inp["ind"]),
                       N.double_array(inp["cc"]))

    def run(self, t0=0, t1=None, beta=None, coeffs_full=None, out=None):
        """The call on test points t0 .. t1 - 1 -> [B, t1 - t0] (numpy); out: accumulate onto this device array."""
        case = self.case
        t1 = case.N if t1 is None else t1
        Nt = t1 - t0
        beta = case.beta if beta is None else beta
        full = self.full if coeffs_full is None else coeffs_full
        if out is None:
            out = self.out0[:, t0:t1].clone() if beta else torch.full((case.B, Nt), float("nan"), device=DEV)
        assert out.is_contiguous()
        wlen = ctypes.c_int64(0)
        N.call("fgp_mt_wide_post_mean_work", Nt, case.n, case.B, case.chunk, ctypes.byref(wlen))
        work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
        order, coef, add, ind, cc = self.tables
        N.call("fgp_mt_wide_post_mean", case.fam, N.ptr(self.xt[t0:t1]), Nt, N.ptr(self.z), case.n, case.d, case.P, order,
               coef, add, ind, cc, case.tbits, N.ptr(self.hyp), case.Gk, N.ptr(full), full.stride(0), case.B, N.ptr(self.w),
               beta, N.ptr(out), Nt, N.ptr(work), case.chunk, _stream())
        return out.cpu().numpy()


def _variant(case):
    fam = "lattice" if case.fam == MM.LAT else "net, t = %d" % case.tbits
    nk, nb = (1 if case.Gk == 1 else 4), (1 if case.B == 1 else 4)
    return "k_wmt_post_mean<%d, %d>, %s%s" % (nk, nb, fam, ", signed" if case.kind == "signed" else "")


@pytest.mark.parametrize("name", [c.name for c in MM.CASES])
def test_mt_wide_post_mean_matches_extended_precision_reference(name):
    case = MM.BY_NAME[name]
    inp, q, Bq, K, BK = MM.reference(name)
    assert cap_ok(case, q, Bq), (name, "cap")
    call = _Call(case, inp)
    dev = call.run()
    assert dev.shape == q.shape and np.isfinite(dev).all(), (name, "not finite")
    C = MM.c_mean(case)
    ratio = _ratio(dev, q, Bq)
    v = _variant(case)
    w = WORST.get(v, (0.0, 0))
    WORST[v] = (max(w[0], ratio), max(w[1], C))
    print("%-70s err / (2^-53 B) = %8.2f   C = %d" % (name, ratio, C))
    assert ratio <= C, (name, ratio, C)
    assert np.array_equal(call.run(), dev), "a second run of the same call"
    # a test point predicted alone carries the bits it has among the others (all of them; 257: every 16th and the last)
    for t in sorted(set(range(0, case.N, 1 if case.N <= 3 else 16)) | {case.N - 1}):
        assert np.array_equal(call.run(t, t + 1), dev[:, t:t + 1]), (name, "alone", t)


@pytest.mark.parametrize("name", [MM.CASES[0].name, [c.name for c in MM.CASES if c.fam == MM.NET and c.B == 5 and c.Gk == 1][0]])
def test_accumulating_twice_is_the_sum_of_two_calls(name):
    """beta = 1 with coefficients c1, then again with c2, onto out = 0: the first leaves v1 exactly, the second one
    rounding of v1 + v2, where v1 and v2 are what two beta = 0 calls give."""
    case = MM.BY_NAME[name]
    inp = MM.reference(name)[0]
    call = _Call(case, inp)
    full2 = (0.5 * call.full + 0.25).contiguous()
    v1, v2 = call.run(beta=0), call.run(beta=0, coeffs_full=full2)
    out = torch.zeros((case.B, case.N), device=DEV)
    first = call.run(beta=1, out=out)
    assert np.array_equal(first, v1)
    both = call.run(beta=1, coeffs_full=full2, out=out)
    exact = PR._x(v1) + PR._x(v2)
    assert (abs(PR._x(both) - exact) <= U * abs(exact)).all()
    assert np.array_equal(out.cpu().numpy(), both)


def test_zz_worst_ratio_per_variant():
    """The table of DESIGN.md section 3.5: worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %d | %.2f |" % (v, WORST[v][1], WORST[v][0]))
