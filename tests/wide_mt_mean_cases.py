"""The case matrix of fgp_mt_wide_post_mean (csrc/fgp_wide_mt.hip: tests/test_gpu_wide_mt_mean_exact.py on the device,
tests/test_wide_mt_mean_cpu.py without one), the inputs of every case and the derived factor C of
|device - reference| <= C 2^-53 B_q (tests/wide_mt_mean_reference.py).  The conventions of tests/wide_mt_cases.py:
'regular' cases have every term of every sum positive (lengthscales in [0.02, 0.25], coefficients in [0.1, 1.1]; with
ind = 0 somewhere one pair only), 'signed' cases are wide_mt_cases' signed kind -- factors of either sign and exactly 0,
weights cc of either sign (cancellation over p) -- with coefficients 1 + randn / 4.

Every case: coeffs is a view of rows of n + pad values (pad = 3 unless the case says 0: a padded coeff_stride), test point
2 mod N is training point 5 (distance 0) where N > 2 and n > 5, w is signed (w[b] = (-1)^b (0.5 + rand)) or NULL, and with
beta = 1 the output holds out0 = sign(w[b]) rand |w[b]| sum_i |K_i c_i| / 2 (non-zero, of the sum's sign in regular cases:
no cancellation against it, and its addition is within the one unit of B_q that C counts for it).

C, the worst-case linear count of roundings on the way of one term into an output, in units of 2^-53 B_q:

  a term K_i               wide_mt_cases.c_rows: c_parts + 5 (the bits fgp_wide_mt_rows writes)
  sum = fma(K_i, c_i, sum) 1 for the product inside the fma, and
  the thread's chain       L = ceil(min(chunk, n) / 256) additions (a thread adds every 256th point of its chunk)
  block_sum                9: the wave tree 6, the 4 waves in order 3
  the chunks               ceil(nchunks / 256) (a lane adds every 256th chunk) + block_sum 9
  w, beta                  2

  C = c_rows + 1 + L + 9 + ceil(nchunks / 256) + 9 + 2        (39 for a lattice case with n = 257 and the default chunk)

Non-vacuity: regular cases satisfy C 2^-53 B_q <= wide_cases.CAP |q| (asserted on the arrays used, on the CPU and again
on the device); signed cases max B_q <= 8 d max |q| -- wide_mt_cases' cap 4 d of one kernel value, and a factor 2 for
the n = 33 terms of either sign that the sum over the training points cancels in part (on the reference alone: at
most 5.2 d).
"""
import collections
import functools

import numpy as np

from tests import predict_cases as PC
from tests import predict_reference as PR
from tests import wide_cases as WC
from tests import wide_mt_cases as MC
from tests import wide_mt_mean_reference as MMR
from tests import wide_mt_reference as MR

LAT, NET = MC.LAT, MC.NET
CAP = WC.CAP
KWG = 256                       # threads of a workgroup: the stride of a thread's chain and the smallest chunk accepted
DEFAULT_CHUNK = 1024

PM = collections.namedtuple("PM", "name fam d P B Gk N n chunk orders tbits pattern kind w beta pad zero_row seed")


def _pm(fam, d=9, P=3, B=3, Gk=None, N=3, n=257, chunk=0, tbits=32, pattern="ones", kind="regular", w=True, beta=1, pad=3,
        zero_row=False, seed=0):
    Gk = B if Gk is None else Gk
    orders = MC.ALL_B if fam == LAT else MC.ALL_W
    name = "mtmean-%s-d%d-P%d-B%d-G%d-N%d-n%d-c%d-%s%s%s-w%d-beta%d-pad%d%s" % (
        "lat" if fam == LAT else "net", d, P, B, Gk, N, n, chunk, pattern, "-t%d" % tbits if fam == NET else "",
        "-signed" if kind == "signed" else "", int(w), beta, pad, "-zero" if zero_row else "")
    return PM(name, fam, d, P, B, Gk, N, n, chunk, tuple(orders), tbits if fam == NET else 0, pattern, kind, w, beta, pad,
              zero_row, seed)


CASES = []
for _fam in (LAT, NET):
    CASES += [_pm(_fam, d) for d in (9, 17, 64)]                                             # P = 3, B = Gk = 3, N = 3, n = 257
    CASES += [_pm(_fam, P=1), _pm(_fam, P=16), _pm(_fam, 64, P=16, n=65)]
    CASES += [_pm(_fam, n=1), _pm(_fam, n=255), _pm(_fam, n=1025), _pm(_fam, n=600, chunk=256)]   # 1, 1, 2 and 3 chunks
    CASES += [_pm(_fam, P=1, B=1, N=1, n=65793, chunk=256)]                                  # 258 chunks: the chunk sum wraps
    CASES += [_pm(_fam, N=1), _pm(_fam, N=257, n=33)]
    CASES += [_pm(_fam, B=1), _pm(_fam, B=3, Gk=1), _pm(_fam, B=5), _pm(_fam, B=5, Gk=1)]    # dead rows of a 4-block
    CASES += [_pm(_fam, w=False, beta=0), _pm(_fam, w=False, beta=1), _pm(_fam, w=True, beta=0, pad=0)]
    CASES += [_pm(_fam, zero_row=True), _pm(_fam, zero_row=True, beta=0, Gk=1)]
    CASES += [_pm(_fam, d, n=33, pattern="mixed", kind="signed") for d in (13, 64)]
CASES += [_pm(NET, 17, tbits=63), _pm(NET, 17, tbits=63, n=33, pattern="mixed", kind="signed")]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def chunk_of(case):
    return case.chunk if case.chunk else DEFAULT_CHUNK


def nchunks_of(case):
    return (case.n + chunk_of(case) - 1) // chunk_of(case)


def work_len(case):
    return max(1, case.B * min(case.N, 65535) * nchunks_of(case))


def c_mean(case):
    L = (min(chunk_of(case), case.n) + KWG - 1) // KWG
    return MC.c_rows(case) + 1 + L + 9 + (nchunks_of(case) + KWG - 1) // KWG + 9 + 2


def inputs(case):
    """dict: xt [N, d], z [d, n], hyp [Gk, 1 + d], the spec tables, coeffs_full [B, n + pad] and its view coeffs [B, n],
    w [B] or None, and u [B, N] in (0, 1]: out0 = sign(w) u |w| sum |K c| / 2 is formed by reference()."""
    g = PC._rng(37, case.fam, case.d, case.P, case.B, case.Gk, case.N, case.n, case.chunk, case.tbits, len(case.pattern),
                int(case.w), case.beta, case.pad, int(case.zero_row), case.seed)
    signed = case.kind == "signed"
    assert signed or case.P == 1 or case.pattern == "ones"
    xt, z = PC._points(g, case.fam, case.d, case.n, case.N, case.tbits)
    hyp = PC._hyp(g, case.Gk, case.d, case.kind)
    order, coef, add, ind, cc = MC.spec_tables(case.fam, case.d, case.P, case.orders, case.pattern, g, signed)
    shape = (case.B, case.n + case.pad)
    full = 1.0 + 0.25 * g.standard_normal(shape) if signed else 0.1 + g.random(shape)
    if case.zero_row:
        full[1, :] = 0.0
    w = (0.5 + g.random(case.B)) * np.where(np.arange(case.B) % 2 == 1, -1.0, 1.0) if case.w else None
    u = 1.0 - g.random((case.B, case.N))
    return dict(xt=xt, z=z, hyp=hyp, order=order, coef=coef, add=add, ind=ind, cc=cc, coeffs_full=full,
                coeffs=full[:, :case.n], w=w, u=u)


@functools.lru_cache(maxsize=2)
def reference(name):
    """(inputs with out0 [B, N] or None, q, B_q, K, B_K), computed once."""
    case = BY_NAME[name]
    inp = inputs(case)
    K, BK = MR.mt_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], inp["add"], inp["ind"],
                      inp["cc"], case.tbits)
    out0 = None
    if case.beta:
        _, mag = MMR.mt_post_mean(abs(K), 0 * BK, np.abs(inp["coeffs"]), None if inp["w"] is None else np.abs(inp["w"]))
        sign = 1.0 if inp["w"] is None else np.sign(inp["w"])[:, None]
        out0 = sign * inp["u"] * PR.to_f64(mag) * 0.5
        if case.zero_row:
            out0[1, :] = 0.5 * inp["u"][1]                     # (a zero row's sum is 0 exactly: out0 comes back as it is)
    inp["out0"] = out0
    q, Bq = MMR.mt_post_mean(K, BK, inp["coeffs"], inp["w"], out0)
    return inp, q, Bq, K, BK
