"""The case matrix of the d <= 8 multitask prediction kernels (csrc/fgp_mt_pred.hip: fgp_mt_rows, fgp_mt_post_mean;
tests/test_gpu_mt_pred_exact.py on the device, tests/test_mt_pred_cpu.py without one) and the derived factors C of
|device - reference| <= C 2^-53 B_q.  The references are the d-agnostic ones of the wide kernels as they stand
(tests/wide_mt_reference.mt_rows, tests/wide_mt_mean_reference.mt_post_mean), the inputs come from the wide generators
(wide_mt_cases._rw / rows_inputs, wide_mt_mean_cases._pm / inputs) called with d <= 8; what is new here is the list of
cases and the rounding counts, which the wide ones may not lend: they rest on b_p >= d |prod_j f_pj| with d >= 9 and
P <= 16 < 2 d, so that the P + 1 roundings of the sum over p and the scale are 2 units of B_q.  At small d a rounding of
a term or of a partial sum over p is up to a full unit.

Rounding counts, in units of 2^-53 B_q (B_q of wide_mt_reference: bf = ind + |l| B_part per factor, b_p = sum_j bf_j
prod_{i != j} |f_i| >= d |prod_j f_pj| because bf_j >= |f_j|, B_K = |scale| sum_p |cc_p| b_p):

  a part          wide_mt_cases.c_parts (the arithmetic is k_mt_parts': wmt_part, fgp_factors.h), on B_part
  the factor      1: f = fma(l, part, ind) rounds once, on a value <= bf
  the product     1: d - 1 products, each one relative rounding of |prod f| <= b_p / d: (d - 1) / d of a unit
  sum over p      the P fmas acc = fma(cc_p, prod_p, acc) and the scale: P + 1 roundings, each of a value whose magnitude
  and scale       is at most sum_p |cc_p| |prod_p| <= B_K / (|scale| d): 1 / d of a unit each, ceil((P + 1) / d) in all

  C_rows = c_parts + 1 + 1 + ceil((P + 1) / d)          (d = 1, P = 16: c_parts + 19;  d = 8, P = 3: c_parts + 3)

and for the mean, wide_mt_mean_cases.c_mean's chain with this C_rows (k_mt_post_mean keeps k_wmt_post_mean's
summation contract: a thread's every 256th point of a chunk, block_sum, the chunks by a lane's every 256th and block_sum,
then w and beta):

  C_mean = C_rows + 1 + L + 9 + ceil(nchunks / 256) + 9 + 2,   L = ceil(min(chunk, n) / 256)

beta = 1 needs no further unit: the cases draw |out0| <= |w| sum_i |K_i c_i| / 2, so the rounding of out0 + v is at
most 2^-53 (3 / 2) |w| sum |K c|, and B_q >= |w| sum_i (|K_i| + B_K,i) |c_i| >= (1 + d) |w| sum |K c|: 3 / (2 (1 + d)) <=
3 / 4 of a unit at d = 1, inside the one unit the "+ 2" has for it (wide_mt_mean_reference's docstring has 1 / 5 from
d >= 9; the argument is the same).

Non-vacuity caps, conditions on the reference alone (asserted in tests/test_mt_pred_cpu.py and again on the device):
regular cases  C 2^-53 B_q <= wide_cases.CAP |q| = 1e-10 |q| for every output;  signed cases (factors of either sign and
exactly 0, weights cc of either sign)  max B_q <= 64 max |q| -- not the wide 4 d: three products of one to eight factors
cancel further than three products of nine and more whose bounds grow with d.  Where a seed's draw misses a cap the seed
is changed (SEEDS below), never C or the cap.
"""
import collections
import functools

import numpy as np

from tests import predict_reference as PR
from tests import wide_cases as WC
from tests import wide_mt_cases as MC
from tests import wide_mt_mean_cases as MM
from tests import wide_mt_mean_reference as MMR
from tests import wide_mt_reference as MR

LAT, NET = MC.LAT, MC.NET
CAP = WC.CAP
SIGNED_CAP = 64
DIMS = (1, 2, 3, 4, 5, 6, 7, 8)
KWG = MM.KWG
U = PR.EPS53

# seeds changed so that the reference alone meets its cap: case name with seed 0 -> the seed used
SEEDS = {}


def _seeded(make, *a, **k):
    case = make(*a, **k)
    seed = SEEDS.get(case.name, 0)
    return case if seed == 0 else make(*a, seed=seed, **k)._replace(name=case.name)


# ------------------------------------------------------------------------------------------------ rows
def _rw(fam, d, **k):
    return _seeded(MC._rw, fam, d, **k)


RW_CASES = []
for _fam in (LAT, NET):
    RW_CASES += [_rw(_fam, d) for d in DIMS]                                       # P = 3, Gk = 4, N = 3, n = 257: every D
    RW_CASES += [_rw(_fam, 3, Gk=G) for G in (1, 5, 8)]                            # NG = 1; a dead row; two full blocks
    RW_CASES += [_rw(_fam, 5, n=n) for n in (1, 255, 8225)]                        # one thread, a tile less one, 33 tiles
    RW_CASES += [_rw(_fam, d, P=1, Gk=1) for d in DIMS]                            # the P == 1 instance, every D
    # (all but one dimension with ind = 0: the kernel value is a bare product of parts.  Even orders for the lattice: an
    # odd B_n vanishes at distance 0, where the pinned test points lie, and a value of exactly 0 has no relative cap)
    RW_CASES += [_rw(_fam, 2, P=1, pattern="mixed"),
                 _rw(_fam, 4, P=1, pattern="allbut1", orders=(2, 4, 6, 8) if _fam == LAT else None),
                 _rw(_fam, 1, P=16), _rw(_fam, 8, P=16, n=65)]
    RW_CASES += [_rw(_fam, 3, N=N, n=N, zp=True, Gk=G) for N, G in ((1, 1), (255, 4), (257, 5))]
    RW_CASES += [_rw(_fam, d, n=33, pattern="mixed", kind="signed") for d in (1, 2, 4, 8)]
RW_CASES += [_rw(LAT, 3, P=1, Gk=1, orders=(o,)) for o in MC.ALL_B]                # every Bernoulli order
for _t in (32, 63):
    RW_CASES += [_rw(NET, 3, P=1, Gk=1, orders=(o,), tbits=_t) for o in MC.ALL_W]  # every Walsh order at both widths
RW_CASES += [_rw(NET, 6, tbits=63), _rw(NET, 6, tbits=63, n=33, pattern="mixed", kind="signed")]
RW_BY_NAME = {c.name: c for c in RW_CASES}
assert len(RW_BY_NAME) == len(RW_CASES)


def c_rows(case):
    return MC.c_parts(case.fam, case.orders, case.tbits) + 2 + -(-(case.P + 1) // case.d)


def pin_origin(case, xt, z):
    """Training point 7 at the origin: test point 0 (all 0.0) lies on it, and test point 1 (all 1.0) lies on it modulo 1
    -- beside test point 2, which the generators put on training point 5."""
    if not getattr(case, "zip", False) and case.n > 7:
        z[:, 7] = 0
        assert (xt[0] == 0.0).all() and (case.N < 2 or (xt[1] == 1.0).all())


def rows_inputs(case):
    inp = MC.rows_inputs(case)
    pin_origin(case, inp["xt"], inp["z"])
    return inp


@functools.lru_cache(maxsize=2)
def rows_reference(name):
    """(inputs, K, B_K), computed once."""
    case = RW_BY_NAME[name]
    inp = rows_inputs(case)
    K, B = MR.mt_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], inp["add"], inp["ind"],
                      inp["cc"], case.tbits, case.zip)
    return inp, K, B


# ------------------------------------------------------------------------------------------------ mean
def _pm(fam, d=3, **k):
    return _seeded(MM._pm, fam, d, **k)


PM_CASES = []
for _fam in (LAT, NET):
    PM_CASES += [_pm(_fam, d) for d in DIMS]                                       # P = 3, B = Gk = 3, N = 3, n = 257
    PM_CASES += [_pm(_fam, d, P=1, B=1) for d in (1, 4, 8)] + [_pm(_fam, 2, P=16), _pm(_fam, 8, P=16, n=65)]
    PM_CASES += [_pm(_fam, n=1), _pm(_fam, n=1023), _pm(_fam, n=1025)]             # 1, 1 and 2 chunks
    PM_CASES += [_pm(_fam, P=1, B=1, N=1, n=258 * 256, chunk=256)]                 # 258 chunks: the chunk sum's second level
    PM_CASES += [_pm(_fam, B=1), _pm(_fam, B=3, Gk=1), _pm(_fam, B=4), _pm(_fam, B=4, Gk=1), _pm(_fam, B=5),
                 _pm(_fam, B=5, Gk=1)]
    PM_CASES += [_pm(_fam, w=False, beta=0), _pm(_fam, w=False, beta=1), _pm(_fam, w=True, beta=0, pad=0)]
    PM_CASES += [_pm(_fam, d, n=33, pattern="mixed", kind="signed") for d in (1, 4, 8)]
PM_CASES += [_pm(NET, 6, tbits=63)]
PM_BY_NAME = {c.name: c for c in PM_CASES}
assert len(PM_BY_NAME) == len(PM_CASES)

chunk_of, nchunks_of, work_len = MM.chunk_of, MM.nchunks_of, MM.work_len


def c_mean(case):
    L = (min(chunk_of(case), case.n) + KWG - 1) // KWG
    return c_rows(case) + 1 + L + 9 + (nchunks_of(case) + KWG - 1) // KWG + 9 + 2


def mean_inputs(case):
    inp = MM.inputs(case)
    pin_origin(case, inp["xt"], inp["z"])
    return inp


@functools.lru_cache(maxsize=2)
def mean_reference(name):
    """(inputs with out0 [B, N] or None, q, B_q, K, B_K), computed once: wide_mt_mean_cases.reference on these inputs."""
    case = PM_BY_NAME[name]
    inp = mean_inputs(case)
    K, BK = MR.mt_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], inp["add"], inp["ind"],
                      inp["cc"], case.tbits)
    out0 = None
    if case.beta:
        _, mag = MMR.mt_post_mean(abs(K), 0 * BK, np.abs(inp["coeffs"]), None if inp["w"] is None else np.abs(inp["w"]))
        sign = 1.0 if inp["w"] is None else np.sign(inp["w"])[:, None]
        out0 = sign * inp["u"] * PR.to_f64(mag) * 0.5
    inp["out0"] = out0
    q, Bq = MMR.mt_post_mean(K, BK, inp["coeffs"], inp["w"], out0)
    return inp, q, Bq, K, BK


# ------------------------------------------------------------------------------------------------ caps and ratios
def cap_ok(kind, C, q, Bq):
    """The non-vacuity cap on the arrays used."""
    q, B = np.abs(PR.to_f64(q)), PR.to_f64(Bq)
    if kind == "regular":
        return bool((C * U * B <= CAP * q).all())
    return bool(B.max() <= SIGNED_CAP * q.max())


def cap_figure(kind, C, q, Bq):
    """What cap_ok compares: max C u B / |q| (regular, against CAP) or max B / max |q| (signed, against SIGNED_CAP)."""
    q, B = np.abs(PR.to_f64(q)), PR.to_f64(Bq)
    if kind == "regular":
        return float((C * U * B / q).max())
    return float(B.max() / q.max())


def ratio(dev, ref, bnd):
    """max |device - reference| / (2^-53 B_q); an error where the bound is 0 is infinite."""
    err = abs(PR._x(np.asarray(dev)) - ref)
    return float(PR.to_f64(np.where(bnd > 0, err / np.where(bnd > 0, U * bnd, 1), np.where(err > 0, np.inf, 0))).max())
