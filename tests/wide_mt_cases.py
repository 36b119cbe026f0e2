"""The case matrix of the wide multitask kernel tests (csrc/fgp_wide_mt.hip: tests/test_gpu_wide_mt_exact.py on the
device, tests/test_wide_mt_reference_cpu.py without one), the inputs of every case and the derived tolerance factors C of
|device - reference| <= C 2^-53 B_q, u = 2^-53.  The counterpart of tests/wide_cases.py, whose conventions it keeps:
'regular' cases have every term of every sum positive (lengthscales in [0.02, 0.25], positive weights and u; where
ind = 0 the part itself is positive), 'signed' cases have factors of either sign, factors that are exactly 0 (ind = 0
and part = 0, and 1 + 4 (-0.25)), weights cc of either sign (every third negative: cancellation over p) and u = 1 + randn.

Rounding counts (B_q of tests/wide_mt_reference.py; b_p >= d |prod_j f_pj|, so one rounding of a term, of a partial
sum over p or of the result is at most 1 / d of a unit of B, and P <= 16 < 2 d of them at most 2 units):

  parts      lattice 10 for every order: even orders as wide_cases.c_parts (the u = t (t - 1) forms); odd orders by
             Horner's rule in t -- order 1: 1, order 3: 3, order 5: 7, order 7: 9 roundings (constants that are not
             dyadic included), each on an intermediate that the monomials' magnitudes bound --, and the product with
             coef 1.  Net: wide_cases.c_parts' count of omega (order 1: 3; orders 2..4: 7, 27, t + 4) + 1 for add + omega
             + 1 for the product with coef.
  k1         5: f = fma(l, p, ind) rounds once on bf (1 unit); the d - 1 products by a factor that is not an exact 1
             (1 unit in all); the P fmas of the sum over p (2); the scale (1 / d, counted 1).
  k1_bwd     dscale 25 + ceil(nblk / 256), dls 28 + ceil(nblk / 256): wide_cases.c_k1_bwd_scale / _ls (22 / 25: the
             factor, the blocked product, u prod or the four roundings of ((u s) p) (pre suf), the wave tree 6, the
             4 waves 3, k_wmt_k1_bwd_sum's strided sum and block_sum 9) + 1 for u cc + 2 for the P additions into the
             wave's LDS slot.
  rows       c_parts + 5: a factor is fma(l, part, ind) of a part formed in the kernel -- the part's c_parts units of
             B_part and the fma's 1 on bf = ind + |l| B_part --, then as k1: the products 1, the sum over p 2, the
             scale 1.

Non-vacuity caps, asserted on the arrays used (tests/test_wide_mt_reference_cpu.py and again on the device): regular
k1, k1_bwd, rows  C u B_q <= wide_cases.CAP |q|;  signed (cancellation over p)  max B_q <= 4 d max |q|, the cap of
tests/test_gpu_wide_exact.py::_check;  parts  wide_cases.parts_cap_ok (points that miss it are drawn again).

Cases changed so that the reference alone meets its cap (never the cap or C):
  * the signed first-column case at d = 13 takes seed 2 (seeds 0 and 1: the 33 terms of dscale cancel to 1 / 70 of
    their bound, past 4 d = 52), and the regular all-but-one rows case seed 1 (seed 0 has a factor l coef B_n next to a
    zero of B_n);
  * signed sums over p have 3 pairs: 16 products of factors of either sign cancel past the cap whatever the weights;
  * the parts of all (x_i, z_k) pairs have 37 x 7 lattice pairs: with 53 z per x no redraw of x clears the band above
    1e-3 for all of them (odd orders carry the monomials' magnitudes and the distance term, B up to 6).
"""
import collections
import functools

import numpy as np

from tests import predict_cases as PC
from tests import predict_reference as PR
from tests import wide_cases as WC
from tests import wide_mt_reference as MR

LAT, NET = PR.LAT, PR.NET
CAP = WC.CAP
DIMS = (9, 16, 17, 33, 63, 64)


# ------------------------------------------------------------------------------------------------ ind patterns
def ind_rows(d, P, pattern):
    """ind [P][d].  'ones': no derivative.  'mixed': pair 0 all ones, then one zero (the last dimension), several
    zeros (1, d // 2, d - 1) and so on in turn.  'allbut1': every pair has a single 1, at dimension p mod d."""
    out = []
    for p in range(P):
        if pattern == "ones" or (pattern == "mixed" and p % 3 == 0):
            r = [1] * d
        elif pattern == "mixed" and p % 3 == 1:
            r = [1] * (d - 1) + [0]
        elif pattern == "mixed":
            r = [0 if j in (1, d // 2, d - 1) else 1 for j in range(d)]
        else:
            r = [1 if j == p % d else 0 for j in range(d)]
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ first column
K1 = collections.namedtuple("K1", "name d P G n pattern kind seed")


def _k1(d, P=3, G=4, n=257, pattern="mixed", kind="regular", seed=0):
    return K1("mtk1-d%d-P%d-G%d-n%d-%s%s" % (d, P, G, n, pattern, "-signed" if kind == "signed" else ""), d, P, G, n,
              pattern, kind, seed)


K1_CASES = [_k1(d) for d in DIMS]                                                # k_wmt_k1_bwd<2..8> at d's edges
K1_CASES += [_k1(d) for d in (24, 25, 41, 49, 57)]                               # the remaining DB
K1_CASES += [_k1(9, G=G) for G in (1, 5, 8)] + [_k1(9, n=n) for n in (1, 255, 8225)]
K1_CASES += [_k1(9, P=1, pattern=p) for p in ("ones", "allbut1")] + [_k1(d, P=16) for d in (9, 64)]
K1_CASES += [_k1(9, P=1, G=1, n=66048)]                                          # 258 blocks: the second-level sum wraps
K1_CASES += [_k1(13, n=33, kind="signed", seed=2), _k1(64, n=33, kind="signed")] + [_k1(9, P=16, n=33, pattern="allbut1", kind="signed")]
K1_BY_NAME = {c.name: c for c in K1_CASES}


def c_k1(case):
    return 5


def c_k1_bwd_scale(case):
    return WC.c_k1_bwd_scale(case) + 3


def c_k1_bwd_ls(case):
    return WC.c_k1_bwd_ls(case) + 3


def k1_inputs(case):
    """dict: parts [P, d, n], ind [P][d], cc [P], scale [G], ls [G, d], u [G, n]."""
    g = PC._rng(31, case.d, case.P, case.G, case.n, len(case.pattern), case.seed)
    signed = case.kind == "signed"
    ind = ind_rows(case.d, case.P, case.pattern)
    shape = (case.P, case.d, case.n)
    if signed:
        parts = (g.random(shape) - 0.5) * 1.2
        cc = (0.5 + g.random(case.P)) * np.where(np.arange(case.P) % 3 == 1, -1.0, 1.0)
        u = 1.0 + g.standard_normal((case.G, case.n))
    else:
        parts = -0.5 + 2.5 * g.random(shape)
        zero = np.asarray(ind) == 0
        parts[zero] = np.abs(parts[zero]) + 0.5                 # ind = 0: the factor l p itself, positive
        cc = 0.5 + g.random(case.P)
        u = 0.1 + g.random((case.G, case.n))
    scale = 0.5 + 1.5 * g.random(case.G)
    ls = 0.02 + 0.23 * g.random((case.G, case.d))
    if signed:
        ls[:, ::3] = 4.0
        for p in range(case.P):                                   # factors exactly 0 at the first 8 points
            j0 = [j for j in range(case.d) if ind[p][j] == 0]
            if j0:
                parts[p, j0[0], :min(8, case.n)] = 0.0           # ind = 0 and l part = 0
            else:
                parts[p, 0, :min(8, case.n)] = -0.25             # 1 + 4 (-0.25)
    return dict(parts=parts, ind=ind, cc=cc, scale=scale, ls=ls, u=u)


@functools.lru_cache(maxsize=2)
def k1_reference(name):
    """(inputs, k1, B, dscale, B, dls, B)."""
    inp = k1_inputs(K1_BY_NAME[name])
    k, Bk = MR.mt_k1(inp["parts"], inp["ind"], inp["cc"], inp["scale"], inp["ls"])
    ds, Bs, dl, Bl = MR.mt_k1_bwd(inp["parts"], inp["ind"], inp["cc"], inp["scale"], inp["ls"], inp["u"])
    return inp, k, Bk, ds, Bs, dl, Bl


# ------------------------------------------------------------------------------------------------ spec tables
def spec_tables(fam, d, P, orders, pattern, g, signed):
    """(order, coef, add, ind, cc) [P][d] / [P]: orders cycle through `orders` over (p, j); net add = 1 where ind = 0
    (the reference's indicator of a derivative) and coef a power of -2 there."""
    ind = ind_rows(d, P, pattern)
    order = [[int(orders[(p * 5 + j) % len(orders)]) for j in range(d)] for p in range(P)]
    if fam == LAT:
        coef = [[float((0.5 + g.random()) * (-1 if (signed and (p + j) % 2) else 1)) for j in range(d)] for p in range(P)]
        add = [[0.0] * d for _ in range(P)]
    else:
        coef = [[(1.0 if ind[p][j] else (-2.0 if signed else 4.0)) for j in range(d)] for p in range(P)]
        add = [[0.0 if ind[p][j] else 1.0 for j in range(d)] for p in range(P)]
    cc = ((0.5 + g.random(P)) * np.where(signed & (np.arange(P) % 3 == 1), -1.0, 1.0)).tolist()
    return order, coef, add, ind, cc


def c_parts(fam, orders, tbits):
    if fam == LAT:
        return 10
    return 2 + max({1: 3}.get(int(o), PC.factor_count(NET, int(o), tbits) - 1) for o in orders)


# ------------------------------------------------------------------------------------------------ parts
PT = collections.namedtuple("PT", "name fam d P N M zip orders tbits seed")


def _pt(fam, d, orders, P=3, N=257, M=1, zp=False, tbits=0):
    tag = "o" + "".join(map(str, orders))
    return PT("mtparts-%s-d%d-P%d-N%d-M%d%s-%s%s" % ("lat" if fam == LAT else "net", d, P, N, M, "-zip" if zp else "", tag,
                                                     "-t%d" % tbits if fam == NET else ""),
              fam, d, P, N, M, zp, tuple(orders), tbits if fam == NET else 0, 0)


ALL_B, ALL_W = (1, 2, 3, 4, 5, 6, 7, 8), (1, 2, 3, 4)
PT_CASES = [_pt(LAT, d, ALL_B) for d in (9, 64)] + [_pt(LAT, 9, (o,), P=1) for o in ALL_B]
PT_CASES += [_pt(LAT, 17, ALL_B, P=16, N=33), _pt(LAT, 9, ALL_B, N=37, M=7), _pt(LAT, 9, ALL_B, N=255, M=255, zp=True)]
for _t in (32, 63):
    PT_CASES += [_pt(NET, d, ALL_W, tbits=_t) for d in (9, 64)] + [_pt(NET, 9, (o,), P=1, tbits=_t) for o in ALL_W]
PT_CASES += [_pt(NET, 9, ALL_W, N=5, M=53, tbits=32), _pt(NET, 9, ALL_W, N=257, M=257, zp=True, tbits=32)]
PT_BY_NAME = {c.name: c for c in PT_CASES}


def _draw(g, fam, shape, tbits):
    return g.random(shape) if fam == LAT else g.integers(0, 2 ** tbits, shape, dtype=np.int64)


def pinned_pair(case):
    """(row of x, row of z, pair index e) of the pair at distance 0, or None: x[5 mod N] is set to the z it meets when
    every x meets one z only (M == 1, or zipped pairs)."""
    if not (case.zip or case.M == 1):
        return None
    r = 5 % case.N
    return (r, r, r) if case.zip else (r, 0, r)


@functools.lru_cache(maxsize=2)
def parts_reference(name):
    """(inputs, parts, B, C): x [N, d] a view of rows of stride d + 3, z [M, d]; pinned_pair's points coincide.  A
    point x[i, j] with a part that misses the parts' cap is drawn again (wide_cases.parts_reference)."""
    case = PT_BY_NAME[name]
    g = PC._rng(33, case.fam, case.d, case.P, case.N, case.M, sum(case.orders), case.tbits, case.seed)
    order, coef, add, _, _ = spec_tables(case.fam, case.d, case.P, case.orders, "mixed", g, True)
    full = _draw(g, case.fam, (case.N, case.d + 3), case.tbits)
    z = _draw(g, case.fam, (case.M, case.d), case.tbits)
    x = full[:, :case.d]
    pin = pinned_pair(case)
    if pin is not None:
        x[pin[0]] = z[pin[1]]
    C = c_parts(case.fam, case.orders, case.tbits)
    E = case.N if case.zip else case.N * case.M
    rows = np.arange(E) if case.zip else np.arange(E) // case.M
    for _ in range(50):
        Pv, Bv = MR.mt_parts(case.fam, x, z, order, coef, add, case.tbits, case.zip)
        bad_e = ~WC.parts_cap_ok(C, Pv, Bv).reshape(case.P, case.d, E).all(0)              # [d, E]
        if not bad_e.any():
            break
        bad = np.zeros((case.N, case.d), dtype=bool)
        for j in range(case.d):
            bad[rows[bad_e[j]], j] = True
        assert pin is None or not bad[pin[0]].any(), "the pair at distance 0 meets the cap as it is"
        x[bad] = _draw(g, case.fam, int(bad.sum()), case.tbits)
    assert not bad_e.any()
    return dict(x_full=full, x=x, z=z, order=order, coef=coef, add=add), Pv, Bv, C


# ------------------------------------------------------------------------------------------------ rows
RW = collections.namedtuple("RW", "name fam d P Gk N n zip orders tbits pattern kind seed")


def _rw(fam, d, P=3, Gk=4, N=3, n=257, zp=False, orders=None, tbits=32, pattern="ones", kind="regular", seed=0):
    orders = tuple(orders if orders is not None else (ALL_B if fam == LAT else ALL_W))
    name = "mtrows-%s-d%d-P%d-G%d-N%d-n%d%s-o%s-%s%s%s" % (
        "lat" if fam == LAT else "net", d, P, Gk, N, n, "-zip" if zp else "", "".join(map(str, orders)), pattern,
        "-t%d" % tbits if fam == NET else "", "-signed" if kind == "signed" else "")
    return RW(name, fam, d, P, Gk, N, n, zp, orders, tbits if fam == NET else 0, pattern, kind, seed)


RW_CASES = []
for _fam in (LAT, NET):
    RW_CASES += [_rw(_fam, d) for d in DIMS]
    RW_CASES += [_rw(_fam, 9, Gk=G) for G in (1, 5, 8)] + [_rw(_fam, 9, n=n, N=1) for n in (1, 255, 8225)]
    RW_CASES += [_rw(_fam, 9, P=1, pattern="mixed"), _rw(_fam, 9, P=1, pattern="allbut1", seed=1), _rw(_fam, 9, P=16), _rw(_fam, 64, P=16, n=65)]
    RW_CASES += [_rw(_fam, 9, N=N, n=N, zp=True, Gk=G) for N, G in ((1, 1), (255, 4), (257, 5))]
    RW_CASES += [_rw(_fam, d, n=33, pattern="mixed", kind="signed") for d in (13, 64)]
RW_CASES += [_rw(NET, 17, tbits=63), _rw(NET, 17, tbits=63, n=33, pattern="mixed", kind="signed")]
RW_BY_NAME = {c.name: c for c in RW_CASES}


def c_rows(case):
    return c_parts(case.fam, case.orders, case.tbits) + 5


def rows_inputs(case):
    """dict: xt [N, d], z [d, n], hyp [Gk, 1 + d] and the spec tables.  Regular cases with ind = 0 somewhere have one
    pair (no sum over p to cancel in); regular sums over p have ind = 1 throughout, where the small lengthscales keep
    every factor positive.  Test point 2 mod N is training point 5 mod n (distance 0)."""
    g = PC._rng(35, case.fam, case.d, case.P, case.Gk, case.N, case.n, sum(case.orders), case.tbits, len(case.pattern), case.seed)
    signed = case.kind == "signed"
    assert signed or case.P == 1 or case.pattern == "ones"
    xt, z = PC._points(g, case.fam, case.d, case.n, case.N, case.tbits)
    hyp = PC._hyp(g, case.Gk, case.d, case.kind)
    order, coef, add, ind, cc = spec_tables(case.fam, case.d, case.P, case.orders, case.pattern, g, signed)
    if case.fam == LAT and not signed:
        # keep 1 + l coef B_n inside (0, 2): |B_n| <= 1/2 for every order, |coef| <= 1.5, l <= 0.25
        pass
    return dict(xt=xt, z=z, hyp=hyp, order=order, coef=coef, add=add, ind=ind, cc=cc)


@functools.lru_cache(maxsize=2)
def rows_reference(name):
    """(inputs, K, B_K)."""
    case = RW_BY_NAME[name]
    inp = rows_inputs(case)
    K, B = MR.mt_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], inp["add"], inp["ind"],
                      inp["cc"], case.tbits, case.zip)
    return inp, K, B
