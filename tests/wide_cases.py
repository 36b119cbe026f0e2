"""The case matrix of the wide-kernel tests (9 <= d <= 64: tests/test_gpu_wide_exact.py on the device,
tests/test_wide_reference_cpu.py without one), the inputs of every case and the derived tolerance factors.  The
counterpart of tests/predict_cases.py, whose inputs, kinds ('regular': lengthscales in [0.02, 0.25], positive
coefficients and u; 'signed': lengthscales in [0.02, 5], randn coefficients and u) and test points (row 0 all 0, row 1
all 1, row 2 training point 5) it takes over.

Tolerance factors C of |device - reference| <= C 2^-53 B_q, counted from each kernel's roundings; u = 2^-53.  The
factor arithmetic is csrc/fgp_factors.h in both widths, so FACTOR_COUNT (predict_cases.factor_count) carries over, and
with B_K >= d |K| the d roundings of a product of d factors and the scale stay at most 1 unit of B_K at every d.

  rows (k_wide_rows)          max_j FACTOR_COUNT + 2, as k_kernel_rows: the product runs over j ascending from 1.0 (the
                              first multiplication is exact), then the scale.
  mean (k_wide_post_mean + k_wide_sum)   max_j FACTOR_COUNT + 3 + min(chunk, n) + ceil(nchunks / 256) + 9, as
                              k_post_mean: the folded form moves d more factors a_j into the scale ((2 d) / d + 1 = 3,
                              the only rounding the wide kernel adds, and the narrow count already has it); a term
                              passes through at most min(chunk, n) accumulating fmas -- the dead points of a slab and of
                              the 8-point register tile add a finite product times 0, exactly --; k_wide_sum is
                              k_sum_chunks.  The fold's own factor u^2 + c' rounds c' = c / a (c's 4 and the division)
                              and once in the fma: below FACTOR_COUNT.
  mean by GEMM                max_j FACTOR_COUNT + 2 + n.
  quadratic form (k_wide_qf_rows + k_qf_cols)   max(rows, 44): the row is formed as k_wide_rows forms it and the tail is
                              k_qf_rows' (predict_cases).
  parts                       lattice 10: the distance's roundings are in the bound; u = fma(x, x, -x) through the
                              polynomial 2.5, its products and inner fmas 5, the last fma 1 (on |B - B(0)|, together
                              9.5), the rounded constant and the last fma 2 on |B(0)|, the product with coef 1 on both:
                              at most 10 on either term.  Net order 1: 3 (1/6 rounded, the subtraction, the product with
                              6); orders 2..4: FACTOR_COUNT - 1 = 7, 27, t + 4 (no factor fma).
  k1 (k_wide_k1)              3: f = fma(l, p, 1) rounds once on |f| <= bf; the d - 1 products (a padded dimension has
                              l = p = 0, f = 1 exactly, an exact product) and the scale are d roundings of |k1|, 1 unit
                              of B; 1 to spare.
  k1_bwd, dscale              22 + ceil(nblk / 256), nblk = ceil(n / 256): the factor's fma 1; the product of the DB
                              blocks of 8 -- 7 roundings within a block, DB between blocks, at most d + DB - 1 that
                              are not by an exact 1 -- is at most 2 units of B (>= d |prod|); u prod 1; the wave tree 6
                              and the 4 waves in order 3; k_wide_k1_bwd_sum: the strided thread sum ceil(nblk / 256),
                              block_sum 6 + 3.
  k1_bwd, dls                 25 + ceil(nblk / 256): the factor's fma 1; the leave-one-out product (blocks before)
                              (prefix) (suffix) (blocks after) has at most d + DB roundings over its d - 1 factors, at
                              most 2 units of B (>= (d - 1) |term|); u s, (u s) p, pre suf and their product 4 on
                              |term|; the sums as for dscale, 18 + ceil(nblk / 256).

The mean's cases, count and caps are kept here and asserted without a device; the device comparison of
fgp_wide_post_mean is not in tests/test_gpu_wide_exact.py yet.

The non-vacuity caps (asserted on the arrays used, through tests/test_wide_reference_cpu.py and again on the device):
regular rows, mean, k1, k1_bwd  C u B_q <= 1e-10 |q|;  quadratic form 1e-11 |q|;  signed and the lengthscale 2000
max B_q <= 4 d max |q|;  parts 1e-12 |q|, or C u B_q <= 1e-14 where |q| <= 1e-3.

Cases changed so that the reference alone meets its cap (never the cap or C):
  * parts: a point whose part lies in the band above 1e-3 where C u B > 1e-12 |q| (next to a zero of B_2a / omega_a),
    or below 1e-3 with C u B > 1e-14 (net order 4 at t = 63: 67 u W_4 = 1.03e-14), is drawn again (parts_reference);
  * the signed first-column cases have n = 33 points, as the signed rows-and-mean cases have.
  * the 1/ev weights take a lengthscale per case (GP_LS) for max ev / min ev in [10, 1e4].
"""
import collections
import functools
import math

import numpy as np

from tests import predict_cases as PC
from tests import predict_reference as PR

LAT, NET = PR.LAT, PR.NET
CAP, CAP_QF, CAP_PARTS, CAP_PARTS_ABS, PARTS_NEAR_ZERO = 1e-10, 1e-11, 1e-12, 1e-14, 1e-3
FOLD_LOG2 = 960.0           # the range W <= 960 in which the folded B4 form stays normal (fold_log2)

RM = collections.namedtuple("RM", "name fam d n N B Gk chunk alphas tbits kind zero_ls ls pad path seed")


def _mixed(d):
    return [1 + j % 4 for j in range(d)]


def _rm(group, fam, d, n=257, N=5, B=1, Gk=None, chunk=32, alphas=None, tbits=32, kind="regular", zero_ls=False, ls=None,
        pad=0, path="direct", seed=0):
    if Gk is None:
        Gk = B
    if alphas is None:
        alphas = [2] * d if fam == LAT else [1] * d
    alphas = [int(a) for a in alphas]
    tag = "u%d" % alphas[0] if len(set(alphas)) == 1 else ("mix" if alphas == _mixed(d) else "".join(map(str, alphas)))
    name = "%s-%s-d%d-n%d-N%d-B%d-G%d-c%d-a%s" % (group, "lat" if fam == LAT else "net", d, n, N, B, Gk, chunk, tag)
    if fam == NET:
        name += "-t%d" % tbits
    for flag, t in ((kind == "signed", "signed"), (zero_ls, "ls0"), (ls, "ls" + str(ls)), (pad, "pad"), (path != "direct", path)):
        if flag:
            name += "-" + t
    return RM(name, fam, d, n, N, B, Gk, chunk, tuple(alphas), tbits if fam == NET else 0, kind, zero_ls, ls, pad, path, seed)


FOLD_LS = ("1e-6", "2e-7", "1e-7", "1e-60", "ard")      # d = 64; "2000" (signed) and d = 9 at 1e-60 besides


def _rm_matrix():
    c = []
    # every dimension at which something changes: d = 64 fills the constants' wave
    for fam in (LAT, NET):
        for d in (9, 16, 17, 33, 63, 64):
            c.append(_rm("dim", fam, d))
    # k_wide_rows<FAM, 1 | 4>: one row, four with one dead, two row blocks with three dead
    for fam in (LAT, NET):
        for Gk in (1, 3, 5):
            c.append(_rm("rows", fam, 9, B=Gk))
    # k_wide_post_mean<FAM, 1 | 4, 0 | 4>
    for d in (9, 64):
        for B in (1, 3):
            for a in (1, 2, 3, 4):
                c.append(_rm("var", LAT, d, B=B, alphas=[a] * d))               # 2: the fold; 1, 3, 4: ORD = 0
            c.append(_rm("var", LAT, d, B=B, alphas=_mixed(d)))
            c.append(_rm("var", LAT, d, B=B, zero_ls=True))                     # the fold refused: a == 0
            c.append(_rm("var", NET, d, B=B))
            c.append(_rm("var", NET, d, B=B, alphas=_mixed(d)))
    for B in (1, 3):
        c.append(_rm("var", NET, 17, B=B, tbits=63))
        c.append(_rm("var", NET, 17, B=B, alphas=_mixed(17), tbits=63))
    # shapes at d = 9: n about the 64-point slab and its 8-point register tile, N about the 256-thread tile
    Ns = (1, 255, 257)
    i = 0
    for fam in (LAT, NET):
        for n in (1, 7, 63, 64, 65, 257, 1025):
            for chunk in (32, 1024):
                c.append(_rm("shape", fam, 9, n=n, N=Ns[i % 3], chunk=chunk))
                i += 1
        c.append(_rm("shape", fam, 9, n=8225, N=1, chunk=32))                    # 258 chunks: k_wide_sum's loop wraps
    # outputs and hyper-parameter rows
    for fam in (LAT, NET):
        for B in (1, 2, 3, 4):
            for Gk in sorted(set((1, B))):
                c.append(_rm("out", fam, 9, B=B, Gk=Gk))
        c.append(_rm("out", fam, 9, B=4, Gk=2))                                  # g = b mod Gk, 1 < Gk < B
        for B in (5, 8, 10):                                                     # block launch, remainder 1, 0, 2
            c.append(_rm("out", fam, 9, B=B, Gk=B))
        c.append(_rm("out", fam, 9, B=8, Gk=1, path="ops"))                      # kernel rows + GEMM
        c.append(_rm("out", fam, 9, B=3, Gk=3, pad=8))                           # coeff_stride = n + 8
    # factors that cross zero, signed coefficients
    for d in (9, 64):
        c.append(_rm("sgn", LAT, d, n=33, B=3, kind="signed"))
        c.append(_rm("sgn", LAT, d, n=33, B=3, alphas=_mixed(d), kind="signed"))
        c.append(_rm("sgn", NET, d, n=33, B=3, alphas=_mixed(d), kind="signed"))
    # the fold's range
    for B in (1, 4):
        for ls in FOLD_LS:
            c.append(_rm("fold", LAT, 64, B=B, ls=ls))
        c.append(_rm("fold", LAT, 64, n=33, B=B, ls="2000", kind="signed"))
        c.append(_rm("fold", LAT, 9, B=B, ls="1e-60"))
    out, seen = [], set()
    for case in c:
        if case.name not in seen:
            seen.add(case.name)
            out.append(case)
    return out


RM_CASES = _rm_matrix()
RM_BY_NAME = {c.name: c for c in RM_CASES}

QF = collections.namedtuple("QF", "name fam m d alphas tbits seed")


def _qf(fam, m, d, alphas, tbits=0):
    tag = "u%d" % alphas[0] if len(set(alphas)) == 1 else "mix"
    return QF("qf-%s-m%d-d%d-a%s" % ("lat" if fam == LAT else "net", m, d, tag), fam, m, d, tuple(alphas),
              tbits if fam == NET else 0, 0)


QF_CASES = [_qf(LAT, 13, 64, [2] * 64), _qf(LAT, 13, 64, _mixed(64))]
for _m in (13, 14, 15, 16):                                                      # P2 = 9..12 (m = 13: d = 64 too)
    QF_CASES += [_qf(LAT, _m, 9, [2] * 9), _qf(LAT, _m, 9, _mixed(9))]
QF_CASES += [_qf(LAT, 17, 9, [2] * 9),                                           # the 32-row column pass
             _qf(NET, 13, 64, [1] * 64, 32), _qf(NET, 14, 17, _mixed(17), 32)]
QF_BY_NAME = {c.name: c for c in QF_CASES}
WA_KINDS, QF_N, QF_P, GP_NOISE = PC.WA_KINDS, PC.QF_N, PC.QF_P, PC.GP_NOISE
# the lengthscale of the GP behind the 1/ev weights, per (family, d): max ev / min ev in [10, 1e4]
GP_LS = {(LAT, 64): 0.01, (LAT, 9): 0.2, (NET, 64): 0.01, (NET, 17): 0.1}

K1 = collections.namedtuple("K1", "name d G n kind seed")


def _k1(d, G=3, n=257, kind="regular"):
    return K1("k1-d%d-G%d-n%d%s" % (d, G, n, "-signed" if kind == "signed" else ""), d, G, n, kind, 0)


K1_CASES = [_k1(d) for d in (9, 16, 17, 24, 25, 33, 41, 49, 57, 64)]            # k_wide_k1_bwd<2..8> at its edges
K1_CASES += [_k1(9, G=G) for G in (1, 5)] + [_k1(9, n=n) for n in (1, 255, 256)]
K1_CASES += [_k1(9, G=1, n=65793)]                                               # 258 blocks: k_wide_k1_bwd_sum's loop wraps
K1_CASES += [_k1(d, n=33, kind="signed") for d in (13, 64)]
K1_BY_NAME = {c.name: c for c in K1_CASES}

PT = collections.namedtuple("PT", "name fam d n orders tbits seed")


def _pt(fam, d, orders, tbits=0):
    tag = "u%d" % orders[0] if len(set(orders)) == 1 else "mix"
    return PT("parts-%s-d%d-o%s%s" % ("lat" if fam == LAT else "net", d, tag, "-t%d" % tbits if fam == NET else ""),
              fam, d, 257, tuple(orders), tbits, 0)


PT_CASES = []
for _d in (9, 64):
    PT_CASES += [_pt(LAT, _d, [o] * _d) for o in (2, 4, 6, 8)] + [_pt(LAT, _d, [2 * a for a in _mixed(_d)])]
    for _t in (32, 63):
        PT_CASES += [_pt(NET, _d, [o] * _d, _t) for o in (1, 2, 3, 4)] + [_pt(NET, _d, _mixed(_d), _t)]
PT_BY_NAME = {c.name: c for c in PT_CASES}


# ------------------------------------------------------------------------------------------------ tolerance factors
c_factor, c_rows, c_mean, c_quadform = PC.c_factor, PC.c_rows, PC.c_mean, PC.c_quadform


def c_parts(case):
    if case.fam == LAT:
        return 10
    return max({1: 3}.get(int(o), PC.factor_count(NET, o, case.tbits) - 1) for o in case.orders)


def c_k1(case):
    return 3


def _nblk_levels(n):
    return (((n + 255) // 256) + 255) // 256


def c_k1_bwd_scale(case):
    return 22 + _nblk_levels(case.n)


def c_k1_bwd_ls(case):
    return 25 + _nblk_levels(case.n)


# ------------------------------------------------------------------------------------------------ inputs
def fold_lengthscales(case, hyp):
    """The lengthscale rows of a fold-range case, set in hyp [Gk, 1 + d]."""
    if case.ls == "ard":
        hyp[:, 1:33] = 1e-12
    elif case.ls is not None:
        hyp[:, 1:] = float(case.ls)
    return hyp


def fold_log2(case, hyp, coef):
    """W = |log2 |scale|| + sum_j (|log2 |a_j|| + log2(1 + |a_j| / 30)) of every hyper-parameter row.  A folded factor is
    u^2 + c' = 1 / a + B4(t) with |B4| <= 1/30, so |u^2 + c'| <= (1 + |a| / 30) / |a|: every partial product of folded
    factors, in any order, is at most 2^W, and every partial product of scale prod_j a_j lies within 2^-W .. 2^W."""
    a = np.abs(hyp[:, 1:] * np.asarray(coef)[None, :])
    with np.errstate(divide="ignore"):
        return np.abs(np.log2(np.abs(hyp[:, 0]))) + (np.abs(np.log2(a)) + np.log2(1 + a / 30)).sum(-1)


def rm_inputs(case):
    """dict: xt [N, d], z [d, n], hyp [Gk, 1 + d], coeffs [B, n] (a view of [B, n + pad]), order, coef."""
    g = PC._rng(21, case.fam, case.d, case.n, case.N, case.B, case.Gk, case.chunk, sum(case.alphas), case.tbits, case.seed)
    xt, z = PC._points(g, case.fam, case.d, case.n, case.N, case.tbits)
    hyp = PC._hyp(g, case.Gk, case.d, "regular" if case.ls == "2000" else case.kind)
    if case.zero_ls:
        hyp[:, 1 + case.d // 2] = 0.0
    fold_lengthscales(case, hyp)
    full = g.standard_normal((case.B, case.n + case.pad)) if case.kind == "signed" else \
        0.1 + g.random((case.B, case.n + case.pad))
    order, coef = PC.pred_args(case.fam, case.alphas)
    return dict(xt=xt, z=z, hyp=hyp, coeffs_full=full, coeffs=full[:, :case.n], order=order, coef=coef)


@functools.lru_cache(maxsize=4)
def rm_reference(name):
    """(inputs, K, B_K, mean, B_mean) of a rows-and-mean case, computed once."""
    case = RM_BY_NAME[name]
    inp = rm_inputs(case)
    K, BK = PR.kernel_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], case.tbits)
    mean, Bm = PR.post_mean(K, BK, inp["coeffs"])
    return inp, K, BK, mean, Bm


def net_sequence(d, seed, t=32):
    import fastgaussianprocesses_amd as F
    from tests.test_gpu_wide import net_matrices
    return F.DigitalNetB2(d, seed=seed, generating_matrices=net_matrices(d, seed, t=t), t=t)


def gp_spectrum(fam, m, d, alphas, seed, ls):
    """ev [n] of a real GP on n = 2^m points (predict_cases.gp_weights: scale 1e-2 / n, noise 1e-4) with every
    lengthscale ls; nets at d > 8 from the generating matrices of tests/test_gpu_wide.net_matrices."""
    import torch

    import fastgaussianprocesses_amd as F
    from oracle import fgp_oracle as O
    n = 1 << m
    lsv = torch.full((d,), float(ls), dtype=torch.float64)
    sc = torch.tensor([1e-2 / n], dtype=torch.float64)
    if fam == LAT:
        x = torch.from_numpy(F.Lattice(d, seed=seed)(0, n))
        parts, tr = O.lattice_k1parts(x, list(alphas)), O.fftbr
    else:
        seq = net_sequence(d, seed)
        xb = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64))
        parts, tr = O.net_k1parts(xb, seq.t, list(alphas)), O.fwht
    k1 = O.kernel_from_parts(parts, sc, lsv)
    ev = math.sqrt(n) * O.ft_stable(k1.to(torch.float64), tr) + GP_NOISE
    return np.ascontiguousarray(ev.real.numpy() if torch.is_complex(ev) else ev.numpy())


def qf_inputs(case):
    """dict: xt [P, N, d], z [P, d, n], hyp [P, 1 + d], wa {kind: [P, n]} (problem 1: twice problem 0's weights, exact),
    ev [n], order, coef.  The stacked run takes everything per problem; the shared run takes xt[0] and z[0] for both
    problems (stride 0) with hyp and wa stacked."""
    n = 1 << case.m
    g = PC._rng(23, case.fam, case.m, case.d, sum(case.alphas), case.seed)
    pts = [PC._points(g, case.fam, case.d, n, QF_N, case.tbits) for _ in range(QF_P)]
    hyp = PC._hyp(g, QF_P, case.d, "regular")
    unif = 0.5 + g.random(n)
    if case.fam == LAT:                               # the weights of a Hermitian spectrum: wa[n - k] = wa[k]
        unif[n // 2 + 1:] = unif[1:n // 2][::-1]
    ev = gp_spectrum(case.fam, case.m, case.d, case.alphas, 7 + case.seed, GP_LS[(case.fam, case.d)])
    wa = {k: np.stack([w, 2.0 * w]) for k, w in (("one", np.ones(n)), ("unif", unif), ("gp", 1.0 / ev))}
    order, coef = PC.pred_args(case.fam, case.alphas)
    return dict(xt=np.stack([p[0] for p in pts]), z=np.stack([p[1] for p in pts]), hyp=hyp, wa=wa, ev=ev, order=order,
                coef=coef)


QF_RUNS = ("stacked", "shared")


@functools.lru_cache(maxsize=2)
def qf_reference(name):
    """(inputs, {run: (rows, B_rows, power)}), each a list over the P problems of [N, n] arrays: the stacked run's
    problem p has (xt[p], z[p], hyp[p]), the shared run's (xt[0], z[0], hyp[p])."""
    case = QF_BY_NAME[name]
    inp = qf_inputs(case)
    K0, B0 = PR.kernel_rows(case.fam, inp["xt"][0], inp["z"][0], inp["hyp"], inp["order"], inp["coef"], case.tbits)
    K1_, B1 = PR.kernel_rows(case.fam, inp["xt"][1], inp["z"][1], inp["hyp"][1:2], inp["order"], inp["coef"], case.tbits)
    pw = [PR.spectrum_power(case.fam, r) for r in (K0[0], K0[1], K1_[0])]
    return inp, dict(stacked=([K0[0], K1_[0]], [B0[0], B1[0]], [pw[0], pw[2]]),
                     shared=([K0[0], K0[1]], [B0[0], B0[1]], [pw[0], pw[1]]))


def k1_inputs(case):
    """dict: parts [d, n], scale [G], ls [G, d], u [G, n].  Regular: parts in [-0.5, 2] (of either sign, but no
    lengthscale gradient is a cancelling sum).  Signed: parts in [-0.6, 0.6], every third lengthscale 4 (factors
    1 + 4 p cross zero) and dimension 0's factor exactly 0 at the first 8 points."""
    g = PC._rng(25, case.d, case.G, case.n, case.seed)
    signed = case.kind == "signed"
    parts = (g.random((case.d, case.n)) - 0.5) * 1.2 if signed else -0.5 + 2.5 * g.random((case.d, case.n))
    scale = 0.5 + 1.5 * g.random(case.G)
    ls = 0.02 + 0.23 * g.random((case.G, case.d))
    u = g.standard_normal((case.G, case.n)) if signed else 0.1 + g.random((case.G, case.n))
    if signed:
        ls[:, ::3] = 4.0
        parts[0, :8] = -0.25
    return dict(parts=parts, scale=scale, ls=ls, u=u)


@functools.lru_cache(maxsize=2)
def k1_reference(name):
    """(inputs, k1, B, dscale, B, dls, B)."""
    case = K1_BY_NAME[name]
    inp = k1_inputs(case)
    k, Bk = PR.k1(inp["parts"], inp["scale"], inp["ls"])
    ds, Bs, dl, Bl = PR.k1_bwd(inp["parts"], inp["scale"], inp["ls"], inp["u"])
    return inp, k, Bk, ds, Bs, dl, Bl


def parts_cap_ok(C, q, B):
    """The parts' cap per output: 1e-12 |q|, or, where |q| <= 1e-3, C u B <= 1e-14."""
    q, e = np.abs(PR.to_f64(q)), C * float(PR.EPS53) * PR.to_f64(B)
    return (e <= CAP_PARTS * q) | ((q <= PARTS_NEAR_ZERO) & (e <= CAP_PARTS_ABS))


def _parts_reference(case, inp):
    if case.fam == LAT:
        return PR.lattice_parts(inp["x"], inp["z"], inp["order"], inp["coef"])
    return PR.net_parts(inp["x"], inp["z"], inp["order"], case.tbits)


@functools.lru_cache(maxsize=2)
def parts_reference(name):
    """(inputs, parts, B): x [n, d] a view of rows of stride d + 3 (lattice: fp64 in [0, 1); net: int64 below 2^t),
    z [d]; point 5 is z itself (distance 0).  Points that miss the parts' cap are drawn again (module docstring)."""
    case = PT_BY_NAME[name]
    g = PC._rng(27, case.fam, case.d, sum(case.orders), case.tbits, case.seed)
    n, d = case.n, case.d

    def draw(shape):
        return g.random(shape) if case.fam == LAT else g.integers(0, 2 ** case.tbits, shape, dtype=np.int64)

    full = draw((n, d + 3))
    z = draw(d)
    x = full[:, :d]
    x[5] = z
    if case.fam == LAT:
        order, coef = list(case.orders), [PC.lattice_coef(o // 2) for o in case.orders]
    else:
        order, coef = list(case.orders), None
    inp = dict(x_full=full, x=x, z=z, order=order, coef=coef)
    C = c_parts(case)
    for _ in range(50):
        P, B = _parts_reference(case, inp)
        bad = ~parts_cap_ok(C, P, B).T                  # [n, d]
        if not bad.any():
            break
        x[bad] = draw(int(bad.sum()))
    assert not bad.any() and (x[5] == z).all()
    return inp, P, B
