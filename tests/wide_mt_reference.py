"""Extended-precision reference of the wide multitask kernels (csrc/fgp_wide_mt.hip), built on
tests/predict_reference.py: the definitions of include/fgp_hip.h evaluated in 80-bit arithmetic from the very fp64 /
int64 arrays handed to a kernel, each value q with a first-order bound B_q such that a correct fp64 kernel satisfies
|device - reference| <= C 2^-53 B_q (tests/wide_mt_cases.py derives C per entry point).

  K_ab(x, z) = scale sum_p cc[p] prod_j f_pj,   f_pj = ind[p][j] + l_j part[p][j](x, z)
  part = coef B_order((x_j - z_j) mod 1)  (lattice, orders 1..8),   coef (add + omega_order(x_j XOR z_j))  (net, 1..4)

mt_parts   parts [P, d, E] and bounds.  Lattice, even orders: |coef| (|B(t) - B(0)| + |B(0)|), the split at the constant
           term (predict_reference: the kernels evaluate even orders in u = t (t - 1)); odd orders are evaluated by
           Horner's rule in t, whose error is bounded by the magnitudes of the monomials, |coef| sum_k |c_k| t^(n - k)
           (an odd B_n vanishes at 0, 1/2 and 1, where no evaluation keeps a relative error).  Both plus the effect of
           the kernel's rounded distance, |coef B'(t)| (|x - z| + [x < z]), as predict_reference.lattice_parts.  Net:
           |coef| (|add| + B_omega), B_omega = 1 + 3 2^(floor(log2 delta) - t) (order 1) or W_a (orders 2..4).
combine    K [G, E] from parts: the bound of a factor is bf = ind + |l| B_part (B_part = |part| for a parts array read
           from memory), through the product to first order b_p = sum_j bf_j prod_{i != j} |f_i|, and
           B_K = |scale| sum_p |cc_p| b_p.  b_p >= d |prod_j f_pj|: the sum of the terms' magnitudes is at most B_K / d.
mt_k1_bwd  dscale [G] = sum_i u_i sum_p cc_p prod_j f_pj;  dls [G, d] = sum_i u_i scale sum_p cc_p part_pj
           prod_{j' != j} f_pj', the leave-one-out product formed as a product; bounds as predict_reference.k1_bwd, summed
           over p with |cc_p|.
"""
from fractions import Fraction as F

import numpy as np

from tests import predict_reference as PR
from tests.predict_reference import LAT, NET, XT, _floor, _pow2, _q, _x, _xs  # noqa: F401

# B_n(t) = sum_k c_k t^(n - k), the odd orders beside predict_reference.BERNOULLI's even ones
BERNOULLI = dict(PR.BERNOULLI)
BERNOULLI.update({
    1: [F(1), F(-1, 2)],
    3: [F(1), F(-3, 2), F(1, 2), F(0)],
    5: [F(1), F(-5, 2), F(5, 3), F(0), F(-1, 6), F(0)],
    7: [F(1), F(-7, 2), F(7, 2), F(0), F(-7, 6), F(0), F(1, 6), F(0)],
})


def bernoulli_terms(order, t):
    """(B_n(t) - B_n(0), B_n(0), B_n'(t), sum of the monomials' magnitudes) of extended t in [0, 1)."""
    c = BERNOULLI[int(order)]
    n = len(c) - 1
    top, der, mag = t * 0, t * 0, t * 0
    pw = t * 0 + 1
    for p in range(1, n + 1):
        ck = c[n - p]
        if ck != 0:
            der = der + _q(ck * p) * pw
        pw = pw * t
        if ck != 0:
            top = top + _q(ck) * pw
            mag = mag + abs(_q(ck)) * pw
    return top, _q(c[n]), der, mag + abs(_q(c[n]))


def mt_parts(family, x, z, order, coef, add, tbits=0, zip_pairs=False):
    """(parts, B) [P, d, E]: x [N, d], z [M, d] (fp64 lattice points / int64 net points; any row stride), order / coef /
    add [P][d]; E = N M (e = i M + k), or N with zip_pairs."""
    x, z = np.asarray(x), np.asarray(z)
    N, d = x.shape
    M = z.shape[0]
    P = len(order)
    ii, kk = (np.arange(N), np.arange(N)) if zip_pairs else [a.reshape(-1) for a in np.meshgrid(np.arange(N), np.arange(M), indexing="ij")]
    out = [[None] * d for _ in range(P)]
    bnd = [[None] * d for _ in range(P)]
    for j in range(d):
        memo = {}
        if family == LAT:
            xj, zj = x[ii, j].astype(np.float64), z[kk, j].astype(np.float64)
            diff = _x(xj) - _x(zj)
            dl = diff - _floor(diff)
            dist = abs(diff) + np.where(xj < zj, 1, 0)
        else:
            delta = x[ii, j].astype(np.uint64) ^ z[kk, j].astype(np.uint64)
        for p in range(P):
            o = int(order[p][j])
            c = _xs(np.float64(coef[p][j]))
            if family == LAT:
                if o not in memo:
                    memo[o] = bernoulli_terms(o, dl)
                top, b0, der, mag = memo[o]
                out[p][j] = c * (top + b0)
                bnd[p][j] = abs(c) * ((abs(top) + abs(b0)) if o % 2 == 0 else mag) + abs(c * der) * dist
            else:
                if o not in memo:
                    if o == 1:
                        w = np.where(delta != 0, 1, 0) * (3 * _pow2(PR.floor_log2(delta) - int(tbits)))
                        memo[o] = (1 - w, 1 + w)
                    else:
                        om = PR.walsh_omega(o, delta, int(tbits))
                        memo[o] = (om, om * 0 + _q(PR.WALSH_W[o]))
                om, bo = memo[o]
                a = _xs(np.float64(add[p][j]))
                out[p][j] = c * (a + om)
                bnd[p][j] = abs(c) * (abs(a) + bo)
    return np.stack([np.stack(r) for r in out]), np.stack([np.stack(r) for r in bnd])


def _factors(parts_p, bparts_p, ind_p, l):
    d = parts_p.shape[0]
    f = [int(ind_p[j]) + l[j] * parts_p[j] for j in range(d)]
    bf = [int(ind_p[j]) + abs(l[j]) * bparts_p[j] for j in range(d)]
    return f, bf


def combine(parts, bparts, ind, cc, scale, ls):
    """(K, B) [G, E] of extended parts [P, d, E] (bparts: their bounds, None = |parts|), ind [P][d], cc [P], scale [G],
    ls [G, d]."""
    parts = parts if parts.dtype != np.float64 else _x(parts)
    bparts = abs(parts) if bparts is None else bparts
    s, lsx, c = _x(np.asarray(scale, dtype=np.float64)), _x(np.asarray(ls, dtype=np.float64)), _x(np.asarray(cc, dtype=np.float64))
    K, B = [], []
    for g in range(s.shape[0]):
        k, b = 0, 0
        for p in range(parts.shape[0]):
            f, bf = _factors(parts[p], bparts[p], ind[p], lsx[g])
            kp, bp = PR._product(s[g] * c[p], f, bf)
            k, b = k + kp, b + bp
        K.append(k)
        B.append(b)
    return np.stack(K), np.stack(B)


def mt_k1(parts, ind, cc, scale, ls):
    """(k1, B) [G, n] of fp64 parts [P, d, n] (fgp_wide_mt_k1)."""
    return combine(_x(np.asarray(parts, dtype=np.float64)), None, ind, cc, scale, ls)


def mt_rows(family, xt, z_dn, hyp, order, coef, add, ind, cc, tbits=0, zip_pairs=False):
    """(K, B) [G, N, n] ([G, N] with zip_pairs) of fp64 test points xt [N, d], training points z_dn [d, n]
    dimension-major and hyp [G, 1 + d] (fgp_wide_mt_rows): the parts from the points, then combine."""
    xt = np.asarray(xt, dtype=np.float64)
    hyp = np.asarray(hyp, dtype=np.float64).reshape(-1, 1 + xt.shape[1])
    x = xt if family == LAT else PR.net_bits(xt, tbits).astype(np.int64)
    z = np.ascontiguousarray(np.asarray(z_dn).T)
    parts, bparts = mt_parts(family, x, z, order, coef, add, tbits, zip_pairs)
    K, B = combine(parts, bparts, ind, cc, hyp[:, 0], hyp[:, 1:])
    if zip_pairs:
        return K, B
    shape = (hyp.shape[0], xt.shape[0], z.shape[0])
    return K.reshape(shape), B.reshape(shape)


def mt_k1_bwd(parts, ind, cc, scale, ls, u):
    """(dscale [G], B [G], dls [G, d], B [G, d]) of fp64 parts [P, d, n] and u [G, n] (fgp_wide_mt_k1_bwd)."""
    pa = _x(np.asarray(parts, dtype=np.float64))
    P, d, n = pa.shape
    s, lsx = _x(np.asarray(scale, dtype=np.float64)), _x(np.asarray(ls, dtype=np.float64))
    c, uu = _x(np.asarray(cc, dtype=np.float64)), _x(np.asarray(u, dtype=np.float64))
    ds, Bs, dl, Bl = [], [], [], []
    for g in range(s.shape[0]):
        dsg, Bsg = 0, 0
        row, brow = [0] * d, [0] * d
        for p in range(P):
            f, bf = _factors(pa[p], abs(pa[p]), ind[p], lsx[g])
            af = [abs(v) for v in f]
            k, b = PR._product(c[p], f, bf)
            dsg, Bsg = dsg + (uu[g] * k).sum(), Bsg + (abs(uu[g]) * b).sum()
            one, zero = f[0] * 0 + 1, f[0] * 0
            sv, sb, sval = [one] * (d + 1), [zero] * (d + 1), [one] * (d + 1)
            for j in range(d - 1, -1, -1):
                sval[j] = sval[j + 1] * f[j]
                sb[j] = sb[j + 1] * af[j] + bf[j] * sv[j + 1]
                sv[j] = sv[j + 1] * af[j]
            pval, pv, pb = one, one, zero
            for j in range(d):
                w = uu[g] * s[g] * c[p] * pa[p][j]
                row[j] = row[j] + (w * (pval * sval[j + 1])).sum()
                brow[j] = brow[j] + (abs(w) * (pb * sv[j + 1] + pv * sb[j + 1] + pv * sv[j + 1])).sum()
                pval = pval * f[j]
                pb = pb * af[j] + bf[j] * pv
                pv = pv * af[j]
        ds.append(dsg)
        Bs.append(Bsg)
        dl.append(np.stack(row))
        Bl.append(np.stack(brow))
    return np.stack(ds), np.stack(Bs), np.stack(dl), np.stack(Bl)
