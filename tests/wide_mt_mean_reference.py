"""Extended-precision reference of the matrix-free multitask posterior mean (fgp_mt_wide_post_mean,
csrc/fgp_wide_mt.hip), an addition to tests/wide_mt_reference.py: one task pair's

  q[b, t] = beta out0[b, t] + w[b] sum_i K^{(g(b))}(xt[t], z[:, i]) coeffs[b, i],   g(b) = b (Gk == B) or 0 (Gk == 1),

evaluated in 80-bit arithmetic from the very fp64 / int64 arrays handed to the kernel -- the kernel rows K and their bounds
B_K are wide_mt_reference.mt_rows' --, with the first-order bound

  B_q[b, t] = |w[b]| sum_i (|K_i c_i| + B_K,i |c_i|)

such that a correct fp64 kernel satisfies |device - reference| <= C 2^-53 B_q (tests/wide_mt_mean_cases.py derives C).
The accumulate onto out0 is one rounding of out0 + v and adds nothing to B_q: the cases draw |out0| <= |w| sum_i |K_i c_i|,
so that rounding is at most 2^-53 2 |w| sum |K c| <= 2^-53 B_q / 5 (B_K >= d |K| and d >= 9: B_q >= 10 |w| sum |K c|)
and is counted as the one unit C has for it.
"""
import numpy as np

from tests import wide_mt_reference as MR
from tests.predict_reference import _x, _xs


def mt_post_mean(K, BK, coeffs, w=None, out0=None):
    """(q, B_q) [B, N] from extended kernel rows K and bounds BK [Gk, N, n] (mt_rows), fp64 coeffs [B, n], w [B] or None
    (1) and out0 [B, N] or None (beta = 0)."""
    c = _x(np.asarray(coeffs, dtype=np.float64))
    B, Gk = c.shape[0], K.shape[0]
    assert Gk in (1, B)
    q, bq = [], []
    for b in range(B):
        g = b if Gk == B else 0
        s = (K[g] * c[b][None, :]).sum(-1)
        bn = ((abs(K[g]) + BK[g]) * abs(c[b])[None, :]).sum(-1)
        if w is not None:
            s, bn = _xs(np.float64(w[b])) * s, abs(_xs(np.float64(w[b]))) * bn
        if out0 is not None:
            s = _x(np.asarray(out0[b], dtype=np.float64)) + s
        q.append(s)
        bq.append(bn)
    return np.stack(q), np.stack(bq)


def mt_post_mean_from_points(family, xt, z_dn, hyp, order, coef, add, ind, cc, tbits, coeffs, w=None, out0=None):
    """(q, B_q, K, B_K): the rows from the points (mt_rows), then mt_post_mean."""
    K, BK = MR.mt_rows(family, xt, z_dn, hyp, order, coef, add, ind, cc, tbits)
    q, bq = mt_post_mean(K, BK, coeffs, w, out0)
    return q, bq, K, BK
