"""Extended-precision reference of the multitask quadratic form (fgp_mt_quadform) and its error bound.

    q[b] = sum_j sum_r |w_{b,r,j}|^2 / D_{g,r,j},   w_b = L_g^-1 v[b],   g = b mod G,

with L D L^H the structured factor of fgp_mt_factor in the packed layout of the lams (include/fgp_hip.h: the T active
tasks sorted by n descending, nmin = n[T-1] frequency classes, R = sum n_k / nmin rows per class, pair (k, l), k <= l,
holds n_k values, value q nmin + j coupling row (k, q) with row (l, q mod (n_l / nmin)) in class j).

`quadform_ref` restates the kernel's forward substitution and sums in numpy longdouble (64-bit significand), taking the
FACTOR AS THE DEVICE PRODUCED IT and the vectors as exact inputs.  `ldl_factor` is a plain float64 restatement of the
LDL^H recurrence of fgp_multitask.hip's header comment, for the CPU comparison against the oracle's dense blocks.

The bound.  u = 2^-53.  The kernel (compiled without contraction) does, per class and vector:

  * forward substitution, a row of task l receiving m_l = sum_{k < l} n_k / n_l updates t <- t - conj(c) w_q:
    the complex product is two components of fma(a, b, fl(c d)), 2 roundings each, so it is off by at most
    2 sqrt(2) u |c| |w_q| < 3 u |c| |w_q| in modulus; each subtraction rounds once, the first operand passing through all
    m_l of them.  With wbar the same substitution on absolute values (wbar_r = |v_r| + sum |c| wbar_q) and the rows a row
    depends on being off by at most c_q u wbar_q, row r of task l is off by at most (m_l + 3 + max c_q) u wbar_r, the
    chain running through every earlier task:  c_w = sum_{l = 1}^{T-1} (m_l + 3).  (The net path's real product rounds
    once; the complex count covers it.)
  * the term |w|^2 / D:  | |w^|^2 - |w|^2 | <= 2 c_w u wbar^2;  fma(x, x, fl(y y)) 2 roundings of positive terms, 1 / D
    one, the product one:  (2 c_w + 4) u wbar^2 / |D| per term.
  * the sum over the R rows of a class in ascending order: R - 1 additions (the first lands on 0 exactly);
  * the workgroup's sum over its 256 classes: 6 butterfly additions and 4 over the waves (the first onto 0): 10;
  * the second level over nblk = ceil(nmin / 256) partials: ceil(nblk / 256) strided additions per thread, then the
    same 10.

  C = 2 c_w + 4 + (R - 1) + 10 + ceil(nblk / 256) + 10,      |device - reference| <= gamma_C B_q,
  gamma_C = C u / (1 - C u),      B_q = sum_j sum_r wbar_rj^2 / |D_rj|

(first order in u made rigorous by gamma_C as usual; the reference's own rounding, the same count at 2^-64, is added).
Nothing here is fitted to what the device returns.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53
KWG = 256


class Layout(object):
    """The packed block layout of sorted active task sizes `ns` (descending powers of two)."""

    def __init__(self, ns):
        self.ns = [int(v) for v in ns]
        assert all(v >= 1 and v & (v - 1) == 0 for v in self.ns) and self.ns == sorted(self.ns, reverse=True)
        self.T = len(self.ns)
        self.nmin = self.ns[-1]
        self.q = [v // self.nmin for v in self.ns]
        self.R = sum(self.q)
        self.rs = [sum(self.q[:k]) for k in range(self.T)]
        self.off = {}
        L = 0
        for k in range(self.T):
            for l in range(k, self.T):
                self.off[k, l] = L
                L += self.ns[k]
        self.L = L

    def seg(self, a, k, l):
        """View [q_k, nmin] of pair (k, l) in the packed array a [L]."""
        o = self.off[k, l]
        return a[o:o + self.ns[k]].reshape(self.q[k], self.nmin)


def pack_blocks(Lam, ns):
    """Dense Hermitian blocks Lam [R, R, nmin] (rows in sorted task order) -> packed lams [L] complex128."""
    lay = Layout(ns)
    out = np.zeros(lay.L, dtype=np.complex128)
    for k in range(lay.T):
        for l in range(k, lay.T):
            s = lay.seg(out, k, l)
            for q in range(lay.q[k]):
                s[q] = Lam[lay.rs[k] + q, lay.rs[l] + q % lay.q[l]]
    return out


def ldl_factor(lams, ns):
    """Structured LDL^H of one problem's packed lams [L] (float64 arithmetic, every class at once):
        D_k[q] = Lambda[(k,q),(k,q)] after the updates of the earlier tasks,   u_kl[q] = c_kl[q] / D_k[q],
        Lambda[(l,p),(m,p mod q_m)] -= conj(u_kl[q]) c_km[q]  for q mod q_l = p,  k < l <= m;
    D on the diagonal pairs, u on the coupling pairs."""
    lay = Layout(ns)
    F = np.array(lams, dtype=np.complex128).copy()
    for k in range(lay.T):
        Dk = lay.seg(F, k, k)
        for q in range(lay.q[k]):
            dq = Dk[q].real.copy()
            Dk[q] = dq
            for l in range(k + 1, lay.T):
                ul = lay.seg(F, k, l)[q] / dq
                for m in range(l, lay.T):
                    lay.seg(F, l, m)[q % lay.q[l]] -= np.conj(ul) * lay.seg(F, k, m)[q]
            for l in range(k + 1, lay.T):
                lay.seg(F, k, l)[q] = lay.seg(F, k, l)[q] / dq
    return F


def quadform_ref(fac, ns, v, G=1):
    """(q [B], B_q [B]) in longdouble: fac [G, L] complex128, v [B, R nmin] complex128 or float64 (the real form:
    the real parts of the couplings), vector b against problem b mod G."""
    lay = Layout(ns)
    fac = np.asarray(fac).reshape(G, lay.L)
    v = np.asarray(v)
    B = v.shape[0]
    assert v.shape[1] == lay.R * lay.nmin and B % G == 0
    real = not np.iscomplexobj(v)
    g = np.arange(B) % G
    w = v.astype(LD if real else CLD).reshape(B, lay.R, lay.nmin).copy()
    wa = np.abs(v).astype(LD).reshape(B, lay.R, lay.nmin)
    q = np.zeros(B, dtype=LD)
    bq = np.zeros(B, dtype=LD)
    for k in range(lay.T):
        for qq in range(lay.q[k]):
            r = lay.rs[k] + qq
            o = lay.off[k, k] + qq * lay.nmin
            D = fac[g, o:o + lay.nmin].real.astype(LD)
            wr = w[:, r]
            a2 = wr * wr if real else wr.real * wr.real + wr.imag * wr.imag
            q += (a2 / D).sum(-1)
            bq += (wa[:, r] * wa[:, r] / np.abs(D)).sum(-1)
            for l in range(k + 1, lay.T):
                o = lay.off[k, l] + qq * lay.nmin
                c = fac[g, o:o + lay.nmin]
                rl = lay.rs[l] + qq % lay.q[l]
                if real:
                    c = c.real.astype(LD)
                    w[:, rl] -= c * wr
                else:
                    c = c.astype(CLD)
                    w[:, rl] -= np.conj(c) * wr
                wa[:, rl] += np.abs(c).astype(LD) * wa[:, r]
    return q, bq


def bound_count(ns):
    """C of the module docstring for sorted active sizes ns."""
    lay = Layout(ns)
    cw = sum(sum(lay.q[k] for k in range(l)) // lay.q[l] + 3 for l in range(1, lay.T))
    nblk = -(-lay.nmin // KWG)
    return 2 * cw + 4 + (lay.R - 1) + 10 + -(-nblk // KWG) + 10


def bound(ns, bq):
    """|device - reference| <= this, elementwise over B_q."""
    C = bound_count(ns)
    return (C * U / (1.0 - C * U) + C * 2.0 ** -64) * np.asarray(bq, dtype=LD)
