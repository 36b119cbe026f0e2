"""Extended-precision reference of the multitask block kernels (fgp_mt_factor, fgp_mt_solve, fgp_mt_selinv,
fgp_mt_mll_grad) and of the three non-block stages of fgp_mt_fit_run (k_mtg_lams, k_mtg_contract + k_mtg_reduce,
k_mtg_step), each with an error bound counted from the kernel's own roundings.

Every stage takes its inputs EXACTLY AS THE DEVICE PRODUCED the previous stage's outputs (the factor for the solve and the
selected inverse, the solutions and the selected inverse for the gradient, glp / z / logdet for the contraction, the totals
for the step), so no conditioning enters a bound: the only disagreement left is the rounding of the stage itself.

How a bound is formed.  u = 2^-53.  A tracked quantity (class Tr) carries its value v in extended precision (numpy
longdouble, 64-bit significand; mpmath at 40 digits where the platform's long double is no wider than a double) and a
twin e >= 0 such that |device - v| <= u e to first order.  The twin is a magnitude: a sum of absolute values of the
intermediate results, one per rounding the kernel commits, each carried to the output through the absolute values of the
factors it then meets -- the `wbar` of tests/mt_qf_reference.py with the counts folded in operation by operation
instead of taken at their maximum.  The library is compiled with -ffp-contract=off, so per device operation:

    a + b, a - b, a * b        one rounding:   e = (propagated) + |v|
    a * b + c written plainly  two roundings:  the product's and the sum's (add(mul(a, b), c))
    __builtin_fma(a, b, c)     one rounding:   e = |a| e_b + |b| e_a + e_c + |v|
    1 / a, sqrt(a)             correctly rounded: e = e_a / a^2 + |v|,  e_a / (2 sqrt a) + |v|
    exp(a), log(a)             ULP_LIBM ulp = 2 ULP_LIBM u relative: e = |v| e_a + 2 ULP_LIBM |v|, e_a / |a| + 2 ULP_LIBM |v|
    -a, 2 a, 0.5 a, 0 + a, 1 a exact

    cmul(a, b)    = (fma(a.x, b.x, -(a.y b.y)), fma(a.x, b.y,   a.y b.x))      fgp_common.h: two roundings per component
    cmulc(a, w)   = (fma(a.x, w.x,   a.y w.y ), fma(a.y, w.x, -(a.x w.y)))     a conj(w)
    cmul_cj(a, b) = (fma(a.x, b.x,   a.y b.y ), fma(a.x, b.y, -(a.y b.x)))     conj(a) b   (fgp_multitask.hip)
    double2 * s   = (a.x s, a.y s),   double2 -= double2 componentwise

The propagated part is first order in u.  It is made rigorous the usual way, by gamma_C = C u / (1 - C u) in place of C u:
along any chain of operations from an input to an output at most C roundings are met, so the neglected products of
errors are below the factor 1 / (1 - C u) on the twin.  C is the length of the longest chain of the stage:

  factor   a pivot of the last task has received m = sum_{k < T-1} n_k / n_{T-1} <= R updates, each 3 roundings (two of
           cmul_cj, one subtraction) from a coupling that carries its own chain through the earlier tasks (T of them) and
           2 more (1 / D and the scaling):  C_factor = (3 + 2) R T.  logdet adds R additions and the logarithms.
  solve    forward: a row receives <= R updates of 3 roundings from rows with their own chains through T tasks; the
           scaling 2; back: T updates of 3 each, through T tasks:  C_solve = 3 R T + 2 + 3 T^2.
  selinv   a coupling entry: T terms of 3 roundings, through T tasks; the diagonal 1 / D and T terms of 3:
           C_selinv = 3 T^2 + 3 T + 1.
  grad     per entry cmulc (2), B / G fmas, one fma, exact doubling:  C_grad = B / G + 3.
  lams     exp (2 ULP_LIBM), d products, 2^d fmas, sqrt, 3 products, the nugget's ~2^d + 8, K_task's 2 rank + 1 + exp:
           C_lams = 2^(d+1) + d + 2 rank + 8 ULP_LIBM + 16.
  contract C_lams for the entry's factors, 2^d fmas of the derivative sums, 6 per term, ceil(L / (256 nblk)) strided
           fmas, 10 of block_sum (6 butterfly additions, 4 waves), ceil(nblk / 256) + 10 of k_mtg_reduce:
           C_contract = C_lams + 2^d + ceil(max(L, B R nmin) / (256 nblk)) + ceil(max(nblk, n_0) / 256) + 32.
  step     G additions per total, 3 for the loss; an element: <= G T (T + 1) terms of 2 roundings, exp:
           C_step = 2 G T (T + 1) + 2 ULP_LIBM + G + 4.

These C only feed the second-order factor 1 / (1 - C u) (C u < 1e-9 for every shape here); the first-order count of each
output element is in its twin.  The reference's own rounding, the same twin at 2^-64 per operation (2^-63 taken), is
added:     |device - reference| <= (u / (1 - C u) + 2^-63) e.       Nothing is fitted to what the device returns.

exp and log.  The accuracy of the device math library's double-precision exp and log could not be confirmed from a
document or header of the ROCm installation the suite was written against (its only statement on ulps, clang's
opencl-c.h, concerns OpenCL's half_ and native_ functions), so the fallback allowance is used: ULP_LIBM = 2 ulp.
sqrt and division count as correctly rounded.  log enters only logdet (an absolute 2 ULP_LIBM u |log| per row).

Sums over a workgroup follow block_sum (fgp_common.h) and k_mtg_reduce: the thread's strided sum in ascending order, six
butterfly additions (lane i with lane i ^ 32, 16, ..., 1), then the four waves added in order onto 0.

Every *_ref takes xt (the arithmetic: XT, or np.float64 for the plain restatement the CPU tests hold against the bound)
and `mutate`, one of the three seeded defects the CPU tests must see break a bound:
    "noconj"  the factor's update multiplies u_kl c_km without the conjugate,
    "qmod"    the factor's update lands on row q mod q_m of block (l, m) instead of q mod q_l,
    "nofac2"  the coupling gradient is not doubled.
"""
import numpy as np

from tests.mt_qf_reference import Layout, pack_blocks  # noqa: F401  (re-exported: the cases and tests take them here)

U = 2.0 ** -53
ULP_LIBM = 2                      # ulps allowed to the device exp / log (see the docstring)
KWG = 256
KMTGQ = 4 + 8                     # kMtgQ = 4 + FGP_MAX_D: the stride of a workgroup's partials

if np.finfo(np.longdouble).eps < 2e-19:
    MP = False
    XT = np.longdouble
    _ufn = {"log": np.log, "exp": np.exp, "sqrt": np.sqrt}
else:                             # long double == double: mpmath, 40 digits, in object arrays
    import mpmath
    MP = True
    mpmath.mp.dps = 40
    XT = object
    _ufn = {k: np.frompyfunc(getattr(mpmath, k), 1, 1) for k in ("log", "exp", "sqrt")}
    _tomp = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)


def _conv(a, xt):
    a = np.asarray(a)
    if xt is object:
        return _tomp(a.astype(np.float64))
    return a.astype(xt)


def _fn(name, a, xt):
    return _ufn[name](a) if xt is object else getattr(np, name)(a)


class Tr(object):
    """A tracked real array: value v and twin e (|device - v| <= u e to first order), both of dtype xt."""
    __slots__ = ("v", "e", "xt")

    def __init__(self, v, e=None, xt=None):
        self.xt = xt if xt is not None else (v.dtype.type if v.dtype != object else object)
        self.v = v
        self.e = e if e is not None else np.zeros(np.shape(v), dtype=self.xt) if self.xt is not object else _conv(
            np.zeros(np.shape(v)), object)

    @staticmethod
    def exact(a, xt=XT):
        return Tr(_conv(a, xt), None, xt)

    def _w(self, o):
        return o if isinstance(o, Tr) else Tr.exact(np.asarray(o, dtype=np.float64), self.xt)

    def __getitem__(self, i):
        return Tr(self.v[i], self.e[i], self.xt)

    def __setitem__(self, i, o):
        self.v[i] = o.v
        self.e[i] = o.e

    def copy(self):
        return Tr(self.v.copy(), self.e.copy(), self.xt)

    def __neg__(self):
        return Tr(-self.v, self.e, self.xt)

    def __add__(self, o):
        o = self._w(o)
        v = self.v + o.v
        return Tr(v, self.e + o.e + abs(v), self.xt)

    def __sub__(self, o):
        o = self._w(o)
        v = self.v - o.v
        return Tr(v, self.e + o.e + abs(v), self.xt)

    def __mul__(self, o):
        o = self._w(o)
        v = self.v * o.v
        return Tr(v, abs(self.v) * o.e + abs(o.v) * self.e + abs(v), self.xt)

    def scaled(self, c):
        """Times a power of two: exact."""
        return Tr(self.v * c, self.e * abs(c), self.xt)

    def inv(self):
        v = 1 / self.v
        return Tr(v, self.e * (v * v) + abs(v), self.xt)

    def div(self, o):
        v = self.v / o.v
        return Tr(v, self.e / abs(o.v) + abs(v) * o.e / abs(o.v) + abs(v), self.xt)

    def sqrt(self):
        v = _fn("sqrt", self.v, self.xt)
        return Tr(v, self.e / (2 * v) + abs(v), self.xt)

    def exp(self):
        v = _fn("exp", self.v, self.xt)
        return Tr(v, v * self.e + 2 * ULP_LIBM * v, self.xt)

    def logabs(self):
        a = abs(self.v)
        v = _fn("log", a, self.xt)
        return Tr(v, self.e / a + 2 * ULP_LIBM * abs(v), self.xt)

    def where(self, mask, o):
        """self where mask, else o."""
        return Tr(np.where(mask, self.v, o.v), np.where(mask, self.e, o.e), self.xt)


def fma(a, b, c):
    """One rounding.  In the float64 restatement the product and the sum are formed in long double and rounded to double
    once more (within u (1 + 2^-10) of the single rounding; a plain a * b + c would round twice and is not what the
    kernels do)."""
    if a.xt is np.float64 and not MP:
        ld = np.longdouble
        v = (np.asarray(a.v, dtype=ld) * np.asarray(b.v, dtype=ld) + np.asarray(c.v, dtype=ld)).astype(np.float64)
    else:
        v = a.v * b.v + c.v
    return Tr(v, abs(a.v) * b.e + abs(b.v) * a.e + c.e + abs(v), a.xt)


class Cx(object):
    """A tracked complex array: components x, y."""
    __slots__ = ("x", "y")

    def __init__(self, x, y):
        self.x, self.y = x, y

    @staticmethod
    def exact(a, xt=XT):
        a = np.asarray(a)
        return Cx(Tr.exact(a.real, xt), Tr.exact(a.imag if np.iscomplexobj(a) else np.zeros(a.shape), xt))

    def __getitem__(self, i):
        return Cx(self.x[i], self.y[i])

    def __setitem__(self, i, o):
        self.x[i] = o.x
        self.y[i] = o.y

    def __sub__(self, o):
        return Cx(self.x - o.x, self.y - o.y)

    def times(self, s):
        return Cx(self.x * s, self.y * s)

    def value(self):
        return self.x.v.astype(np.float64) + 1j * self.y.v.astype(np.float64)

    def err(self):
        """The twin of the modulus: |device - v| <= u hypot(e_x, e_y) <= u (e_x + e_y); per component e_x, e_y."""
        return self.x.e, self.y.e


def cmul(a, b):
    return Cx(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x))


def cmulc(a, w):
    return Cx(fma(a.x, w.x, a.y * w.y), fma(a.y, w.x, -(a.x * w.y)))


def cmul_cj(a, b):
    return Cx(fma(a.x, b.x, a.y * b.y), fma(a.x, b.y, -(a.y * b.x)))


def _zero(shape, xt):
    return Tr.exact(np.zeros(shape), xt)


def bound(e, C):
    """|device - reference| <= this, elementwise over the twin e."""
    assert C * U < 1e-6
    return (U / (1.0 - C * U) + 2.0 ** -63) * e


def counts(ns, B=1, G=1, d=1, rank=0, nblk=1):
    """The chain lengths C of the module docstring."""
    lay = Layout(ns)
    R, T = lay.R, lay.T
    c_lams = 2 ** (d + 1) + d + 2 * rank + 8 * ULP_LIBM + 16
    return {
        "factor": 5 * R * T + R + 2 * ULP_LIBM,
        "solve": 3 * R * T + 2 + 3 * T * T,
        "selinv": 3 * T * T + 3 * T + 1,
        "grad": B // G + 3,
        "lams": c_lams,
        "contract": c_lams + 2 ** d + -(-max(lay.L, B * R * lay.nmin) // (KWG * nblk)) + -(-max(nblk, lay.ns[0]) // KWG) + 32,
        "step": 2 * G * T * (T + 1) + 2 * ULP_LIBM + G + 4,
    }


# ------------------------------------------------------------------------------------------------ block stages
def _rows(a, lay, G):
    """packed [G, L] -> [G, E, nmin] (E = L / nmin rows: pair (k, l)'s row q at off[k, l] / nmin + q)."""
    return np.asarray(a).reshape(G, lay.L // lay.nmin, lay.nmin)


def _unrows(c, lay, G):
    return c.value().reshape(G, lay.L), c.x.e.reshape(G, lay.L), c.y.e.reshape(G, lay.L)


def factor_ref(lams, ns, G=1, xt=XT, mutate=None):
    """mt_ldl_class.  lams [G, L] complex128 -> dict: fac [G, L] complex128 (the reference rounded to double),
    fac_x / fac_y [G, L] xt (its components unrounded), ex / ey [G, L] (the components' twins), logdet / logdet_e
    [G, nmin], bad [G, nmin] (a pivot not > 0), info (any bad)."""
    lay = Layout(ns)
    F = Cx.exact(_rows(lams, lay, G), xt)
    F = Cx(F.x.copy(), F.y.copy())
    o = {kl: v // lay.nmin for kl, v in lay.off.items()}
    ld = None
    bad = np.zeros((G, lay.nmin), dtype=bool)
    for k in range(lay.T):
        for q in range(lay.q[k]):
            dq = F.x[:, o[k, k] + q]
            bad |= ~(dq.v > 0)
            lg = dq.logabs()
            ld = lg if ld is None else ld + lg
            F.y[:, o[k, k] + q] = _zero((G, lay.nmin), xt)
            idq = dq.inv()
            for l in range(k + 1, lay.T):
                ul = F[:, o[k, l] + q].times(idq)
                for m in range(l, lay.T):
                    cm = F[:, o[k, m] + q]
                    row = o[l, m] + (q % lay.q[m] if mutate == "qmod" else q % lay.q[l])
                    F[:, row] = F[:, row] - (cmul(ul, cm) if mutate == "noconj" else cmul_cj(ul, cm))
            for l in range(k + 1, lay.T):
                F[:, o[k, l] + q] = F[:, o[k, l] + q].times(idq)
    fac, ex, ey = _unrows(F, lay, G)
    return {"fac": fac, "fac_x": F.x.v.reshape(G, lay.L), "fac_y": F.y.v.reshape(G, lay.L), "ex": ex, "ey": ey,
            "logdet": ld.v, "logdet_e": ld.e, "bad": bad, "info": int(bad.any())}


def solve_ref(fac, ns, v, G=1, xt=XT):
    """mt_solve_class.  fac [G, L] (as the device produced it), v [B, R nmin] complex128, vector b against problem
    b mod G -> (z_x, z_y, ex, ey), each [B, R nmin] xt."""
    lay = Layout(ns)
    v = np.asarray(v)
    B = v.shape[0]
    g = np.arange(B) % G
    F = Cx.exact(_rows(fac, lay, G)[g], xt)
    w = Cx.exact(v.reshape(B, lay.R, lay.nmin), xt)
    w = Cx(w.x.copy(), w.y.copy())
    o = {kl: val // lay.nmin for kl, val in lay.off.items()}
    for k in range(lay.T):
        for q in range(lay.q[k]):
            wq = w[:, lay.rs[k] + q]
            for l in range(k + 1, lay.T):
                r = lay.rs[l] + q % lay.q[l]
                w[:, r] = w[:, r] - cmul_cj(F[:, o[k, l] + q], wq)
    for k in range(lay.T):
        for q in range(lay.q[k]):
            r = lay.rs[k] + q
            w[:, r] = w[:, r].times(F.x[:, o[k, k] + q].inv())
    for k in range(lay.T - 1, -1, -1):
        for q in range(lay.q[k]):
            s = w[:, lay.rs[k] + q]
            for l in range(k + 1, lay.T):
                s = s - cmul(F[:, o[k, l] + q], w[:, lay.rs[l] + q % lay.q[l]])
            w[:, lay.rs[k] + q] = s
    n = lay.R * lay.nmin
    return w.x.v.reshape(B, n), w.y.v.reshape(B, n), w.x.e.reshape(B, n), w.y.e.reshape(B, n)


def selinv_ref(fac, ns, G=1, xt=XT):
    """mt_selinv_class.  fac [G, L] -> (z_x, z_y, ex, ey) [G, L]: the inverse's entries on the coupling pattern."""
    lay = Layout(ns)
    F = Cx.exact(_rows(fac, lay, G), xt)
    E = lay.L // lay.nmin
    Z = Cx(_zero((G, E, lay.nmin), xt), _zero((G, E, lay.nmin), xt))
    o = {kl: val // lay.nmin for kl, val in lay.off.items()}

    def zpat(l, pl, m, pm):
        if l <= m:
            return Z[:, o[l, m] + pl]
        z = Z[:, o[m, l] + pm]
        return Cx(z.x, -z.y)

    for k in range(lay.T - 1, -1, -1):
        for q in range(lay.q[k]):
            for m in range(k + 1, lay.T):
                s = None
                for l in range(k + 1, lay.T):
                    t = cmul(F[:, o[k, l] + q], zpat(l, q % lay.q[l], m, q % lay.q[m]))
                    s = Cx(-t.x, -t.y) if s is None else s - t          # 0 - t: exact
                Z[:, o[k, m] + q] = s
            s = F.x[:, o[k, k] + q].inv()
            for l in range(k + 1, lay.T):
                u, zc = F[:, o[k, l] + q], Z[:, o[k, l] + q]
                s = s - fma(u.x, zc.x, u.y * zc.y)
            Z[:, o[k, k] + q] = Cx(s, _zero((G, lay.nmin), xt))
    return (Z.x.v.reshape(G, lay.L), Z.y.v.reshape(G, lay.L), Z.x.e.reshape(G, lay.L), Z.y.e.reshape(G, lay.L))


def grad_ref(zinv, z, gn, gl, ns, B, G=1, xt=XT, mutate=None):
    """mt_grad_class.  zinv [G, L], z [B, R nmin] (both as the device produced them), gn [B], gl [G] ->
    (g_x, g_y, ex, ey) [G, L]."""
    lay = Layout(ns)
    Z = Cx.exact(_rows(zinv, lay, G), xt)
    zz = Cx.exact(np.asarray(z).reshape(B, lay.R, lay.nmin), xt)
    gn = Tr.exact(np.asarray(gn, dtype=np.float64).reshape(B, 1), xt)
    glg = Tr.exact(np.asarray(gl, dtype=np.float64).reshape(G, 1), xt)
    E = lay.L // lay.nmin
    out = Cx(_zero((G, E, lay.nmin), xt), _zero((G, E, lay.nmin), xt))
    o = {kl: val // lay.nmin for kl, val in lay.off.items()}
    for (k, l), ok in o.items():
        for q in range(lay.q[k]):
            r, c = lay.rs[k] + q, lay.rs[l] + q % lay.q[l]
            wx, wy = _zero((G, lay.nmin), xt), _zero((G, lay.nmin), xt)
            for i in range(B // G):
                bs = slice(i * G, (i + 1) * G)               # vectors b = g + i G of every problem g
                p = cmulc(zz[bs, r], zz[bs, c])
                wx, wy = fma(gn[bs], p.x, wx), fma(gn[bs], p.y, wy)
            a = Z[:, ok + q]
            if r == c:
                out[:, ok + q] = Cx(fma(glg, a.x, -wx), _zero((G, lay.nmin), xt))
            else:
                s = 1.0 if mutate == "nofac2" else 2.0
                out[:, ok + q] = Cx(fma(glg, a.x, -wx).scaled(s), fma(glg, a.y, -wy).scaled(s))
    return (out.x.v.reshape(G, lay.L), out.y.v.reshape(G, lay.L), out.x.e.reshape(G, lay.L), out.y.e.reshape(G, lay.L))


def dense_blocks(lams, ns):
    """One problem's packed lams [L] -> the dense Hermitian class blocks [nmin, R, R] complex128."""
    lay = Layout(ns)
    dense = np.zeros((lay.nmin, lay.R, lay.R), dtype=np.complex128)
    for (k, l) in lay.off:
        s = lay.seg(np.asarray(lams), k, l)
        for q in range(lay.q[k]):
            r, c = lay.rs[k] + q, lay.rs[l] + q % lay.q[l]
            if k == l:
                dense[:, r, r] = s[q].real
            else:
                dense[:, r, c] = s[q]
                dense[:, c, r] = np.conj(s[q])
    return dense


# ------------------------------------------------------------------------------------------------ fit stages
class FitSpec(object):
    """The host-side description of one fgp_mt_fit_run problem (tests/mt_fit_cases.py builds it; the fields are those of
    fgp_mt_fit_desc): ns, d, dl, B, G, task [T], T_all, rank, vtask_exp, rows [5, G] int, nrows [5], spectra (list over
    the sorted pairs of [2^d, n_k] complex128), y [G, B, R nmin] complex128, nug_coef ([T, 2^d] complex128 or None),
    nug_ref, grad_norm, grad_logdet, logdet_weight, mll_const."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.lay = Layout(self.ns)
        T = self.lay.T
        self.P = T * (T + 1) // 2
        nr = [max(1, int(v)) for v in self.nrows]
        self.l_off = nr[0]
        self.n_off = self.l_off + nr[1] * self.dl
        self.f_off = self.n_off + nr[2]
        self.v_off = self.f_off + nr[3] * self.T_all * self.rank
        self.n_params = self.v_off + nr[4] * self.T_all
        lay = self.lay
        cover = max(lay.L, self.B * lay.R * lay.nmin, lay.nmin)
        self.nblk = min(1024, -(-cover // KWG))
        self.pairs = [(k, l) for k in range(T) for l in range(k, T)]

    def i_s(self, g):
        return int(self.rows[0][g])

    def i_l(self, g, j):
        return self.l_off + int(self.rows[1][g]) * self.dl + (j if self.dl > 1 else 0)

    def i_n(self, g):
        return self.n_off + int(self.rows[2][g])

    def i_f(self, g):
        return self.f_off + int(self.rows[3][g]) * self.T_all * self.rank

    def i_v(self, g):
        return self.v_off + int(self.rows[4][g]) * self.T_all

    def counts(self):
        return counts(self.ns, self.B, 1, self.d, self.rank, self.nblk)

    def class_lds(self):
        """mtc_lds: the LDS bytes of the wave-per-class kernel (the class's entries, its selected inverse, its B vectors,
        log|pivot| and 1 / pivot per row), 0 where they exceed its 60 KB."""
        b = (2 * (self.lay.L // self.lay.nmin) + self.B * self.lay.R) * 16 + self.lay.R * 16
        return b if b <= 60 * 1024 else 0


def _fill(t, n):
    """A tracked scalar repeated n times."""
    return Tr(np.broadcast_to(t.v, (n,)).copy(), np.broadcast_to(t.e, (n,)).copy(), t.xt)


def _scalar(v, xt):
    return Tr.exact(np.asarray(float(v)).reshape(()), xt)


def _ktask(fs, raw, g, a, b, xt):
    """mtg_kt: sum_r F[a, r] F[b, r] (a product and an addition each, the first onto 0) + [a == b] v_a."""
    fo, vo = fs.i_f(g), fs.i_v(g)
    s = _scalar(0.0, xt)
    for r in range(fs.rank):
        t = _scalar(raw[fo + a * fs.rank + r], xt) * _scalar(raw[fo + b * fs.rank + r], xt)
        s = t if r == 0 else s + t
    if a == b:
        va = _scalar(raw[vo + a], xt)
        va = va.exp() if fs.vtask_exp else va
        s = va if fs.rank == 0 else s + va
    return s


def _lpow(fs, raw, g, xt):
    """mtg_lpow: l^S, the product over the set bits of S in ascending j (1 l = l exactly)."""
    ls = [_scalar(raw[fs.i_l(g, j)], xt).exp() for j in range(fs.d)]
    out = []
    for S in range(1 << fs.d):
        w = None
        for j in range(fs.d):
            if (S >> j) & 1:
                w = ls[j] if w is None else w * ls[j]
        out.append(_scalar(1.0, xt) if w is None else w)
    return out


def _poly(fs, p, lpow, xt, der):
    """mtg_poly of every entry of pair p: P = sum_S l^S Phi_S (fma per term, ascending S; 0 + first rounds once) and
    dp[j] over the S that contain j."""
    ph = Cx.exact(fs.spectra[p], xt)
    n = fs.spectra[p].shape[1]
    P = Cx(_zero(n, xt), _zero(n, xt))
    dp = [Cx(_zero(n, xt), _zero(n, xt)) for _ in range(fs.d if der else 0)]
    for S in range(1 << fs.d):
        f, w = ph[S], lpow[S]
        P = Cx(fma(w, f.x, P.x), fma(w, f.y, P.y))
        for j in range(len(dp)):
            if (S >> j) & 1:
                dp[j] = Cx(fma(w, f.x, dp[j].x), fma(w, f.y, dp[j].y))
    return P, dp


def _nug_ratio(fs, k, lpow, xt, der):
    """mtg_nug_ratio: r = |A_k| / |A_ref| and dr[j] = r (Re(conj(A_k) A_kj) / |A_k|^2 - the same of ref)."""
    A, Aj = [], []
    for kk in (k, fs.nug_ref):
        c = Cx.exact(fs.nug_coef[kk], xt)
        a = Cx(_scalar(0.0, xt), _scalar(0.0, xt))
        aj = [Cx(_scalar(0.0, xt), _scalar(0.0, xt)) for _ in range(fs.d if der else 0)]
        for S in range(1 << fs.d):
            cs = c[S]
            a = Cx(fma(lpow[S], cs.x, a.x), fma(lpow[S], cs.y, a.y))
            for j in range(len(aj)):
                if (S >> j) & 1:
                    aj[j] = Cx(fma(lpow[S], cs.x, aj[j].x), fma(lpow[S], cs.y, aj[j].y))
        A.append(a)
        Aj.append(aj)
    a2 = fma(A[0].x, A[0].x, A[0].y * A[0].y)
    b2 = fma(A[1].x, A[1].x, A[1].y * A[1].y)
    r = a2.sqrt().div(b2.sqrt())
    dr = []
    for j in range(fs.d if der else 0):
        ga = fma(A[0].x, Aj[0][j].x, A[0].y * Aj[0][j].y).div(a2)
        gb = fma(A[1].x, Aj[1][j].x, A[1].y * Aj[1][j].y).div(b2)
        dr.append(r * (ga - gb))
    return r, dr


def fit_lams_ref(fs, raw, xt=XT):
    """k_mtg_lams: (x, y, ex, ey) [G, L] of the packed lams from the pair spectra and the raw parameters."""
    lay = fs.lay
    outs = [np.zeros((fs.G, lay.L), dtype=xt) if xt is not object else _conv(np.zeros((fs.G, lay.L)), object) for _ in range(4)]
    for g in range(fs.G):
        lpow = _lpow(fs, raw, g, xt)
        sc = _scalar(raw[fs.i_s(g)], xt).exp()
        nz = _scalar(raw[fs.i_n(g)], xt).exp()
        for p, (k, l) in enumerate(fs.pairs):
            P, _ = _poly(fs, p, lpow, xt, False)
            rn = _scalar(float(lay.ns[l]), xt).sqrt()
            vx, vy = rn * (sc * P.x), rn * (sc * P.y)
            if k == l:
                vx = vx + (nz * _nug_ratio(fs, k, lpow, xt, False)[0] if fs.nug_coef is not None else nz)
            kt = _ktask(fs, raw, g, fs.task[k], fs.task[l], xt)
            vx, vy = vx * kt, vy * kt
            sl = slice(lay.off[k, l], lay.off[k, l] + lay.ns[k])
            for a, val in zip(outs, (vx.v, vy.v, vx.e, vy.e)):
                a[g, sl] = val
    return tuple(outs)


def wg_sum(x):
    """The workgroup-order sum over the last axis of a tracked array (k_mtg_reduce; block_sum after the threads'
    sums): thread t's strided sum over t, t + 256, ... ascending (onto 0: the first exact), six butterfly additions
    (lane i with lane i ^ 32, ..., 1), the four waves added in order (the first onto 0)."""
    n = x.v.shape[-1]
    steps = max(1, -(-n // KWG))
    pad = steps * KWG - n
    lead = x.v.shape[:-1]

    def shaped(a):
        if pad:
            a = np.concatenate([a, np.zeros(lead + (pad,), dtype=a.dtype) if a.dtype != object else _conv(
                np.zeros(lead + (pad,)), object)], -1)
        return a.reshape(lead + (steps, KWG))

    v, e = shaped(x.v), shaped(x.e)
    s = Tr(v[..., 0, :], e[..., 0, :], x.xt)
    for i in range(1, steps):
        # a thread past the end at this step adds nothing (no rounding)
        live = (np.arange(KWG) + i * KWG) < n
        s = (s + Tr(v[..., i, :], e[..., i, :], x.xt)).where(live, s)
    return tree_sum(s)


def tree_sum(s):
    """block_sum's fixed tree over a last axis of 256 thread values."""
    s = Tr(s.v.reshape(s.v.shape[:-1] + (4, 64)), s.e.reshape(s.e.shape[:-1] + (4, 64)), s.xt)
    for o in (32, 16, 8, 4, 2, 1):
        s = s[..., :o] + s[..., o:2 * o]
    s = s[..., 0]
    tot = s[..., 0]
    for w in range(1, 4):
        tot = tot + s[..., w]
    return tot


def fit_contract_ref(fs, raw, glp, z, logdet, xt=XT):
    """k_mtg_contract + k_mtg_reduce: (sums, e) [G, 4 + d + P] from the device glp [G, L], z [G, B, R nmin], logdet
    [G, nmin], the spectra and raw.  Columns: norm, logdet, dnoise / noise, draw_scale, draw_l[d], dL/dK_task per pair."""
    lay, d = fs.lay, fs.d
    NQ = 4 + d + fs.P
    nt = fs.nblk * KWG
    sv = np.zeros((fs.G, NQ), dtype=xt) if xt is not object else _conv(np.zeros((fs.G, NQ)), object)
    se = sv.copy()
    for g in range(fs.G):
        lpow = _lpow(fs, raw, g, xt)
        sc = _scalar(raw[fs.i_s(g)], xt).exp()
        nz = _scalar(raw[fs.i_n(g)], xt).exp()
        c = Cx.exact(np.asarray(glp)[g], xt)
        # per-entry factors of the accumulations acc[q] = fma(fa, fb, acc[q]); two passes for acc[4 + j] with the nugget
        fa = {q: Tr.exact(np.zeros(lay.L), xt) for q in range(2, 4 + d)}
        fb = {q: Tr.exact(np.zeros(lay.L), xt) for q in range(2, 4 + d)}
        fa2 = {q: Tr.exact(np.zeros(lay.L), xt) for q in range(4, 4 + d)}
        fb2 = {q: Tr.exact(np.zeros(lay.L), xt) for q in range(4, 4 + d)}
        diag = np.zeros(lay.L, dtype=bool)
        dkt = Tr.exact(np.zeros(lay.L), xt)
        for p, (k, l) in enumerate(fs.pairs):
            sl = slice(lay.off[k, l], lay.off[k, l] + lay.ns[k])
            ce = c[sl]
            P, dp = _poly(fs, p, lpow, xt, True)
            rn = _scalar(float(lay.ns[l]), xt).sqrt()
            kt = _ktask(fs, raw, g, fs.task[k], fs.task[l], xt)
            f = kt * rn * sc
            fa[3][sl], fb[3][sl] = _fill(f, lay.ns[k]), fma(ce.x, P.x, ce.y * P.y)
            for j in range(d):
                fa[4 + j][sl] = fa[3][sl]
                fb[4 + j][sl] = fma(ce.x, dp[j].x, ce.y * dp[j].y)
            bx, by = rn * (sc * P.x), rn * (sc * P.y)
            if k == l:
                diag[sl] = True
                if fs.nug_coef is not None:
                    r, dr = _nug_ratio(fs, k, lpow, xt, True)
                    bx = bx + nz * r
                    ktr = kt * r
                    fa[2][sl] = _fill(ktr, lay.ns[k])
                    fb[2][sl] = ce.x
                    for j in range(d):
                        nd = nz * dr[j]
                        fa2[4 + j][sl] = kt * ce.x
                        fb2[4 + j][sl] = _fill(nd, lay.ns[k])
                else:
                    bx = bx + nz
                    fa[2][sl] = _fill(kt, lay.ns[k])
                    fb[2][sl] = ce.x
            dkt[sl] = fma(ce.x, bx, ce.y * by)
        steps = -(-lay.L // nt)

        def padded(t):
            padn = steps * nt - lay.L
            zv = np.zeros(padn) if xt is not object else _conv(np.zeros(padn), object)
            return Tr(np.concatenate([t.v, zv.astype(t.v.dtype)]).reshape(steps, nt),
                      np.concatenate([t.e, zv.astype(t.e.dtype)]).reshape(steps, nt), xt)

        live_all = (np.arange(steps * nt) < lay.L).reshape(steps, nt)
        dg = np.concatenate([diag, np.zeros(steps * nt - lay.L, dtype=bool)]).reshape(steps, nt)
        acc = {q: Tr.exact(np.zeros(nt), xt) for q in range(4 + d)}
        pa, pb = {q: padded(fa[q]) for q in fa}, {q: padded(fb[q]) for q in fb}
        pa2, pb2 = {q: padded(fa2[q]) for q in fa2}, {q: padded(fb2[q]) for q in fb2}
        for i in range(steps):
            live = live_all[i]
            acc[3] = fma(pa[3][i], pb[3][i], acc[3]).where(live, acc[3])
            for j in range(d):
                acc[4 + j] = fma(pa[4 + j][i], pb[4 + j][i], acc[4 + j]).where(live, acc[4 + j])
            on = live & dg[i]
            acc[2] = fma(pa[2][i], pb[2][i], acc[2]).where(on, acc[2])
            if fs.nug_coef is not None:
                for j in range(d):
                    acc[4 + j] = fma(pa2[4 + j][i], pb2[4 + j][i], acc[4 + j]).where(on, acc[4 + j])
        # the norm: Re(conj(y) z) over the problem's B R nmin elements; the logdet over its classes
        rnm = fs.B * lay.R * lay.nmin
        yy, zz = Cx.exact(np.asarray(fs.y)[g].reshape(-1), xt), Cx.exact(np.asarray(z)[g].reshape(-1), xt)
        for i in range(-(-rnm // nt)):
            lo, hi = i * nt, min(rnm, (i + 1) * nt)
            m = hi - lo
            new = fma(yy.x[lo:hi], zz.x[lo:hi], fma(yy.y[lo:hi], zz.y[lo:hi], acc[0][:m]))
            acc[0][:m] = new
        ldv = Tr.exact(np.asarray(logdet)[g], xt)
        for i in range(-(-lay.nmin // nt)):
            lo, hi = i * nt, min(lay.nmin, (i + 1) * nt)
            m = hi - lo
            acc[1][:m] = ldv[lo:hi] if i == 0 else acc[1][:m] + ldv[lo:hi]
        for q in range(4 + d):
            a = acc[q]
            part = tree_sum(Tr(a.v.reshape(fs.nblk, KWG), a.e.reshape(fs.nblk, KWG), xt))      # [nblk]
            tot = wg_sum(part)
            sv[g, q], se[g, q] = tot.v, tot.e
        for p, (k, l) in enumerate(fs.pairs):
            tot = wg_sum(dkt[lay.off[k, l]:lay.off[k, l] + lay.ns[k]])
            sv[g, 4 + d + p], se[g, 4 + d + p] = tot.v, tot.e
    return sv, se


def fit_step_ref(fs, raw, sums, xt=XT):
    """k_mtg_step's loss row and gradient from the device totals sums [G, 4 + d + P] (columns as fit_contract_ref) and
    raw: (loss [3], loss_e [3], grad [n_params], grad_e [n_params])."""
    lay, d, G, T = fs.lay, fs.d, fs.G, fs.lay.T
    S = Tr.exact(np.asarray(sums, dtype=np.float64), xt)

    def sq(g, q):
        return S[g, q]

    def chain(terms):
        s = None
        for t in terms:
            s = t if s is None else s + t                       # 0 + first: exact
        return s if s is not None else _scalar(0.0, xt)

    t0 = chain([sq(g, 0) for g in range(G)])
    t1 = chain([sq(g, 1) for g in range(G)])
    term2 = _scalar(fs.logdet_weight, xt) * t1
    loss = [((t0 + term2) + _scalar(fs.mll_const, xt)).scaled(0.5), t0, term2]
    gv = np.zeros(fs.n_params, dtype=xt) if xt is not object else _conv(np.zeros(fs.n_params), object)
    ge = gv.copy()
    rows = fs.rows
    for x in range(fs.n_params):
        terms = []
        if x < fs.l_off:
            terms = [sq(g, 3) for g in range(G) if rows[0][g] == x]
        elif x < fs.n_off:
            rr, j = divmod(x - fs.l_off, fs.dl)
            for g in range(G):
                if rows[1][g] != rr:
                    continue
                terms.append(sq(g, 4 + j) if fs.dl > 1 else chain([sq(g, 4 + jj) for jj in range(d)]))
        elif x < fs.f_off:
            nz = _scalar(raw[x], xt).exp()
            terms = [nz * sq(g, 2) for g in range(G) if rows[2][g] == x - fs.n_off]
        elif x < fs.v_off:
            TR = fs.T_all * fs.rank
            rr, u = divmod(x - fs.f_off, TR)
            c, r = divmod(u, fs.rank)
            fo = fs.f_off + rr * TR
            for g in range(G):
                if rows[3][g] != rr:
                    continue
                p = 0
                for k in range(T):
                    a = fs.task[k]
                    for l in range(k, T):
                        b = fs.task[l]
                        gvv = sq(g, 4 + d + p + l - k)
                        if a == c:
                            terms.append(gvv * _scalar(raw[fo + b * fs.rank + r], xt))
                        if b == c:
                            terms.append(gvv * _scalar(raw[fo + a * fs.rank + r], xt))
                    p += T - k
        else:
            rr, c = divmod(x - fs.v_off, fs.T_all)
            ev = _scalar(raw[x], xt).exp() if fs.vtask_exp else None
            for g in range(G):
                if rows[4][g] != rr:
                    continue
                for k in range(T):
                    if fs.task[k] == c:
                        gvv = sq(g, 4 + d + k * T - k * (k - 1) // 2)
                        terms.append(gvv * ev if fs.vtask_exp else gvv)
        tot = chain(terms)
        gv[x], ge[x] = tot.v, tot.e
    lv = np.array([t.v for t in loss], dtype=xt if xt is not object else object)
    le = np.array([t.e for t in loss], dtype=xt if xt is not object else object)
    return lv, le, gv, ge


def rprop_f64(grad, raw, prev, step, rg_mask, eta_minus, eta_plus, step_min, step_max):
    """k_mtg_step's torch.optim.Rprop element update in float64, bit for bit: (raw, prev, step, prod) after the update
    of the elements where rg_mask."""
    grad, raw, prev, step = (np.array(a, dtype=np.float64) for a in (grad, raw, prev, step))
    prod = grad * prev
    sgn = np.where(prod > 0.0, eta_plus, np.where(prod < 0.0, eta_minus, 1.0))
    st = np.minimum(np.maximum(step * sgn, step_min), step_max)
    gg = np.where(sgn == eta_minus, 0.0, grad)
    gs = np.where(gg > 0.0, 1.0, np.where(gg < 0.0, -1.0, 0.0))
    new_raw = raw + (-1.0) * (gs * st)
    m = np.asarray(rg_mask, dtype=bool)
    return np.where(m, new_raw, raw), np.where(m, gg, prev), np.where(m, st, step), prod


def _c128(x, y):
    return np.asarray(x, dtype=np.float64) + 1j * np.asarray(y, dtype=np.float64)


def fit_chain(fs, raw, xt=XT, mutate=None):
    """One evaluation of fgp_mt_fit_run's loss and gradient with every stage from `xt` arithmetic, each stage fed the
    previous one's values rounded to double (what the device hands on): dict of the stages' (value, twin) tuples."""
    lay, G, B = fs.lay, fs.G, fs.B
    out = {}
    out["lams"] = fit_lams_ref(fs, raw, xt)
    lams = _c128(out["lams"][0], out["lams"][1])
    f = factor_ref(lams, fs.ns, G, xt, mutate)
    out["factor"] = f
    # the fit keeps problem g's B vectors together; the entry points take vector b against problem b mod G
    v = np.asarray(fs.y).transpose(1, 0, 2).reshape(B * G, -1)
    out["z"] = solve_ref(f["fac"], fs.ns, v, G, xt)
    z = _c128(out["z"][0], out["z"][1])
    out["zinv"] = selinv_ref(f["fac"], fs.ns, G, xt)
    zinv = _c128(out["zinv"][0], out["zinv"][1])
    out["glp"] = grad_ref(zinv, z, np.full(B * G, fs.grad_norm), np.full(G, fs.grad_logdet), fs.ns, B * G, G, xt, mutate)
    glp = _c128(out["glp"][0], out["glp"][1])
    zg = z.reshape(B, G, -1).transpose(1, 0, 2)
    out["sums"] = fit_contract_ref(fs, raw, glp, zg, np.asarray(f["logdet"], dtype=np.float64), xt)
    out["step"] = fit_step_ref(fs, raw, np.asarray(out["sums"][0], dtype=np.float64), xt)
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def ratio(got, want, e, C):
    """max |got - want| / bound over the elements (0 / 0 = 0: an exact element reproduced exactly; x / 0 = inf)."""
    err = abs(_conv(np.asarray(got, dtype=np.float64), XT) - want)
    bnd = bound(e, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.where(bnd == 0, 1.0, bnd))
        r = np.where((bnd == 0) & (err != 0), np.inf, r)
    return float(np.max(r.astype(np.float64))) if r.size else 0.0


def complex_ratio(got, ref, C):
    x, y, ex, ey = ref
    got = np.asarray(got).reshape(np.shape(x))
    return max(ratio(got.real, x, ex, C), ratio(got.imag, y, ey, C))


def block_stage_ratios(dev, lams, v, gn, gl, ns, G):
    """max err / bound per stage of the block entry points: dev = {fac, logdet [G, nmin], z [B, R nmin], zinv, glp} as a
    device (or a restatement) produced them, every stage from the previous one's output."""
    B = np.asarray(v).shape[0]
    C = counts(ns, B, G)
    f = factor_ref(lams, ns, G)
    return {"fac": complex_ratio(dev["fac"], (f["fac_x"], f["fac_y"], f["ex"], f["ey"]), C["factor"]),
            "logdet": ratio(dev["logdet"], f["logdet"], f["logdet_e"], C["factor"]),
            "z": complex_ratio(dev["z"], solve_ref(dev["fac"], ns, v, G), C["solve"]),
            "zinv": complex_ratio(dev["zinv"], selinv_ref(dev["fac"], ns, G), C["selinv"]),
            "glp": complex_ratio(dev["glp"], grad_ref(dev["zinv"], dev["z"], gn, gl, ns, B, G), C["grad"])}, f


def block_stages(lams, v, gn, gl, ns, G, xt=np.float64, mutate=None):
    """The four block stages chained in `xt` arithmetic (the plain restatement a device run is exchanged for on the CPU)."""
    B = np.asarray(v).shape[0]
    f = factor_ref(lams, ns, G, xt, mutate)
    z = solve_ref(f["fac"], ns, v, G, xt)
    zi = selinv_ref(f["fac"], ns, G, xt)
    dev = {"fac": f["fac"], "logdet": np.asarray(f["logdet"], dtype=np.float64), "z": _c128(z[0], z[1]), "zinv": _c128(zi[0], zi[1])}
    g = grad_ref(dev["zinv"], dev["z"], gn, gl, ns, B, G, xt, mutate)
    dev["glp"] = _c128(g[0], g[1])
    return dev


def fit_stage_ratios(fs, raw, dev):
    """max err / bound of the non-block stages of one fgp_mt_fit_run iteration at parameters raw: dev = {lams [G, L], glp
    [G, L], z [G, B, R nmin], logdet [G, nmin], sums [G, 4 + d + P], loss [3], grad [n_params]} as the device left them."""
    C = fs.counts()
    sv, se = fit_contract_ref(fs, raw, dev["glp"], dev["z"], dev["logdet"])
    lv, le, gv, ge = fit_step_ref(fs, raw, dev["sums"])
    return {"lams": complex_ratio(dev["lams"], fit_lams_ref(fs, raw), C["lams"]),
            "sums": ratio(dev["sums"], sv, se, C["contract"]),
            "loss": ratio(dev["loss"], lv, le, C["step"]),
            "grad": ratio(dev["grad"], gv, ge, C["step"])}


def fit_stages_f64(fs, raw, mutate=None):
    """`dev` of fit_stage_ratios from the float64 restatement."""
    o = fit_chain(fs, raw, np.float64, mutate)
    B, G = fs.B, fs.G
    z = _c128(o["z"][0], o["z"][1]).reshape(B, G, -1).transpose(1, 0, 2)
    return {"lams": _c128(o["lams"][0], o["lams"][1]), "glp": _c128(o["glp"][0], o["glp"][1]), "z": z,
            "logdet": np.asarray(o["factor"]["logdet"], dtype=np.float64), "sums": np.asarray(o["sums"][0], dtype=np.float64),
            "loss": np.asarray(o["step"][0], dtype=np.float64), "grad": np.asarray(o["step"][2], dtype=np.float64)}
