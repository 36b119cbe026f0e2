"""Extended-precision reference of the prediction kernels (csrc/fgp_predict.hip, d <= 8; generic in d, so also of the
wide ones, 9 <= d <= 64: csrc/fgp_wide.hip and k_wide_qf_rows) and of the wide first column, with first-order bounds.

The same arithmetic setup as tests/spectral_reference.py (np.longdouble where its eps is below 2e-19, mpmath at 40
digits otherwise; its _x / _xs widen fp64 inputs exactly).  Every function takes the very fp64 / int64 arrays handed to
a kernel and evaluates the operation's definition from them -- nothing is recomputed in fp64, no nugget or solve sits
between the inputs and the output -- and returns, next to each value q, a bound B_q formed in the same pass such that a
correct fp64 kernel satisfies |device - reference| <= C 2^-53 B_q with C its count of roundings per term and per
summation level (tests/predict_cases.py derives C per variant).  Values and bounds are extended-precision arrays.

kernel_rows   K[g, t, i] = scale_g prod_j f_gj,  f = 1 + l_gj part_j(x_t, z_i)
    lattice   part = coef_j B_n((x - z) mod 1), n = order_j, B_n the Bernoulli polynomial as its textbook sum of
              monomials (the kernels evaluate polynomials in u = t (t - 1) of |x - z| instead).
    net       delta = floor((x mod 1) 2^t) XOR z; order 1: part = 1 - 3 2^(floor(log2 delta) - t), 1 at delta = 0;
              orders 2..4: part = omega_a(delta / 2^t), the digit recursion of oracle.fgp_oracle.walsh_omega.
    Bound of a factor: the magnitudes of the terms that make it up,
        lattice  bf = 1 + |a| (|B_n(t) - B_n(0)| + |B_n(0)|),  a = l coef
                 (the split at the constant term: no evaluation in u cancels more than that; the textbook monomials
                 themselves cancel up to 190-fold at order 8 and would only loosen the bound),
        net 1    bf = 1 + l + 3 l 2^(floor(log2 delta) - t)                          (1 + l at delta = 0),
        net a    bf = 1 + l W_a, W_a = sum_k 2^-mu_a(k) = omega_a(0) = 3/2, 25/18, 407/294 (every |wal_k| = 1),
    plus, lattice, the effect of the fp64 rounding of x - z on the factor, |a B_n'(t)| t with t = |x - z| (in units of
    2^-53; rows regenerated from the lattice index: |a B_n'(t)| 2, i.e. 2 2^-53 absolute on t).  Through the product,
    to first order:  B_K = |scale| sum_j (bf_j + df_j) prod_{i != j} |f_i|.

post_mean     sum_i K[g, t, i] c[b, i], g = b mod Gk;  B = sum_i (|K_i c_i| + B_{K_i} |c_i|).

quadform      q = sum_k wa_k |ft(r)_k|^2, ft the orthonormal transform of include/fgp_hip.h: lattice, the DFT of the
              bit-reversed input (fgp_fftbr: y = fft(x[bitrev]) / sqrt(n)); net, the Sylvester-order FWHT / sqrt(n).
              Both are the radix-2 butterfly network applied to the input as it lies, m vectorised stages here.
    Bound     B = S + 2 sqrt(S) sqrt(max |wa|) ||delta||_2,  S = sum_k |wa_k| |r~_k|^2 (the summation term; sqrt(S) =
              || sqrt|wa| r~ ||_2 and || sqrt|wa| delta ||_2 <= sqrt(max |wa|) ||delta||_2), with the transform's error
                  ||delta||_2 <= c (1 + m) ||r - mean(r)||_2 + 2 |r~_0| + ||B_r||_2        (units of 2^-53).
    The constant c, from the pass structure of the kernels (csrc/fgp_common.h): every kernel is the radix-2 network of
    m stages (radix-16 register passes are four of them; the half-length form has m - 1 and the mirror split, one more
    butterfly with one more twiddle) applied to the row with its mean taken out per pass, the mean re-entering bin 0
    only.  A stage computes a +- w b; a unitary stage passes earlier errors on unchanged in the 2-norm, so the stages'
    errors add: per stage mu + gamma_4 (sqrt 2 + mu) relative to the data's norm (Higham, Accuracy and Stability,
    Thm 24.2), gamma_4 = 4 u for the complex multiply-add, mu the twiddle's own error.  A twiddle here is the
    product of a rounded table entry and a rounded compile-time root or second table entry (inter_tw, RowTwiddle):
    mu <= u + u + sqrt(5) u < 4.3 u.  Per stage 4.3 + 4 (1.42 + 0) = 10 u: c = 10 for lattices.  The one inter-pass
    twiddle multiplication and the subtraction of the means are the "1 +".  Nets: w = 1, a stage is one rounded
    addition per element, sqrt 2 u per stage: c = 2.  What the data's norm is: the kernels transform r minus the mean of
    each pass, hence ||r - mean(r)||_2; the means re-added to bin 0 (mean * length, once per pass: two roundings of
    size u |r~_0|) land on bin 0 and, through the second pass and the half-length split, on the bins of column 0 --
    the 2 |r~_0|.  ||B_r||_2 is the rows' own bound.

post_var      max(0, K(x, x) - q), K(x, x) = scale prod_j (1 + l_j part0_j);  B = B_q + K(x, x).

lattice_parts, net_parts   the parts arrays [d, n] of the first column (fgp_wide_lattice_parts / fgp_wide_net_parts),
              bounds as for a factor's part above.
k1, k1_bwd    k1[g, i] = s_g prod_j (1 + l_gj p_ji) (fgp_wide_k1) and its adjoint for the natural scale and lengthscale
              rows (fgp_wide_k1_bwd), bf_j = 1 + |l_j p_j|; see the functions.
"""
from fractions import Fraction

import numpy as np

from tests import spectral_reference as R
from tests.spectral_reference import EPS53, MP, XT, _x, _xs  # noqa: F401  (re-exported for the tests)

LAT, NET = 0, 1
FFT_C = {LAT: 10.0, NET: 2.0}

if MP:
    import mpmath
    _floor = np.frompyfunc(mpmath.floor, 1, 1)
    _cos, _sin, _sqrt = np.frompyfunc(mpmath.cos, 1, 1), np.frompyfunc(mpmath.sin, 1, 1), np.frompyfunc(mpmath.sqrt, 1, 1)
    _PI = mpmath.pi
    _DT = object

    def _pow2(e):
        return np.frompyfunc(lambda v: mpmath.ldexp(mpmath.mpf(1), int(v)), 1, 1)(np.asarray(e))
else:
    _floor, _cos, _sin, _sqrt = np.floor, np.cos, np.sin, np.sqrt
    _PI = 4 * np.arctan(np.longdouble(1))
    _DT = np.longdouble

    def _pow2(e):
        return np.ldexp(np.longdouble(1), np.asarray(e, dtype=np.int64).astype(np.int32))


def _q(fr):
    return XT(fr.numerator) / XT(fr.denominator)


def _full(shape, v):
    a = np.empty(shape, dtype=_DT)
    a[...] = v
    return a


def to_f64(a):
    return np.asarray(a).astype(np.float64)


# Bernoulli polynomials B_n(t) = sum_k c_k t^(n - k), k = 0..n (textbook coefficients, exact rationals)
F = Fraction
BERNOULLI = {
    2: [F(1), F(-1), F(1, 6)],
    4: [F(1), F(-2), F(1), F(0), F(-1, 30)],
    6: [F(1), F(-3), F(5, 2), F(0), F(-1, 2), F(0), F(1, 42)],
    8: [F(1), F(-4), F(14, 3), F(0), F(-7, 3), F(0), F(2, 3), F(0), F(-1, 30)],
}
WALSH_W = {2: F(3, 2), 3: F(25, 18), 4: F(407, 294)}


def bernoulli_split(order, t):
    """(B_n(t) - B_n(0), B_n(0), B_n'(t)) of extended t, the polynomial as its sum of monomials."""
    c = BERNOULLI[int(order)]
    n = len(c) - 1
    top, der = t * 0, t * 0
    pw = t * 0 + 1                                    # t^(p - 1)
    for p in range(1, n + 1):                         # the monomial c_{n - p} t^p and its derivative
        ck = c[n - p]
        if ck != 0:
            der = der + _q(ck * p) * pw
        pw = pw * t
        if ck != 0:
            top = top + _q(ck) * pw
    return top, _q(c[n]), der


def _product(scale, f, b):
    """K = scale prod_j f_j and B_K = |scale| sum_j b_j prod_{i != j} |f_i| (f, b: lists over j)."""
    K = f[0] * 0 + scale
    for fj in f:
        K = K * fj
    BK = f[0] * 0
    for bj, lo in zip(b, _leave_one_out([abs(fj) for fj in f])):
        BK = BK + bj * lo
    return K, abs(scale) * BK


def _leave_one_out(f):
    """[prod_{i != j} f_i for j]: prefix times suffix products, never a quotient (a factor may be zero)."""
    d = len(f)
    suf = [f[0] * 0 + 1] * (d + 1)
    for j in range(d - 1, -1, -1):
        suf[j] = suf[j + 1] * f[j]
    out, pre = [], f[0] * 0 + 1
    for j in range(d):
        out.append(pre * suf[j + 1])
        pre = pre * f[j]
    return out


def net_bits(x, tbits):
    """floor((x mod 1) 2^t) of fp64 x as uint64 -- every step exact in fp64."""
    x = np.asarray(x, dtype=np.float64)
    return np.floor(np.remainder(x, 1.0) * 2.0 ** int(tbits)).astype(np.uint64)


def floor_log2(delta):
    """floor(log2 delta) of uint64 delta (0 where delta = 0), exact."""
    delta = np.asarray(delta, dtype=np.uint64)
    hi, lo = (delta >> np.uint64(32)).astype(np.float64), (delta & np.uint64(0xffffffff)).astype(np.float64)
    return np.where(hi > 0, 32 + np.frexp(hi)[1] - 1, np.frexp(np.maximum(lo, 1.0))[1] - 1).astype(np.int64)


def walsh_omega(order, delta, t):
    """omega_a(delta / 2^t), a = order in 2..4: the digit recursion of oracle.fgp_oracle.walsh_omega (its definition,
    line for line) in extended precision.  delta: uint64 array."""
    delta = np.asarray(delta, dtype=np.uint64)
    r1 = order - 1
    c = _pow2(-(t + 1))[()]

    def prodq(r):
        p = XT(1)
        for i in range(1, r + 1):
            p = p * (1 - _pow2(-i)[()])
        return p

    e = [_full(delta.shape, XT(1))]
    for r in range(1, order):
        e.append(_full(delta.shape, c ** r * _pow2(-(r * (r - 1) // 2))[()] / prodq(r)))
    nz = delta != 0
    beta = np.where(nz, t - floor_log2(delta), 1 << 30)
    E = _full(delta.shape, XT(0))
    half = XT(1) / 2
    for a in range(t - 1, -1, -1):
        bit = ((delta >> np.uint64(t - 1 - a)) & np.uint64(1)).astype(np.int64)
        s = _x(1.0 - 2.0 * bit)
        E = E + np.where(a < beta, 1, 0) * (half * s * e[r1])
        y = s * _pow2(-(a + 1))[()]
        for r in range(r1, 0, -1):
            e[r] = e[r] + y * e[r - 1]
    Kc = _pow2(-(r1 * (r1 - 1) // 2))[()] / prodq(r1)
    tail = half * Kc * _pow2(-(t + 2) * r1)[()] / (1 - _pow2(-r1)[()])
    E = E + np.where(nz, 0, 1) * tail
    out = E
    for r in range(1, order):
        out = out + e[r]
    return out


def kernel_rows(family, xt, z, hyp, orders, coef, tbits, regenerated=False):
    """(K, B_K), each [G, N, n].  xt [N, d] fp64; z [d, n] fp64 (lattice) / int64 (net); hyp [G, 1 + d] (scale,
    lengthscales); orders [d]: Bernoulli orders 2 alpha (lattice), Walsh orders 1..4 (net); coef [d] (lattice);
    regenerated: the rows of a kernel that forms the distance from the lattice index (bound only)."""
    xt = np.asarray(xt, dtype=np.float64)
    hyp = np.asarray(hyp, dtype=np.float64).reshape(-1, 1 + xt.shape[1])
    N, d = xt.shape
    G = hyp.shape[0]
    h = _x(hyp)
    per = []                                          # per dimension: what the factor of every g is built from
    for j in range(d):
        if family == LAT:
            diff = _x(xt[:, j])[:, None] - _x(np.asarray(z[j], dtype=np.float64))[None, :]
            dl = diff - _floor(diff)                  # (x - z) mod 1, exact
            tk = abs(diff)
            top, b0, _ = bernoulli_split(orders[j], dl)
            _, _, der = bernoulli_split(orders[j], tk)
            per.append((top, b0, abs(der) * (2 if regenerated else tk)))
        else:
            delta = net_bits(xt[:, j], tbits)[:, None] ^ np.asarray(z[j]).astype(np.uint64)[None, :]
            if int(orders[j]) <= 1:
                w = np.where(delta != 0, 1, 0) * (3 * _pow2(floor_log2(delta) - int(tbits)))
                per.append((1 - w, 1 + w))            # part, and the magnitudes 1 + 3 2^(..) of its terms
            else:
                per.append((walsh_omega(int(orders[j]), delta, int(tbits)), _q(WALSH_W[int(orders[j])])))
    K, BK = [], []
    for g in range(G):
        f, b = [], []
        for j in range(d):
            l = h[g, 1 + j]
            if family == LAT:
                a = l * _xs(coef[j])
                top, b0, dterm = per[j]
                f.append(1 + a * (top + b0))
                b.append(1 + abs(a) * (abs(top) + abs(b0)) + abs(a) * dterm)
            else:
                part, mag = per[j]
                f.append(1 + l * part)
                b.append(1 + abs(l) * mag + part * 0)
        k, bk = _product(h[g, 0], f, b)
        K.append(k)
        BK.append(bk)
    return np.stack(K), np.stack(BK)


def post_mean(K, BK, coeffs):
    """(mean, B) [B, N]: sum_i K[b mod Gk, t, i] coeffs[b, i] and sum_i (|K c| + B_K |c|)."""
    c = _x(coeffs)
    Gk = K.shape[0]
    out, bnd = [], []
    for b in range(c.shape[0]):
        g = b % Gk
        out.append((K[g] * c[b][None, :]).sum(-1))
        bnd.append(((abs(K[g]) + BK[g]) * abs(c[b])[None, :]).sum(-1))
    return np.stack(out), np.stack(bnd)


def ft(family, rows):
    """The orthonormal transform of real extended rows [R, n]: (re, im) [R, n] (im = 0 for nets).  Lattice:
    fft(x[bitrev]) / sqrt(n), i.e. the radix-2 decimation-in-time stages run on the input as it lies; net: the
    Sylvester-order Walsh-Hadamard butterflies / sqrt(n)."""
    Rn, n = rows.shape
    m = n.bit_length() - 1
    assert n == 1 << m
    re, im = rows + 0, rows * 0
    h = 1
    while h < n:
        sh = (Rn, n // (2 * h), 2, h)
        ar, br = re.reshape(sh)[:, :, 0, :], re.reshape(sh)[:, :, 1, :]
        if family == LAT:
            ai, bi = im.reshape(sh)[:, :, 0, :], im.reshape(sh)[:, :, 1, :]
            ang = -(_PI / h) * _x(np.arange(h, dtype=np.float64))          # w_j = exp(-2 pi i j / (2 h))
            wr, wi = _cos(ang), _sin(ang)
            tr, ti = br * wr - bi * wi, br * wi + bi * wr
            re = np.stack([ar + tr, ar - tr], 2).reshape(Rn, n)
            im = np.stack([ai + ti, ai - ti], 2).reshape(Rn, n)
        else:
            re = np.stack([ar + br, ar - br], 2).reshape(Rn, n)
        h *= 2
    s = 1 / _sqrt(_xs(n))
    return re * s, im * s


def spectrum_power(family, rows):
    """|ft(r)_k|^2 [R, n]; the part of quadform that does not depend on the weights."""
    re, im = ft(family, rows)
    return re * re + im * im


def quadform(family, rows, Brows, wa, power=None):
    """(q, B_q) [R]: sum_k wa_k |ft(r)_k|^2 of real extended rows [R, n] with bounds Brows, weights wa [n] or [R, n]
    (fp64).  power: spectrum_power(family, rows) if already at hand."""
    n = rows.shape[-1]
    m = n.bit_length() - 1
    p = spectrum_power(family, rows) if power is None else power
    w = _x(np.broadcast_to(np.asarray(wa, dtype=np.float64), rows.shape))
    q = (w * p).sum(-1)
    S = (abs(w) * p).sum(-1)
    mean = rows.sum(-1) / n
    cen = rows - mean[:, None]
    dnorm = (FFT_C[family] * (1 + m) * _sqrt((cen * cen).sum(-1)) + 2 * _sqrt(p[:, 0]) + _sqrt((Brows * Brows).sum(-1)))
    wmax = abs(w).max(-1)
    return q, S + 2 * _sqrt(S) * _sqrt(wmax) * dnorm


def kxx(hyp, part0):
    """K(x, x) = scale prod_j (1 + l_j part0_j) [G] of hyp [G, 1 + d]."""
    h = _x(np.asarray(hyp, dtype=np.float64))
    p0 = _x(part0)
    out = h[:, 0]
    for j in range(h.shape[1] - 1):
        out = out * (1 + h[:, 1 + j] * p0[j])
    return out


def post_var(k0, q, Bq):
    """(max(0, K(x, x) - q), B_q + K(x, x)); k0 broadcasts against q."""
    v = k0 - q
    return v * np.where(v > 0, 1, 0), Bq + abs(k0)


# ------------------------------------------------------------------------------------------------ first column
def lattice_parts(x, z, orders, coef):
    """(parts, B) [d, n]: coef_j B_order_j((x[i, j] - z[j]) mod 1) of fp64 x [n, d] (any row stride) and z [d].  B:
    |coef| (|B_n(t) - B_n(0)| + |B_n(0)|), the split at the constant term, plus the effect on the part of the kernel's
    rounded distance, |coef B_n'(t)| (|x - z| + [x < z]): the subtraction rounds at |x - z|, and the shift of a
    negative remainder into [0, 1) rounds once more, below 1."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    P, B = [], []
    for j in range(d):
        diff = _x(x[:, j]) - _xs(np.float64(z[j]))
        dl = diff - _floor(diff)
        top, b0, der = bernoulli_split(orders[j], dl)
        c = _xs(np.float64(coef[j]))
        P.append(c * (top + b0))
        B.append(abs(c) * (abs(top) + abs(b0)) + abs(c * der) * (abs(diff) + np.where(x[:, j] < z[j], 1, 0)))
    return np.stack(P), np.stack(B)


def net_parts(xb, z, orders, t):
    """(parts, B) [d, n] of int64 xb [n, d] and z [d], delta = xb XOR z: order 1 the closed form
    1 - 3 2^(floor(log2 delta) - t) (1 at delta = 0) with B = 1 + 3 2^(..), orders 2..4 walsh_omega with B = W_a."""
    xb = np.asarray(xb)
    n, d = xb.shape
    P, B = [], []
    for j in range(d):
        delta = xb[:, j].astype(np.uint64) ^ np.uint64(int(z[j]))
        if int(orders[j]) <= 1:
            w = np.where(delta != 0, 1, 0) * (3 * _pow2(floor_log2(delta) - int(t)))
            P.append(1 - w)
            B.append(1 + w)
        else:
            om = walsh_omega(int(orders[j]), delta, int(t))
            P.append(om)
            B.append(om * 0 + _q(WALSH_W[int(orders[j])]))
    return np.stack(P), np.stack(B)


def _k1_factors(parts, ls, g):
    l = _x(np.asarray(ls, dtype=np.float64))[g]
    p = _x(np.asarray(parts, dtype=np.float64))
    d = p.shape[0]
    return p, [1 + l[j] * p[j] for j in range(d)], [1 + abs(l[j] * p[j]) for j in range(d)]


def k1(parts, scale, ls):
    """(k1, B) [G, n]: scale_g prod_j f_gji, f = 1 + l_gj parts[j, i], of fp64 parts [d, n], scale [G], ls [G, d];
    B through _product with bf_j = 1 + |l_j p_j|."""
    s = _x(np.asarray(scale, dtype=np.float64))
    K, B = [], []
    for g in range(s.shape[0]):
        _, f, bf = _k1_factors(parts, ls, g)
        k, b = _product(s[g], f, bf)
        K.append(k)
        B.append(b)
    return np.stack(K), np.stack(B)


def k1_bwd(parts, scale, ls, u):
    """(dscale [G], B [G], dls [G, d], B [G, d]) of u [G, n]:
        dscale_g = sum_i u_gi prod_j f_gji,   dls_gj = sum_i u_gi s_g p_ji prod_{j' != j} f_gj'i,
    the leave-one-out product formed as a product.  Bound of a term: that of the product of its factors (_product
    over them), times |u| (and |s p|), summed over i."""
    s = _x(np.asarray(scale, dtype=np.float64))
    uu = _x(np.asarray(u, dtype=np.float64))
    ds, Bs, dl, Bl = [], [], [], []
    for g in range(s.shape[0]):
        p, f, bf = _k1_factors(parts, ls, g)
        d = len(f)
        af = [abs(v) for v in f]
        k, b = _product(XT(1), f, bf)
        ds.append((uu[g] * k).sum())
        Bs.append((abs(uu[g]) * b).sum())
        # leave-one-out values, and the bounds sum_{i != j} bf_i prod_{k != i, j} |f_k| from prefix / suffix pairs:
        # (pv, pb) = (prod |f|, sum_i bf_i prod_{k != i} |f_k|) of the factors before j, (sv, sb) of those after
        one, zero = f[0] * 0 + 1, f[0] * 0
        sv, sb = [one] * (d + 1), [zero] * (d + 1)
        sval = [one] * (d + 1)
        for j in range(d - 1, -1, -1):
            sval[j] = sval[j + 1] * f[j]
            sb[j] = sb[j + 1] * af[j] + bf[j] * sv[j + 1]
            sv[j] = sv[j + 1] * af[j]
        pval, pv, pb = one, one, zero
        row, brow = [], []
        for j in range(d):
            w = uu[g] * s[g] * p[j]
            row.append((w * (pval * sval[j + 1])).sum())
            brow.append((abs(w) * (pb * sv[j + 1] + pv * sb[j + 1])).sum())
            pval = pval * f[j]
            pb = pb * af[j] + bf[j] * pv
            pv = pv * af[j]
        dl.append(np.stack(row))
        Bl.append(np.stack(brow))
    return np.stack(ds), np.stack(Bs), np.stack(dl), np.stack(Bl)
