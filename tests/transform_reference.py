"""Extended-precision reference of the transforms (csrc/fgp_transforms.hip and the half-length kernels of
csrc/fgp_nll.hip), with derived bounds.

The arithmetic setup of tests/spectral_reference.py / tests/predict_reference.py (np.longdouble, eps 1.1e-19; mpmath
where long double is a double).  Every function takes the very arrays handed to a kernel (fp32 / complex64 arrays are
widened exactly) and returns extended (re, im) arrays.

Network form     fftbr / ifftbr / fwht: the radix-2 butterfly network in extended precision (on the rows centred in
                 extended precision, transform()), the generalisation of
                 predict_reference.ft to complex rows and to the adjoint (for real rows the same operations in the same
                 order: the same values bit for bit, tests/test_transform_reference_cpu.py).
                   fftbr[k]  = n^-1/2 sum_i x_i exp(-2 pi i k brev(i) / n)     (DIT stages h = 1, 2, .., n/2)
                   ifftbr[i] = n^-1/2 sum_k X_k exp(+2 pi i k brev(i) / n)     (the transposed-conjugate stages, DIF)
                   fwht[k]   = n^-1/2 sum_i x_i (-1)^popcount(i & k)
Closed form      sparse_fftbr / sparse_ifftbr / sparse_fwht: the sums above over the s non-zeros only, for the
                 requested outputs only; the phase k brev(i) mod n is reduced exactly in int64 before the 80-bit
                 cos / sin (k, brev(i) < 2^24: the product is below 2^48).
Element-wise     double_update, sum_sq, sum_sq_half, product (the x o f fused into an inverse's load).

Bounds (units of u; tests/transform_cases.py derives c, m_eff and the DC constant per variant):
  dense rows, 2-norm per row    || device - ref ||_2 <= u (c (1 + m_eff) ||data||_2 + dcc D)
      data = x minus the means the path's FIRST pass takes out (centred(); later passes centre a vector of no
      larger norm, by Parseval), D = || x - data ||_2, the norm of what is re-added (the same, by Parseval, on the
      frequency side).  On the bins outside the path's DC set the dcc D term is absent.
  sparse rows, per output       | device - ref |_k <= u (c (1 + m_eff) + dcc [k in DC set]) B,
      B = (1 + stable) ||x||_1 / sqrt(n): every path from an input to an output crosses m_eff butterflies, the
      l1 mass of the centred data is at most twice that of x (L |mean| = |sum| <= l1).
"""
import numpy as np

from tests import predict_reference as PR
from tests.predict_reference import LAT, NET, XT, _x, _xs, to_f64  # noqa: F401

_cos, _sin, _sqrt, _PI = PR._cos, PR._sin, PR._sqrt, PR._PI
U64, U32 = 2.0 ** -53, 2.0 ** -24


def brev(i, m):
    """Bit reversal of int64 indices over m bits (exact)."""
    i = np.asarray(i, dtype=np.int64)
    r = np.zeros_like(i)
    for b in range(m):
        r |= ((i >> b) & 1) << (m - 1 - b)
    return r


def widen(a):
    """(re, im) extended arrays of a real / complex fp64 or fp32 array (exact); im = None for real input."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return _x(a.real.astype(np.float64)), _x(a.imag.astype(np.float64))
    return _x(a.astype(np.float64)), None


def _twiddles(h):
    ang = -(_PI / h) * _x(np.arange(h, dtype=np.float64))          # w_j = exp(-2 pi i j / (2 h))
    return _cos(ang), _sin(ang)


def network(family, re, im, adjoint=False):
    """The orthonormal radix-2 network on extended rows re, im [R, n] (im ignored for nets).  Forward: the DIT stages
    of predict_reference.ft on the input as it lies (bit-reversed input, natural output); adjoint: the stages'
    conjugate transposes in reverse order (natural input, bit-reversed output)."""
    Rn, n = re.shape
    m = n.bit_length() - 1
    assert n == 1 << m
    hs = [1 << s for s in range(m)]
    for h in (hs[::-1] if adjoint else hs):
        sh = (Rn, n // (2 * h), 2, h)
        ar, br = re.reshape(sh)[:, :, 0, :], re.reshape(sh)[:, :, 1, :]
        if family == NET:
            re = np.stack([ar + br, ar - br], 2).reshape(Rn, n)
            continue
        ai, bi = im.reshape(sh)[:, :, 0, :], im.reshape(sh)[:, :, 1, :]
        wr, wi = _twiddles(h)
        if not adjoint:
            tr, ti = br * wr - bi * wi, br * wi + bi * wr
            re = np.stack([ar + tr, ar - tr], 2).reshape(Rn, n)
            im = np.stack([ai + ti, ai - ti], 2).reshape(Rn, n)
        else:
            dr, di = ar - br, ai - bi
            re = np.stack([ar + br, dr * wr + di * wi], 2).reshape(Rn, n)      # (a - b) conj(w)
            im = np.stack([ai + bi, di * wr - dr * wi], 2).reshape(Rn, n)
    s = 1 / _sqrt(_xs(n))
    return re * s, im * s


def transform(family, re, im, adjoint=False):
    """network() of the rows centred by their own mean in extended precision, the mean re-added to index 0 (where both
    directions put a constant row): the same operation exactly, with the reference's own rounding relative to the
    centred data -- on a row of 2^16 + noise the plain network's 2^-64 ||x||_2 is 32 u on the noise's scale."""
    n = re.shape[-1]
    mr, mi = re.sum(-1) / n, im.sum(-1) / n
    yr, yi = network(family, re - mr[:, None], im - mi[:, None], adjoint)
    rootn = _sqrt(_xs(n))
    yr[:, 0] = yr[:, 0] + mr * rootn
    if family == LAT:
        yi[:, 0] = yi[:, 0] + mi * rootn
    return yr, yi


def _rows(x):
    re, im = widen(x)
    re = re.reshape(-1, re.shape[-1])
    im = re * 0 if im is None else im.reshape(re.shape)
    return re, im


def fftbr(x):
    """(re, im) [R, n] of real or complex rows x."""
    re, im = _rows(x)
    return transform(LAT, re, im)


def ifftbr(x):
    re, im = _rows(x)
    return transform(LAT, re, im, adjoint=True)


def fwht(x):
    re, _ = _rows(x)
    return transform(NET, re, re * 0)[0]


def ft(family, rows):
    """predict_reference.ft: the forward network of real extended rows."""
    return network(family, rows + 0, rows * 0)


# ------------------------------------------------------------------------------------------------ closed forms
def _phase(p, n):
    """cos, sin of 2 pi p / n for exact int64 p in [0, n)."""
    ang = _PI * (_x((2 * p).astype(np.float64)) / _xs(n))
    return _cos(ang), _sin(ang)


def _sparse_dft(pos, val, m, outs, sign):
    n = 1 << m
    vr, vi = widen(np.asarray(val, dtype=np.complex128))
    outs = np.asarray(outs, dtype=np.int64)
    re, im = _x(np.zeros(outs.shape)), _x(np.zeros(outs.shape))
    for j in range(len(pos)):
        p = (outs * int(pos[j])) % n if sign < 0 else (brev(outs, m) * int(pos[j])) % n
        c, s = _phase(p, n)
        s = s * sign
        re = re + (vr[j] * c - vi[j] * s)
        im = im + (vr[j] * s + vi[j] * c)
    sc = 1 / _sqrt(_xs(n))
    return re * sc, im * sc


def sparse_fftbr(idx, val, m, ks):
    """fftbr[k] = n^-1/2 sum_j x_j exp(-2 pi i k brev(i_j) / n) at the outputs ks."""
    return _sparse_dft(brev(idx, m), val, m, ks, -1)


def sparse_ifftbr(kidx, val, m, outs):
    """ifftbr[i] = n^-1/2 sum_j X_j exp(+2 pi i k_j brev(i) / n) at the outputs i."""
    return _sparse_dft(np.asarray(kidx, dtype=np.int64), val, m, outs, +1)


def _parity(v):
    v = np.asarray(v, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v ^ (v >> s)
    return v & 1


def sparse_fwht(idx, val, m, ks):
    ks = np.asarray(ks, dtype=np.int64)
    v = _x(np.asarray(val, dtype=np.float64))
    out = _x(np.zeros(ks.shape))
    for j in range(len(idx)):
        out = out + v[j] * _x(1.0 - 2.0 * _parity(ks & int(idx[j])))
    return out / _sqrt(_xs(1 << m))


# ------------------------------------------------------------------------------------------------ element-wise
def product(x, f):
    """x o f in extended precision, f broadcast over the rows: (re, im), im None if both are real."""
    xr, xi = widen(x)
    fr, fi = widen(f)
    if xi is None and fi is None:
        return xr * fr, None
    xi = xr * 0 if xi is None else xi
    fi = fr * 0 if fi is None else fi
    return xr * fr - xi * fi, xr * fi + xi * fr


def double_update(family, prev, nxt):
    """(re, im, B) [batch, 2n]: out[k], out[k + n] = (prev[k] +- w^k nxt[k]) / sqrt 2, w = exp(-pi i / n) (lattice) or 1;
    B = (|prev_k| + |nxt_k|) / sqrt 2, the magnitudes of the two terms."""
    pr, pi_ = widen(prev)
    nr, ni = widen(nxt)
    n = pr.shape[-1]
    if family == LAT:
        ang = -(_PI * (_x(np.arange(n, dtype=np.float64)) / _xs(n)))
        c, s = _cos(ang), _sin(ang)
        tr, ti = nr * c - ni * s, nr * s + ni * c
        mag = _sqrt(pr * pr + pi_ * pi_) + _sqrt(nr * nr + ni * ni)
    else:
        pi_, tr, ti = pr * 0, nr, nr * 0
        mag = abs(pr) + abs(nr)
    r = 1 / _sqrt(_xs(2))
    cat = lambda a, b: np.concatenate([a, b], -1)                            # noqa: E731
    return cat(pr + tr, pr - tr) * r, cat(pi_ + ti, pi_ - ti) * r, cat(mag, mag) * r


def sum_sq(x, G):
    """Y[g, k] = sum_r |x[r G + g, k]|^2 (extended) -- its terms are positive, so Y is its own bound."""
    re, im = widen(x)
    p = re * re + (0 if im is None else im * im)
    return p.reshape(-1, G, p.shape[-1]).sum(0)


def sum_sq_half(xh, n, G):
    """sum_sq of the Hermitian halves xh [R G, n/2 + 1], mirrored to k > n/2."""
    y = sum_sq(xh, G)
    return np.concatenate([y, y[:, 1:n // 2][:, ::-1]], -1)


def hermitian_full(xh, n):
    """The full rows [R, n] (complex128) of half rows [R, n/2 + 1]: X_{n-k} = conj X_k."""
    xh = np.asarray(xh)
    return np.concatenate([xh, np.conj(xh[:, 1:n // 2][:, ::-1])], -1)


# ------------------------------------------------------------------------------------------------ bounds
def centred(re, im, first):
    """(data_re, data_im): the rows minus the means of the path's first pass.  first = None (no centring), ("seg", L):
    means over consecutive segments of L (a row pass, or the whole row when L = n), ("col", N2): means over the columns
    k2 = index mod N2 (a column pass first)."""
    if first is None:
        return re, im
    kind, L = first
    Rn, n = re.shape

    def cen(a):
        if kind == "seg":
            b = a.reshape(Rn, n // L, L)
            return (b - (b.sum(-1) / L)[..., None]).reshape(Rn, n)
        b = a.reshape(Rn, n // L, L)
        return (b - (b.sum(1) / (n // L))[:, None, :]).reshape(Rn, n)
    return cen(re), cen(im)


def norm2(re, im=None):
    s = (re * re).sum(-1)
    if im is not None:
        s = s + (im * im).sum(-1)
    return _sqrt(s)


def dense_brackets(re, im, first):
    """(||data||_2, D) per row of the extended input rows re, im (the arrays the butterflies see: x, or x o f)."""
    dr, di = centred(re, im, first)
    return norm2(dr, di), norm2(re - dr, im - di)


def l1(re, im=None):
    return (abs(re) if im is None else _sqrt(re * re + im * im)).sum(-1)
