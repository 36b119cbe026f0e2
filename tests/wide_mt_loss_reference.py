"""Extended-precision restatement of the GCV / CV stage of fgp_wide_mt_fit_run (csrc/fgp_wide_mt_fit.hip:
k_wide_mt_loss_sums, k_wide_mt_loss_grad, wmf_loss_coef and the loss row of k_wide_mt_fit_step), operation by operation,
in the tracked arithmetic of tests/mt_block_reference.py (Tr: a value in numpy.longdouble and its first-order twin, one
|intermediate| per rounding the kernel commits) -- T tasks of EQUAL n, B data vectors, one problem.

Inputs are the device's own arrays of the stage before: zinv [np n] (the selected inverse: with equal n the whole dense
A_j = Lambda_j^-1, upper triangle, packed as the lams, pair (k, l) at (offk[k] + (l - k) n)), z [B, T n] and, for the
gradient and the loss row, the partials pl [NT, 2, nbx] -- so no conditioning enters a bound.

  sums   per thread j: GCV s0 = fma(z.x, z.x, fma(z.y, z.y, s0)) over b ascending, t ascending inside; s1 += Re A[t, t]
         over t (onto 0: the first exact).  CV: the same for the one task of the workgroup.  Then block_sum.
         Chain: 2 B T + T + 10 (block_sum's 6 + 4).                                      C_sums = 2 B T + T + 10
  coef   GCV: q = Tr / (T n), D = q q, loss = N / D, c1 = 1 / D, c2 = 2 N / (D Tr): 3 to D, 2 more to c2.
         CV:  D = S S, c1 = w n^2 / D, loss_t = c1 N, c2 = 2 loss_t / S (w n^2 and the doubling exact): 4.
  grad   the second level ceil(nbx / 256) + 10, coef 5; per t: B accumulations of a cmulc (2) and an addition, three
         products (2 each, 1 for a net's real A) and an addition, two fmas; T of them in a chain; the doubling exact.
                                                                                         C_grad = ceil(nbx / 256) + 15 + T (3 B + 9)
  row    second level, coef, T additions (CV).                                           C_row = ceil(nbx / 256) + 15 + T

The C only feed the second-order factor 1 / (1 - C u) of mt_block_reference.bound; the first-order count of every output
is in its twin.  Nets (FAM 1): the kernel reads the real parts of A only and drops the products with the (identically
zero) imaginary parts -- the bits and the roundings of the complex form on a zero imaginary part, so one restatement
serves both families (pass zinv with zero imaginary parts).

`mutate` = "noc2": the c2 term of the gradient (GCV: the -2 N / (D Tr) dTr term) dropped -- the seeded defect a test must
see break the bound.

closed_forms(): the same functions from dense Hermitian blocks and data, for the CPU test that holds the closed forms
and the glp convention against torch autograd."""
import numpy as np

from tests.mt_block_reference import KWG, XT, Cx, Tr, cmul, cmulc, fma, wg_sum
from tests.wide_fit_reference import _chain, _ex, _wg_partials

LOSS_GCV, LOSS_CV = 1, 2


def nbx_of(n):
    return -(-n // KWG)


def counts(T, n, B):
    lvl2 = -(-nbx_of(n) // KWG)
    return {"sums": 2 * B * T + T + 10, "grad": lvl2 + 15 + T * (3 * B + 9), "row": lvl2 + 15 + T}


def offk(T, n):
    """Packed offset of pair (k, k); pair (k, l) at offk[k] + (l - k) n."""
    return [n * (k * T - k * (k - 1) // 2) for k in range(T)]


def _cx(a, shape, xt):
    """A complex array (or an already tracked Cx) as a Cx of the given shape."""
    if isinstance(a, Cx):
        return Cx(Tr(a.x.v.reshape(shape), a.x.e.reshape(shape), xt), Tr(a.y.v.reshape(shape), a.y.e.reshape(shape), xt))
    return Cx.exact(np.asarray(a).reshape(shape), xt)


def _cadd(a, b):
    return b if a is None else Cx(a.x + b.x, a.y + b.y)


def _stack(rows, xt):
    return Tr(np.stack([r.v for r in rows]), np.stack([r.e for r in rows]), xt)


def _ainv(Z, T, n, r, t):
    """A[r, t] over the frequencies, from the packed upper triangle Z [np, n] (conjugated below the diagonal)."""
    lo, hi = min(r, t), max(r, t)
    e = Z[offk(T, 1)[lo] + (hi - lo)]
    return e if r <= t else Cx(e.x, -e.y)


def loss_sums_ref(T, n, B, zinv, z, cv, xt=XT):
    """k_wide_mt_loss_sums: the partials [NT, 2, nbx] as Tr (NT = T under CV, else 1)."""
    Z = _cx(zinv, (T * (T + 1) // 2, n), xt)
    zz = _cx(z, (B, T, n), xt)
    zero = _ex(np.zeros(n), xt)
    rows = []
    for grp in ([[t] for t in range(T)] if cv else [list(range(T))]):
        s0 = zero
        for b in range(B):
            for t in grp:
                zv = zz[b, t]
                s0 = fma(zv.x, zv.x, fma(zv.y, zv.y, s0))
        s1 = _chain([_ainv(Z, T, n, t, t).x for t in grp])
        rows.append(_stack([_wg_partials(s0, n), _wg_partials(s1, n)], xt))
    return _stack(rows, xt)


def loss_coef(cv, N, S, T, n, w):
    """wmf_loss_coef: (loss, c1, c2, D) of Tr scalars; w n^2 is exact (n a power of two)."""
    xt = N.xt
    if cv:
        D = S * S
        c1 = _ex(np.full(np.shape(D.v), float(w) * float(n) * float(n)), xt).div(D)
        loss = c1 * N
        return loss, c1, loss.scaled(2.0).div(S), D
    q = S.div(_ex(np.full(np.shape(S.v), float(T) * float(n)), xt))
    D = q * q
    return N.div(D), D.inv(), N.scaled(2.0).div(D * S), D


def totals(pl, xt=XT):
    """The second level over the device partials pl [NT, 2, nbx] (float64; or tracked already) -> Tr [NT, 2]."""
    return wg_sum(pl if isinstance(pl, Tr) else _ex(np.asarray(pl, dtype=np.float64), xt))


def loss_row_ref(T, n, pl, cv, w, xt=XT):
    """The history row of k_wide_mt_fit_step: (loss, N, D) under GCV, (loss, NaN, NaN) under CV, as Tr [3]."""
    tot = totals(pl, xt)
    terms, N, D = [], None, None
    for t in range(T if cv else 1):
        loss, _, _, D = loss_coef(cv, tot[t, 0], tot[t, 1], T, n, w)
        N = tot[t, 0]
        terms.append(loss)
    loss = _chain(terms)
    nan = _ex(np.array(np.nan), xt)
    return _stack([loss, nan, nan] if cv else [loss, N, D], xt)


def loss_grad_ref(T, n, B, zinv, z, pl, cv, w, xt=XT, mutate=None):
    """k_wide_mt_loss_grad: glp (x, y) as Tr [np n] from the device's zinv, z and partials."""
    npairs = T * (T + 1) // 2
    Z = _cx(zinv, (npairs, n), xt)
    zz = _cx(z, (B, T, n), xt)
    tot = totals(pl, xt)
    c1s, c2s = [], []
    for t in range(T if cv else 1):
        _, c1, c2, _ = loss_coef(cv, tot[t, 0], tot[t, 1], T, n, w)
        if mutate == "noc2":
            c2 = _ex(np.zeros(np.shape(c2.v)), xt)
        c1s.append(Tr(np.broadcast_to(c1.v, (n,)).copy(), np.broadcast_to(c1.e, (n,)).copy(), xt))
        c2s.append(Tr(np.broadcast_to(c2.v, (n,)).copy(), np.broadcast_to(c2.e, (n,)).copy(), xt))
    GX, GY = _ex(np.zeros((npairs, n)), xt), _ex(np.zeros((npairs, n)), xt)
    zero = _ex(np.zeros(n), xt)
    ok = offk(T, 1)
    for r in range(T):
        for c in range(r, T):
            wx, wy = zero, zero
            for t in range(T):
                art, act = _ainv(Z, T, n, r, t), _ainv(Z, T, n, c, t)
                srt = stc = None
                for b in range(B):
                    zr, zt, zc = zz[b, r], zz[b, t], zz[b, c]
                    srt = _cadd(srt, cmulc(zr, zt))
                    stc = _cadd(stc, cmulc(zt, zc))
                e1 = cmulc(art, act)
                e2 = _cadd(cmulc(srt, act), cmul(art, stc))
                c1, c2 = c1s[t if cv else 0], c2s[t if cv else 0]
                wx = fma(-c1, e2.x, fma(c2, e1.x, wx))
                wy = fma(-c1, e2.y, fma(c2, e1.y, wy))
            e = ok[r] + (c - r)
            if r == c:
                GX[e], GY[e] = wx, zero
            else:
                GX[e], GY[e] = wx.scaled(2.0), wy.scaled(2.0)
    flat = lambda t: Tr(t.v.reshape(-1), t.e.reshape(-1), xt)       # noqa: E731
    return flat(GX), flat(GY)


# ------------------------------------------------------------------------------------------------ from dense blocks
def pack_upper(M):
    """Dense [n, T, T] -> the packed upper triangle [np n] (pair (k, l) row-major, the frequency fastest)."""
    T = M.shape[-1]
    return np.concatenate([M[:, k, l] for k in range(T) for l in range(k, T)])


def inverse_ld(lam):
    """The inverses of the dense blocks lam [n, T, T] complex128 to long double accuracy: numpy's float64 inverse refined
    by two Newton steps X <- X (2 I - lam X) in long double (real and imaginary parts kept apart: numpy has no
    long-double linear algebra)."""
    ld = np.longdouble
    X = np.linalg.inv(lam)
    xr, xi = X.real.astype(ld), X.imag.astype(ld)
    ar, ai = lam.real.astype(ld), lam.imag.astype(ld)
    eye2 = 2 * np.eye(lam.shape[-1], dtype=ld)
    mm = lambda a, b: np.einsum("nij,njk->nik", a, b)               # noqa: E731
    for _ in range(2):
        pr, pi = mm(ar, xr) - mm(ai, xi), mm(ar, xi) + mm(ai, xr)
        qr, qi = eye2 - pr, -pi
        xr, xi = mm(xr, qr) - mm(xi, qi), mm(xr, qi) + mm(xi, qr)
    return xr, xi


def closed_forms(lam, y, cv, w, mutate=None):
    """(loss, dL/dlams packed x, y) of the two kernels' restatement in long double, from dense Hermitian blocks lam
    [n, T, T] and data y [B, T, n] (transform domain): A and z = A y in long double, then loss_sums_ref, loss_row_ref and
    loss_grad_ref on them, the partials handed on in long double (no float64 rounding anywhere between)."""
    ld = np.longdouble
    n, T = lam.shape[0], lam.shape[-1]
    B = y.shape[0]
    xr, xi = inverse_ld(lam)
    yr, yi = y.real.astype(ld), y.imag.astype(ld)
    zr = np.einsum("nts,bsn->btn", xr, yr) - np.einsum("nts,bsn->btn", xi, yi)
    zi = np.einsum("nts,bsn->btn", xr, yi) + np.einsum("nts,bsn->btn", xi, yr)
    Z = Cx(Tr.exact(pack_upper(xr), ld), Tr.exact(pack_upper(xi), ld))
    zz = Cx(Tr.exact(zr, ld), Tr.exact(zi, ld))
    pl = loss_sums_ref(T, n, B, Z, zz, cv, ld)
    row = loss_row_ref(T, n, pl, cv, w, ld)
    gx, gy = loss_grad_ref(T, n, B, Z, zz, pl, cv, w, ld, mutate)
    return row.v[0], gx.v, gy.v
