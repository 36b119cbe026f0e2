"""Extended-precision reference of the wide fit loops' own kernels, each with an error bound counted from the kernel's
roundings (the tracked values Tr of tests/mt_block_reference.py: a value in extended precision and its first-order twin):

  fgp_wide_fit_run      k_wide_fit_eig, k_wide_fit_loss_sums, k_wide_fit_loss_grad, k_wide_fit_step
  fgp_wide_mt_fit_run   k_wide_mt_lams, k_wide_mt_contract, k_wide_mt_fit_step

Every *_ref takes its inputs EXACTLY AS THE DEVICE PRODUCED the stage before (lambda for the terms, the partials for
the step, glp / z / logdet for the contraction), so no conditioning -- of the transform, the nugget or the adjoint --
enters a bound: the only disagreement left is the rounding of the stage itself.  The stages made of entry points that
are pinned elsewhere (k1, the transforms, the block calls, k1_bwd) are compared bit for bit with those entry points by
the GPU tests and have no reference here.

Roundings per operation as in mt_block_reference (-ffp-contract=off: a * b + c is two; __builtin_fma one; 1 / x and
sqrt correctly rounded; exp and log ULP_LIBM ulp; times a power of two exact; 0 + x exact).  sqrt(n) of the single-task
kernels is a host double handed to the kernel: an exact input; a power of two for even log2n, where its products are
exact.  gamma_C with the chain lengths below covers the second order, 2^-63 the reference's own arithmetic.

  C_terms     exp 2 ULP_LIBM, sqrt(n) l, + noise, 1 / ev, Y r, w -, * r, * hs: 7; log 2 ULP_LIBM; a lane's 2 kWfV terms;
              block_sum's 6 + 4:                              7 + 4 ULP_LIBM + 2 kWfV + 10
  C_sums      exp, 5 per element, the lane, block_sum:         6 + 2 ULP_LIBM + 2 kWfV + 10
  C_grad      the partials' second level ceil(nbe / 256) + 10, wide_loss_coef 6, the element 9, exp:
                                                               ceil(nbe / 256) + 25 + 2 ULP_LIBM
  C_step      second level ceil(nbe / 256) + 10, the coefficients 6, d additions (dl = 1), exp, 4 products / sums:
                                                               ceil(nbe / 256) + d + 20 + 2 ULP_LIBM
  C_mt_lams   sqrt, 2 products, exp, +, K_task's 2 rank + 1 + exp:            2 rank + 6 + 4 ULP_LIBM
  C_mt_contract  C_mt_lams, 3 for the entry, block_sum 10, ceil(B R nmin / (256 nbx)) strided fmas (2 each):
                                                               C_mt_lams + 13 + 2 ceil(B R nmin / (256 nbx))
  C_mt_step   second level ceil(nbx / 256) + 10, np additions of dsum, d more (dl = 1), T (T + 1) terms of 2, exp:
                                                               ceil(nbx / 256) + np + d + 2 T (T + 1) + 14 + 2 ULP_LIBM

`mutate` seeds one defect the CPU tests must see break a bound:
    "hs"      k_wide_fit_eig: hs = sqrt(n) for 1/2 sqrt(n)
    "pair"    k_wide_fit_eig / k_wide_fit_loss_sums: the pair's second element dropped from the partials
    "cv_w2"   k_wide_fit_loss_grad: CV's w2 taken as r^2
    "nk"      k_wide_mt_lams: sqrt(n_k) for sqrt(n_l)
    "nocj"    k_wide_mt_contract: the conjugate dropped in g~
    "tot"     k_wide_mt_fit_step: tot[2 p] read for tot[2 p + 1]
"""
import math

import numpy as np

from tests.mt_block_reference import (KWG, MP, U, ULP_LIBM, XT, Layout, Tr, _conv, bound, fma, ratio,  # noqa: F401
                                      rprop_f64, tree_sum, wg_sum)

KWFV = 4
KWF_BLOCK = KWG * 2 * KWFV            # frequencies per k_wide_fit_eig workgroup
LOSS_MLL, LOSS_GCV, LOSS_CV = 0, 1, 2
LAT, NET = 0, 1


def nbe_of(n):
    return -(-n // KWF_BLOCK)


def counts(n, d):
    lvl2 = -(-nbe_of(n) // KWG)
    return {"terms": 7 + 4 * ULP_LIBM + 2 * KWFV + 10, "sums": 6 + 2 * ULP_LIBM + 2 * KWFV + 10,
            "grad": lvl2 + 25 + 2 * ULP_LIBM, "step": lvl2 + d + 20 + 2 * ULP_LIBM}


def _ex(a, xt):
    return Tr.exact(np.asarray(a, dtype=np.float64), xt)


def _zeros(shape, xt):
    return _ex(np.zeros(shape), xt)


def _pow2(c):
    m, _ = math.frexp(abs(float(c)))
    return m == 0.5


def _mulc(t, c):
    """Times the exact double c: exact where c is a power of two."""
    return t.scaled(float(c)) if _pow2(c) else t * _ex(float(c), t.xt)


def _chain(terms):
    """Ascending sum onto 0 (the first exact)."""
    s = None
    for t in terms:
        s = t if s is None else s + t
    return s


def _f64(t):
    return np.asarray(t.v, dtype=np.float64) if t.xt is not object else np.array(t.v, dtype=np.float64)


def _nan_like(t):
    return Tr(np.full(np.shape(t.v), np.nan).astype(t.v.dtype) if t.xt is not object else np.full(np.shape(t.v), np.nan),
              np.zeros(np.shape(t.v)) if t.xt is not object else np.zeros(np.shape(t.v)), t.xt)


# ------------------------------------------------------------------------------------------------ single task
def lane_partials(terms, n, drop_second=False):
    """The per-workgroup partials of terms [G, n] in k_wide_fit_eig's order -> [G, nbe]: lane tid of workgroup blk holds
    k = blk 2048 + 512 v + 2 tid + e and adds its terms in (v, e) order onto 0 (its live terms are a prefix: n is a power
    of two), then block_sum."""
    G = terms.v.shape[0]
    nbe = nbe_of(n)
    pad = nbe * KWF_BLOCK - n

    def shaped(a):
        if pad:
            z = np.zeros((G, pad))
            a = np.concatenate([a, z.astype(a.dtype) if a.dtype != object else _conv(z, object)], -1)
        return a.reshape(G, nbe, KWFV, KWG, 2)

    v, e = shaped(terms.v), shaped(terms.e)
    live = np.broadcast_to(np.arange(n + pad) < n, (G, n + pad)).reshape(G, nbe, KWFV, KWG, 2)
    s = None
    for vv in range(KWFV):
        for ee in range(2):
            if drop_second and ee == 1:
                continue
            t = Tr(v[:, :, vv, :, ee], e[:, :, vv, :, ee], terms.xt)
            on = live[:, :, vv, :, ee]
            s = t.where(on, _zeros(t.v.shape, terms.xt)) if s is None else (s + t).where(on, s)
    return tree_sum(s)


def _ev(lam, raw_noise, n, xt):
    """(lp = sqrt(n) l, noise) of the device's lambda (real parts) [G, n] and raw_noise [G]."""
    sqrtn = float(np.sqrt(np.float64(n)))
    G = np.shape(lam)[0]
    noise = _ex(np.asarray(raw_noise).reshape(G, 1), xt).exp()
    noise = Tr(np.broadcast_to(noise.v, np.shape(lam)).copy(), np.broadcast_to(noise.e, np.shape(lam)).copy(), xt)
    return _mulc(_ex(lam, xt), sqrtn), noise, sqrtn


def eig_ref(lam, Y, raw_noise, n, w, xt=XT, mutate=None):
    """k_wide_fit_eig: {"gt": g~ [G, n], "pe": partials [G, 3, nbe]} as Tr."""
    lp, noise, sqrtn = _ev(lam, raw_noise, n, xt)
    y = _ex(Y, xt)
    ev = lp + noise
    r = ev.inv()
    yr = y * r
    t = (_ex(float(w), xt) - yr) * r
    hs = sqrtn if mutate == "hs" else 0.5 * sqrtn
    drop = mutate == "pair"
    rows = [lane_partials(q, n, drop) for q in (yr, ev.logabs(), t)]
    pe = Tr(np.stack([q.v for q in rows], 1), np.stack([q.e for q in rows], 1), xt)
    return {"gt": _mulc(t, hs), "pe": pe}


def loss_sums_ref(lam, Y, raw_noise, n, cv, xt=XT, mutate=None):
    """k_wide_fit_loss_sums: the partials [G, 4 (CV: 3), nbe] = (N1, T, S1, S2)."""
    lp, noise, _ = _ev(lam, raw_noise, n, xt)
    y = _ex(Y, xt)
    r = (lp + noise).inv()
    r2 = r * r
    yr2 = y * r2
    qs = [yr2, lp.inv() if cv else r, yr2 * r] + ([] if cv else [r2])
    rows = [lane_partials(q, n, mutate == "pair") for q in qs]
    return Tr(np.stack([q.v for q in rows], 1), np.stack([q.e for q in rows], 1), xt)


def loss_coef(N1, T, n, w, cv):
    """wide_loss_coef: (loss, c1, c2, t1, t2); T / n, n I^2 and n n D are exact (n a power of two)."""
    xt = N1.xt
    q = T.scaled(1.0 / n)
    D = q * q
    if cv:
        loss = _mulc(N1, w).div(D)
        c1 = _ex(np.full(np.shape(D.v), -2.0 * w), xt).div(D)
        c2 = _mulc(N1, 2.0 * w).div(D.scaled(float(n)) * q)
        return loss, c1, c2, _nan_like(loss), _nan_like(loss)
    loss = N1.div(D)
    c1 = _ex(np.full(np.shape(D.v), -2.0), xt).div(D)
    c2 = (N1.scaled(2.0) * T).div(D.scaled(float(n) * float(n)) * D)
    return loss, c1, c2, N1, D


def totals(pe):
    """The second level over the device partials pe [G, Q, nbe] (wide_fit_total / k_wide_fit_step's loops) -> [G, Q]."""
    return wg_sum(pe if isinstance(pe, Tr) else _ex(pe, XT))


def loss_grad_ref(lam, Y, raw_noise, pl, n, w, cv, xt=XT, mutate=None):
    """k_wide_fit_loss_grad: g~ [G, n] from the device's lambda and partials pl [G, 4, nbe] (row 3 unread under CV)."""
    lp, noise, sqrtn = _ev(lam, raw_noise, n, xt)
    y = _ex(Y, xt)
    tot = wg_sum(_ex(np.asarray(pl)[:, :2], xt))
    _, c1, c2, _, _ = loss_coef(tot[:, 0], tot[:, 1], n, w, cv)
    G = np.shape(lam)[0]
    c1 = Tr(c1.v.reshape(G, 1), c1.e.reshape(G, 1), xt)
    c2 = Tr(c2.v.reshape(G, 1), c2.e.reshape(G, 1), xt)
    r = (lp + noise).inv()
    r2 = r * r
    w2 = r2
    if cv and mutate != "cv_w2":
        rl = lp.inv()
        w2 = rl * rl
    return _mulc(c1 * ((y * r2) * r) + c2 * w2, sqrtn)


def step_ref(loss, pe, dscale, dls, nat_scale, nat_ls, raw, G, d, dl, n, w, mll_const, cv_weight, xt=XT):
    """k_wide_fit_step in mode 1 / 2 from the device's partials pe [G, 3 or 4, nbe], dscale [G], dls [G, d], the natural
    rows and raw: {"loss": [G, 3], "grad": [n_params]} as Tr."""
    cv = loss == LOSS_CV
    nq = 3 if loss in (LOSS_MLL, LOSS_CV) else 4
    S = wg_sum(_ex(np.asarray(pe)[:, :nq], xt))
    raw = np.asarray(raw, dtype=np.float64)
    if loss == LOSS_MLL:
        t2 = _mulc(S[:, 1], w)
        rows = [(S[:, 0] + t2).scaled(0.5) + _ex(np.full(G, float(mll_const)), xt), S[:, 0], t2]
        gnoise = S[:, 2].scaled(0.5)
    else:
        l0, c1, c2, t1, t2 = loss_coef(S[:, 0], S[:, 1], n, cv_weight, cv)
        rows = [l0, t1, t2]
        gnoise = c1 * S[:, 2] if cv else c1 * S[:, 2] + c2 * S[:, 3]
    lh = Tr(np.stack([q.v for q in rows], 1), np.stack([q.e for q in rows], 1), xt)
    ds, dl_, ns, nl = (_ex(a, xt) for a in (dscale, np.asarray(dls).reshape(G, d), nat_scale, np.asarray(nat_ls).reshape(G, d)))
    g_scale = ns * ds
    if dl == d:
        g_ls = nl * dl_
        g_ls = Tr(g_ls.v.reshape(-1), g_ls.e.reshape(-1), xt)
    else:
        g_ls = nl[:, 0] * _chain([dl_[:, j] for j in range(d)])
    g_noise = _ex(raw[G + G * dl:], xt).exp() * gnoise
    grad = Tr(np.concatenate([g_scale.v, g_ls.v, g_noise.v]), np.concatenate([g_scale.e, g_ls.e, g_noise.e]), xt)
    return {"loss": lh, "grad": grad}


def nat_ref(raw, G, d, dl, xt=XT):
    """The natural rows the step writes for the next k1: (nat_scale [G], nat_ls [G, d]) = exp of the raw rows."""
    raw = np.asarray(raw, dtype=np.float64)
    ls = raw[G:G + G * dl].reshape(G, dl)
    return _ex(raw[:G], xt).exp(), _ex(ls if dl == d else np.repeat(ls, d, 1), xt).exp()


def rg_mask(G, dl, rg):
    return np.concatenate([np.full(G, bool(rg[0])), np.full(G * dl, bool(rg[1])), np.full(G, bool(rg[2]))])


def rel(got, t, C):
    """max err / bound of a device (or restated) float64 array against the tracked reference t; NaN must meet NaN."""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(t.v))
    tv = np.array(t.v, dtype=np.float64) if t.xt is object else t.v
    nan = np.isnan(np.asarray(tv, dtype=np.float64))
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    if nan.all():
        return 0.0
    keep = ~nan
    return ratio(got[keep], t.v[keep], t.e[keep], C)


def vacuity(t, C):
    """||u e||_1 / (100 2^-53 C ||value||_1) over the finite elements (<= 1 asserted), and whether every twin is finite."""
    v = np.abs(np.asarray(t.v, dtype=np.float64)).reshape(-1)
    e = np.asarray(t.e, dtype=np.float64).reshape(-1)
    keep = ~np.isnan(v)
    fin = bool(np.isfinite(e[keep]).all())
    den = 100.0 * C * float(v[keep].sum())
    num = float(e[keep].sum())
    return (num / den if den > 0 else (0.0 if num == 0 else float("inf"))), fin


# ------------------------------------------------------------------------------------------------ multitask
class MtSpec(object):
    """One fgp_wide_mt_fit_run problem on the host: ns (descending), d, dl, B, family, task [T], T_all, rank, vtask_exp,
    conj [np] (0 / 1 per sorted pair), logdet_weight, mll_const."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.lay = Layout(self.ns)
        T = self.T = self.lay.T
        self.np = T * (T + 1) // 2
        self.pairs = [(k, l) for k in range(T) for l in range(k, T)]
        self.noise_off = 1 + self.dl
        self.f_off = self.noise_off + 1
        self.v_off = self.f_off + self.T_all * self.rank
        self.n_params = self.v_off + self.T_all
        self.nbx = -(-self.ns[0] // KWG)
        self.rn = self.lay.R * self.lay.nmin

    def counts(self):
        T = self.T
        c_lams = 2 * self.rank + 6 + 4 * ULP_LIBM
        return {"lams": c_lams, "contract": c_lams + 13 + 2 * -(-self.B * self.rn // (KWG * self.nbx)),
                "step": -(-self.nbx // KWG) + self.np + self.d + 2 * T * (T + 1) + 14 + 2 * ULP_LIBM}

    def rg_mask(self, rg):
        m = np.zeros(self.n_params, dtype=bool)
        for flag, lo, hi in zip(rg, (0, 1, self.noise_off, self.f_off, self.v_off),
                                (1, self.noise_off, self.f_off, self.v_off, self.n_params)):
            m[lo:hi] = bool(flag)
        return m


def _sc(v, xt):
    return Tr.exact(np.asarray(float(v)).reshape(()), xt)


def _kt(sp, raw, a, b, xt):
    """wmf_kt: sum_r F[a, r] F[b, r] (onto 0: the first exact) + [a == b] v_a."""
    s = None
    for r in range(sp.rank):
        t = _sc(raw[sp.f_off + a * sp.rank + r], xt) * _sc(raw[sp.f_off + b * sp.rank + r], xt)
        s = t if s is None else s + t
    if a == b:
        va = _sc(raw[sp.v_off + a], xt)
        va = va.exp() if sp.vtask_exp else va
        s = va if s is None else s + va
    return s if s is not None else _sc(0.0, xt)


def _rootn(n, xt):
    r = math.isqrt(n)
    return _sc(float(r), xt) if r * r == n else _sc(float(n), xt).sqrt()


def _fill(t, n):
    return Tr(np.broadcast_to(t.v, (n,)).copy(), np.broadcast_to(t.e, (n,)).copy(), t.xt)


def _entry(sp, raw, lam, p, xt, mutate=None):
    """(bx, by, K_task, sqrt(n_l), cj) of the entries of pair p: b = sqrt(n_l) lam^ + noise [k == l]."""
    k, l = sp.pairs[p]
    lay = sp.lay
    sl = slice(lay.off[k, l], lay.off[k, l] + lay.ns[k])
    cj = bool(sp.conj[p])
    lam = np.asarray(lam)
    vx = _ex(lam.real[sl], xt)
    vy = _ex(lam.imag[sl] if np.iscomplexobj(lam) else np.zeros(lay.ns[k]), xt)
    if cj:
        vy = -vy
    rn = _rootn(lay.ns[k] if mutate == "nk" else lay.ns[l], xt)
    rnf = _fill(rn, lay.ns[k])
    bx, by = rnf * vx, rnf * vy
    if k == l:
        bx = bx + _fill(_sc(raw[sp.noise_off], xt).exp(), lay.ns[k])
    return sl, bx, by, _kt(sp, raw, sp.task[k], sp.task[l], xt), rn, cj


def mt_lams_ref(sp, raw, lam, xt=XT, mutate=None):
    """k_wide_mt_lams: (x, y) Tr [L] from the device's lambda [L] (complex128 lattice / float64 net)."""
    L = sp.lay.L
    X, Y = _zeros(L, xt), _zeros(L, xt)
    for p in range(sp.np):
        sl, bx, by, kt, _, _ = _entry(sp, raw, lam, p, xt, mutate)
        ktf = _fill(kt, bx.v.shape[0])
        X[sl] = bx * ktf
        Y[sl] = by * ktf
    return X, Y


def _wg_partials(t, n):
    """block_sum per workgroup of 256 entries of t [n] (lanes past n add 0) -> [ceil(n / 256)]."""
    nb = -(-n // KWG)
    pad = nb * KWG - n

    def shaped(a):
        if pad:
            z = np.zeros(pad)
            a = np.concatenate([a, z.astype(a.dtype) if a.dtype != object else _conv(z, object)])
        return a.reshape(nb, KWG)

    return tree_sum(Tr(shaped(t.v), shaped(t.e), t.xt))


def mt_contract_ref(sp, raw, glp, lam, y, z, logdet, xt=XT, mutate=None):
    """k_wide_mt_contract from the device's glp [L], lambda [L], z [B, R nmin], logdet [nmin] and y: {"gx", "gy": g~ [L],
    "part": [np + 1, 2, nbx] (NaN where the kernel writes nothing), "written": bool [np + 1, 2, nbx]}."""
    lay, L, nbx = sp.lay, sp.lay.L, sp.nbx
    GX, GY = _zeros(L, xt), _zeros(L, xt)
    pv = np.full((sp.np + 1, 2, nbx), np.nan, dtype=np.float64 if xt is object else xt)
    pe = np.zeros((sp.np + 1, 2, nbx), dtype=np.float64 if xt is object else xt)
    if xt is object:
        pv, pe = pv.astype(object), pe.astype(object)
    written = np.zeros((sp.np + 1, 2, nbx), dtype=bool)
    glp = np.asarray(glp)
    for p in range(sp.np):
        sl, bx, by, kt, rn, cj = _entry(sp, raw, lam, p, xt)
        nk = bx.v.shape[0]
        gx, gy = _ex(glp.real[sl], xt), _ex(glp.imag[sl], xt)
        f = _fill(kt * rn, nk)
        s1 = fma(gx, bx, gy * by)
        GX[sl] = f * gx
        fy = f * gy
        GY[sl] = -fy if (cj and mutate != "nocj") else fy
        nb = -(-nk // KWG)
        for q, t in ((0, gx), (1, s1)):
            tot = _wg_partials(t, nk)
            pv[p, q, :nb], pe[p, q, :nb] = tot.v, tot.e
            written[p, q, :nb] = True
    if sp.family == NET:
        GY = _zeros(L, xt)
    # row np: thread t0 = blk 256 + tid over e = t0, t0 + nt, ...
    nt = nbx * KWG
    yy, zz = np.asarray(y).reshape(-1), np.asarray(z).reshape(-1)
    yz = sp.B * sp.rn
    acc0, acc1 = _zeros(nt, xt), _zeros(nt, xt)
    for i in range(-(-yz // nt)):
        lo, hi = i * nt, min(yz, (i + 1) * nt)
        m = hi - lo
        yx, yi, zx, zi = (_ex(a[lo:hi], xt) for a in (yy.real, yy.imag, zz.real, zz.imag))
        acc0[:m] = fma(yx, zx, fma(yi, zi, acc0[:m]))
    ld = _ex(logdet, xt)
    for i in range(-(-lay.nmin // nt)):
        lo, hi = i * nt, min(lay.nmin, (i + 1) * nt)
        m = hi - lo
        acc1[:m] = ld[lo:hi] if i == 0 else acc1[:m] + ld[lo:hi]
    for q, a in ((0, acc0), (1, acc1)):
        tot = tree_sum(Tr(a.v.reshape(nbx, KWG), a.e.reshape(nbx, KWG), xt))
        pv[sp.np, q], pe[sp.np, q] = tot.v, tot.e
        written[sp.np, q] = True
    return {"gx": GX, "gy": GY, "part": Tr(pv, pe, xt), "written": written}


def mt_step_ref(sp, raw, part, dsl, nat, xt=XT, mutate=None):
    """k_wide_mt_fit_step in mode 1 / 2 from the device's partials part [np + 1, 2, nbx], dsl [np, 1 + d] and the natural
    row nat [1 + d]: {"loss": [3], "grad": [n_params]} as Tr.  Only the first ceil(n_k / 256) partials of a pair are read."""
    T, d, dl, npairs = sp.T, sp.d, sp.dl, sp.np
    raw = np.asarray(raw, dtype=np.float64)
    part = np.asarray(part, dtype=np.float64)
    tot = {}
    for p in range(npairs + 1):
        cnt = sp.nbx
        if p < npairs:
            k, l = sp.pairs[p]
            cnt = -(-sp.ns[k] // KWG)
        for q in range(2):
            if p < npairs and q == 0 and k != l and mutate != "tot":
                continue
            tot[2 * p + q] = wg_sum(_ex(part[p, q, :cnt], xt))
    D = _ex(dsl, xt)
    dsum = [_chain([D[p, t] for p in range(npairs)]) for t in range(1 + d)]
    N = _ex(nat, xt)
    diag = [k * T - k * (k - 1) // 2 for k in range(T)]
    rd = (lambda p: tot[2 * p]) if mutate == "tot" else (lambda p: tot[2 * p + 1])
    gs = []
    for x in range(sp.n_params):
        if x == 0:
            g = N[0] * dsum[0]
        elif x < sp.noise_off:
            j = x - 1
            g = N[1 + j] * dsum[1 + j] if dl == d else N[1] * _chain([dsum[1 + jj] for jj in range(d)])
        elif x == sp.noise_off:
            a = _chain([_kt(sp, raw, sp.task[k], sp.task[k], xt) * tot[2 * diag[k]] for k in range(T)])
            g = _sc(raw[x], xt).exp() * a
        elif x < sp.v_off:
            c, r = divmod(x - sp.f_off, sp.rank)
            terms = []
            for p, (k, l) in enumerate(sp.pairs):
                a, b = sp.task[k], sp.task[l]
                if a == c:
                    terms.append(rd(p) * _sc(raw[sp.f_off + b * sp.rank + r], xt))
                if b == c:
                    terms.append(rd(p) * _sc(raw[sp.f_off + a * sp.rank + r], xt))
            g = _chain(terms) if terms else _sc(0.0, xt)
        else:
            c = x - sp.v_off
            terms = [rd(diag[k]) * _sc(raw[x], xt).exp() if sp.vtask_exp else rd(diag[k]) for k in range(T) if sp.task[k] == c]
            g = _chain(terms) if terms else _sc(0.0, xt)
        gs.append(g)
    grad = Tr(np.array([g.v for g in gs], dtype=None if xt is object else xt).reshape(-1),
              np.array([g.e for g in gs], dtype=None if xt is object else xt).reshape(-1), xt)
    t1 = tot[2 * npairs]
    t2 = _mulc(tot[2 * npairs + 1], sp.logdet_weight)
    rows = [(t1 + t2).scaled(0.5) + _sc(sp.mll_const, xt), t1, t2]
    loss = Tr(np.array([q.v for q in rows], dtype=None if xt is object else xt).reshape(-1),
              np.array([q.e for q in rows], dtype=None if xt is object else xt).reshape(-1), xt)
    return {"loss": loss, "grad": grad}


def mt_nat_ref(sp, raw, xt=XT):
    raw = np.asarray(raw, dtype=np.float64)
    ls = raw[1:1 + sp.dl]
    return _ex(np.concatenate([raw[:1], ls if sp.dl == sp.d else np.repeat(ls, sp.d)]), xt).exp()
