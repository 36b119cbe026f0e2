"""Extended-precision reference of ONE spectral fit iteration (csrc/fgp_spectral.hip), with a first-order bound.

The spectral iteration reads the part-product spectra Phi [2^d, K], Y [K] and 2 + d natural parameters and returns a
loss row and a gradient.  This module evaluates the same closed form from the same arrays in 80-bit arithmetic
(np.longdouble, eps 1.1e-19; mpmath at 40 digits where the platform's long double is no wider than a double), so the
only disagreement left with a kernel is the kernel's own fp64 rounding -- the nugget does not amplify anything,
unlike a comparison with a lambda recomputed by another fp64 transform.

With weights w (lattice, K = n/2 + 1: w_0 = w_{n/2} = 1, else 2; net, K = n: 1) and
    T_{S,k} = (prod_{j in S} l_j) Phi_S[k],  P_k = sum_S T_{S,k},  dP_{j,k} = sum_{S contains j} T_{S,k},
    ev_k = sqrt(n) scale P_k + noise:
MLL   norm = sum w Y / ev, logdet = sum w log|ev|, loss = (norm + wl logdet + mll_const) / 2, g = wl / ev - Y / ev^2,
      dL/draw_scale = 1/2 sum w g sqrt(n) scale P, dL/draw_l_j = 1/2 sum w g sqrt(n) scale dP_j,
      dL/draw_noise = 1/2 noise sum w g;                                   history row [loss, norm, wl logdet]
GCV   N1 = sum w Y / ev^2, T = sum w / ev, loss = N1 / (T / n)^2           history row [loss, N1, (T / n)^2]
CV    N1 as GCV, T = sum w / (sqrt(n) scale P), loss = cv_weight N1 / (T / n)^2      history row [loss, nan, nan]
      (include/fgp_hip.h, ABI 16 block of fgp_nll_desc); both: dL/dtheta = c1 S1 + c2 S2 with
      S1 = sum w Y / ev^3 dev/dtheta, S2 = sum w x^-2 dx/dtheta (x = ev; CV: x = sqrt(n) scale P, no noise term),
      c1 = -2 cw n^2 / T^2, c2 = 2 cw N1 n^2 / T^3.

Error bound B_q of every output q (same pass): the fp64 evaluation of P_k carries an absolute error of order
eps A_k, A_k = sum_S |T_{S,k}| (A_{j,k} over S containing j), i.e. delta_k = sqrt(n) scale A_k on ev_k; every sum
carries eps times the sum of the magnitudes of its terms.  To first order
    B_norm = sum w (|Y / ev| + |Y / ev^2| delta),  B_logdet = sum w (|log|ev|| + 1 + delta / |ev|)
    dg = (wl / ev^2 + 2 Y / |ev|^3) delta,  B_scale = 1/2 sum w (|g| sqrt(n) scale A + dg sqrt(n) scale |P|),
    B_{l_j} likewise with A_j, |dP_j|,  B_noise = 1/2 noise sum w (|g| + dg),
    B_loss = (B_norm + wl B_logdet + |mll_const|) / 2
(the + 1 in B_logdet: the kernels accumulate the product of frexp mantissas, an absolute eps per term however small
|log ev| is).  GCV / CV: the bounds of the sums N1, T, S1, S2, formed the same way, propagated through the quotient
to first order, |df/ds| B_s summed over the sums s.  A kernel must satisfy |device - reference| <= C 2^-53 B_q with C
the number of roundings it makes per term and per summation level (tests/test_gpu_spectral_exact.py).
"""
import numpy as np

if np.finfo(np.longdouble).eps < 2e-19:
    MP = False
    XT = np.longdouble

    def _x(a):
        return np.asarray(a, dtype=np.float64).astype(np.longdouble)

    def _xs(v):
        return np.longdouble(float(v))

    _log, _sqrt = np.log, np.sqrt
else:                                                       # long double == double: mpmath, 40 digits
    import mpmath
    MP = True
    mpmath.mp.dps = 40
    XT = mpmath.mpf
    _tomp = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)

    def _x(a):
        return _tomp(np.asarray(a, dtype=np.float64))

    def _xs(v):
        return mpmath.mpf(float(v))

    _log, _sqrt = np.frompyfunc(mpmath.log, 1, 1), np.frompyfunc(mpmath.sqrt, 1, 1)

EPS53 = 2.0 ** -53
assert MP or np.finfo(np.longdouble).eps < 2e-19
KEYS = ("loss", "t1", "t2", "scale", "ls", "noise")


def spec_K(n, net):
    return n if net else n // 2 + 1


def weights(n, net):
    w = np.full(spec_K(n, net), 1.0 if net else 2.0)
    if not net:
        w[0] = w[-1] = 1.0
    return w


def chunked(dense):
    """[(G,) 2^d, K] -> the kernels' layout [(G,) Q, 2^d, 64], zero past K (fgp_spec_basis)."""
    dense = np.asarray(dense, dtype=np.float64)
    K = dense.shape[-1]
    Q = (K + 63) // 64
    pad = np.zeros(dense.shape[:-1] + (Q * 64,))
    pad[..., :K] = dense
    return np.ascontiguousarray(np.moveaxis(pad.reshape(dense.shape[:-1] + (Q, 64)), -2, -3))


def dense(chunks, K):
    """[(G,) Q, 2^d, 64] -> [(G,) 2^d, K] (fit_engine.spec_dense)."""
    c = np.moveaxis(np.asarray(chunks, dtype=np.float64), -3, -2)
    return np.ascontiguousarray(c.reshape(c.shape[:-2] + (c.shape[-2] * 64,))[..., :K])


def even_extend(Yh, n):
    """Y [.., n/2 + 1] of a lattice -> [.., n] with Y[n - k] = Y[k]."""
    Yh = np.asarray(Yh, dtype=np.float64)
    out = np.empty(Yh.shape[:-1] + (n,))
    out[..., :n // 2 + 1] = Yh
    out[..., n // 2 + 1:] = Yh[..., 1:n // 2][..., ::-1]
    return out


def _f(v):
    return float(v)


def evaluate(Phi, Y, scale, ls, noise, n, net, loss="MLL", wl=1.0, mll_const=0.0, cv_weight=1.0, w=None):
    """One problem: (val, bnd), dicts over KEYS ('ls' a float64 array [d], the rest floats; t1 / t2 the history
    columns 1 and 2, nan for CV) of the values and of their first-order bounds B_q.  `w` replaces the frequency
    weights (the tests' own sensitivity check: what a kernel with one wrong weight would return)."""
    Phi = np.asarray(Phi, dtype=np.float64)
    NS, K = Phi.shape
    d = NS.bit_length() - 1
    assert NS == 1 << d and K == spec_K(n, net) and len(ls) == d and np.shape(Y) == (K,)
    ph, y, w = _x(Phi), _x(Y), _x(weights(n, net) if w is None else w)
    sc, nz, l = _xs(scale), _xs(noise), _x(ls)
    rootn = _sqrt(_xs(n))
    lS = np.array([XT(1)] * NS, dtype=object if MP else np.longdouble)
    for S in range(NS):
        for j in range(d):
            if (S >> j) & 1:
                lS[S] = lS[S] * l[j]
    Tm = lS[:, None] * ph
    P, A = Tm.sum(0), abs(Tm).sum(0)
    has = [[S for S in range(NS) if (S >> j) & 1] for j in range(d)]
    dP = [Tm[has[j]].sum(0) for j in range(d)]
    Aj = [abs(Tm[has[j]]).sum(0) for j in range(d)]
    rs = rootn * sc
    lp = rs * P
    ev = lp + nz
    delta = rs * A
    aev = abs(ev)
    val, bnd = {}, {}
    if loss == "MLL":
        wlx, cx = _xs(wl), _xs(mll_const)
        norm = (w * y / ev).sum()
        lg = _log(aev)
        logdet = (w * lg).sum()
        g = wlx / ev - y / ev ** 2
        Bn = (w * (abs(y / ev) + abs(y / ev ** 2) * delta)).sum()
        Bl = (w * (abs(lg) + 1 + delta / aev)).sum()
        dg = (abs(wlx) / ev ** 2 + 2 * abs(y) / aev ** 3) * delta
        ag = abs(g)
        val["loss"], bnd["loss"] = _f((norm + wlx * logdet + cx) / 2), _f((Bn + abs(wlx) * Bl + abs(cx)) / 2)
        val["t1"], bnd["t1"] = _f(norm), _f(Bn)
        val["t2"], bnd["t2"] = _f(wlx * logdet), _f(abs(wlx) * Bl)
        val["scale"] = _f((w * g * lp).sum() / 2)
        bnd["scale"] = _f((w * (ag * delta + dg * abs(lp))).sum() / 2)
        val["ls"] = np.array([_f((w * g * rs * dP[j]).sum() / 2) for j in range(d)])
        bnd["ls"] = np.array([_f((w * (ag * rs * Aj[j] + dg * rs * abs(dP[j]))).sum() / 2) for j in range(d)])
        val["noise"], bnd["noise"] = _f(nz * (w * g).sum() / 2), _f(nz * (w * (ag + dg)).sum() / 2)
        return val, bnd
    assert loss in ("GCV", "CV")
    cv = loss == "CV"
    cw = _xs(cv_weight) if cv else XT(1)
    nn = _xs(n)
    ay = abs(y)
    x = lp if cv else ev
    ax = abs(x)
    N1 = (w * y / ev ** 2).sum()
    B_N1 = (w * (ay / ev ** 2 + 2 * ay / aev ** 3 * delta)).sum()
    T = (w / x).sum()
    B_T = (w * (1 / ax + delta / x ** 2)).sum()
    w1, w2 = y / ev ** 3, 1 / x ** 2
    dw1, dw2 = 3 * ay / ev ** 4 * delta, 2 / ax ** 3 * delta

    def sums(X, AX, X2, AX2):
        """S1, S2 and their bounds for dev/dtheta = X (magnitude bound AX) and dx/dtheta = X2 (AX2)."""
        return ((w * w1 * X).sum(), (w * w2 * X2).sum(),
                (w * (abs(w1) * AX + dw1 * abs(X))).sum(), (w * (w2 * AX2 + dw2 * abs(X2))).sum())

    c1, c2 = -2 * cw * nn ** 2 / T ** 2, 2 * cw * N1 * nn ** 2 / T ** 3

    def grad(X, AX, X2, AX2):
        S1, S2, B1, B2 = sums(X, AX, X2, AX2)
        dN1 = 2 * cw * nn ** 2 / T ** 3 * S2
        dT = 4 * cw * nn ** 2 / T ** 3 * S1 - 6 * cw * N1 * nn ** 2 / T ** 4 * S2
        return _f(c1 * S1 + c2 * S2), _f(abs(c1) * B1 + abs(c2) * B2 + abs(dN1) * B_N1 + abs(dT) * B_T)

    L = cw * N1 * nn ** 2 / T ** 2
    val["loss"] = _f(L)
    bnd["loss"] = _f(abs(cw) * nn ** 2 / T ** 2 * B_N1 + abs(2 * L / T) * B_T)
    if cv:
        val["t1"] = val["t2"] = bnd["t1"] = bnd["t2"] = float("nan")
    else:
        val["t1"], bnd["t1"] = _f(N1), _f(B_N1)
        val["t2"], bnd["t2"] = _f((T / nn) ** 2), _f(2 * abs(T) / nn ** 2 * B_T)
    val["scale"], bnd["scale"] = grad(lp, delta, lp, delta)
    gl = [grad(rs * dP[j], rs * Aj[j], rs * dP[j], rs * Aj[j]) for j in range(d)]
    val["ls"], bnd["ls"] = np.array([v for v, _ in gl]), np.array([b for _, b in gl])
    one = w * 0 + 1
    val["noise"], bnd["noise"] = grad(nz * one, 0 * one, (0 if cv else nz) * one, 0 * one)
    return val, bnd


def split_raw(raw, layout, G, d):
    """The natural parameters (scale, ls [d], noise) of every problem from the raw (log) vector
    [scale S][lengthscales Sl x Dl][noise Sn], layout = (S, Sl, Dl, Sn)."""
    S, Sl, Dl, Sn = layout
    raw = np.asarray(raw, dtype=np.float64)
    assert raw.shape == (S + Sl * Dl + Sn,)
    out = []
    for g in range(G):
        rs = raw[g if S > 1 else 0]
        rl = raw[S + (g if Sl > 1 else 0) * Dl:S + (g if Sl > 1 else 0) * Dl + Dl]
        rn = raw[S + Sl * Dl + (g if Sn > 1 else 0)]
        ls = np.exp(rl) if Dl == d else np.full(d, np.exp(rl[0]))
        out.append((float(np.exp(rs)), ls, float(np.exp(rn))))
    return out


def evaluate_many(Phi, Y, raw, layout, n, net, loss="MLL", wl=1.0, mll_const=0.0, cv_weight=1.0, per_problem=True):
    """G problems: Phi [2^d, K] shared or [G, 2^d, K], Y [G, K], raw in the layout (S, Sl, Dl, Sn).
    -> (rows, grad, rows_bnd, grad_bnd): history rows [G, 3] (per_problem) or [1, 3] (one summed loss; GCV / CV
    columns 1, 2 nan unless G == 1), the gradient in raw's layout (one lengthscale for all dimensions: the sum over
    the dimensions; a shared parameter: the sum over the problems), and their bounds."""
    Y = np.asarray(Y, dtype=np.float64)
    G = Y.shape[0]
    Phi = np.asarray(Phi, dtype=np.float64)
    d = Phi.shape[-2].bit_length() - 1
    S, Sl, Dl, Sn = layout
    hyp = split_raw(raw, layout, G, d)
    res = []
    for g in range(G):
        sc, ls, nz = hyp[g]
        c = mll_const if (per_problem or loss != "MLL") else 0.0
        res.append(evaluate(Phi[g] if Phi.ndim == 3 else Phi, Y[g], sc, ls, nz, n, net, loss, wl, c, cv_weight))
    rows = np.array([[v["loss"], v["t1"], v["t2"]] for v, _ in res])
    rb = np.array([[b["loss"], b["t1"], b["t2"]] for _, b in res])
    if not per_problem:
        if loss == "MLL":                                # 1/2 (sum norm + wl sum logdet + mll_const)
            rows = rows.sum(0, keepdims=True)
            rows[0, 0] += 0.5 * mll_const
            rb = rb.sum(0, keepdims=True)
            rb[0, 0] += 0.5 * abs(mll_const)
        else:
            keep = G == 1
            rows = np.array([[rows[:, 0].sum(), rows[0, 1] if keep else np.nan, rows[0, 2] if keep else np.nan]])
            rb = np.array([[rb[:, 0].sum(), rb[0, 1] if keep else np.nan, rb[0, 2] if keep else np.nan]])
    grad, gb = np.zeros(S + Sl * Dl + Sn), np.zeros(S + Sl * Dl + Sn)
    for g, (v, b) in enumerate(res):
        for dst, src in ((grad, v), (gb, b)):
            dst[g if S > 1 else 0] += src["scale"]
            o = S + (g if Sl > 1 else 0) * Dl
            if Dl == d:
                dst[o:o + d] += src["ls"]
            else:
                dst[o] += src["ls"].sum()
            dst[S + Sl * Dl + (g if Sn > 1 else 0)] += src["noise"]
    return rows, grad, rb, gb
