"""The case matrix of the spectral fit-iteration tests (tests/test_gpu_spectral_exact.py on the device,
tests/test_spectral_reference_cpu.py without one) and the inputs of every case.

A case names the kernel variant it is meant to reach (`expect`: fields of fgp_spec_geometry's answer); the CPU test
asserts that for every case, so a changed dispatch threshold fails there instead of silently moving a case to another
kernel.  The shapes are the smallest that reach each variant.

Inputs: 'syn' -- non-negative random spectra whose magnitude is spread over 1 .. 1e-12 across the frequencies and a
non-negative Y around twice the eigenvalues at unit parameters (so dL/dlambda keeps one sign over most frequencies
and no gradient component sits near zero: the non-vacuity cap B_q <= 100 |q|); 'real' -- the part-product spectra of a
small lattice (alpha 2) or digital net and Y = |ytilde|^2 of Ackley data, built by the device in the GPU test
(fit_engine.spec_basis) and by the CPU oracle's transforms in the CPU test.
"""
import collections
import math

import numpy as np

from tests import spectral_reference as R

LAT, NET = 0, 1
GEOM = ("tile", "ppw", "pg", "pgp", "ck", "nb", "kpl", "ps", "nsl", "nq")

Case = collections.namedtuple("Case", "name fam m d G src noise pp layout own loss wl tile0 alpha expect seed")


def _case(group, fam, m, d, G=1, src="syn", noise=1e-2, pp=True, layout=None, own=False, loss="MLL", wl=1.0,
          tile0=False, alpha=None, expect=None, seed=0):
    if layout is None:
        layout = (G, G, d, G)
    if alpha is None:
        alpha = 2 if fam == LAT else 1
    S, Sl, Dl, Sn = layout
    name = "%s-%s-m%d-d%d-G%d-%s-nz%g" % (group, "lat" if fam == LAT else "net", m, d, G, src, noise)
    if not pp:
        name += "-sum%d.%d.%d.%d-wl%g" % (S, Sl, Dl, Sn, wl)
    if own:
        name += "-own"
    if loss != "MLL":
        name += "-" + loss
    if tile0:
        name += "-notile"
    if src == "real" and fam == NET:
        name += "-a%d" % alpha
    return Case(name, fam, m, d, G, src, noise, pp, layout, own, loss, wl, tile0, alpha, dict(expect or {}), seed)


def _both(group, fam, m, d, **kw):
    """A synthetic case at both noise levels."""
    return [_case(group, fam, m, d, noise=nz, **kw) for nz in (1e-8, 1e-2)]


def _matrix():
    c = []
    pw = dict(tile=0, ppw=1)
    # per-wave kernel, one problem: K = 33 inside one chunk (lattice m = 6), K = 65 with the Nyquist frequency alone
    # in the second chunk (m = 7)
    for m, d in ((4, 1), (5, 4), (6, 2), (7, 3), (8, 5)):
        c.append(_case("pw1", LAT, m, d, src="real", noise=1e-8, expect=pw, seed=int(m == 8)))
    for m, d in ((6, 5), (7, 6), (7, 1)):
        c += _both("pw1", LAT, m, d, expect=pw)
    c.append(_case("pw1", NET, 4, 2, src="real", noise=1e-8, alpha=1, expect=pw))
    c.append(_case("pw1", NET, 7, 1, src="real", noise=1e-8, alpha=2, expect=pw))
    c.append(_case("pw1", NET, 6, 3, src="real", noise=1e-8, alpha=2, expect=pw))
    for m, d in ((6, 6), (7, 4)):
        c += _both("pw1", NET, m, d, expect=pw)
    # per-wave kernel, several problems sharing the spectra: 2 per wave, 4 per wave (G > 8, d <= 3), 1 at d = 6;
    # ragged last wave group at odd G
    c += _both("pwG", LAT, 7, 2, G=2, expect=dict(tile=0, ppw=2, pg=1))
    c += _both("pwG", NET, 6, 3, G=3, expect=dict(tile=0, ppw=2, pg=2))
    c += _both("pwG", LAT, 10, 1, G=3, tile0=True, expect=dict(tile=0, ppw=2, pg=2))
    c += _both("pwG", LAT, 7, 3, G=9, expect=dict(tile=0, ppw=4, pg=3))
    c += _both("pwG", NET, 7, 2, G=13, expect=dict(tile=0, ppw=4, pg=4))
    c += _both("pwG", NET, 8, 3, G=13, tile0=True, expect=dict(tile=0, ppw=4, pg=4))
    c += _both("pwG", LAT, 6, 4, G=13, expect=dict(tile=0, ppw=2, pg=7), seed=1)
    c += _both("pwG", NET, 6, 5, G=9, expect=dict(tile=0, ppw=2, pg=5))
    c += _both("pwG", LAT, 7, 6, G=2, expect=dict(tile=0, ppw=1, pg=2))
    # per-wave kernel, spectra of each problem's own
    c += _both("own", LAT, 7, 2, G=3, own=True, expect=dict(tile=0, ppw=1, pg=3))
    c += _both("own", NET, 6, 5, G=3, own=True, expect=dict(tile=0, ppw=1, pg=3))
    # tile kernel, G <= 8: every (ppw, pgp) and both families
    c.append(_case("tile", LAT, 9, 1, G=1, src="real", noise=1e-8, expect=dict(tile=1, ppw=1, pgp=1, ps=0)))
    c.append(_case("tile", LAT, 10, 3, G=2, src="real", noise=1e-8, expect=dict(tile=1, ppw=2, pgp=1, ps=0)))
    c.append(_case("tile", NET, 8, 3, G=1, src="real", noise=1e-8, alpha=2, expect=dict(tile=1, ppw=1, pgp=1, ps=0)))
    c.append(_case("tile", NET, 8, 1, G=4, src="real", noise=1e-8, alpha=1, expect=dict(tile=1, ppw=2, pgp=2, ps=0)))
    c += _both("tile", LAT, 10, 3, G=3, expect=dict(tile=1, ppw=2, pgp=2, ps=0))
    c += _both("tile", LAT, 9, 3, G=6, expect=dict(tile=1, ppw=2, pg=3, pgp=4, ps=0))      # last wave group empty
    c += _both("tile", LAT, 10, 1, G=8, expect=dict(tile=1, ppw=2, pgp=4, ps=0))
    c += _both("tile", LAT, 10, 5, G=8, expect=dict(tile=1, ppw=2, pgp=4, ps=0))
    c += _both("tile", NET, 8, 5, G=6, expect=dict(tile=1, ppw=2, pg=3, pgp=4, ps=0))
    c += _both("tile", NET, 8, 3, G=8, expect=dict(tile=1, ppw=2, pgp=4, ps=0))
    c += _both("tile", LAT, 10, 3, G=1, expect=dict(tile=1, ppw=1, pgp=1, ps=0))
    # shapes the tile kernel's LDS ring does not take (an odd number of rows 2^d + G at 64-frequency chunks, G = 5;
    # the 2^5 + 2 rows of d = 5 at 256-frequency chunks): the per-wave kernel at a tile size
    c += _both("tile", LAT, 9, 3, G=5, expect=dict(tile=0, ppw=2, pg=3))
    c += _both("tile", NET, 8, 5, G=2, expect=dict(tile=0, ppw=2, pg=1))
    # tile kernel over problem slices, G > 8: slices of 16 (d <= 3) or 8 problems, ragged last slice
    c += _both("slice", LAT, 10, 2, G=17, expect=dict(tile=1, ppw=4, ps=16, nsl=2))
    c += _both("slice", LAT, 10, 3, G=33, expect=dict(tile=1, ppw=4, ps=16, nsl=3))
    c += _both("slice", LAT, 10, 4, G=9, expect=dict(tile=1, ppw=2, ps=8, nsl=2))
    c += _both("slice", NET, 8, 5, G=17, expect=dict(tile=1, ppw=2, ps=8, nsl=3), seed=1)
    c += _both("slice", NET, 8, 2, G=33, expect=dict(tile=1, ppw=4, ps=16, nsl=3))
    c += _both("slice", NET, 8, 4, G=9, expect=dict(tile=1, ppw=2, ps=8, nsl=2))
    # more than 32 k blocks: both levels of the reduction
    c += _both("nb64", LAT, 15, 2, G=1, expect=dict(nb=64))
    c += _both("nb64", LAT, 15, 2, G=3, expect=dict(nb=64))
    c += _both("nb64", NET, 14, 3, G=1, expect=dict(nb=64))
    # ONE loss summed over G problems (k_spec_step_many and its last-arriver part), mixed parameter layouts
    i = 0
    for G in (3, 20):
        for lay in ("1,1,d,1", "G,G,d,1", "1,G,d,1", "G,1,1,1", "G,G,1,G", "1,1,1,1"):
            fam, m, d = ((LAT, 7, 3), (NET, 6, 2), (LAT, 10, 2), (NET, 8, 4))[i % 4]
            S, Sl, Dl, Sn = [dict(G=G, d=d)[t] if t in "Gd" else int(t) for t in lay.split(",")]
            c += _both("sum", fam, m, d, G=G, pp=False, layout=(S, Sl, Dl, Sn), wl=(1.0, 2.5)[i % 2],
                       expect=dict(nq=4 + d))
            i += 1
    # GCV and CV (k_spec_loss_iter / k_spec_loss_step): per problem and summed (at most 16 problems)
    for loss in ("GCV", "CV"):
        lq = lambda d: dict(tile=0, ppw=1, nq=6 + 2 * d)
        c += _both("alt", LAT, 4, 1, G=1, loss=loss, expect=lq(1), seed=2)
        c += _both("alt", NET, 7, 3, G=3, loss=loss, expect=lq(3))
        c += _both("alt", LAT, 7, 3, G=16, loss=loss, expect=lq(3))
        c += _both("alt", NET, 10, 1, G=1, loss=loss, pp=False, layout=(1, 1, 1, 1), expect=lq(1))
        c += _both("alt", NET, 4, 6, G=3, loss=loss, pp=False, layout=(1, 3, 6, 1), expect=lq(6))
        # (d = 6 at noise 1e-8: the 2^6 subset products leave the noise negligible at every frequency, both losses
        # are then invariant under the scale and the gradient cancels -- B_q / |q| ~ 1e5 for every seed; noise 1e-2 only)
        c.append(_case("alt", LAT, 10, 6, G=16, loss=loss, pp=False, layout=(16, 16, 1, 1), expect=lq(6)))
        c.append(_case("alt", LAT, 10, 3, G=3, loss=loss, src="real", noise=1.0, expect=lq(3)))
        # (real spectra: both losses are invariant under the scale while the noise is negligible, so their
        # gradient cancels to nothing at noise 1e-8 -- B_q / |q| ~ 1e8; at noise 1 it is 40)
    return c


CASES = _matrix()
assert len(set(c.name for c in CASES)) == len(CASES)
BY_NAME = {c.name: c for c in CASES}
MLL_CONST = 3.25          # any constant: the kernels add it to the loss as given
CV_WEIGHT = 0.75


def _rng(case):
    return np.random.default_rng([case.seed, case.fam, case.m, case.d, case.G, int(-math.log10(case.noise)),
                                  sum(case.layout), len(case.name)])


def raw_params(case):
    """The raw (log) parameter vector [scale S][lengthscales Sl x Dl][noise Sn]: scale 1.7 (x 1 + g / 10 per problem),
    random lengthscales off the default, the case's noise (x 1 + g / 4)."""
    S, Sl, Dl, Sn = case.layout
    g = np.random.default_rng([7, case.m, case.d, case.G, case.seed])
    sc = np.log(1.7 * (1 + np.arange(S) / 10.0))
    ls = 0.6 * g.standard_normal((Sl, Dl))
    nz = np.log(case.noise * (1 + np.arange(Sn) / 4.0))
    return np.concatenate([sc, ls.reshape(-1), nz])


def synthetic(case):
    """(Phi [2^d, K] or [G, 2^d, K], Y [G, K]) of a 'syn' case.  Y is a random multiple of the problem's own
    eigenvalues ev (fp64, at the case's parameters): 60 .. 120 ev at noise 1e-8 (the data term dominates: g < 0 at every
    frequency, logdet_weight <= 2.5), 0.02 .. 0.08 ev at noise 1e-2 (the logdet term dominates: g > 0), so the terms
    of every gradient sum share one sign."""
    g = _rng(case)
    n, net = 1 << case.m, case.fam == NET
    K = R.spec_K(n, net)
    P = case.G if case.own else 1
    mag = 10.0 ** (-12.0 * g.random((P, 1, K)))
    Phi = mag * (0.2 + 0.8 * g.random((P, 1 << case.d, K)))
    Y = np.empty((case.G, K))
    for p, (sc, ls, nz) in enumerate(R.split_raw(raw_params(case), case.layout, case.G, case.d)):
        lS = np.array([np.prod([ls[j] for j in range(case.d) if (S >> j) & 1]) for S in range(1 << case.d)])
        ev = math.sqrt(n) * sc * (lS[:, None] * Phi[p if case.own else 0]).sum(0) + nz
        u = g.random(K)
        if case.loss != "MLL":
            # GCV / CV: a Y proportional to ev would make the loss stationary (N1 / T constant); Y follows the
            # eigenvalues at unit parameters instead
            Y[p] = math.sqrt(n) * Phi[p if case.own else 0].sum(0) * (0.5 + 3.0 * u)
        else:
            Y[p] = ev * ((60.0 + 60.0 * u) if case.noise < 1e-5 else (0.02 + 0.06 * u))
    return (Phi if case.own else Phi[0]), Y


def real_cpu(case):
    """(Phi [2^d, K], Y [G, K]) of a 'real' case from the CPU oracle's parts and stable transforms -- what the device
    builds (fit_engine.spec_basis, |ytilde|^2) up to the transforms' rounding; for the checks that need no device."""
    import torch

    import fastgaussianprocesses_amd as F
    from oracle import fgp_oracle as O
    n, d = 1 << case.m, case.d
    K = R.spec_K(n, case.fam == NET)
    if case.fam == LAT:
        x = torch.from_numpy(F.Lattice(d, seed=REAL_SEED + case.seed)(0, n))
        parts, tr = O.lattice_k1parts(x, case.alpha), O.fftbr
    else:
        seq = F.DigitalNetB2(d, seed=REAL_SEED + case.seed)
        xb = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64))
        x = xb.to(torch.float64) * 2.0 ** -seq.t
        parts, tr = O.net_k1parts(xb, seq.t, case.alpha), O.fwht
    Phi = np.empty((1 << d, K))
    for S in range(1 << d):
        b = torch.ones(n, dtype=torch.float64)
        for j in range(d):
            if (S >> j) & 1:
                b = b * parts[:, j]
        Phi[S] = O.ft_stable(b, tr).real[:K].numpy()
    yt = O.ft_stable(O.f_ackley(x), tr)
    return Phi, y_rows(case, (yt.abs() ** 2)[:K].numpy())


REAL_SEED = 7


def y_rows(case, Y1):
    """G rows of a 'real' case from the one |ytilde|^2 row: row g scaled by 1 + g / G."""
    return np.asarray(Y1, dtype=np.float64).reshape(1, -1) * (1 + np.arange(case.G) / case.G)[:, None]


def tolerance_factor(d, kpl):
    """C of |device - reference| <= C 2^-53 B_q: 8 (2^d + 32 + kpl) -- the roundings of one output are at most
    2^d + d (the l^S and P), ~10 (the per-frequency term), kpl + 6 (a lane's chunks and the wave sum), 32 + 16 (the
    two reduction levels): below 2^d + kpl + 80 as a worst-case linear sum, so C keeps a factor 3 over it."""
    return 8.0 * (2 ** d + 32 + kpl)


def layout_flags(case):
    """The parameter-layout fields of fgp_nll_desc as fit_engine.FusedMLL sets them."""
    S, Sl, Dl, Sn = case.layout
    G, d = case.G, case.d
    return dict(scale_off=0, scale_pp=int(S == G and G > 1), ls_off=S, ls_pp=int(Sl == G and G > 1),
                ls_pd=int((Dl == d and Dl > 1) or d == 1), noise_off=S + Sl * Dl, noise_pp=int(Sn == G and G > 1))


def geometry(case, allow_tile=1):
    """fgp_spec_geometry's answer for the case's desc (no device needed), as a dict over GEOM.  The caller sets
    FGP_SPEC_TILE=0 for a `tile0` case, as it does for the launch."""
    import ctypes

    from fastgaussianprocesses_amd import _native as N
    n = 1 << case.m
    Q = (R.spec_K(n, case.fam == NET) + 63) // 64
    desc = N.NllDesc(family=case.fam, log2n=case.m, d=case.d, G=case.G, parts=0, parts_stride=0, ysq=0, ysq_stride=n,
                     raw=0, logdet_weight=case.wl, grad_lam=0, work=0, partials=0, **layout_flags(case))
    desc.basis = 64                                   # any non-NULL value: the query follows no pointer
    desc.basis_stride = Q * (1 << case.d) * 64 if case.own else 0
    desc.ysq_chunked = 1
    desc.loss_metric = {"MLL": N.LOSS_MLL, "GCV": N.LOSS_GCV, "CV": N.LOSS_CV}[case.loss]
    out = (ctypes.c_int * 10)()
    N.call("fgp_spec_geometry", desc, int(allow_tile), out)
    return dict(zip(GEOM, [int(v) for v in out]))
