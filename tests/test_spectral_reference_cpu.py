"""The extended-precision reference of the spectral fit iteration (tests/spectral_reference.py), pinned without a GPU:

  * against torch fp64 autograd of the dense statement of the same formulas -- MLL, GCV, CV, per problem and as one
    loss over G problems in every parameter layout of the GPU matrix -- so the closed-form gradients are checked by
    something that does not share them: 1e-11 on well-conditioned synthetic inputs (noise 1e-2, spectra within 1e-3);
  * against the CPU oracle (oracle.fgp_oracle.OracleFastGP: loss, term1, the gradients including the noise) with the
    spectra built from the oracle's own ft_stable of the part products: 1e-9 -- the oracle rounds lambda in fp64 and
    the 1e-8 nugget amplifies that (4e-10 at m = 10), which is the effect the reference removes;
  * the non-vacuity cap B_q <= 100 |q| of every case of the GPU matrix (tests/spectral_cases.py), so the derived
    tolerance C 2^-53 B_q of tests/test_gpu_spectral_exact.py is at most ~1e-11 relative;
  * fgp_spec_geometry (ABI 20; no HIP call) reports, for every case, the kernel variant the case is meant to reach,
    and every variant is reached by some case.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd.fit_engine import spec_dense
from oracle import fgp_oracle as O
from tests import spectral_cases as SC
from tests import spectral_reference as R

torch.set_default_dtype(torch.float64)

LAYOUTS = ["1,1,d,1", "G,G,d,1", "1,G,d,1", "G,1,1,1", "G,G,1,G", "1,1,1,1", "G,G,d,G"]


def test_extended_precision_is_extended():
    assert R.MP or np.finfo(np.longdouble).eps < 2e-19


def test_layout_helpers_round_trip():
    g = np.random.default_rng(1)
    for K in (9, 33, 64, 65, 513):
        a = g.standard_normal((3, 4, K))
        c = R.chunked(a)
        Q = (K + 63) // 64
        assert c.shape == (3, Q, 4, 64)
        assert np.array_equal(R.dense(c, K), a)
        full = np.moveaxis(c, -3, -2).reshape(3, 4, Q * 64)
        assert not full[..., K:].any()
        n = 2 * (K - 1)
        if n >= 16 and n & (n - 1) == 0:              # the engine's own helper on the same chunks
            assert np.array_equal(spec_dense(torch.from_numpy(c), 0, n).numpy(), a)
    y = g.random((2, 9))
    e = R.even_extend(y, 16)
    assert e.shape == (2, 16) and np.array_equal(e[:, :9], y)
    assert all(np.array_equal(e[:, 16 - k], y[:, k]) for k in range(1, 8))
    assert R.weights(16, False).tolist() == [1.0] + [2.0] * 7 + [1.0] and R.weights(16, True).tolist() == [1.0] * 16


def _dense_loss(Phi, Y, raw, layout, n, net, loss, wl, c, cw, pp):
    """The dense torch statement: per-problem losses [G] (pp) or their sum [1]."""
    S, Sl, Dl, Sn = layout
    G, K = Y.shape
    d = int(math.log2(Phi.shape[-2]))
    w = torch.from_numpy(R.weights(n, net))
    out = []
    for g in range(G):
        sc = torch.exp(raw[g if S > 1 else 0])
        o = S + (g if Sl > 1 else 0) * Dl
        ls = torch.exp(raw[o:o + Dl]).expand(d) if Dl != d else torch.exp(raw[o:o + d])
        nz = torch.exp(raw[S + Sl * Dl + (g if Sn > 1 else 0)])
        ph = Phi[g] if Phi.dim() == 3 else Phi
        lam = torch.zeros(K)
        for s in range(1 << d):
            t = ph[s]
            for j in range(d):
                if (s >> j) & 1:
                    t = t * ls[j]
            lam = lam + t
        lp = math.sqrt(n) * sc * lam
        ev = lp + nz
        if loss == "MLL":
            out.append(0.5 * ((w * Y[g] / ev).sum() + wl * (w * torch.log(ev.abs())).sum() + (c if pp else 0.0)))
        elif loss == "GCV":
            out.append((w * Y[g] / ev ** 2).sum() / ((w / ev).sum() / n) ** 2)
        else:
            out.append(cw * (w * Y[g] / ev ** 2).sum() / ((w / lp).sum() / n) ** 2)
    L = torch.stack(out)
    if not pp:
        L = L.sum(0, keepdim=True) + (0.5 * c if loss == "MLL" else 0.0)
    return L


@pytest.mark.parametrize("loss", ["MLL", "GCV", "CV"])
@pytest.mark.parametrize("net", [False, True])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_reference_matches_autograd_of_the_dense_statement(loss, net, lay):
    G, d, m = 3, 3, 5
    n = 1 << m
    K = R.spec_K(n, net)
    layout = tuple(dict(G=G, d=d)[t] if t in "Gd" else int(t) for t in lay.split(","))
    pp = lay == "G,G,d,G"
    g = np.random.default_rng([m, d, len(lay), int(net)])
    own = lay in ("G,G,d,1", "G,G,d,G")
    Phi = 10.0 ** (-3.0 * g.random((G if own else 1, 1, K))) * (0.2 + 0.8 * g.random((G if own else 1, 1 << d, K)))
    Phi = Phi if own else Phi[0]
    Y = math.sqrt(n) * (Phi.sum(-2) if own else np.broadcast_to(Phi.sum(0), (G, K))) * (0.5 + 3.0 * g.random((G, K)))
    S, Sl, Dl, Sn = layout
    raw0 = np.concatenate([np.log(1.7 + 0.1 * np.arange(S)), 0.5 * g.standard_normal(Sl * Dl),
                           np.log(1e-2 * (1 + np.arange(Sn)))])
    wl, c, cw = 2.5, 3.25, 0.75
    rows, grad, rb, gb = R.evaluate_many(Phi, Y, raw0, layout, n, net, loss, wl, c, cw, pp)
    raw = torch.tensor(raw0, requires_grad=True)
    L = _dense_loss(torch.from_numpy(Phi), torch.from_numpy(Y), raw, layout, n, net, loss, wl, c, cw, pp)
    (ag,) = torch.autograd.grad(L.sum(), raw)
    assert np.abs(rows[:, 0] - L.detach().numpy()).max() <= 1e-11 * np.abs(rows[:, 0]).max()
    assert np.abs(grad - ag.numpy()).max() <= 1e-11 * np.abs(grad).max(), (grad, ag)
    assert (rb[:, 0] > 0).all() and (gb > 0).all()
    if loss == "GCV" and pp:                            # the history columns: numer, denom
        assert np.allclose(rows[:, 0], rows[:, 1] / rows[:, 2], rtol=1e-14)
    if loss == "CV":
        assert np.isnan(rows[:, 1:]).all()


@pytest.mark.parametrize("noise", [1e-8, 1e-3])
@pytest.mark.parametrize("fam,m,d", [(0, 4, 1), (0, 6, 2), (0, 7, 3), (0, 8, 6), (0, 10, 2), (1, 4, 2), (1, 7, 3)])
def test_reference_matches_oracle_mll(fam, m, d, noise):
    case = SC._case("oracle", fam, m, d, src="real", noise=noise, alpha=2)
    n = 1 << m
    Phi, Y = SC.real_cpu(case)
    import fastgaussianprocesses_amd as F
    if fam == 0:
        x = torch.from_numpy(F.Lattice(d, seed=SC.REAL_SEED)(0, n))
        o = O.OracleFastGP("lattice", x, None, O.f_ackley(x), alpha=2, noise=noise, requires_grad_noise=True)
    else:
        seq = F.DigitalNetB2(d, seed=SC.REAL_SEED)
        xb = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64))
        x = xb.to(torch.float64) * 2.0 ** -seq.t
        o = O.OracleFastGP("net", x, xb, O.f_ackley(x), alpha=2, t=seq.t, noise=noise, requires_grad_noise=True)
    raw = SC.raw_params(case)
    with torch.no_grad():
        o.raw_scale.copy_(torch.tensor(raw[:1]))
        o.raw_lengthscales.copy_(torch.tensor(raw[1:1 + d]))
    oloss, ot1, ot2 = o.mll_loss()
    gs, gl, gn = torch.autograd.grad(oloss, [o.raw_scale, o.raw_lengthscales, o.raw_noise])
    rows, grad, _, _ = R.evaluate_many(Phi, Y, raw, case.layout, n, fam == 1, "MLL", 1.0, n * math.log(2 * math.pi))
    og = torch.cat([gs.reshape(-1), gl.reshape(-1), gn.reshape(-1)]).numpy()
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))
    errs = dict(loss=rel(rows[0, 0], oloss.item()), t1=rel(rows[0, 1], ot1.item()), t2=rel(rows[0, 2], ot2.item()),
                grad=rel(grad, og))
    print(case.name, errs)
    assert max(errs.values()) <= 1e-9, errs


def _inputs(case):
    return SC.synthetic(case) if case.src == "syn" else SC.real_cpu(case)


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_bound_is_not_vacuous(name):
    """B_q <= 100 |q| for every output of every case of the GPU matrix (the reference alone decides it)."""
    c = SC.BY_NAME[name]
    Phi, Y = _inputs(c)
    rows, grad, rb, gb = R.evaluate_many(Phi, Y, SC.raw_params(c), c.layout, 1 << c.m, c.fam == SC.NET, c.loss, c.wl,
                                         SC.MLL_CONST, SC.CV_WEIGHT, c.pp)
    ok = ~np.isnan(rows)
    assert (ok == ~np.isnan(rb)).all() and ok[:, 0].all()
    worst = max(float((rb[ok] / np.abs(rows[ok])).max()), float((gb / np.abs(grad)).max()))
    assert worst <= 100.0, worst
    assert (rb[ok] > 0).all() and (gb > 0).all()


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_case_reaches_its_variant(name, monkeypatch):
    c = SC.BY_NAME[name]
    if c.tile0:
        monkeypatch.setenv("FGP_SPEC_TILE", "0")
    else:
        monkeypatch.delenv("FGP_SPEC_TILE", raising=False)
    monkeypatch.delenv("FGP_SPEC_SLICE_NB", raising=False)
    g = SC.geometry(c)
    assert c.expect and {k: g[k] for k in c.expect} == c.expect, g
    n = 1 << c.m
    main = n if c.fam == SC.NET else n // 2
    assert g["nb"] * g["kpl"] * 64 >= main and 1 <= g["nb"] <= 512
    assert g["nq"] == (4 + c.d if c.loss == "MLL" else 6 + 2 * c.d)
    # allow_tile = 0 is the per-wave geometry, whatever the environment says
    p = SC.geometry(c, allow_tile=0)
    assert p["tile"] == 0 and p["pgp"] == 0 and p["ps"] == 0 and p["nsl"] == 1


def test_every_variant_is_reached(monkeypatch):
    monkeypatch.delenv("FGP_SPEC_SLICE_NB", raising=False)
    seen = set()
    for c in SC.CASES:
        if c.tile0:
            monkeypatch.setenv("FGP_SPEC_TILE", "0")
        else:
            monkeypatch.delenv("FGP_SPEC_TILE", raising=False)
        g = SC.geometry(c)
        fam = "net" if c.fam == SC.NET else "lat"
        if c.loss != "MLL":
            seen.add(("loss", c.loss, fam, c.pp))
        elif g["tile"] and g["ps"]:
            seen.add(("slice", g["ps"], fam))
            assert g["nsl"] >= 2 and c.G % g["ps"] != 0            # ragged last slice
        elif g["tile"]:
            seen.add(("tile", g["ppw"], g["pgp"]))
            seen.add(("tile", fam))
        else:
            seen.add(("iter", g["ppw"], fam))
            seen.add(("iter-own", c.own))
        if g["nb"] > 32:
            seen.add(("two-level", fam))
        if not c.pp and c.loss == "MLL":
            seen.add(("many", c.layout[0] > 1, c.layout[1] > 1, c.layout[2] > 1, c.layout[3] > 1, c.G > 16))
    want = {("iter", p, f) for p in (1, 2, 4) for f in ("lat", "net")}
    want |= {("iter-own", True), ("tile", "lat"), ("tile", "net"), ("two-level", "lat"), ("two-level", "net")}
    want |= {("tile", 1, 1), ("tile", 2, 1), ("tile", 2, 2), ("tile", 2, 4)}
    want |= {("slice", ps, f) for ps in (8, 16) for f in ("lat", "net")}
    want |= {("loss", l, f, pp) for l in ("GCV", "CV") for f in ("lat", "net") for pp in (True, False)}
    for G16 in (False, True):
        want |= {("many", False, False, True, False, G16), ("many", True, True, True, False, G16),
                 ("many", False, True, True, False, G16), ("many", True, False, False, False, G16),
                 ("many", True, True, False, True, G16), ("many", False, False, False, False, G16)}
    assert want <= seen, sorted(want - seen, key=str)


@pytest.mark.parametrize("name,k", [("nb64-lat-m15-d2-G1-syn-nz1e-08", 0), ("nb64-lat-m15-d2-G1-syn-nz0.01", 1 << 14),
                                    ("nb64-lat-m15-d2-G1-syn-nz0.01", 4097), ("nb64-net-m14-d3-G1-syn-nz1e-08", 16383),
                                    ("pw1-lat-m7-d1-G1-syn-nz0.01", 64), ("pw1-lat-m7-d1-G1-syn-nz1e-08", 0)])
def test_one_wrong_frequency_weight_exceeds_the_tolerance(name, k):
    """The bound is tight enough to see ONE frequency of the largest cases (2^14 + 1 of them) with a wrong fold
    weight -- the lattice's k = 0 or Nyquist correction left out, or any other frequency counted once too often: every
    output then moves by more than the tolerance C 2^-53 B_q of tests/test_gpu_spectral_exact.py."""
    c = SC.BY_NAME[name]
    n, net = 1 << c.m, c.fam == SC.NET
    Phi, Y = SC.synthetic(c)
    (sc, ls, nz), = R.split_raw(SC.raw_params(c), c.layout, 1, c.d)
    v, b = R.evaluate(Phi, Y[0], sc, ls, nz, n, net, "MLL", c.wl, SC.MLL_CONST)
    w = R.weights(n, net)
    w[k] += 1.0
    v2, _ = R.evaluate(Phi, Y[0], sc, ls, nz, n, net, "MLL", c.wl, SC.MLL_CONST, w=w)
    C = SC.tolerance_factor(c.d, SC.geometry(c)["kpl"])
    for q in ("loss", "t1", "t2", "scale", "ls", "noise"):
        assert (np.abs(np.asarray(v2[q]) - np.asarray(v[q])) > 10 * C * R.EPS53 * np.asarray(b[q])).all(), q


def test_geometry_query_validates_without_a_device():
    c = SC.CASES[0]
    out = (ctypes.c_int * 10)()
    desc = N.NllDesc(family=0, log2n=c.m, d=c.d, G=1)
    with pytest.raises(RuntimeError, match="basis"):
        N.call("fgp_spec_geometry", desc, 1, out)
    desc.basis = 64
    with pytest.raises(RuntimeError, match="null out"):
        N.call("fgp_spec_geometry", desc, 1, None)
    desc.d = 7
    with pytest.raises(RuntimeError, match="d = 7"):
        N.call("fgp_spec_geometry", desc, 1, out)
    desc.d, desc.log2n = 2, 3
    with pytest.raises(RuntimeError, match="log2n"):
        N.call("fgp_spec_geometry", desc, 1, out)
    assert N.lib().fgp_abi_version() == 20 == N.ABI_VERSION and "fgp_spec_geometry" in N.exported_symbols()
