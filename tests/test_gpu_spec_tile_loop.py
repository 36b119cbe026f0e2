"""k_spec_tile's chunk loop against the per-wave kernel k_spec_iter (FGP_SPEC_TILE=0), bit for bit.

The tile kernel streams the spectra and Y through an LDS ring and evaluates, per frequency, exactly the arithmetic of
k_spec_iter in the same order, block by block: its block partials, the loss rows, the gradient and the raw parameters of
a short fit must be EQUAL (torch.equal), whatever the loop does about its LDS reads, its waits and its DMA addresses.
One evaluation (the stage launches) and a 4-iteration fit (fgp_fit_run) per case, at the smallest shapes that reach each
state of the loop:

| case | family  | n    | d | G  | covers                                                                    |
|------|---------|------|---|----|---------------------------------------------------------------------------|
| 1    | lattice | 2^13 | 3 | 1  | NBW = 4, PPW = 1                                                          |
| 2    | lattice | 2^14 | 4 | 3  | odd G: an inactive problem slot, NBW = 2                                  |
| 3    | lattice | 2^15 | 5 | 8  | the C4 instance (PPW = 2, NBW = 1), 4 chunks per block: the ring in steady state |
| 3a   | lattice | 2^9  | 5 | 8  | ... 1 chunk per block: the ring not wrapped                               |
| 3b   | lattice | 2^10 | 5 | 8  | ... 2 chunks per block: the ring wrapped once                             |
| 4    | net     | 2^13 | 3 | 8  | NET                                                                       |
| 5    | lattice | 2^14 | 3 | 17 | problem slices (a ragged last slice), PPW = 4                             |
| 6    | lattice | 2^13 | 3 | 2  | the persistent instance (FGP_SPEC_PERSIST=1) through fgp_fit_run          |

Cases 1, 2 and 6 were first written down with d = 5.  spec_geometry cannot route d = 5 to the tile kernel with fewer
than four problem groups at any n (the chunk of 2^d + G rows x 64 NBW frequencies must fit kSpecMaxDma 1-KiB DMA
instructions per wave and, twice, kSpecLdsMax), so they take the largest d that it does route there, with the family,
n, G and the covered loop state as listed; every case asserts on the descriptor's geometry that it runs the tile
kernel, and the instance, it is listed for.  fgp_spec_geometry reports 4 chunks per block for every n >= 2^11, so the
unwrapped and once-wrapped ring of case 3 are the two added shapes 3a and 3b.
"""
import ctypes

import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd.fit_engine import mll_constant, spec_basis
from oracle import fgp_oracle as O
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

GEOM = ("tile", "ppw", "pg", "pgp", "ck", "nb", "kpl", "ps", "nsl", "nq")
ITERS = 4

#        id      family     m  d   G  persist  geometry the case is listed for
CASES = [("1", "lattice", 13, 3, 1, False, dict(ppw=1, pgp=1, ps=0)),
         ("2", "lattice", 14, 4, 3, False, dict(ppw=2, pgp=2, ps=0)),
         ("3", "lattice", 15, 5, 8, False, dict(ppw=2, pgp=4, ps=0, kpl=4)),
         ("3a", "lattice", 9, 5, 8, False, dict(ppw=2, pgp=4, ps=0, kpl=1)),
         ("3b", "lattice", 10, 5, 8, False, dict(ppw=2, pgp=4, ps=0, kpl=2)),
         ("4", "net", 13, 3, 8, False, dict(ppw=2, pgp=4, ps=0)),
         ("5", "lattice", 14, 3, 17, False, dict(ppw=4, pgp=4, ps=16, nsl=2)),
         ("6", "lattice", 13, 3, 2, True, dict(ppw=2, pgp=1, ps=0))]


def _inputs(family, m, d, G):
    """(family id, spectra, Y rows [G, n], raw scale [G], raw lengthscales [G, d], raw noise [G]) of G problems on one
    set of spectra: the |ytilde|^2 of Ackley data scaled per problem, every parameter off its default.  (Up to 8
    problems are independent GPs with their own loss, as C4's shifts; more share one loss, as per-output parameters.)"""
    n = 2 ** m
    if family == "lattice":
        gp = F.FastGPLattice(F.Lattice(d, seed=7), device=DEV)
    else:
        gp = F.FastGPDigitalNetB2(F.DigitalNetB2(d, seed=7), device=DEV)
    x = gp.get_x_next(n)
    gp.add_y_next(O.f_ackley(x.cpu()).to(DEV))
    basis = spec_basis(gp._FAMILY, gp._k1parts(n), n)
    ysq = gp._ysq(*gp._problem_batch()).reshape(1, n)
    ysq = (ysq * (1.0 + torch.arange(G, device=ysq.device)[:, None] / G) ** 2).contiguous()
    g = torch.Generator().manual_seed(100 * m + 10 * d + G)
    rs = 0.3 * torch.randn(G, generator=g)
    rl = 0.3 * torch.randn((G, d), generator=g)
    rn = torch.full((G,), -16.0) + 0.3 * torch.randn(G, generator=g)
    return gp._FAMILY, basis, ysq, rs.to(DEV), rl.to(DEV), rn.to(DEV)


def _engine(inp, n):
    fam, basis, ysq, rs, rl, rn = inp
    return F.FusedMLL(fam, None, ysq, rs.clone(), rl.clone(), rn.clone(), 1.0, mll_constant(1, n),
                      requires_grad=(True, True, True), per_problem=ysq.shape[0] <= 8, basis=basis, max_iters=ITERS)


def _geometry(eng):
    out = (ctypes.c_int * 10)()
    N.call("fgp_spec_geometry", eng._nll, 1, out)
    return dict(zip(GEOM, [int(v) for v in out]))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tile_loop_equals_per_wave_kernel(case, monkeypatch):
    _, family, m, d, G, persist, expect = case
    for var in ("FGP_SPEC_SLICE_NB", "FGP_FIT_STREAMS", "FGP_FIT_PERSIST", "FGP_FIT_GRAPH"):
        monkeypatch.delenv(var, raising=False)
    n = 2 ** m
    inp = _inputs(family, m, d, G)
    res = {}
    for tile in ("1", "0"):
        monkeypatch.setenv("FGP_SPEC_TILE", tile)
        monkeypatch.setenv("FGP_SPEC_PERSIST", "1" if persist and tile == "1" else "0")
        eng = _engine(inp, n)
        g = _geometry(eng)
        if tile == "1":
            assert g["tile"] == 1 and {k: g[k] for k in expect} == expect, g     # the tile kernel, the listed instance
        else:
            assert g["tile"] == 0, g
        loss, _, _, grad = eng.evaluate()
        part = eng.partials[:G * g["nq"] * g["nb"]].clone()
        row = eng.loss_hist[0].clone()
        fit = _engine(inp, n)
        fit.run(0, ITERS)
        torch.cuda.synchronize()
        res[tile] = (g["nb"], part.cpu(), row.cpu(), grad, fit.loss_hist[:ITERS].cpu().clone(),
                     fit.raw_hist[:ITERS].cpu().clone(), fit.raw.cpu().clone(), fit.grad.cpu().clone())
    a, b = res["1"], res["0"]
    assert a[0] == b[0]                                                          # the same blocks
    names = ("block partials", "loss row", "gradient", "fit loss rows", "fit parameter rows", "fitted parameters",
             "fit gradient")
    for name, x, y in zip(names, a[1:], b[1:]):
        assert torch.isfinite(x[~torch.isnan(y)]).all(), name
        assert torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)), name
    # the fit moved every parameter (Rprop): the rows compared are evaluations at different parameters
    assert (a[5][-1] != a[5][0]).all()
