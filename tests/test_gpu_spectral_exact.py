"""The spectral fit-iteration kernels against the extended-precision reference (tests/spectral_reference.py).

Every case of tests/spectral_cases.py builds a fit_engine.FusedMLL on part-product spectra and compares the loss row
and the gradient the kernels write (history row, grad_out) with the closed form evaluated in 80-bit arithmetic from
the very arrays the engine was given (device-built spectra are read back, nothing is recomputed), for every driver:

  * evaluate(): the stage launches (k_spec_iter / k_spec_tile / k_spec_loss_iter, then k_spec_reduce_step /
    k_spec_step_many / k_spec_loss_step through fgp_fit_step), twice -- bit-identical;
  * run(0, 2) of per-problem descs: the fused k_spec_tile path where the geometry allows it (G <= 8), the launch per
    stage otherwise; row 0 at the initial parameters, row 1 and the gradient at raw_hist[1], the parameters the
    kernel itself recorded after its Rprop step (the ping-pong partial buffers of the fused run);
  * run_persist for one iteration wherever persist_ok() (k_spec_persist).

Tolerance, derived and not measured: |device - reference| <= C 2^-53 B_q for every output q, B_q the reference's
first-order bound and C = 8 (2^d + 32 + kpl) with kpl from fgp_spec_geometry (spectral_cases.tolerance_factor: the
worst-case linear count of roundings is below 2^d + kpl + 80).  With the non-vacuity cap B_q <= 100 |q| (asserted
for every case in tests/test_spectral_reference_cpu.py, and here on the arrays used) that is at most ~1e-11
relative, typically 1e-13.  The worst observed |device - reference| / (2^-53 B_q) per variant is printed (-s) and
tabulated in DESIGN.md section 3.
"""
import math

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd.fit_engine import spec_basis
from oracle import fgp_oracle as O
from tests import spectral_cases as SC
from tests import spectral_reference as R
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

WORST = {}          # variant -> worst err / (2^-53 B_q)
PERSIST_RAN = set()


def _inputs(case):
    """(Phi dense, Y [G, K], basis on the device, ysq [G, n] on the device)."""
    n = 1 << case.m
    net = case.fam == SC.NET
    K = R.spec_K(n, net)
    if case.src == "syn":
        Phi, Y = SC.synthetic(case)
        basis = torch.from_numpy(R.chunked(Phi)).to(DEV)
        ysq = torch.from_numpy(Y if net else R.even_extend(Y, n)).to(DEV)
        return Phi, Y, basis, ysq
    if net:
        gp = F.FastGPDigitalNetB2(F.DigitalNetB2(case.d, seed=SC.REAL_SEED + case.seed), alpha=case.alpha, device=DEV)
    else:
        gp = F.FastGPLattice(F.Lattice(case.d, seed=SC.REAL_SEED + case.seed), alpha=case.alpha, device=DEV)
    x = gp.get_x_next(n)
    gp.add_y_next(O.f_ackley(x.cpu()).to(DEV))
    basis = spec_basis(gp._FAMILY, gp._k1parts(n), n)
    rows = SC.y_rows(case, gp._ysq(*gp._problem_batch()).cpu().numpy().reshape(-1))      # [G, n]
    Phi = R.dense(basis.cpu().numpy(), K)
    return Phi, np.ascontiguousarray(rows[:, :K]), basis, torch.from_numpy(rows).to(DEV)


def _engine(case, basis, ysq, raw):
    S, Sl, Dl, Sn = case.layout
    r = torch.from_numpy(raw).to(DEV)
    return F.FusedMLL(case.fam, None, ysq, r[:S].clone(), r[S:S + Sl * Dl].reshape(Sl, Dl).clone(),
                      r[S + Sl * Dl:].clone(), case.wl, SC.MLL_CONST, requires_grad=(True, True, True),
                      per_problem=case.pp, basis=basis, loss_metric=case.loss, cv_weight=SC.CV_WEIGHT)


def _variant(case, g, driver):
    if case.loss != "MLL":
        v = "k_spec_loss_iter %s" % case.loss
    elif driver == "persist":
        v = "k_spec_persist"
    elif g["tile"] and g["ps"]:
        v = "k_spec_tile slices of %d" % g["ps"]
    elif g["tile"]:
        v = "k_spec_tile ppw %d pgp %d%s" % (g["ppw"], g["pgp"], " fused" if driver == "run" and case.G <= 8 else "")
    else:
        v = "k_spec_iter ppw %d%s" % (g["ppw"], " own spectra" if case.own else "")
    if driver != "persist":
        v += " + " + ("summed step" if not case.pp else "per-problem step")
    if g["nb"] > 32:
        v += ", nb > 32"
    return v


def _check(case, g, driver, Phi, Y, raw, rows_dev, grad_dev, what):
    n = 1 << case.m
    rows, grad, rb, gb = R.evaluate_many(Phi, Y, raw, case.layout, n, case.fam == SC.NET, case.loss, case.wl,
                                         SC.MLL_CONST, SC.CV_WEIGHT, case.pp)
    C = SC.tolerance_factor(case.d, g["kpl"])
    ok = ~np.isnan(rows)
    assert rows_dev.shape == rows.shape and (np.isnan(rows_dev) == ~ok).all(), (rows_dev, rows)
    ratio = float((np.abs(rows_dev[ok] - rows[ok]) / (R.EPS53 * rb[ok])).max())
    if grad_dev is not None:
        ratio = max(ratio, float((np.abs(grad_dev - grad) / (R.EPS53 * gb)).max()))
    v = _variant(case, g, driver)
    WORST[v] = max(WORST.get(v, 0.0), ratio)
    print("%-48s %-9s %-14s err / (2^-53 B) = %8.2f   C = %d" % (case.name, driver, what, ratio, C))
    assert ratio <= C, (case.name, driver, what, ratio, C)
    return rows, grad, rb, gb


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_iteration_matches_extended_precision_reference(name, monkeypatch):
    case = SC.BY_NAME[name]
    if case.tile0:
        monkeypatch.setenv("FGP_SPEC_TILE", "0")
    else:
        monkeypatch.delenv("FGP_SPEC_TILE", raising=False)
    for var in ("FGP_SPEC_SLICE_NB", "FGP_FIT_STREAMS", "FGP_FIT_PERSIST"):
        monkeypatch.delenv(var, raising=False)
    g = SC.geometry(case)
    assert {k: g[k] for k in case.expect} == case.expect, g         # the variant this case is meant to reach
    Phi, Y, basis, ysq = _inputs(case)
    raw0 = SC.raw_params(case)
    hg = case.G if case.pp else 1

    # evaluate(): the stage launches, no update; twice, bit-identical
    eng = _engine(case, basis, ysq, raw0)
    eng.evaluate()
    rows_d, grad_d = eng.loss_hist[0].cpu().numpy().reshape(hg, 3), eng.grad.cpu().numpy()
    rows, grad, rb, gb = _check(case, g, "evaluate", Phi, Y, raw0, rows_d, grad_d, "row 0 + grad")
    # the non-vacuity cap on the arrays actually used
    ok = ~np.isnan(rows)
    assert (rb[ok] <= 100 * np.abs(rows[ok])).all() and (gb <= 100 * np.abs(grad)).all()
    assert np.array_equal(eng.raw_hist[0].cpu().numpy(), raw0) and np.array_equal(eng.raw.cpu().numpy(), raw0)
    eng.evaluate()
    assert np.array_equal(eng.loss_hist[0].cpu().numpy().reshape(hg, 3), rows_d, equal_nan=True)
    assert np.array_equal(eng.grad.cpu().numpy(), grad_d)

    # run(0, 2) of a per-problem desc: row 0 at the initial parameters, row 1 + gradient at the recorded ones
    if case.pp:
        eng = _engine(case, basis, ysq, raw0)
        eng.run(0, 2)
        torch.cuda.synchronize()
        lh, rh = eng.loss_hist[:2].cpu().numpy(), eng.raw_hist[:2].cpu().numpy()
        assert np.array_equal(rh[0], raw0)
        assert (np.abs(rh[1] - raw0) > 0.05).all()                   # every parameter stepped (Rprop, lr 0.1)
        _check(case, g, "run", Phi, Y, raw0, lh[0].reshape(hg, 3), None, "row 0")
        _check(case, g, "run", Phi, Y, rh[1], lh[1].reshape(hg, 3), eng.grad.cpu().numpy(), "row 1 + grad")
        assert np.array_equal(lh[0].reshape(hg, 3), rows_d, equal_nan=True)      # the stage launches' row, bit for bit

    # the single-launch fit, one iteration
    if case.G == 1 and case.pp:
        eng = _engine(case, basis, ysq, raw0)
        if eng.persist_ok():
            last = eng.run_persist(1, math.log(1.05), 20)
            assert last == 1, "fgp_fit_persist gave up at a barrier"
            lh, rh = eng.loss_hist[:2].cpu().numpy(), eng.raw_hist[:2].cpu().numpy()
            assert np.array_equal(rh[0], raw0)
            _check(case, g, "persist", Phi, Y, raw0, lh[0].reshape(1, 3), None, "row 0")
            _check(case, g, "persist", Phi, Y, rh[1], lh[1].reshape(1, 3), eng.grad.cpu().numpy(), "row 1 + grad")
            PERSIST_RAN.add((case.fam, g["nb"] > 32))


def test_zz_worst_ratio_per_variant():
    """The table of DESIGN.md section 3: worst err / (2^-53 B_q) per kernel variant over the matrix above."""
    print()
    for v in sorted(WORST):
        print("| `%s` | %.1f |" % (v, WORST[v]))
    if len(WORST) > 20:                                              # the whole matrix ran
        assert {(SC.LAT, False), (SC.NET, False)} <= PERSIST_RAN, PERSIST_RAN
