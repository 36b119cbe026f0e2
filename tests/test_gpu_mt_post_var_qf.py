"""post_var of the multitask / derivative-informed classes by the transform-domain quadratic form (multitask.py
_post_var_qf -> fgp_mt_quadform): against the golden fixtures and the oracle at the existing tolerances under
FGP_MT_POST_VAR_QF=1, chunking bit for bit, and the routing with its default threshold."""
import os

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native as N
from golden_util import load_golden
from tests import test_gpu_adaptive as TA
from tests import test_gpu_multitask as TM
from tests import test_gpu_multitask_batch as TB
from tests import test_gpu_wide_mt as TW
from tests import test_oracle_multitask as OM
from tests import test_wide_mt_cpu as WM
from tests.gpu_fixtures import DEV, abs_err
from tests.test_mt_qf_cpu import D8_NAMES

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)


def _recorded(monkeypatch):
    calls = []
    real = N.call

    def call(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, "call", call)
    return calls


def _check_against_fixture(gp, o, g, kxx, tol_pvar, compare_new):
    xt = torch.from_numpy(g["x_test"])
    xd = xt.to(DEV)
    pv = gp.post_var(xd)
    e_o, e_g = abs_err(pv, o.post_var(xt)), abs_err(pv, g["pvar"])
    print("pvar: vs oracle %.3g, vs reference %.3g (tol %.3g)" % (e_o, e_g, tol_pvar * kxx))
    assert e_o <= tol_pvar * kxx and e_g <= tol_pvar * kxx
    assert (pv >= 0).all()
    if compare_new:
        ns_new = [int(v) for v in g["n_new"]]
        pv_new = gp.post_var(xd, n=torch.tensor(ns_new))
        tol_new = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
        e_new = abs_err(pv_new, g["pvar_new"])
        print("pvar_new: vs reference %.3g (tol %.3g)" % (e_new, tol_new))
        assert e_new <= tol_new and (pv_new >= 0).all()
    pc = gp.post_cov(xd, xd)
    T = pc.size(-4)
    r0, r1 = torch.arange(T), torch.arange(pc.size(-1))
    assert torch.allclose(pc[..., r0, r0, :, :][..., r1, r1], pv)
    return pv


@pytest.mark.parametrize("path", TW.SWITCHES)
@pytest.mark.parametrize("name", WM.NAMES)
def test_wide_fixtures_by_the_form(name, path, monkeypatch):
    TW._switch(monkeypatch, path)
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    g = WM.load_wide_mt(name)
    gp = TW.product_mt(g)
    calls = _recorded(monkeypatch)
    _check_against_fixture(gp, WM.make_oracle(g), g, WM.kxx_scale(g), 1e-8, True)
    assert "fgp_mt_quadform" in calls


@pytest.mark.parametrize("name", D8_NAMES)
def test_multitask_fixtures_by_the_form(name, monkeypatch):
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    g = load_golden(name)
    gp = TM.product_mt(g)
    calls = _recorded(monkeypatch)
    _check_against_fixture(gp, OM.make_oracle(g), g, TM.kxx_scale(g), OM.pred_tol(name, "pvar", 1e-8),
                           OM.pred_tol(name, "pvar_new", 0.0) is not None)
    assert "fgp_mt_quadform" in calls


def _both_routes(gp, xd, monkeypatch, **kw):
    out = {}
    for env in ("1", "0"):
        monkeypatch.setenv("FGP_MT_POST_VAR_QF", env)
        calls = _recorded(monkeypatch)
        out[env] = gp.post_var(xd, **kw)
        assert ("fgp_mt_quadform" in calls) == (env == "1") and ("fgp_mt_solve" in calls) == (env == "0")
    return out["1"], out["0"]


@pytest.mark.parametrize("name", TB.NAMES)
def test_parameter_batched_fit_by_the_form(name, monkeypatch):
    """The hyper-parameter batch goes through _factor's G problems: the fitted GP's post_var against the reference's."""
    g = np.load(os.path.join(TB.BDIR, name + ".npz"))
    gp = TB.build(g)
    its = len(g["fit_loss_hist"]) - 1
    gp.fit(iterations=its, verbose=0, stop_crit_wait_iterations=its + 5)
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    pv, pv0 = _both_routes(gp, xt, monkeypatch)
    tol = 1e-8 * max(1.0, float(np.abs(g["fit_pvar"]).max()))
    print("batched: vs reference %.3g, vs rows-and-solve %.3g (tol %.3g)" % (abs_err(pv, g["fit_pvar"]), abs_err(pv, pv0), tol))
    assert tuple(pv.shape) == g["fit_pvar"].shape
    assert abs_err(pv, g["fit_pvar"]) <= tol and (pv >= 0).all()


def test_adaptive_nugget_fit_by_the_form(monkeypatch):
    g = np.load(os.path.join(TA.ADIR, "lattice_m8_d2_a2_T2.npz"))
    gp = TA.build(g)
    its = len(g["fit_loss_hist"]) - 1
    gp.fit(iterations=its, verbose=0, stop_crit_wait_iterations=its + 5)
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    pv, pv0 = _both_routes(gp, xt, monkeypatch)
    kxx = float(np.abs(g["fit_pvar"]).max()) + float(torch.exp(gp.raw_scale.detach()).max())
    print("adaptive: vs reference %.3g, vs rows-and-solve %.3g (tol %.3g)" % (abs_err(pv, g["fit_pvar"]), abs_err(pv, pv0), 1e-8 * kxx))
    assert abs_err(pv, g["fit_pvar"]) <= 1e-8 * kxx and (pv >= 0).all()


def _plain_gp(d, ns, family="lattice", seed=11):
    T = len(ns)
    ls = torch.linspace(0.05, 0.3, d)
    if family == "lattice":
        gp = F.FastGPLattice([F.Lattice(d, seed=seed + l) for l in range(T)], num_tasks=T, alpha=2, device=DEV,
                             lengthscales=ls)
    else:
        gp = F.FastGPDigitalNetB2([F.DigitalNetB2(d, seed=seed + l, randomize="DS") for l in range(T)], num_tasks=T,
                                  alpha=2, device=DEV, lengthscales=ls)
    xs = gp.get_x_next(n=list(ns))
    gp.add_y_next([torch.sin(3 * x).mean(1) + 0.1 * l for l, x in enumerate(xs)])
    return gp


@pytest.mark.parametrize("family,d", [("lattice", 12), ("net", 3)])
def test_integer_task_subset_and_an_empty_task(family, d, monkeypatch):
    """An unequal-n GP with an empty task (n = [64, 0, 256]): every way of asking for tasks, both routes."""
    gp = _plain_gp(d, [64, 0, 256], family)
    xd = torch.rand((9, d), generator=torch.Generator().manual_seed(5)).to(DEV)
    kxx = 10 * max(1.0, float(gp.post_var(xd).max()))
    allv, all0 = _both_routes(gp, xd, monkeypatch)
    assert tuple(allv.shape) == (3, 9) and abs_err(allv, all0) <= 1e-8 * kxx and (allv >= 0).all()
    one, one0 = _both_routes(gp, xd, monkeypatch, task=2)
    assert tuple(one.shape) == (9,) and abs_err(one, one0) <= 1e-8 * kxx
    sub, sub0 = _both_routes(gp, xd, monkeypatch, task=[2, 0])
    assert tuple(sub.shape) == (2, 9) and abs_err(sub, sub0) <= 1e-8 * kxx
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    # a task's variance has the same bits however it is asked for: alone, in a subset, among all
    assert torch.equal(one, allv[2]) and torch.equal(sub[0], allv[2]) and torch.equal(sub[1], allv[0])
    grown, grown0 = _both_routes(gp, xd, monkeypatch, n=torch.tensor([64, 32, 512]))
    assert abs_err(grown, grown0) <= 1e-8 * kxx
    # post_error and post_ci inherit the route through post_var
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    calls = _recorded(monkeypatch)
    assert torch.equal(gp.post_error(xd)[0], allv) and torch.equal(gp.post_ci(xd)[1], allv)
    assert calls.count("fgp_mt_quadform") == 2


@pytest.mark.parametrize("family,d", [("lattice", 10), ("net", 8)])
def test_chunks_of_1_7_and_40_points_give_the_same_bits(family, d, monkeypatch):
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    gp = _plain_gp(d, [128, 32, 128], family)
    xd = torch.rand((40, d), generator=torch.Generator().manual_seed(6)).to(DEV)
    ns, tasks = list(gp._ns), [0, 1, 2]
    per = gp._post_var_qf_bytes(ns)                              # bytes per (requested task, test point)
    calls = _recorded(monkeypatch)
    with torch.no_grad():
        # chunks of 1, 7 and 40 points of one task, and all three tasks' 40 points in one chunk
        outs = [gp._post_var_qf(xd, tasks, ns, work_bytes=per * C) for C in (1, 7, 40, 120)]
    assert calls.count("fgp_mt_quadform") == 3 * 40 + 3 * 6 + 3 + 1
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    with torch.no_grad():
        assert torch.equal(gp._post_var_qf(xd, tasks, ns, work_bytes=1), outs[0]), "one point is always allowed"
        assert torch.equal(gp._post_var_qf(xd, tasks, ns, work_bytes=per * 85), outs[0])      # two tasks, then one


def _inverse_transforms(calls):
    return [c for c in calls if c.startswith("fgp_ifftbr")]


def test_routing_threshold_and_peak_memory(monkeypatch):
    """T = 2, d = 12 lattice: n = [2^12, 2^12] takes the form by default, FGP_MT_POST_VAR_QF=0 the rows and the solve;
    n = [2^11, 2^11] stays on rows-and-solve, and so does a call whose test points need a second chunk."""
    monkeypatch.delenv("FGP_MT_POST_VAR_QF", raising=False)
    d = 12
    xd = torch.rand((64, d), generator=torch.Generator().manual_seed(9)).to(DEV)
    gp = _plain_gp(d, [1 << 12, 1 << 12])
    with torch.no_grad():
        gp._factor(list(gp._ns))                                  # (shared by both routes, cached)
    pv, peak = {}, {}
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("FGP_MT_POST_VAR_QF", env)
        calls = _recorded(monkeypatch)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pv[env] = gp.post_var(xd)
        torch.cuda.synchronize()
        peak[env] = torch.cuda.max_memory_allocated() - base
        if env is None:
            assert "fgp_mt_quadform" in calls and "fgp_mt_solve" not in calls and not _inverse_transforms(calls)
        else:
            assert "fgp_mt_quadform" not in calls and "fgp_mt_solve" in calls and _inverse_transforms(calls)
    kxx = 10 * max(1.0, float(pv["0"].max()))
    print("routes: |form - rows-and-solve| = %.3g (tol %.3g); peak %d vs %d bytes" % (
        abs_err(pv[None], pv["0"]), 1e-8 * kxx, peak[None], peak["0"]))
    assert abs_err(pv[None], pv["0"]) <= 1e-8 * kxx
    assert peak[None] < peak["0"], peak
    monkeypatch.delenv("FGP_MT_POST_VAR_QF", raising=False)
    # 700 test points of a task need more than one 2^28-byte chunk (393216 bytes each): rows-and-solve by default
    many = torch.rand((700, d), generator=torch.Generator().manual_seed(10)).to(DEV)
    assert 64 * gp._post_var_qf_bytes(list(gp._ns)) <= 1 << 28 < 700 * gp._post_var_qf_bytes(list(gp._ns))
    calls = _recorded(monkeypatch)
    pv_many = gp.post_var(many)
    assert "fgp_mt_quadform" not in calls and "fgp_mt_solve" in calls
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    assert abs_err(gp.post_var(many), pv_many) <= 1e-8 * kxx
    monkeypatch.delenv("FGP_MT_POST_VAR_QF", raising=False)
    small = _plain_gp(d, [1 << 11, 1 << 11])
    calls = _recorded(monkeypatch)
    small.post_var(xd)
    assert "fgp_mt_quadform" not in calls and "fgp_mt_solve" in calls


def test_an_autograd_graph_keeps_the_dense_statement(monkeypatch):
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    gp = _plain_gp(3, [32, 32])
    xd = torch.rand((5, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    calls = _recorded(monkeypatch)
    pv = gp.post_var(xd, eval=False)
    assert pv.requires_grad and "fgp_mt_quadform" not in calls
