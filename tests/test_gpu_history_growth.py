"""fit_engine.FitEngine.ensure_history on the device: when the histories grow in the middle of a fit, every engine's
descriptor must follow them (_history_moved) -- a descriptor left at the old buffers would write the later rows where
nobody reads them.  Engine A runs two iterations, grows past its first 16 rows and runs the third; engine B, built the
same way, runs the three in one call: the rows must be equal bit for bit."""
import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd.fit_engine import FusedMLL
from fastgaussianprocesses_amd.multitask import MtGeneralEngine
from fastgaussianprocesses_amd.wide_fit import WideMLL
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)
N = 16


def _f(x):
    return torch.cos(2 * np.pi * x).sum(1) + x[:, 0] * x[:, -1]


def _single(d):
    gp = F.FastGPLattice(F.Lattice(d, seed=3), device=DEV)
    gp.add_y_next(_f(gp.get_x_next(N)))
    return gp


def _multitask(**kw):
    gp = F.FastGPLattice(2, seed_for_seq=7, num_tasks=2, device=DEV, **kw)
    xs = gp.get_x_next(n=[N, N])
    gp.add_y_next([_f(xs[0]), _f(xs[1]) + xs[1][:, 0]])
    return gp


def _transform():
    return _single(2)._fused_engine(2, 0.1), FusedMLL, lambda e: e.basis is None


def _spectral():
    return _single(2)._fused_engine(2, 0.1), FusedMLL, lambda e: e.basis is not None and e.mt is None


def _wide():
    gp = _single(9)
    assert gp._wide_fit_ok()
    return gp._fused_engine(2, 0.1), WideMLL, lambda e: True


def _mt_general():
    gp = _multitask()
    assert gp._mt_general_ok() and not gp._mt_fused_ok()
    return gp._fused_engine(2, 0.1), MtGeneralEngine, lambda e: True


def _mt_fused():
    gp = _multitask(requires_grad_factor_task_kernel=False, requires_grad_noise_task_kernel=False)
    assert gp._mt_fused_ok()
    return gp._fused_engine(2, 0.1), FusedMLL, lambda e: e.mt is not None


CASES = {"transform": ("transform", _transform), "spectral": ("spectral", _spectral), "wide": ("", _wide),
         "mt_general": ("", _mt_general), "mt_fused": ("", _mt_fused)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_history_growth_repoints_the_descriptor(name, monkeypatch):
    path, make = CASES[name]
    monkeypatch.setenv("FGP_ENGINE_CACHE", "0")            # A and B are distinct engines
    monkeypatch.setenv("FGP_FIT_PATH", path)
    a, cls, is_path = make()
    b = make()[0]
    assert a is not b and type(a) is cls and type(b) is cls and is_path(a) and is_path(b)
    assert a.max_iters == 16 and b.max_iters == 16
    a.run(0, 2)
    lh01, rh01 = a.loss_hist[:2].clone(), a.raw_hist[:2].clone()
    old = (a.loss_hist.data_ptr(), a.raw_hist.data_ptr())
    a.ensure_history(40)
    assert a.max_iters == 40 and a.loss_hist.shape[0] == 40 and a.raw_hist.shape[0] == 40
    assert (a.loss_hist.data_ptr(), a.raw_hist.data_ptr()) != old
    a.run(2, 1, True)
    b.run(0, 3, True)
    assert b.max_iters == 16
    la, ra, lb, rb = (t.cpu().numpy() for t in (a.loss_hist[:3], a.raw_hist[:3], b.loss_hist[:3], b.raw_hist[:3]))
    assert np.isfinite(lb).all() and np.isfinite(rb).all()
    assert not np.array_equal(rb[0], rb[1]) and not np.array_equal(rb[1], rb[2])      # the updates moved the parameters
    assert np.array_equal(la, lb) and np.array_equal(ra, rb)
    assert torch.equal(a.loss_hist[:2], lh01) and torch.equal(a.raw_hist[:2], rh01)
    assert not a.loss_hist[3:].any() and not a.raw_hist[3:].any()
