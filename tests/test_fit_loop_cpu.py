"""fit_loop (the early-stopping rule, the chunk schedule, the device-side best iterate, the history flags, the
strategies that drive an engine) and fit_engine.FitEngine's history growth, on CPU tensors: no GPU and no GP object."""
import math
import types

import pytest
import torch

from fastgaussianprocesses_amd.fit_engine import FitEngine
from fastgaussianprocesses_amd.fit_loop import (FitLog, StopRule, chunk_schedule, first_minimum, fit_all_rows,
                                                fit_chunked, hist_flags)

nan = math.nan
LOGTOL = math.log(1.05)
# (stop, best_i) for stop_crit_wait_iterations 1, 2, 10, iterations = len(L) - 1, computed on the CPU from the rule as
# the generic autograd loop stated it before StopRule existed
TABLE = {
    "decreasing": ([10 - 0.5 * i for i in range(40)], (39, 39), (39, 39), (39, 39)),
    "plateau": ([5.0] * 40, (1, 0), (2, 0), (10, 0)),
    "tie": ([3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], (3, 2), (4, 2), (12, 2)),
    "nan_mid": ([3, 2, nan, 1.5, nan, nan, 1.4, 1.39, 1.38, 1.37, 1.36, 1.35, 1.34, 1.33, 1.32, 1.31, 1.3],
                (2, 1), (5, 3), (16, 16)),
    "slow": ([10 * math.exp(-0.01 * i) for i in range(200)], (73, 73), (144, 144), (199, 199)),
    "rise_fall": ([1, 2, 3, 0.5, 0.6, 0.7, 0.2] + [0.2] * 30, (1, 0), (2, 0), (16, 6)),
}


def _drive(rule, L):
    for i, lv in enumerate(L):
        if rule.push(i, lv):
            return
    raise AssertionError("the rule did not stop by iteration %d" % rule.iterations)


@pytest.mark.parametrize("name", sorted(TABLE))
@pytest.mark.parametrize("col,wait", [(1, 1), (2, 2), (3, 10)])
def test_stop_rule_table(name, col, wait):
    L = TABLE[name][0]
    rule = StopRule(len(L) - 1, LOGTOL, wait)
    assert rule.stop is None
    _drive(rule, L)
    assert (rule.stop, rule.best_i) == TABLE[name][col]
    assert rule.can_stop_early == (not wait > len(L) - 1)


def test_stop_rule_zero_iterations_and_can_stop_early():
    rule = StopRule(0, LOGTOL, 10)
    assert rule.push(0, 7.0) and (rule.stop, rule.best_i) == (0, 0)
    for iterations in (0, 1, 5, 10):
        for wait in (1, 5, 6, 10, 11):
            assert StopRule(iterations, LOGTOL, wait).can_stop_early == (not wait > iterations)


def test_chunk_schedule():
    T, F = True, False
    assert list(chunk_schedule(1)) == [(0, 1, T)]
    assert list(chunk_schedule(5)) == [(0, 4, F), (4, 1, T)]
    assert list(chunk_schedule(51)) == [(0, 4, F), (4, 8, F), (12, 16, F), (28, 23, T)]
    assert list(chunk_schedule(200)) == [(0, 4, F), (4, 8, F), (12, 16, F), (28, 32, F), (60, 64, F), (124, 64, F),
                                         (188, 12, T)]


def test_first_minimum():
    col = torch.tensor([nan, 3, 1, 1, nan, 0.5, 0.5])
    r = first_minimum(col)
    assert torch.is_tensor(r) and r.dim() == 0 and int(r) == 5
    r = first_minimum(torch.tensor([nan, nan]))
    assert torch.is_tensor(r) and int(r) == 0
    m = torch.stack([col, torch.tensor([2, 1, 1, nan, 4, 4, 4.0]), torch.full((7,), nan)], 1)      # [rows, P]
    r = first_minimum(m)
    assert torch.is_tensor(r) and r.tolist() == [5, 1, 0]


class _Engine(FitEngine):
    """A FitEngine on CPU tensors: the losses come from a sequence, run() records its calls and writes its rows."""

    def __init__(self, losses=(), problems=1, n_params=3):
        self.device = torch.device("cpu")
        self.P, self.n_params, self.sizes = problems, n_params, (1, n_params - 2, 1)
        self.losses, self.calls, self.moved, self.desc = list(losses), [], 0, None
        self.raw = torch.zeros(n_params)

    def _hist_problems(self):
        return self.P

    def _history_moved(self):
        self.moved += 1
        self.desc = (self.loss_hist.data_ptr(), self.raw_hist.data_ptr())

    def run(self, iter0, iters, final_no_update=False):
        self.ensure_history(iter0 + iters)
        self.calls.append((iter0, iters, final_no_update))
        for i in range(iter0, iter0 + iters):
            self.loss_hist[i, :, 0] = self.losses[i]
            self.loss_hist[i, :, 1:] = torch.tensor([10.0 + i, 20.0 + i])
            self.raw_hist[i] = float(i)


def _logged(capsys):
    """The iterations of the rows a FitLog printed (the lines after the header and its rule)."""
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split("|")[0].strip().startswith("iter of") and set(lines[1].strip()) == {"~"}
    return [int(float(ln.split("|")[0])) for ln in lines[2:]]


def test_chunked_strategy_stops_early(capsys):
    L = TABLE["tie"][0]
    eng = _Engine(L)
    rule = StopRule(14, LOGTOL, 2)
    last_i, best_i, losses = fit_chunked(eng, rule, FitLog(2, 4, 14))
    assert eng.calls == [(0, 4, False), (4, 8, False)]
    assert (last_i, best_i) == (4, 2) and rule.stop == 4
    assert losses == [(float(L[i]), 10.0 + i, 20.0 + i) for i in range(5)]
    assert _logged(capsys) == [0, 2, 4]


def test_all_rows_strategy_decides_on_the_device(capsys):
    L = TABLE["tie"][0]
    eng = _Engine(L)
    rule = StopRule(14, LOGTOL, 20)
    assert not rule.can_stop_early
    last_i, best_i, losses = fit_all_rows(eng, rule, FitLog(0, 4, 14), False)
    assert eng.calls == [(0, 15, True)]
    assert last_i == 14 and torch.is_tensor(best_i) and int(best_i) == 2 and losses == []
    assert capsys.readouterr().out == ""
    # the same fit with its losses wanted and logged: still one enqueue, every row read back
    eng = _Engine(L)
    last_i, best_i, losses = fit_all_rows(eng, StopRule(14, LOGTOL, 20), FitLog(5, 0, 14), True)
    assert eng.calls == [(0, 15, True)] and int(best_i) == 2 and [v[0] for v in losses] == [float(v) for v in L]
    assert _logged(capsys) == [0, 5, 10, 14]


def test_ensure_history_growth():
    eng = _Engine(problems=3, n_params=5)
    assert eng.max_iters == 0 and eng.loss_hist is None and eng.raw_hist is None
    eng.ensure_history(1)
    assert eng.max_iters == 16 and eng.moved == 1
    assert tuple(eng.loss_hist.shape) == (16, 3, 3) and tuple(eng.raw_hist.shape) == (16, 5)
    assert eng.loss_hist.dtype == torch.float64 and not eng.loss_hist.any() and not eng.raw_hist.any()
    eng.ensure_history(16)
    assert eng.max_iters == 16 and eng.moved == 1
    eng.loss_hist[:16] = torch.arange(16.0 * 9).reshape(16, 3, 3) + 1
    eng.raw_hist[:16] = torch.arange(16.0 * 5).reshape(16, 5) + 1
    lh, rh = eng.loss_hist.clone(), eng.raw_hist.clone()
    eng.ensure_history(17)
    assert eng.max_iters == 32 and eng.moved == 2
    assert tuple(eng.loss_hist.shape) == (32, 3, 3) and tuple(eng.raw_hist.shape) == (32, 5)
    assert eng.desc == (eng.loss_hist.data_ptr(), eng.raw_hist.data_ptr())
    assert torch.equal(eng.loss_hist[:16], lh) and torch.equal(eng.raw_hist[:16], rh)
    assert not eng.loss_hist[16:].any() and not eng.raw_hist[16:].any()
    eng.ensure_history(20)
    assert eng.max_iters == 32 and eng.moved == 2
    eng.ensure_history(100)
    assert eng.max_iters == 100 and eng.moved == 3 and tuple(eng.loss_hist.shape) == (100, 3, 3)
    assert torch.equal(eng.loss_hist[:16], lh) and torch.equal(eng.raw_hist[:16], rh)
    one = _Engine()
    one.ensure_history(2)
    assert tuple(one.loss_hist.shape) == (16, 1, 3) and FitEngine._hist_problems(one) == 1


def test_engine_defaults_and_split_raw():
    eng = _Engine(n_params=5)
    assert eng.persist_ok() is False and eng.release_inputs() is None
    row = torch.arange(5.0)
    assert eng.split_task(row) is None and eng.task_kernel_rows(row[None]) is None
    s, l, nz = eng.split_raw(torch.arange(10.0).reshape(2, 5))
    assert s.tolist() == [[0], [5]] and l.tolist() == [[1, 2, 3], [6, 7, 8]] and nz.tolist() == [[4], [9]]


def _gp(scale=False, lengthscales=False, noise=False, factor=False, task_noise=False):
    def rg(on):
        return types.SimpleNamespace(requires_grad=on)
    return types.SimpleNamespace(raw_scale=rg(scale), raw_lengthscales=rg(lengthscales), raw_noise=rg(noise),
                                 raw_factor_task_kernel=rg(factor), raw_noise_task_kernel=rg(task_noise))


def test_hist_flags():
    keys = ("loss", "scale", "lengthscales", "noise", "task_kernel")
    assert hist_flags(_gp()) == dict.fromkeys(keys, False)
    assert hist_flags(_gp(), store_hists=True) == dict.fromkeys(keys, True)         # store_hists wins
    assert hist_flags(_gp(), store_loss_hist=True) == dict(dict.fromkeys(keys, False), loss=True)
    every = dict(store_loss_hist=True, store_scale_hist=True, store_lengthscales_hist=True, store_noise_hist=True,
                 store_task_kernel_hist=True)
    assert hist_flags(_gp(), **every) == dict(dict.fromkeys(keys, False), loss=True)
    assert hist_flags(_gp(scale=True), store_scale_hist=True)["scale"] is True
    assert hist_flags(_gp(scale=False, noise=True), store_scale_hist=True)["scale"] is False
    assert hist_flags(_gp(scale=True))["scale"] is False
    assert hist_flags(_gp(lengthscales=True), **every) == dict(dict.fromkeys(keys, False), loss=True, lengthscales=True)
    assert hist_flags(_gp(noise=True), **every) == dict(dict.fromkeys(keys, False), loss=True, noise=True)
    for kw in (dict(factor=True), dict(task_noise=True), dict(factor=True, task_noise=True)):
        assert hist_flags(_gp(**kw), store_task_kernel_hist=True)["task_kernel"] is True
    assert hist_flags(_gp(scale=True), store_task_kernel_hist=True)["task_kernel"] is False
