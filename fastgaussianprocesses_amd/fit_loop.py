"""The rules every fit loop shares, stated once: AbstractGP.fit's early-stopping rule (fastgps/abstract_gp.py:236-284),
the schedule of the chunks a device loop enqueues between two host reads, the best iterate found on the device, which
histories a fit keeps, the fit's table on stdout -- and the four ways a fit_engine.FitEngine is driven through a fit
(DESIGN.md section 3.7).  No GPU dependency: the engines, the GPs and the batch loop import this module.
"""
import math

import torch


class StopRule(object):
    """abstract_gp.py:276-284 on one problem's losses: `best` / `best_i` the first minimum so far (NaN never best),
    `save` the best loss when the last improvement by more than `logtol` was seen, `waited` the iterations since,
    `stop` the iteration the fit ended at (None while it runs)."""

    def __init__(self, iterations, logtol, wait_max):
        self.iterations, self.logtol, self.wait_max = iterations, logtol, wait_max
        self.best, self.best_i, self.save, self.waited, self.stop = math.inf, 0, math.inf, 0, None

    @property
    def can_stop_early(self):
        """False: every iteration runs whatever the losses are, so nothing has to be decided on the host."""
        return self.wait_max <= self.iterations

    def push(self, i, lv):
        """Iteration i evaluated the loss lv; True when the fit ends with it (no update follows)."""
        if lv < self.best:
            self.best, self.best_i = lv, i
        if (self.save - lv) > self.logtol:
            self.waited = 0
            self.save = self.best
        else:
            self.waited += 1
        if i == self.iterations or self.waited == self.wait_max:
            self.stop = i
            return True
        return False


def chunk_schedule(total):
    """(iter0, k, final_no_update) of the chunks of `total` iterations: 4, 8, 16, 32, 64, 64, ... (short first chunks:
    an early stop costs few discarded iterations; long later ones: few host reads), the last clipped."""
    i0, chunk = 0, 4
    while i0 < total:
        k = min(chunk, total - i0)
        yield i0, k, i0 + k == total
        i0 += k
        chunk = min(64, chunk * 2)


def first_minimum(loss):
    """Index along dim 0 of the first minimum of a loss history, NaN never chosen: the host rule `lv < best` of a fit
    that cannot stop early, as a tensor on the history's device (no host read)."""
    return torch.where(torch.isnan(loss), torch.full_like(loss, math.inf), loss).argmin(0)


def hist_flags(gp, store_hists=False, store_loss_hist=False, store_scale_hist=False, store_lengthscales_hist=False,
               store_noise_hist=False, store_task_kernel_hist=False):
    """Which histories a fit returns (abstract_gp.py:196-200): a parameter's if it is learned, or with store_hists."""
    return dict(loss=store_hists or store_loss_hist,
                scale=store_hists or (store_scale_hist and gp.raw_scale.requires_grad),
                lengthscales=store_hists or (store_lengthscales_hist and gp.raw_lengthscales.requires_grad),
                noise=store_hists or (store_noise_hist and gp.raw_noise.requires_grad),
                task_kernel=store_hists or (store_task_kernel_hist and (
                    gp.raw_factor_task_kernel.requires_grad or gp.raw_noise_task_kernel.requires_grad)))


class FitLog(object):
    """The fit's table on stdout (abstract_gp.py:237-240, 274-275): the header, every `verbose`-th row and the last."""

    def __init__(self, verbose, indent, iterations):
        self.verbose, self.pad = verbose, " " * indent
        if verbose:
            s = "%16s | %-10s | %-10s | %-10s" % ("iter of %.1e" % iterations, "loss", "term1", "term2")
            print(self.pad + s)
            print(self.pad + "~" * len(s))

    def row(self, i, loss, t1, t2, last):
        """(t1, t2: floats, or tensors, which are read only for a row that is printed: nan unless of one element)"""
        if self.verbose and (i % self.verbose == 0 or last):
            t1, t2 = [(t.item() if t.numel() == 1 else math.nan) if torch.is_tensor(t) else t for t in (t1, t2)]
            print(self.pad + "%16.2e | %-10.2e | %-10.2e | %-10.2e" % (i, loss, t1, t2))


# The four ways to drive an engine through iterations 0 .. rule.iterations.  Each returns (last_i, best_i, losses) --
# best_i a device tensor where no host read decided it, None where the engine's raw vector already holds the best
# iterate; losses the rows (loss, term1, term2) read back, [] when none were -- or None after a barrier give-up of the
# single launch, which restored the entry state: the caller then takes fit_all_rows / fit_chunked (the same trajectory).

def fit_persist_deferred(eng, iterations, logtol, wait_max, restore):
    """The whole fit in one launch (run_persist), which leaves the best iterate in the engine's raw parameters:
    `restore(eng, eng.raw)` installs them while the launch runs, and the control word is read after that (the host work
    overlaps the fit instead of following it).  For a fit that logs nothing and returns no history: the rule runs on
    the device alone, so this strategy takes its numbers and builds no StopRule / FitLog (the small fits' host time)."""
    ip = eng.run_persist(iterations, logtol, wait_max, defer=True)
    if ip is None:
        return None
    restore(eng, eng.raw)
    if ip < 0:
        ip = eng.persist_result()
    return None if ip is None else (ip, None, [])


def fit_persist(eng, rule, log, want_losses):
    """The whole fit in one launch (the early-stopping rule on the device); the last iteration and the failure word
    are read back, the loss rows only where the host needs them (an early stop's best iterate, the log, the history)."""
    ip = eng.run_persist(rule.iterations, rule.logtol, rule.wait_max)
    if ip is None:
        return None
    best_i = None if rule.can_stop_early else first_minimum(eng.loss_hist[:rule.iterations + 1, 0, 0])
    losses = []
    if rule.can_stop_early or log.verbose or want_losses:
        losses = [tuple(r) for r in eng.loss_hist[:ip + 1, 0].cpu().tolist()]
        for r, row in enumerate(losses):
            rule.push(r, row[0])
            log.row(r, row[0], row[1], row[2], r == ip)
    return ip, (rule.best_i if best_i is None else best_i), losses


def fit_all_rows(eng, rule, log, want_losses):
    """No early stop is possible: every iteration in one enqueue, the best iterate found on the device -- no host
    synchronisation unless losses are logged or returned."""
    total = rule.iterations + 1
    eng.run(0, total, final_no_update=True)
    lh = eng.loss_hist[:total, 0]
    best_i = first_minimum(lh[:, 0])
    losses = []
    if log.verbose or want_losses:
        losses = [tuple(r) for r in lh.cpu().tolist()]
        for r, row in enumerate(losses):
            log.row(r, row[0], row[1], row[2], r == rule.iterations)
    return rule.iterations, best_i, losses


def fit_chunked(eng, rule, log):
    """The early-stopping loop: a chunk of iterations is enqueued, its losses are read back and the rule applied row by
    row; the iterations of a chunk after the stop are discarded (the best iterate comes from the history)."""
    losses = []
    for i0, k, last in chunk_schedule(rule.iterations + 1):
        eng.run(i0, k, final_no_update=last)
        for r, row in enumerate(eng.loss_hist[i0:i0 + k, 0].cpu().tolist()):
            losses.append(tuple(row))
            brk = rule.push(i0 + r, row[0])
            log.row(i0 + r, row[0], row[1], row[2], brk)
            if brk:
                return i0 + r, rule.best_i, losses
