"""Device-resident fit loop (MLL, GCV or CV) of wide GPs, 9 <= d <= 64 (fgp_wide_fit_run of include/fgp_hip.h).

`WideMLL` is the wide counterpart of fit_engine.FusedMLL for G independent eigen-problems of size n = 2^m: the kernel
parts ([d, n] shared by every problem, or [G, d, n]), Y[g, k] = sum over the outputs of problem g of |ytilde[k]|^2, the
raw vector [G scales, G dl lengthscales, G noises], the workspace, the Rprop state and the histories, behind the
interface of fit_engine.FitEngine.  Every problem is its own GP (own loss, Rprop state and reduction order): a
problem's trajectory does not depend on the others in the engine.
"""
import ctypes
import math

import torch

from . import _native as N
from .fit_engine import RPROP_ETAS, RPROP_STEPS, FitEngine
from .ops import log2_exact, require_device


def wide_mll_constant(d_out, n):
    """1/2 d_out n log(2 pi): fgp_wide_fit_desc.mll_const, added to 1/2 (norm + w logdet) (abstract_gp.py:235)."""
    return 0.5 * d_out * n * math.log(2 * math.pi)


class WideMLL(FitEngine):
    def __init__(self, family, parts, ysq, raw_scale, raw_lengthscales, raw_noise, logdet_weight, d_out,
                 requires_grad=(True, True, False), lr=0.1, max_iters=1, loss_metric="MLL", cv_weight=1.0):
        """
        family: 0 lattice (FFT) / 1 net (FWHT)
        parts:  [d, n] shared by the G problems, or [G, d, n]
        ysq:    [G, n]
        raw_scale [G], raw_lengthscales [G, dl] with dl in {1, d}, raw_noise [G]
        d_out:  outputs in each problem's loss (the constant 1/2 d_out n log(2 pi))
        loss_metric: "MLL", "GCV" or "CV" (fgp_wide_fit_desc.loss_metric); cv_weight: CV's scalar weight.  The history
                rows of GCV are (loss, numer, denom), of CV (loss, nan, nan); neither uses logdet_weight or d_out.
        """
        require_device(ysq, "WideMLL")
        self.device = ysq.device
        self.family = int(family)
        G, n = ysq.shape
        self.G, self.n, self.m = int(G), int(n), log2_exact(n)
        d = int(parts.shape[-2])
        if not (N.MAX_D < d <= N.WIDE_MAX_D):
            raise ValueError("the wide fit loop takes %d <= d <= %d" % (N.MAX_D + 1, N.WIDE_MAX_D))
        if tuple(parts.shape) not in ((d, n), (G, d, n)):
            raise ValueError("parts must be [d, n] or [G, d, n]")
        self.d = d
        self.parts = parts.to(torch.float64).contiguous()
        self.ysq = ysq.to(torch.float64).contiguous()
        dl = int(raw_lengthscales.shape[-1])
        if raw_scale.numel() != G or raw_noise.numel() != G or tuple(raw_lengthscales.shape) != (G, dl) or dl not in (1, d):
            raise ValueError("raw_scale [G], raw_lengthscales [G, 1 or d], raw_noise [G]")
        self.dl = dl
        self.sizes = (G, G * dl, G)
        self.n_params = G * (2 + dl)
        self.raw = torch.cat([raw_scale.reshape(-1), raw_lengthscales.reshape(-1), raw_noise.reshape(-1)]).to(
            device=self.device, dtype=torch.float64).contiguous()
        np_ = self.n_params
        st = torch.zeros((3, np_), dtype=torch.float64, device=self.device)
        self.prev, self.step, self.grad = st[0], st[1], st[2]
        self.requires_grad = tuple(int(bool(r)) for r in requires_grad)
        self.lr = float(lr)
        self.logdet_weight = float(logdet_weight)
        self.mll_const = wide_mll_constant(d_out, n)
        if loss_metric not in ("MLL", "GCV", "CV"):
            raise ValueError("loss_metric must be MLL, GCV or CV")
        self.loss_metric = loss_metric
        self.cv_weight = float(cv_weight)
        self._desc = N.WideFitDesc(
            family=self.family, log2n=self.m, d=d, G=self.G, parts=self.parts.data_ptr(),
            parts_stride=(d * n if self.parts.dim() == 3 else 0), ysq=self.ysq.data_ptr(), raw=self.raw.data_ptr(),
            dl=dl, scale_rg=self.requires_grad[0], ls_rg=self.requires_grad[1], noise_rg=self.requires_grad[2],
            logdet_weight=self.logdet_weight, mll_const=self.mll_const, rprop_prev=self.prev.data_ptr(),
            rprop_step=self.step.data_ptr(), lr=self.lr, eta_minus=RPROP_ETAS[0], eta_plus=RPROP_ETAS[1],
            step_min=RPROP_STEPS[0], step_max=RPROP_STEPS[1], loss_hist=0, raw_hist=0, grad_out=self.grad.data_ptr(),
            work=0, loss_metric={"MLL": N.LOSS_MLL, "GCV": N.LOSS_GCV, "CV": N.LOSS_CV}[loss_metric],
            cv_weight=self.cv_weight)
        wlen = ctypes.c_int64(0)
        N.call("fgp_wide_fit_work", self._desc, ctypes.byref(wlen))
        self.work = torch.empty((wlen.value,), dtype=torch.float64, device=self.device)
        self._desc.work = self.work.data_ptr()
        self.ensure_history(max(int(max_iters), 16))

    def _hist_problems(self):
        return self.G

    def _history_moved(self):
        self._desc.loss_hist = self.loss_hist.data_ptr()
        self._desc.raw_hist = self.raw_hist.data_ptr()

    def run(self, iter0, iters, final_no_update=False):
        """Enqueue `iters` fit iterations writing history rows iter0 .. iter0 + iters - 1 (fgp_wide_fit_run: plain
        launches on the current stream, no host synchronisation).  iter0 = 0 starts a new fit (Rprop state reset)."""
        self.ensure_history(iter0 + iters)
        N.call("fgp_wide_fit_run", self._desc, int(iter0), int(iters), int(bool(final_no_update)),
               N.stream_ptr(self.device))
