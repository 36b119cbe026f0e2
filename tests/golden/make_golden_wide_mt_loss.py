"""Golden 6-iteration GCV and CV fit trajectories of MULTITASK and DERIVATIVE-INFORMED fast GPs on wide inputs
(9 <= d <= 64) with the SAME n in every task, from the REAL reference, into tests/golden/wide_mt_loss/<case>_<metric>.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_mt_loss.py [fixture names...]

Same import route as make_golden_wide_mt_fit.py (oracle/refshim) and the same gen_case (make_golden_wide_mt.py), which
builds the GP, the data and the fit.  gen_case fits the MLL; here it is handed the reference's GP classes with fit()
bound to the metric (fit(loss_metric=..., cv_weights=CV_WEIGHT)), nothing else changed.  Only what a fit test needs is
kept: the point sets, the data, the histories and the posterior mean at 7 test points.

Cases (the smallest shapes at which the loss stage of fgp_wide_mt_fit_run can go wrong):
  mt_lattice_d12_a2_T3_n64      lattice alpha = 2, T = 3, n = [64, 64, 64], learned rank-1 task kernel: one wave of
                                frequencies in a partly filled workgroup
  mt_net_d9_a2_T2_n512_b2       net alpha = 2, T = 2, n = [512, 512], shape_batch = [2]: two workgroups (the second
                                level of the sums) and B > 1
  deriv_lattice_d12_a2_n64      lattice alpha = 2, (f, df/dx0, df/dx11), n = [64, 64, 64]: the fixed task kernel,
                                derivative pairs with P > 1 and conjugated pairs

The oracle's multitask fit knows only the MLL, so the guard against a sign-driven Rprop fork (which would pin nothing) is
the reference against itself: the same case with y scaled by (1 + eps), eps = 1e-12, -1e-12 and 1e-10, must give
histories that agree to 1e-9 (both losses scale with the square of y; the parameter histories must not move).  The
script asserts it; change the data seed if a case fails.

The net case is built with noise = 1e-8 (the lattice family's default) in place of the net family's default 1e-16.
At 1e-16 both losses are invariant to the kernel's scale down to rounding, the sign of d loss / d raw_scale is noise, and
the reference's own scale history is a coin flip per iteration: over 30 data seeds its loss, lengthscale and task-kernel
histories repeated to 2e-12 under y (1 + 1e-12) while the scale histories differed by 6 - 66 %; the two seeds that
passed one perturbation failed the next.  No seed can mend that, so the noise is what the fixture changes; it is stored
(`ctor_noise`) and the tests build their GP with it.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle.refshim.load_reference import import_reference  # noqa: E402
from make_golden_wide_mt import _e, gen_case  # noqa: E402

OUT = os.path.join(HERE, "wide_mt_loss")
FIT_ITS = 6
N_TEST = 7
CV_WEIGHT = 0.75
PERTURB = (1e-12, -1e-12, 1e-10)
NET_NOISE = 1e-8
HISTS = ("loss_hist", "scale_hist", "lengthscales_hist", "task_kernel_hist")
KEEP = ("family", "kind", "d", "alpha", "ns", "B", "lengthscales", "z", "C", "t", "shifts", "x_test", "fit_iterations",
        "fit_loss_hist", "fit_scale_hist", "fit_lengthscales_hist", "fit_task_kernel_hist", "fit_pmean")
KEEP_PREFIX = ("x_", "y_", "derivatives_")


def _cases():
    d12 = [_e(12)[None], _e(12, 0)[None], _e(12, 11)[None]]
    return [
        # name, family, d, alpha, ns, B, derivatives, derivatives_coeffs, seed, constructor arguments
        ("mt_lattice_d12_a2_T3_n64", "lattice", 12, 2, [64, 64, 64], 0, None, None, 11, {}),
        ("mt_net_d9_a2_T2_n512_b2", "net", 9, 2, [512, 512], 2, None, None, 11, {"noise": NET_NOISE}),
        ("deriv_lattice_d12_a2_n64", "lattice", 12, 2, [64, 64, 64], 0, d12, None, 11, {}),
    ]


def _with_metric(fg, metric, yscale, ctor_kw):
    """The reference module as gen_case takes it, its two GP classes built with ctor_kw on top of gen_case's arguments and
    fitting `metric` on data scaled by yscale."""
    def bind(cls):
        class Bound(cls):
            def __init__(self, *a, **kw):
                kw.update(ctor_kw)
                super().__init__(*a, **kw)

            def add_y_next(self, ys, *a, **kw):
                return super().add_y_next([y * yscale for y in ys], *a, **kw)

            def fit(self, *a, **kw):
                kw.update(loss_metric=metric)
                if metric == "CV":
                    kw.update(cv_weights=CV_WEIGHT)
                return super().fit(*a, **kw)
        Bound.__name__ = cls.__name__
        return Bound
    return types.SimpleNamespace(FastGPLattice=bind(fg.FastGPLattice), FastGPDigitalNetB2=bind(fg.FastGPDigitalNetB2))


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for name, family, d, alpha, ns, B, derivs, dcoeffs, seed, ctor_kw in _cases():
        for metric in ("GCV", "CV"):
            full_name = "%s_%s" % (name, metric.lower())
            if only and full_name not in only and name not in only:
                continue
            full = None
            for eps in (0.0,) + PERTURB:
                run = gen_case(_with_metric(fg, metric, 1.0 + eps, ctor_kw), qmcpy, family, d, alpha, ns, B, derivs, dcoeffs,
                               seed=seed, fit_its=FIT_ITS)
                assert int(run["fit_iterations"]) == FIT_ITS
                if full is None:
                    full = run
                    continue
                errs = {k: _rel(run["fit_" + k], full["fit_" + k]) for k in HISTS}
                print(full_name, "reference vs reference on y (1 + %g):" % eps, {k: "%.2e" % v for k, v in errs.items()})
                assert all(v < 1e-9 for v in errs.values()), "%s: the trajectory forks; change the data seed" % full_name
            out = {k: v for k, v in full.items() if k in KEEP or k.startswith(KEEP_PREFIX)}
            out["x_test"] = full["x_test"][:N_TEST]
            out["fit_pmean"] = full["fit_pmean"][..., :N_TEST]
            out["metric"] = np.array(metric)
            out["cv_weight"] = np.array(CV_WEIGHT if metric == "CV" else 1.0)
            for k, v in ctor_kw.items():
                out["ctor_" + k] = np.array(v)
            fn = os.path.join(OUT, full_name + ".npz")
            np.savez_compressed(fn, **out)
            print("wrote %s (%d KB)  fit loss %s" % (full_name, os.path.getsize(fn) // 1024, out["fit_loss_hist"].reshape(-1)))


if __name__ == "__main__":
    main()
