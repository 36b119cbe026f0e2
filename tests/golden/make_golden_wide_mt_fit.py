"""Golden 12-iteration fit trajectories of MULTITASK and DERIVATIVE-INFORMED fast GPs on wide inputs (9 <= d <= 64),
from the REAL reference, into tests/golden/wide_mt_fit/*.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_mt_fit.py [fixture names...]

Same import route as make_golden_wide_mt.py (oracle/refshim), whose gen_case builds the GP, the data and the fit; only
what a fit test needs is kept (the point sets, the data, the test points and the fit's histories and posterior mean).
Over 12 iterations torch.optim.Rprop's sign flips and step shrinking are exercised, which the 3-iteration trajectories
of tests/golden/wide_mt/ do not reach.

Cases:
  deriv_lattice_d12_a2_it12   lattice alpha = 2, (f, df/dx0, df/dx11), n = [64, 64, 64]
  mt_net_d9_a2_T2_it12        net alpha = 2, T = 2 (the default learned rank-1 task kernel), n = [32, 128]

A case is kept only if OracleMultiTaskFastGP.fit on the CPU follows the reference's histories within the tolerances of
the trajectory tests (loss 2e-7, parameter histories 1e-10, posterior mean 1e-7): a sign-driven Rprop step that forks
between two correct implementations would pin nothing.  The script asserts it; change the data seed if it fails.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle.refshim.load_reference import import_reference  # noqa: E402
from make_golden_wide_mt import _e, gen_case  # noqa: E402

OUT = os.path.join(HERE, "wide_mt_fit")
FIT_ITS = 12
KEEP = ("family", "kind", "d", "alpha", "ns", "B", "lengthscales", "z", "C", "t", "shifts", "x_test", "fit_iterations",
        "fit_loss_hist", "fit_scale_hist", "fit_lengthscales_hist", "fit_task_kernel_hist", "fit_pmean")
KEEP_PREFIX = ("x_", "y_", "derivatives_")


def _cases():
    d12 = [_e(12)[None], _e(12, 0)[None], _e(12, 11)[None]]
    return [
        # name, family, d, alpha, ns, B, derivatives, derivatives_coeffs, seed
        ("deriv_lattice_d12_a2_it12", "lattice", 12, 2, [64, 64, 64], 0, d12, None, 11),
        ("mt_net_d9_a2_T2_it12", "net", 9, 2, [32, 128], 0, None, None, 11),
    ]


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def oracle_follows(out):
    """OracleMultiTaskFastGP.fit on the stored inputs against the stored histories; the worst relative errors."""
    from oracle.fgp_oracle_mt import OracleMultiTaskFastGP
    T = len(out["ns"])
    ys = [torch.from_numpy(out["y_%d" % l]) for l in range(T)]
    derivs = dcoeffs = None
    if str(out["kind"]) == "deriv":
        derivs = [torch.from_numpy(out["derivatives_%d" % l]) for l in range(T)]
        dcoeffs = [torch.from_numpy(out["derivatives_coeffs_%d" % l]) for l in range(T)]
    lattice = str(out["family"]) == "lattice"
    o = OracleMultiTaskFastGP(str(out["family"]), out["z"] if lattice else out["C"], out["shifts"], ys,
                              alpha=int(out["alpha"]), t=32 if lattice else int(out["t"]), derivatives=derivs,
                              derivatives_coeffs=dcoeffs)
    with torch.no_grad():
        o.raw_lengthscales.copy_(torch.log(torch.from_numpy(out["lengthscales"])))
    its = int(out["fit_iterations"])
    data = o.fit(iterations=its, stop_crit_wait_iterations=its + 5)
    errs = {k: _rel(data[k].numpy(), out["fit_" + k]) for k in ("loss_hist", "scale_hist", "lengthscales_hist",
                                                               "task_kernel_hist")}
    errs["pmean"] = _rel(o.post_mean(torch.from_numpy(out["x_test"])).detach().numpy(), out["fit_pmean"])
    ok = data["iterations"] == its and errs["loss_hist"] < 2e-7 and errs["pmean"] < 1e-7 and all(
        errs[k] < 1e-10 for k in ("scale_hist", "lengthscales_hist", "task_kernel_hist"))
    return ok, errs


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for name, family, d, alpha, ns, B, derivs, dcoeffs, seed in _cases():
        if only and name not in only:
            continue
        full = gen_case(fg, qmcpy, family, d, alpha, ns, B, derivs, dcoeffs, seed=seed, fit_its=FIT_ITS)
        out = {k: v for k, v in full.items() if k in KEEP or k.startswith(KEEP_PREFIX)}
        assert int(out["fit_iterations"]) == FIT_ITS
        ok, errs = oracle_follows(out)
        print(name, "oracle vs reference:", {k: "%.2e" % v for k, v in errs.items()})
        assert ok, "%s: the CPU oracle does not follow the reference's trajectory; change the data seed" % name
        fn = os.path.join(OUT, name + ".npz")
        np.savez_compressed(fn, **out)
        print("wrote %s (%d KB)  fit loss %s" % (name, os.path.getsize(fn) // 1024, out["fit_loss_hist"].reshape(-1)))


if __name__ == "__main__":
    main()
