"""The wide (d > 8) path alone, for timing and for `rocprofv3 --kernel-trace --stats` passes:

    python tools/wide_kernels.py time [m]    # ms per MLL loss + gradient evaluation, FGP_WIDE_FUSED=1 vs 0
                                             # (alternating), and ms per wide post_mean; one JSON line
    python tools/wide_kernels.py trace [m]   # the fused evaluations and the post_mean only (kernel names k_wide_*)
    python tools/wide_kernels.py trace0 [m]  # the evaluations with the torch formulation of k1 (FGP_WIDE_FUSED=0)
    python tools/wide_kernels.py --fit [m]   # ms per Rprop iteration (time / 21 evaluations) of a 20-iteration fit: the
                                             # device loop (FGP_WIDE_FIT_DEVICE=1, fgp_wide_fit_run) and the generic
                                             # autograd loop alternating in one process, 5 repetitions each and their
                                             # medians; one JSON line
    python tools/wide_kernels.py --fit-trace [m]   # one 20-iteration device-loop fit only (launches per iteration)
    --metric MLL|GCV|CV                      # with --fit / --fit-trace: the loss of the fit (default MLL; CV with
                                             # cv_weights = 0.5); the JSON line names it and the last loss of each loop

    python tools/wide_kernels.py --post-var [m]    # ms per post_var of 64 test points: the Parseval quadratic form
                                             # (fgp_wide_post_var_qf, "qf") and rows-and-solve (FGP_WIDE_POST_VAR_QF=0,
                                             # "rows") in one process, alternating qf - rows - qf per repetition, medians
                                             # of 5, each timing ended by a synchronise after a warm-up of both paths;
                                             # the spread of the two qf series (A - A) and the peak allocation of both
                                             # paths; one JSON line
    --d D / --family lattice|net             # with --post-var: the dimension (default 16) and the family (net: alpha = 1,
                                             # unit-upper-triangular matrices; d = 64: lengthscales linspace(0.01, 0.05))

d = 16, n = 2^m, m = 16 by default (lattice, alpha = 2, lengthscales linspace(0.05, 0.3, d)), one hyper-parameter row; post_mean at
N = 4096 test points, one output.  Byte / operation models:
    k_wide_k1       8 d n + 8 n        bytes
    k_wide_k1_bwd   8 d n + 16 n       bytes  (parts + u read; the partials are d + 1 doubles per 256 points)
    k_wide_post_mean  (4 d + 1) N n    FP64 lane-ops (per pair and dimension: t = |x - z|, u = t^2 - t, u^2 + c', the
                                       product; + the accumulate), as k_post_mean's model
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastgaussianprocesses_amd as F  # noqa: E402
from oracle.fgp_oracle import f_ackley  # noqa: E402

D, M, NT = 16, 16, 4096
VALU_PEAK = 3.93e13      # FP64 lane-ops / s


def make():
    torch.set_default_dtype(torch.float64)
    gp = F.FastGPLattice(F.Lattice(D, seed=3), lengthscales=torch.linspace(0.05, 0.3, D), device="cuda")
    gp.add_y_next(f_ackley(gp.get_x_next(2 ** M)))
    return gp


def evaluate(gp):
    gp._cache = {k: v for k, v in gp._cache.items() if not k[2]}
    loss, _, _, _ = gp._loss_generic("MLL", None, 1, 1)
    loss.backward()
    gp.raw_scale.grad = gp.raw_lengthscales.grad = None
    return loss


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


FIT_ITERS = 20
METRIC = "MLL"


def fit_once(gp, raw0, device_loop):
    """One 20-iteration fit of the loss METRIC from the parameters raw0 (no early stop), by the device loop or the
    generic one."""
    os.environ["FGP_WIDE_FIT_DEVICE"] = "1" if device_loop else "0"
    for name, val in raw0.items():
        old = gp._parameters[name]
        gp._parameters[name] = torch.nn.Parameter(val.clone(), requires_grad=old.requires_grad)
    gp._cache = {k: v for k, v in gp._cache.items() if not k[2]}
    gp._snap = None
    kw = dict(cv_weights=0.5) if METRIC == "CV" else {}
    return gp.fit(loss_metric=METRIC, iterations=FIT_ITERS, verbose=0, stop_crit_wait_iterations=FIT_ITERS + 5,
                  store_loss_hist=True, **kw)


def fit_mode(trace):
    gp = make()
    raw0 = {k: p.detach().clone() for k, p in gp.named_parameters()}
    if trace:
        fit_once(gp, raw0, True)
        torch.cuda.synchronize()
        return
    res = {"d": D, "n": 2 ** M, "metric": METRIC, "iterations": FIT_ITERS,
           "ms_per_iteration": {"device": [], "generic": []}, "last_loss": {}}
    for key, dev in (("device", True), ("generic", False)):
        res["last_loss"][key] = float(fit_once(gp, raw0, dev)["loss_hist"][-1])
    for _ in range(5):                      # alternate the two loops in one process
        for key, dev in (("device", True), ("generic", False)):
            ms = timed(lambda: fit_once(gp, raw0, dev), 1)
            res["ms_per_iteration"][key].append(round(ms / (FIT_ITERS + 1), 4))
    res["median_ms_per_iteration"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms_per_iteration"].items()}
    print(json.dumps(res))


def net_matrices(d, seed, t=32, mcols=32):
    """Unit-upper-triangular generating matrices (column k: bit t-1-k plus random more significant bits)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    C = np.zeros((d, mcols), dtype=np.uint64)
    for j in range(d):
        for k in range(mcols):
            hi = int(rng.integers(0, 1 << k)) if k > 0 else 0
            C[j, k] = np.uint64((1 << (t - 1 - k)) | (hi << (t - k)))
    return C


PV_N = 64


def post_var_mode(family):
    torch.set_default_dtype(torch.float64)
    ls = torch.linspace(0.01, 0.05, D) if D == 64 else torch.linspace(0.05, 0.3, D)
    if family == "lattice":
        gp = F.FastGPLattice(F.Lattice(D, seed=3), lengthscales=ls, device="cuda")
    else:
        seq = F.DigitalNetB2(D, seed=3, generating_matrices=net_matrices(D, 3))
        gp = F.FastGPDigitalNetB2(seq, alpha=1, lengthscales=ls, device="cuda")
    gp.add_y_next(f_ackley(gp.get_x_next(2 ** M)))
    xt = torch.rand((PV_N, D), generator=torch.Generator().manual_seed(5)).to("cuda")

    def run(flag):
        os.environ["FGP_WIDE_POST_VAR_QF"] = flag
        return gp.post_var(xt)

    res = {"family": family, "d": D, "n": 2 ** M, "N": PV_N, "ms": {"qf": [], "rows": [], "qf_again": []}, "peak_bytes": {}}
    pv = {}
    for key, flag in (("qf", "1"), ("rows", "0")):          # warm-up of both paths, and their peak allocation
        run(flag)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pv[key] = run(flag)
        torch.cuda.synchronize()
        res["peak_bytes"][key] = torch.cuda.max_memory_allocated() - base
    res["max_abs_diff_over_kxx"] = float((pv["qf"] - pv["rows"]).abs().max() / gp._kdiag(xt).detach().abs().max())
    for _ in range(5):
        for key, flag in (("qf", "1"), ("rows", "0"), ("qf_again", "1")):
            res["ms"][key].append(round(timed(lambda: run(flag), 1), 4))
    med = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["median_ms"] = med
    res["aa_spread_ms"] = round(abs(med["qf"] - med["qf_again"]), 4)
    res["speedup"] = round(med["rows"] / max(med["qf"], med["qf_again"]), 3)
    print(json.dumps(res))


def main():
    global M, METRIC, D
    argv = list(sys.argv)
    family = "lattice"
    if "--d" in argv:
        i = argv.index("--d")
        D = int(argv[i + 1])
        del argv[i:i + 2]
    if "--family" in argv:
        i = argv.index("--family")
        family = argv[i + 1]
        assert family in ("lattice", "net"), "--family lattice|net"
        del argv[i:i + 2]
    if "--metric" in argv:
        i = argv.index("--metric")
        METRIC = argv[i + 1].upper()
        assert METRIC in ("MLL", "GCV", "CV"), "--metric MLL|GCV|CV"
        del argv[i:i + 2]
    mode = argv[1] if len(argv) > 1 else "time"
    M = int(argv[2]) if len(argv) > 2 else M
    if mode in ("--fit", "--fit-trace"):
        return fit_mode(mode == "--fit-trace")
    if mode == "--post-var":
        return post_var_mode(family)
    gp = make()
    n = 2 ** M
    xt = torch.rand((NT, D), generator=torch.Generator().manual_seed(5)).to("cuda")
    with torch.no_grad():
        gp.coeffs
    if mode in ("trace", "trace0"):
        os.environ["FGP_WIDE_FUSED"] = "1" if mode == "trace" else "0"
        for _ in range(25):
            evaluate(gp)
        for _ in range(10 if mode == "trace" else 0):
            gp.post_mean(xt)
        torch.cuda.synchronize()
        return
    res = {"d": D, "n": n, "N": NT, "eval_ms": {"1": [], "0": []}}
    for flag in ("1", "0"):
        os.environ["FGP_WIDE_FUSED"] = flag
        for _ in range(5):
            evaluate(gp)
    for _ in range(4):                      # alternate the two versions in one process
        for flag in ("1", "0"):
            os.environ["FGP_WIDE_FUSED"] = flag
            res["eval_ms"][flag].append(round(timed(lambda: evaluate(gp), 50), 4))
    os.environ["FGP_WIDE_FUSED"] = "1"
    for _ in range(3):
        gp.post_mean(xt)
    pm = [round(timed(lambda: gp.post_mean(xt), 20), 4) for _ in range(3)]
    res["post_mean_ms"] = pm
    res["post_mean_valu_share_end_to_end"] = round((4 * D + 1) * NT * n / (min(pm) * 1e-3) / VALU_PEAK, 3)
    res["k1_bytes"] = 8 * D * n + 8 * n
    res["k1_bwd_bytes"] = 8 * D * n + 16 * n
    res["post_mean_lane_ops"] = (4 * D + 1) * NT * n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
