"""ms per post_mean call of a multitask / derivative-informed GP on wide inputs (9 <= d <= 64): the matrix-free sum
(fgp_mt_wide_post_mean, FGP_WIDE_MT_POST_MEAN=1) against the kernel rows and an einsum (FGP_WIDE_MT_POST_MEAN=0), in one
process, with the peak device memory of each route.

    python tools/prof_wide_mt_post_mean.py [--rounds R] [--out FILE.json] [config names...]

One untimed call per switch warms up every shape; then R rounds (default 5), each timing 2 calls of one route and 2 of
the other, the order alternating, every call ending in a device synchronise.  The figure is the median over the 2 R
timings of a route with the minimum and maximum beside it; the baseline is the rows route of the same run.  The
coefficients are cached before the first call (both routes share the solve).  Peak memory:
torch.cuda.max_memory_allocated over one call of the route, above what is allocated before it.  Needs a GPU.

Configurations (all tasks requested; rows_bytes = 8 T N sum n):
  deriv_lat_d16_N256     lattice, f and two first partial derivatives (T = 3), n = 2^16 each, d = 16, N = 256
  deriv_lat_d64_N256     the same at d = 64
  mt_net_d16_N256        digital net, T = 3 tasks, n = 2^16 each, d = 16, N = 256
  deriv_lat_d16_N64      the first with N = 64 (302 MB of rows)
  deriv_lat_d16_N4096    N = 4096 against n = 2^14 each
  deriv_lat_d16_small    N = 64 against n = 2^12 each (19 MB of rows)
  deriv_lat_d16_n1024    N = 64 against n = 2^10 each (4.7 MB): just above the default threshold 2^22
  deriv_lat_d16_n256     N = 64 against n = 2^8 each (1.2 MB): below it
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastgaussianprocesses_amd as F  # noqa: E402

DEV = "cuda"
SWITCH = "FGP_WIDE_MT_POST_MEAN"
# name -> (family, d, n per task, N, derivative-informed)
CONFIGS = {"deriv_lat_d16_N256": ("lattice", 16, 1 << 16, 256, True), "deriv_lat_d64_N256": ("lattice", 64, 1 << 16, 256, True),
           "mt_net_d16_N256": ("net", 16, 1 << 16, 256, False), "deriv_lat_d16_N64": ("lattice", 16, 1 << 16, 64, True),
           "deriv_lat_d16_N4096": ("lattice", 16, 1 << 14, 4096, True), "deriv_lat_d16_small": ("lattice", 16, 1 << 12, 64, True),
           "deriv_lat_d16_n1024": ("lattice", 16, 1 << 10, 64, True), "deriv_lat_d16_n256": ("lattice", 16, 1 << 8, 64, True)}
T = 3


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def _net_matrices(d, seed, t=32, mcols=32):
    """Unit-upper-triangular generating matrices (tools/wide_kernels.py)."""
    rng = np.random.default_rng(seed)
    C = np.zeros((d, mcols), dtype=np.uint64)
    for j in range(d):
        for k in range(mcols):
            hi = int(rng.integers(0, 1 << k)) if k > 0 else 0
            C[j, k] = np.uint64((1 << (t - 1 - k)) | (hi << (t - k)))
    return C


def make_gp(name):
    fam, d, n, _, deriv = CONFIGS[name]
    kw = dict(num_tasks=T, alpha=2, device=DEV, lengthscales=0.05)
    if deriv:
        kw["derivatives"] = [torch.zeros((1, d), dtype=torch.int64)] + \
            [torch.eye(d, dtype=torch.int64)[j:j + 1] for j in range(T - 1)]
    if fam == "lattice":
        gp = F.FastGPLattice([F.Lattice(d, seed=3 + l) for l in range(T)], **kw)
    else:
        C = _net_matrices(d, 3)
        gp = F.FastGPDigitalNetB2([F.DigitalNetB2(d, seed=3 + l, generating_matrices=C) for l in range(T)], **kw)
    xs = gp.get_x_next(n=[n] * T)
    ys = []
    for l, x in enumerate(xs):
        if deriv:
            x = x.clone().requires_grad_()
            y = _smooth(x)
            if l > 0:
                y = torch.autograd.grad(y.sum(), x)[0][:, l - 1]
            ys.append(y.detach())
        else:
            ys.append(_smooth(x) * (1 + 0.2 * l) + 0.1 * l)
    gp.add_y_next(ys)
    return gp


def measure(name, rounds):
    gp = make_gp(name)
    points = CONFIGS[name][3]
    xd = torch.rand((points, gp.d), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        gp.coeffs
    out, peak, ms = {}, {}, {"1": [], "0": []}

    def call(env):
        os.environ[SWITCH] = env
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[env] = gp.post_mean(xd)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for env in ("1", "0"):                                  # warm-up of every shape, and the peak of one call
        out.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call(env)
        peak[env] = torch.cuda.max_memory_allocated() - base
    for r in range(rounds):
        for env in (("1", "0") if r % 2 else ("0", "1")):
            ms[env] += [call(env), call(env)]
    os.environ.pop(SWITCH, None)
    mf, rw = statistics.median(ms["1"]), statistics.median(ms["0"])
    diff = float((out["1"] - out["0"]).abs().max() / out["0"].abs().max())
    return dict(config=name, d=gp.d, ns=list(gp._ns), points=points, rounds=rounds,
                rows_bytes=8 * T * points * sum(gp._ns),
                matrix_free_ms=mf, matrix_free_ms_min_max=[min(ms["1"]), max(ms["1"])],
                rows_einsum_ms=rw, rows_einsum_ms_min_max=[min(ms["0"]), max(ms["0"])],
                ratio_rows_over_matrix_free=rw / mf,
                matrix_free_peak_bytes=peak["1"], rows_einsum_peak_bytes=peak["0"], max_rel_diff=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("configs", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_wide_mt_post_mean: no GPU; nothing is measured without one")
    torch.set_default_dtype(torch.float64)
    rows = []
    for name in a.configs:
        rows.append(measure(name, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
