"""ms per prediction call of a multitask / derivative-informed GP at d <= 8: the fused task-pair kernel (fgp_mt_rows,
fgp_mt_post_mean; the default) against the parent route FGP_MT_FUSED_ROWS=0 (fgp_mt_parts + the torch formulation), in
one process, with the peak device memory of each route.

    python tools/prof_mt_narrow_pred.py [--rounds R] [--out FILE.json] [config names...]

Routes timed per configuration (environment switches set around each call):
  post_mean   parent (FGP_MT_FUSED_ROWS=0), fused rows + einsum (FGP_WIDE_MT_POST_MEAN=0), matrix-free (=1)
  post_var    the quadratic form (FGP_MT_POST_VAR_QF=1) and rows-and-solve (=0), each parent and fused

One untimed call per route warms up every shape and gives its peak memory (torch.cuda.max_memory_allocated over the call,
above what is allocated before it); then R rounds (default 5), each timing 2 calls of every route of a method, the order
of the routes reversed every other round, every call ending in a device synchronise.  The figure is the median over the
2 R timings with the minimum and maximum beside it: the parent's own minimum .. maximum is the spread a difference is
held against.  The coefficients and the factor are cached before the first call (all routes share them).  Needs a GPU.

Configurations: T = 3 tasks (lattice, alpha = 2) at d in {1, 3, 6}, n in {2^12, 2^16} per task, N in {64, 256} test
points, named mt_d<d>_n<log2 n>_N<N>; grad_d4_n14_N256: f and its first two partial derivatives at d = 4, n = 2^14.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastgaussianprocesses_amd as F  # noqa: E402

DEV = "cuda"
T = 3
# name -> (d, log2 n per task, N, derivative-informed)
CONFIGS = {"mt_d%d_n%d_N%d" % (d, m, N): (d, m, N, False) for d in (1, 3, 6) for m in (12, 16) for N in (64, 256)}
CONFIGS["grad_d4_n14_N256"] = (4, 14, 256, True)
SWITCHES = ("FGP_MT_FUSED_ROWS", "FGP_WIDE_MT_POST_MEAN", "FGP_MT_POST_VAR_QF")
# method -> route -> the switches' values
ROUTES = {
    "post_mean": {"parent": ("0", "0", None), "fused_rows": ("1", "0", None), "fused_matrix_free": ("1", "1", None)},
    "post_var": {"parent_qf": ("0", None, "1"), "fused_qf": ("1", None, "1"), "parent_rows_solve": ("0", None, "0"),
                 "fused_rows_solve": ("1", None, "0")},
}

# the parent route a route is held against (a parent route: itself; post_mean's routes: "parent")
BASE = {"fused_qf": "parent_qf", "fused_rows_solve": "parent_rows_solve", "parent_qf": "parent_qf",
        "parent_rows_solve": "parent_rows_solve"}


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def make_gp(name):
    d, m, _, deriv = CONFIGS[name]
    kw = dict(num_tasks=T, alpha=2, device=DEV, lengthscales=0.05)
    if deriv:
        kw["derivatives"] = [torch.zeros((1, d), dtype=torch.int64)] + \
            [torch.eye(d, dtype=torch.int64)[j:j + 1] for j in range(T - 1)]
    gp = F.FastGPLattice([F.Lattice(d, seed=3 + l) for l in range(T)], **kw)
    xs = gp.get_x_next(n=[1 << m] * T)
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


def _set(values):
    for k, v in zip(SWITCHES, values):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def measure(name, rounds):
    gp = make_gp(name)
    points = CONFIGS[name][2]
    xd = torch.rand((points, gp.d), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        gp.coeffs
    row = dict(config=name, d=gp.d, ns=list(gp._ns), points=points, rounds=rounds, rows_bytes=8 * T * points * sum(gp._ns))
    for method, routes in ROUTES.items():
        fn = getattr(gp, method)
        out, peak, ms = {}, {}, {r: [] for r in routes}

        def call(route):
            _set(routes[route])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[route] = fn(xd)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for route in routes:                                # warm-up of every shape, and the peak of one call
            out.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            call(route)
            peak[route] = torch.cuda.max_memory_allocated() - base
        order = list(routes)
        for r in range(rounds):
            for route in (order if r % 2 == 0 else order[::-1]):
                ms[route] += [call(route), call(route)]
        _set((None, None, None))
        parent = [r for r in routes if r.startswith("parent")][0]
        scale = float(out[parent].abs().max())
        res = {}
        for route in routes:
            base_route = BASE.get(route, parent)
            res[route] = dict(ms=statistics.median(ms[route]), ms_min_max=[min(ms[route]), max(ms[route])],
                              peak_bytes=peak[route], against=base_route,
                              parent_over_this=statistics.median(ms[base_route]) / statistics.median(ms[route]),
                              max_abs_diff_over_max=float((out[route] - out[base_route]).abs().max()) / scale)
        row[method] = res
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("configs", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_mt_narrow_pred: no GPU; nothing is measured without one")
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
