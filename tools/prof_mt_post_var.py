"""ms per post_var call (64 test points) of a multitask / derivative-informed GP: the transform-domain quadratic form
(fgp_mt_quadform, FGP_MT_POST_VAR_QF=1) against the kernel rows and the transform solve (FGP_MT_POST_VAR_QF=0), in one
process, with the peak device memory of each route.

    python tools/prof_mt_post_var.py [--calls K] [--rounds R] [--points N] [--out FILE.json] [config names...]

Each round times K calls of one route and K of the other, alternating, each window ending in a device synchronise; the
figure is the median over the rounds with the minimum and maximum beside it.  One untimed round warms up every shape.
The factor is cached before the first window (both routes share it).  Peak memory: torch.cuda.max_memory_allocated over
one call of the route, above what is allocated before it.  The largest difference of the two routes' results is
reported relative to 10 max(1, max post_var), the scale of the tests' 1e-8 tolerance.  Needs a GPU: no CPU fallback.

Configurations (lattice, alpha = 2):
  mt_T3_d3_n65536      T = 3 tasks, n = 2^16 each, d = 3
  mt_T3_d16_n65536     the same, d = 16
  mt_T3_d64_n65536     the same, d = 64
  deriv_T5_d16_n16384  f and four first partial derivatives, n = 2^14 each, d = 16
  mt_T2_d12_n4096      T = 2, n = 2^12 each, d = 12: the default routing threshold (sum n = 2^13)
  mt_T2_d12_n2048      T = 2, n = 2^11 each: below the threshold
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
CONFIGS = {"mt_T3_d3_n65536": (3, 3, 1 << 16, False), "mt_T3_d16_n65536": (16, 3, 1 << 16, False),
           "mt_T3_d64_n65536": (64, 3, 1 << 16, False), "deriv_T5_d16_n16384": (16, 5, 1 << 14, True),
           "mt_T2_d12_n4096": (12, 2, 1 << 12, False), "mt_T2_d12_n2048": (12, 2, 1 << 11, False)}


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def make_gp(name):
    d, T, n, deriv = CONFIGS[name]
    seqs = [F.Lattice(d, seed=3 + l) for l in range(T)]
    kw = dict(num_tasks=T, alpha=2, device=DEV, lengthscales=0.05 if d > 8 else 0.5)
    if deriv:
        kw["derivatives"] = [torch.zeros((1, d), dtype=torch.int64)] + \
            [torch.eye(d, dtype=torch.int64)[j:j + 1] for j in range(T - 1)]
    gp = F.FastGPLattice(seqs, **kw)
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


def measure(name, calls, rounds, points):
    gp = make_gp(name)
    xd = torch.rand((points, gp.d), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        gp._factor(list(gp._ns))
    out, peak, ms = {}, {}, {"1": [], "0": []}

    def run(env, k):
        os.environ["FGP_MT_POST_VAR_QF"] = env
        for _ in range(k):
            out[env] = gp.post_var(xd)

    for env in ("1", "0"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(env, 1)
        torch.cuda.synchronize()
        peak[env] = torch.cuda.max_memory_allocated() - base
    for r in range(rounds + 1):                             # round 0: warm-up of every shape of the timed windows
        for env in (("1", "0") if r % 2 else ("0", "1")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(env, calls)
            torch.cuda.synchronize()
            if r > 0:
                ms[env].append((time.perf_counter() - t0) * 1e3 / calls)
    os.environ.pop("FGP_MT_POST_VAR_QF", None)
    scale = 10 * max(1.0, float(out["0"].max()))
    qf, rs = statistics.median(ms["1"]), statistics.median(ms["0"])
    return dict(config=name, d=gp.d, ns=list(gp._ns), points=points, calls=calls, rounds=rounds,
                form_ms=qf, form_ms_min_max=[min(ms["1"]), max(ms["1"])],
                rows_solve_ms=rs, rows_solve_ms_min_max=[min(ms["0"]), max(ms["0"])],
                ratio_rows_solve_over_form=rs / qf,
                form_peak_bytes=peak["1"], rows_solve_peak_bytes=peak["0"],
                max_abs_diff_over_10kxx=float((out["1"] - out["0"]).abs().max()) / scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("configs", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_mt_post_var: no GPU; nothing is measured without one")
    torch.set_default_dtype(torch.float64)
    rows = []
    for name in a.configs:
        rows.append(measure(name, a.calls, a.rounds, a.points))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
