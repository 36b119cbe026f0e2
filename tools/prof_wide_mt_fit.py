"""ms per fit iteration of a multitask / derivative-informed GP on wide inputs: the device-resident loop
(fgp_wide_mt_fit_run, FGP_WIDE_FIT_DEVICE=1) against the generic autograd loop (the default path), in one process.

    python tools/prof_wide_mt_fit.py [--metric MLL|GCV|CV] [--iters K] [--rounds R] [--out FILE.json] [config names...]

Each round times K iterations of the device loop and K of the generic loop, alternating, each window ending in a device
synchronise; the figure is the median over the rounds (the spread is printed beside it).  One untimed round warms up
every shape.  The generic iteration is AbstractFastGP._fit_generic's body (caches dropped, _loss_generic, the loss read
back for the stopping rule, backward, torch.optim.Rprop.step).  Launch counts: the device loop's entry-point calls per
iteration are 3 T (T + 1) / 2 + 2 T + 7 by construction (one more under GCV / CV); the generic loop's are the native
entry points Python calls per iteration (counted by a spy on _native.call in a separate untimed iteration) -- its torch
glue kernels come on top and are not counted.  Needs a GPU: there is no CPU fallback.

--metric GCV / CV times fit(loss_metric=...) (CV with the scalar weight 0.75).  The generic CV loss of several tasks
solves the identity of size sum(n) (util.py:387-393): (sum n)^2 complex128 values per temporary.  Where eight of them do
not fit the device's free memory the generic loop is not attempted and the row says so (generic_ms_per_iter = null,
generic_skipped = the reason); the device loop is measured all the same.

Configurations (mt_T<T>_d<d>_n<n>: any power-of-two n):
  mt_T3_d16_n65536     lattice, T = 3 tasks, n = 2^16 each, d = 16
  mt_T3_d64_n65536     the same, d = 64
  mt_T3_d16_n4096      T = 3, n = 2^12, d = 16: the largest of these at which the generic CV loop runs
  deriv_T5_d16_n16384  lattice, f and four first partial derivatives, n = 2^14 each, d = 16
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
from fastgaussianprocesses_amd import _native as N  # noqa: E402

DEV = "cuda"


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def make_gp(name):
    if name.startswith("mt_T3"):
        d = 64 if "d64" in name else 16
        T, n = 3, int(name.rsplit("_n", 1)[1])
        seqs = [F.Lattice(d, seed=3 + l) for l in range(T)]
        gp = F.FastGPLattice(seqs, num_tasks=T, alpha=2, device=DEV, lengthscales=0.05)
        xs = gp.get_x_next(n=[n] * T)
        gp.add_y_next([_smooth(x) * (1 + 0.2 * l) + 0.1 * l for l, x in enumerate(xs)])
        return gp
    d, T, n = 16, 5, 1 << 14
    derivs = [torch.zeros((1, d), dtype=torch.int64)] + [torch.eye(d, dtype=torch.int64)[j:j + 1] for j in range(4)]
    seqs = [F.Lattice(d, seed=3 + l) for l in range(T)]
    gp = F.FastGPLattice(seqs, num_tasks=T, alpha=2, device=DEV, lengthscales=0.05, derivatives=derivs)
    xs = gp.get_x_next(n=[n] * T)
    ys = []
    for l, x in enumerate(xs):
        x = x.clone().requires_grad_()
        y = _smooth(x)
        if l > 0:
            y = torch.autograd.grad(y.sum(), x)[0][:, l - 1]
        ys.append(y.detach())
    gp.add_y_next(ys)
    return gp


CV_WEIGHT = 0.75


def generic_iteration(gp, opt, metric="MLL"):
    gp._cache = {k: v for k, v in gp._cache.items() if not k[2]}
    loss = gp._loss_generic(metric, None, CV_WEIGHT if metric == "CV" else 1, 1)[0]
    lv = loss.item()
    loss.backward()
    opt.step()
    opt.zero_grad()
    return lv


def window(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k


def generic_skipped(gp, metric):
    """Why the generic loop is not attempted, or None."""
    if metric != "CV" or gp.num_tasks == 1:
        return None
    need = 8 * 16 * sum(gp._ns) ** 2
    free = torch.cuda.mem_get_info()[0]
    if need > free:
        return "the generic CV loss solves the identity of size sum(n) = %d: about %.0f GB, %.0f GB free" % (
            sum(gp._ns), need / 1e9, free / 1e9)
    return None


def measure(name, iters, rounds, metric="MLL"):
    os.environ["FGP_WIDE_FIT_DEVICE"] = "1"
    gp_dev, gp_gen = make_gp(name), make_gp(name)
    assert gp_dev._mt_wide_ok(), name
    if metric == "MLL":
        eng = gp_dev._fused_engine(iters, 0.1)
    else:
        assert gp_dev._device_fit_args(metric, None, None, CV_WEIGHT) is not None, (name, metric)
        eng = gp_dev._fused_engine(iters, 0.1, loss_metric=metric, cv_weight=CV_WEIGHT)
    assert type(eng).__name__ == "WideMtEngine"
    skipped = generic_skipped(gp_gen, metric)
    opt = gp_gen.get_default_optimizer(None)
    T = eng.lo.T
    raw0 = eng.raw.clone()
    par0 = [p.detach().clone() for p in gp_gen.parameters()]
    spy, real = [], N.call
    N.call = lambda nm, *a: (spy.append(nm), real(nm, *a))[1]
    try:
        if skipped is None:
            generic_iteration(gp_gen, opt, metric)          # (also the generic loop's first warm-up iteration)
    finally:
        N.call = real

    def dev_k(k):
        eng.run(0, k)

    def gen_k(k):
        o = gp_gen.get_default_optimizer(None)
        for _ in range(k):
            generic_iteration(gp_gen, o, metric)

    def reset():
        """Every window starts from the initial parameters (both loops then walk the same trajectory)."""
        eng.raw.copy_(raw0)
        with torch.no_grad():
            for p, v in zip(gp_gen.parameters(), par0):
                p.copy_(v)

    dev, gen = [], []
    for r in range(rounds + 1):                             # round 0: warm-up of every shape of the timed windows
        reset()
        td = window(dev_k, iters)
        tg = window(gen_k, iters) if skipped is None else None
        if r > 0:
            dev.append(td)
            gen.append(tg)
    row = dict(config=name, metric=metric, d=gp_dev.d, ns=list(gp_dev._ns), iters=iters, rounds=rounds,
               device_ms_per_iter=statistics.median(dev), device_ms_min_max=[min(dev), max(dev)],
               device_entry_point_calls_per_iter=3 * (T * (T + 1) // 2) + 2 * T + 7 + (metric != "MLL"))
    if skipped is None:
        row.update(generic_ms_per_iter=statistics.median(gen), generic_ms_min_max=[min(gen), max(gen)],
                   ratio_generic_over_device=statistics.median(gen) / statistics.median(dev),
                   generic_native_calls_per_iter=len(spy))
    else:
        row.update(generic_ms_per_iter=None, generic_skipped=skipped)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--metric", default="MLL", choices=["MLL", "GCV", "CV"])
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    ap.add_argument("configs", nargs="*", default=["mt_T3_d16_n65536", "mt_T3_d64_n65536", "deriv_T5_d16_n16384"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_wide_mt_fit: no GPU; nothing is measured without one")
    torch.set_default_dtype(torch.float64)
    rows = []
    if a.append and a.out and os.path.isfile(a.out):
        with open(a.out) as f:
            rows = json.load(f)
    for name in a.configs:
        rows.append(measure(name, a.iters, a.rounds, a.metric))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
