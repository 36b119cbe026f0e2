"""ms per fit iteration of a PARAMETER-BATCHED multitask GP on wide inputs: the device-resident loop over G problems
(fgp_wide_mt_fit_batch_run, FGP_WIDE_MT_FIT_BATCH=1) against the generic autograd loop (the default
path), in one process.

    python tools/prof_wide_mt_fit_batch.py [--iters K] [--rounds R] [--out FILE.json] [config names...]

The method of tools/prof_wide_mt_fit.py: each round times K iterations of the device loop and K of the generic loop,
alternating, each window ending in a device synchronise; the figure is the median over the rounds (min and max beside
it); one untimed round warms up every shape.  Peak device memory (torch's allocator, which holds every buffer of either
loop) is recorded per loop over its timed windows, the GP's own caches included.  The device loop's entry-point calls per
iteration are 3 T (T + 1) / 2 + 2 T + 8 by construction, whatever G; the generic loop's are the native entry points
Python calls per iteration (a spy on _native.call in a separate untimed iteration; its torch glue kernels come on top).
Needs a GPU: there is no CPU fallback.

Configurations (bmt_d<d>_n<n>): lattice, alpha = 2, T = 3 tasks of n points each, shape_batch = [2, 3, 4] (G = 24) with the
staggered parameter shapes of docs/examples/batch_multitask (scale and task factor over [2, 3, 4], lengthscales and task
noise over [3, 4], noise over [4]).
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
SHAPE_BATCH = [2, 3, 4]
T = 3


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def make_gp(name):
    d = int(name.split("_d")[1].split("_")[0])
    n = int(name.rsplit("_n", 1)[1])
    sb = SHAPE_BATCH
    seqs = [F.Lattice(d, seed=3 + l) for l in range(T)]
    gp = F.FastGPLattice(seqs, num_tasks=T, alpha=2, device=DEV, lengthscales=0.05, shape_batch=sb, shape_scale=sb + [1],
                         shape_lengthscales=sb[1:] + [d], shape_noise=sb[2:] + [1], shape_factor_task_kernel=sb + [T, T],
                         shape_noise_task_kernel=sb[1:] + [T])
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in gp.parameters():
            p.add_((0.1 * (torch.rand(p.shape, generator=gen) - 0.5)).to(DEV))
    xs = gp.get_x_next(n=[n] * T)
    amp = (1 + 0.05 * torch.arange(24, device=DEV, dtype=torch.float64)).reshape(sb + [1])
    gp.add_y_next([amp * (_smooth(x) * (1 + 0.2 * l) + 0.1 * l) for l, x in enumerate(xs)])
    return gp


def generic_iteration(gp, opt, d_out):
    gp._cache = {k: v for k, v in gp._cache.items() if not k[2]}
    loss = gp._loss_generic("MLL", None, 1, d_out)[0]
    lv = loss.item()
    loss.backward()
    opt.step()
    opt.zero_grad()
    return lv


def window(fn, k):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k, torch.cuda.max_memory_allocated()


def measure(name, iters, rounds):
    os.environ["FGP_WIDE_MT_FIT_BATCH"] = "1"
    gp_dev, gp_gen = make_gp(name), make_gp(name)
    assert gp_dev._mt_wide_batch_ok() and gp_dev._device_fit_args("MLL", None, None, 1) is not None, name
    eng = gp_dev._fused_engine(iters, 0.1)
    assert type(eng).__name__ == "WideMtEngine" and eng.G == 24
    d_out = 24
    opt = gp_gen.get_default_optimizer(None)
    raw0 = eng.raw.clone()
    par0 = [p.detach().clone() for p in gp_gen.parameters()]
    spy, real = [], N.call
    N.call = lambda nm, *a: (spy.append(nm), real(nm, *a))[1]
    try:
        generic_iteration(gp_gen, opt, d_out)               # (also the generic loop's first warm-up iteration)
    finally:
        N.call = real

    def dev_k(k):
        eng.run(0, k)

    def gen_k(k):
        o = gp_gen.get_default_optimizer(None)
        for _ in range(k):
            generic_iteration(gp_gen, o, d_out)

    def reset():
        """Every window starts from the initial parameters (both loops then walk the same trajectory)."""
        eng.raw.copy_(raw0)
        with torch.no_grad():
            for p, v in zip(gp_gen.parameters(), par0):
                p.copy_(v)

    dev, gen, pd, pg = [], [], 0, 0
    for r in range(rounds + 1):                             # round 0: warm-up of every shape of the timed windows
        reset()
        td, md = window(dev_k, iters)
        tg, mg = window(gen_k, iters)
        if r > 0:
            dev.append(td)
            gen.append(tg)
            pd, pg = max(pd, md), max(pg, mg)
    Tn = eng.lo.T
    return dict(config=name, metric="MLL", d=gp_dev.d, ns=list(gp_dev._ns), shape_batch=SHAPE_BATCH, G=eng.G,
                n_params=eng.n_params, iters=iters, rounds=rounds,
                device_ms_per_iter=statistics.median(dev), device_ms_min_max=[min(dev), max(dev)],
                generic_ms_per_iter=statistics.median(gen), generic_ms_min_max=[min(gen), max(gen)],
                ratio_generic_over_device=statistics.median(gen) / statistics.median(dev),
                device_entry_point_calls_per_iter=3 * (Tn * (Tn + 1) // 2) + 2 * Tn + 8,
                generic_native_calls_per_iter=len(spy),
                device_peak_bytes=pd, generic_peak_bytes=pg, device_work_bytes=int(eng.work.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("configs", nargs="*", default=["bmt_d16_n4096", "bmt_d64_n4096", "bmt_d16_n65536", "bmt_d64_n65536"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_wide_mt_fit_batch: no GPU; nothing is measured without one")
    torch.set_default_dtype(torch.float64)
    rows = []
    for name in a.configs:
        rows.append(measure(name, a.iters, a.rounds))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
