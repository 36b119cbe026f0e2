"""Golden vectors for PARAMETER-BATCHED multitask GPs on wide inputs (9 <= d <= 64), from the REAL reference, into
tests/golden/wide_batch_mt/*.npz: the shapes of docs/examples/batch_multitask/fgp_lattice.ipynb cell 6 (scale
shape_batch + [1], lengthscales shape_batch[1:] + [d], noise shape_batch[2:] + [1], task factor shape_batch + [T, T], task
noise shape_batch[1:] + [T]) at shape_batch = [2, 3], T = 3 tasks with n = [64, 32, 16], alpha = 2: a lattice at d = 12
and a digital net at d = 9.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_batch_mt.py

Modelled on make_golden_batch_mt.py (same import route, oracle/refshim; the notebook's data function), with the point
sets of make_golden_wide.py (lattice_z / net_matrices), one shift per task.  At the default lengthscale 1 a d = 12 kernel
pins nothing, so the raw parameters start from make_golden_wide.lengthscales_for's small lengthscales, every row of every
block perturbed differently (a shared row and a per-output row must not be confusable).  Stored: the inputs, the initial
raw parameters, the reference's MLL and gradient there, fit(iterations=4) (early stopping off) loss history and every
fitted raw parameter, and post_mean at 12 test points after the fit.

Rprop follows the gradient's signs: an element whose initial gradient is tiny against the largest could flip its first
step under a rounding difference, so the generator refuses a seed for which any element is below 1e-5 of the largest.
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
from make_golden import _np  # noqa: E402
from make_golden_wide import lattice_z, lengthscales_for, net_matrices  # noqa: E402

OUT = os.path.join(HERE, "wide_batch_mt")
ITS = 4
SHAPE_BATCH = [2, 3]
T = 3
NS = [64, 32, 16]
CASES = [("lattice", 12, 2), ("net", 9, 2)]
PNAMES = ("raw_scale", "raw_lengthscales", "raw_noise", "raw_factor_task_kernel", "raw_noise_task_kernel")


def data_fn(d, rng):
    """The notebook's f(l, x) (cell 4)."""
    def f(l, x):
        consts = torch.arange(int(np.prod(SHAPE_BATCH))).reshape(SHAPE_BATCH).to(torch.float64)
        return (consts[..., None, None] * x ** torch.arange(1, d + 1)).sum(-1) + \
            torch.randn(SHAPE_BATCH + [x.size(0)], generator=rng) / (3 + l)
    return f


def gen(fg, qmcpy, family, d, alpha, seed=7):
    sb = SHAPE_BATCH
    out = {"family": np.array(family), "d": np.array(d), "alpha": np.array(alpha), "T": np.array(T),
           "shape_batch": np.array(sb)}
    kw = dict(alpha=alpha, num_tasks=T, shape_batch=sb, shape_scale=sb + [1], shape_lengthscales=sb[1:] + [d],
              shape_noise=sb[2:] + [1], shape_factor_task_kernel=sb + [T, T], shape_noise_task_kernel=sb[1:] + [T])
    if family == "lattice":
        z = lattice_z(d)
        shifts = np.stack([np.random.default_rng(seed + l).uniform(size=d) for l in range(T)])
        seqs = [qmcpy.Lattice(d, randomize="SHIFT", generating_vector=z, shift=shifts[l]) for l in range(T)]
        out["z"] = np.array(z, dtype=np.int64)
        out["shifts"] = shifts
        gp = fg.FastGPLattice(seqs, **kw)
    else:
        t = 32
        C = net_matrices(d, t=t)
        shifts = np.stack([np.random.default_rng(seed + l).integers(0, 2 ** t, size=d, dtype=np.uint64) for l in range(T)])
        seqs = [qmcpy.DigitalNetB2(d, randomize="DS", generating_matrices=C, t=t, shift=shifts[l]) for l in range(T)]
        out["C"] = C.astype(np.int64)
        out["t"] = np.array(t)
        out["shifts"] = shifts.astype(np.int64)
        gp = fg.FastGPDigitalNetB2(seqs, **kw)
    # the initial raw parameters: small lengthscales, every row of every block its own perturbation
    rng = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        gp.raw_lengthscales.copy_(torch.log(lengthscales_for(d, 0, False)).expand_as(gp.raw_lengthscales))
        for nm in PNAMES:
            p = getattr(gp, nm)
            p.add_(0.2 * (torch.rand(p.shape, generator=rng) - 0.5))
    for nm in PNAMES:
        out["init_" + nm] = _np(getattr(gp, nm)).copy()     # the fit steps the parameters in place
    out["ns"] = np.array(NS, dtype=np.int64)
    xs = gp.get_x_next(n=torch.tensor(NS))
    f = data_fn(d, torch.Generator().manual_seed(seed))
    ys = [f(l, xs[l]) for l in range(T)]
    gp.add_y_next(ys)
    for l in range(T):
        out["x_%d" % l] = _np(xs[l])
        out["y_%d" % l] = _np(ys[l])
    # MLL and its gradient at the initial parameters (abstract_gp.py:235,253-260,294)
    os.environ["FASTGP_FORCE_RECOMPILE"] = "True"
    cache = gp.get_inv_log_det_cache()
    norm_term, logdet = cache.get_norm_term_logdet_term()
    d_out = int(np.prod(sb))
    loss = 0.5 * (norm_term.sum() + d_out / torch.tensor(logdet.shape).prod() * logdet.sum() +
                  d_out * gp.n.sum() * np.log(2 * np.pi))
    names = [nm for nm in PNAMES if getattr(gp, nm).requires_grad]
    grads = torch.autograd.grad(loss, [getattr(gp, nm) for nm in names])
    del os.environ["FASTGP_FORCE_RECOMPILE"]
    gmax = max(float(g.abs().max()) for g in grads)
    gmin = min(float(g.abs().min()) for g in grads)
    assert gmin >= 1e-5 * gmax, ("an initial gradient element is below 1e-5 of the largest: take another seed", gmin, gmax)
    out["loss"] = _np(loss)
    out["grad_names"] = np.array(names)
    for nm, g in zip(names, grads):
        out["grad_" + nm] = _np(g)
    data = gp.fit(iterations=ITS, store_hists=True, verbose=0, stop_crit_wait_iterations=ITS + 5)
    out["fit_loss_hist"] = _np(data["loss_hist"])
    for nm in PNAMES:
        out["fit_" + nm] = _np(getattr(gp, nm)).copy()
    xt = torch.rand((12, d), generator=torch.Generator().manual_seed(17))
    out["x_test"] = _np(xt)
    out["fit_pmean"] = _np(gp.post_mean(xt))
    return out


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    for family, d, alpha in CASES:
        name = "%s_d%d_a%d_T%d_b%s" % (family, d, alpha, T, "x".join(str(v) for v in SHAPE_BATCH))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **gen(fg, qmcpy, family, d, alpha))
        print("wrote", name)


if __name__ == "__main__":
    main()
