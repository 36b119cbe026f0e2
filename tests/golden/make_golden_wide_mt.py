"""Golden vectors for MULTITASK and DERIVATIVE-INFORMED fast GPs on wide inputs (9 <= d <= 64), from the REAL
reference, into tests/golden/wide_mt/*.npz (a subdirectory: tests.golden_util.golden_names() globs tests/golden/*.npz
only, so the existing parametrised tests keep their cases).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_mt.py [fixture names...]

Same import route as make_golden_multitask.py (oracle/refshim).  Point sets are those of make_golden_wide.py
(lattice_z / net_matrices), one shift per task, stored in the fixture.  The keys are make_golden_multitask.gen_case's
(pair parts and lam, ytilde, inv, logdet, loss and gradients, coeffs, every posterior, the n_new projections and a
3-iteration fit trajectory) with the derivative multi-indices and their coefficients stored per task
(derivatives_<l> [p_l, d], derivatives_coeffs_<l> [p_l]) and the `lengthscales` the GP was built with: at the default
lengthscale 1 the d = 12 posterior variances are of order 1e4, which pins nothing, so the fixtures start from
make_golden_wide.lengthscales_for's small, pairwise different values.

Cases:
  mt_lattice_d12_a2_T3       lattice alpha = 2, T = 3 tasks, n = [64, 8, 256], learned rank-1 task kernel
  deriv_lattice_d12_a2       lattice alpha = 2, (f, df/dx0, df/dx11), n = [64, 8, 256]
  deriv_net_d12_a4           net alpha = 4, (f, df/dx0, df/dx11), n = [128, 128, 128]
  mt_net_d9_a2_T2_b2         net alpha = 2, T = 2, n = [32, 128], shape_batch = [2]
  deriv_lattice_d17_a3_c2    lattice alpha = 3, d = 17, n = [64, 64]: task 0 = f, task 1 = 0.5 df/dx0 - 1.5 d2f/dx3 dx16
                             (two multi-indices, non-unit derivatives_coeffs)
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
from make_golden import _np, f_ackley  # noqa: E402
from make_golden_wide import lattice_z, lengthscales_for, net_matrices  # noqa: E402

OUT = os.path.join(HERE, "wide_mt")


def _e(d, *js):
    v = torch.zeros(d, dtype=torch.int64)
    for j in js:
        v[j] += 1
    return v


def _smooth(x):
    return torch.exp(-((x - 0.3) ** 2).mean(1)) + torch.sin(3 * x).mean(1)


def _deriv_of(f, x, beta):
    """sum-free mixed partial derivative of f at the rows of x, by autograd (beta: multi-index of orders 0 / 1)."""
    x = x.clone().requires_grad_()
    y = f(x)
    for j in [int(j) for j in torch.nonzero(beta).reshape(-1)]:
        y = torch.autograd.grad(y.sum(), x, create_graph=True)[0][:, j]
    return y.detach()


def _cases():
    d12 = [_e(12)[None], _e(12, 0)[None], _e(12, 11)[None]]
    return [
        # name, family, d, alpha, ns, B, derivatives, derivatives_coeffs
        ("mt_lattice_d12_a2_T3", "lattice", 12, 2, [64, 8, 256], 0, None, None),
        ("deriv_lattice_d12_a2", "lattice", 12, 2, [64, 8, 256], 0, d12, None),
        ("deriv_net_d12_a4", "net", 12, 4, [128, 128, 128], 0, d12, None),
        ("mt_net_d9_a2_T2_b2", "net", 9, 2, [32, 128], 2, None, None),
        ("deriv_lattice_d17_a3_c2", "lattice", 17, 3, [64, 64], 0,
         [_e(17)[None], torch.stack([_e(17, 0), _e(17, 3, 16)])], [torch.ones(1), torch.tensor([0.5, -1.5])]),
    ]


def gen_case(fg, qmcpy, family, d, alpha, ns, B, derivs, dcoeffs, seed=11, fit_its=3):
    T = len(ns)
    ls = lengthscales_for(d, 0, False)
    out = {"family": np.array(family), "kind": np.array("deriv" if derivs is not None else "multitask"),
           "d": np.array(d), "alpha": np.array(alpha), "ns": np.array(ns, dtype=np.int64), "B": np.array(B),
           "lengthscales": _np(ls)}
    kw = dict(alpha=alpha, num_tasks=T, shape_batch=[B] if B > 0 else [], lengthscales=ls.clone())
    if derivs is not None:
        kw["derivatives"] = [v.clone() for v in derivs]
        if dcoeffs is not None:
            kw["derivatives_coeffs"] = [c.clone() for c in dcoeffs]
        for l in range(T):
            out["derivatives_%d" % l] = _np(derivs[l])
            out["derivatives_coeffs_%d" % l] = _np(dcoeffs[l] if dcoeffs is not None else torch.ones(len(derivs[l])))
    seqs = []
    if family == "lattice":
        z = lattice_z(d)
        shifts = np.stack([np.random.default_rng(seed + l).uniform(size=d) for l in range(T)])
        for l in range(T):
            seqs.append(qmcpy.Lattice(d, randomize="SHIFT", generating_vector=z, shift=shifts[l]))
        out["z"] = np.array(z, dtype=np.int64)
        out["shifts"] = shifts
        fgp = fg.FastGPLattice(seqs, **kw)
    else:
        t = 32
        C = net_matrices(d, t=t)
        shifts = np.stack([np.random.default_rng(seed + l).integers(0, 2 ** t, size=d, dtype=np.uint64) for l in range(T)])
        for l in range(T):
            seqs.append(qmcpy.DigitalNetB2(d, randomize="DS", generating_matrices=C, t=t, shift=shifts[l]))
        out["C"] = C.astype(np.int64)
        out["t"] = np.array(t)
        out["shifts"] = shifts.astype(np.int64)
        fgp = fg.FastGPDigitalNetB2(seqs, **kw)
    xs = fgp.get_x_next(n=list(ns))
    ys = []
    for l in range(T):
        if derivs is not None:
            c = dcoeffs[l] if dcoeffs is not None else torch.ones(len(derivs[l]))
            y = sum(float(c[p]) * _deriv_of(_smooth, xs[l], derivs[l][p]) for p in range(len(derivs[l])))
        else:
            y = [f_ackley(xs[l], c=0), f_ackley(xs[l]), torch.cos(2 * np.pi * xs[l]).sum(1)][l]
        if B > 0:
            y = torch.stack([y * (1 + 0.1 * b) + 0.01 * b for b in range(B)], 0)
        ys.append(y)
    fgp.add_y_next(ys)
    for l in range(T):
        out["x_%d" % l] = _np(xs[l])
        out["xb_%d" % l] = _np(fgp.get_xb(l))
        out["y_%d" % l] = _np(ys[l])
    for l0 in range(T):
        for l1 in range(l0, T):
            out["k1parts_%d%d" % (l0, l1)] = _np(fgp.get_k1parts(l0, l1, n=max(ns[l0], ns[l1])))
            out["lam_%d%d" % (l0, l1)] = _np(fgp.get_lam(l0, l1, n=max(ns[l0], ns[l1])))
        out["ytilde_%d" % l0] = _np(fgp.get_ytilde(l0))
    out["gram_matrix_tasks"] = _np(fgp.gram_matrix_tasks)
    named = (("raw_scale", fgp.raw_scale), ("raw_lengthscales", fgp.raw_lengthscales), ("raw_noise", fgp.raw_noise),
             ("raw_factor_task_kernel", fgp.raw_factor_task_kernel), ("raw_noise_task_kernel", fgp.raw_noise_task_kernel))
    names = [nm for nm, p in named if p.requires_grad]
    params = [p for nm, p in named if p.requires_grad]
    out["grad_names"] = np.array(names)
    os.environ["FASTGP_FORCE_RECOMPILE"] = "True"
    cache = fgp.get_inv_log_det_cache()
    inv, _ = cache()
    out["inv"] = _np(inv)
    norm_term, logdet = cache.get_norm_term_logdet_term()
    d_out = int(torch.tensor(fgp.shape_batch).prod())
    mll_const = d_out * fgp.n.sum() * np.log(2 * np.pi)
    loss = 0.5 * (norm_term.sum() + d_out / torch.tensor(logdet.shape).prod() * logdet.sum() + mll_const)
    grads = torch.autograd.grad(loss, params)
    del os.environ["FASTGP_FORCE_RECOMPILE"]
    out["norm_term"] = _np(norm_term)
    out["logdet"] = _np(logdet)
    out["loss"] = _np(loss)
    for nm, g in zip(names, grads):
        out["grad_" + nm] = _np(g)
    xt = torch.rand((12, d), generator=torch.Generator().manual_seed(17))
    out["x_test"] = _np(xt)
    out["coeffs"] = _np(fgp.coeffs)
    out["pmean"] = _np(fgp.post_mean(xt))
    out["pvar"] = _np(fgp.post_var(xt))
    out["pcov"] = _np(fgp.post_cov(xt[:4], xt[4:9]))
    out["pcmean"] = _np(fgp.post_cubature_mean())
    out["pcvar"] = _np(fgp.post_cubature_var())
    out["pccov"] = _np(fgp.post_cubature_cov())
    n_new = fgp.n * torch.tensor([4, 2, 8][:T])
    out["n_new"] = _np(n_new)
    out["pvar_new"] = _np(fgp.post_var(xt, n=n_new))
    out["pcvar_new"] = _np(fgp.post_cubature_var(n=n_new))
    data = fgp.fit(iterations=fit_its, store_hists=True, verbose=0, stop_crit_wait_iterations=fit_its + 5)
    out["fit_iterations"] = np.array(data["iterations"])
    for k in ("loss_hist", "scale_hist", "lengthscales_hist", "task_kernel_hist"):
        out["fit_" + k] = _np(data[k])
    out["fit_pmean"] = _np(fgp.post_mean(xt))
    out["fit_pvar"] = _np(fgp.post_var(xt))
    return out


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for name, family, d, alpha, ns, B, derivs, dcoeffs in _cases():
        if only and name not in only:
            continue
        out = gen_case(fg, qmcpy, family, d, alpha, ns, B, derivs, dcoeffs)
        fn = os.path.join(OUT, name + ".npz")
        np.savez_compressed(fn, **out)
        print("wrote %s (%d KB) loss=%.10e  max pvar=%.3g  fit loss %s" % (
            name, os.path.getsize(fn) // 1024, float(out["loss"]), float(np.max(np.abs(out["pvar"]))),
            out["fit_loss_hist"].reshape(-1)[:4]))


if __name__ == "__main__":
    main()
