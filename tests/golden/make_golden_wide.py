"""Golden vectors for wide inputs (9 <= d <= 64 dimensions) from the REAL reference, into tests/golden/wide/*.npz
(a subdirectory: tests.golden_util.golden_names() globs tests/golden/*.npz only, so the existing parametrised
tests keep their cases).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py [fixture names...]

Each fixture holds the keys of make_golden.gen_case plus the `lengthscales` the GP was built with.  Point sets are
explicit:
  lattices  DEFAULT_LATTICE_Z extended by the rule of seqs.Lattice.__init__ (z.append((z[-1] * 182667) % 2**20 | 1));
  nets      unit-upper-triangular generating matrices, t = 32: column k has bit t-1-k set plus seeded random bits in
            the more significant positions (any such matrices keep the Gram matrix dyadic; the built-in Sobol' table
            ends at d = 8); C is stored.
With the default lengthscale 1 the kernel's diagonal is prod_j (1 + 2.16 l_j), ~1e6 at d = 12, so the fixtures use
small, pairwise different lengthscales (a swapped or dropped dimension shows): linspace(0.05, 0.3, d), and
linspace(0.01, 0.05, d) at d = 64.

Walsh alpha = 2 (net_m7_d13_a2) runs the reference's pipeline over the stand-in's restated weighted_walsh_funcs: parity
is unpinned at the qmcpy boundary there, as for every net fixture of order 2-4.

Beyond gen_case's keys:
  net_m8_d12_a1_b0      gcv_* / cv_*: fit(loss_metric="GCV" / "CV"), 4 iterations (as make_golden_losses.py; the
                        reference's lattice GCV / CV raise, see there)
  lattice_m8_d12_a2_b0  adam_*: fit(optimizer=torch.optim.Adam(lr=0.05), iterations=3)
  *_b3*                 mask_*: fit(masks=[[0, 2]], iterations=3)
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
from make_golden import LATTICE_Z, _np, make_y  # noqa: E402

OUT = os.path.join(HERE, "wide")
ALT_ITS = 4

CASES = [
    # family, m, d, alpha, B, per_output
    ("lattice", 8, 12, 2, 0, False),
    ("lattice", 6, 9, 3, 0, False),
    ("lattice", 7, 64, 2, 0, False),
    ("lattice", 8, 12, 2, 3, True),
    ("net", 8, 12, 1, 0, False),
    ("net", 7, 13, 2, 0, False),        # Walsh order 2: parity unpinned at the qmcpy boundary
    ("net", 6, 64, 1, 0, False),
    ("net", 8, 12, 1, 3, False),
]


def case_name(c):
    family, m, d, alpha, B, po = c
    return "%s_m%d_d%d_a%d_b%d%s" % (family, m, d, alpha, B, "_po" if po else "")


def lattice_z(d):
    z = list(LATTICE_Z)
    while len(z) < d:
        z.append(int((z[-1] * 182667) % (1 << 20)) | 1)
    return z[:d]


def net_matrices(d, t=32, mcols=32):
    rng = np.random.default_rng(1000 + d)
    C = np.zeros((d, mcols), dtype=np.uint64)
    for j in range(d):
        for k in range(mcols):
            hi = int(rng.integers(0, 1 << k)) if k > 0 else 0       # k random bits above the diagonal one
            C[j, k] = np.uint64((1 << (t - 1 - k)) | (hi << (t - k)))
    return C


def lengthscales_for(d, B, po):
    ls = torch.linspace(0.01, 0.05, d) if d == 64 else torch.linspace(0.05, 0.3, d)
    if po:
        return torch.stack([ls, ls.flip(0), ls / 2])[:B]
    return ls


def build(fg, qmcpy, c, out=None, seed=7):
    """A fresh reference GP of case c with its data; fills the inputs into `out`."""
    family, m, d, alpha, B, po = c
    n = 2 ** m
    ls = lengthscales_for(d, B, po)
    kw = dict(alpha=alpha, shape_batch=[B] if B > 0 else [], lengthscales=ls.clone())
    if po:
        kw["shape_scale"] = [B, 1]
    if family == "lattice":
        z = lattice_z(d)
        shift = np.random.default_rng(seed).uniform(size=d)
        seq = qmcpy.Lattice(d, randomize="SHIFT", generating_vector=z, shift=shift)
        gp = fg.FastGPLattice(seq, **kw)
        pts = {"z": np.array(z, dtype=np.int64), "shift": shift}
    else:
        t = 32
        C = net_matrices(d, t=t)
        shift = np.random.default_rng(seed).integers(0, 2 ** t, size=d, dtype=np.uint64)
        seq = qmcpy.DigitalNetB2(d, randomize="DS", generating_matrices=C, t=t, shift=shift)
        gp = fg.FastGPDigitalNetB2(seq, **kw)
        pts = {"C": C.astype(np.int64), "t": np.array(t), "shift": shift.astype(np.int64)}
    x = gp.get_x_next(n)
    y = make_y(x, B)
    gp.add_y_next(y)
    if out is not None:
        out.update(pts)
        out.update({"family": np.array(family), "m": np.array(m), "d": np.array(d), "alpha": np.array(alpha),
                    "B": np.array(B), "per_output": np.array(po), "lengthscales": _np(ls),
                    "x": _np(x), "xb": _np(gp.get_xb(0)), "y": _np(y)})
    return gp


def gen_case(fg, qmcpy, c, fit_its=3):
    family, m, d, alpha, B, po = c
    n = 2 ** m
    out = {}
    fgp = build(fg, qmcpy, c, out)
    g = torch.Generator().manual_seed(100 + m)
    ft_in = torch.randn((3, n), generator=g) + 5.0
    out["ft_in"] = _np(ft_in)
    out["ft_out"] = _np(fgp.ft(ft_in))
    if family == "lattice":
        ift_in = torch.randn((3, n), generator=g) + 1j * torch.randn((3, n), generator=g)
    else:
        ift_in = torch.randn((3, n), generator=g)
    out["ift_in"] = _np(ift_in)
    out["ift_out"] = _np(fgp.ift(ift_in))
    out["k1parts"] = _np(fgp.get_k1parts(0, 0))
    out["lam"] = _np(fgp.get_lam(0, 0))
    out["ytilde"] = _np(fgp.get_ytilde(0))
    # MLL + autograd gradient exactly as fit() forms it (abstract_gp.py:235,253-260,294)
    os.environ["FASTGP_FORCE_RECOMPILE"] = "True"
    cache = fgp.get_inv_log_det_cache()
    norm_term, logdet = cache.get_norm_term_logdet_term()
    d_out = int(torch.tensor(fgp.shape_batch).prod())
    mll_const = d_out * fgp.n.sum() * np.log(2 * np.pi)
    term1 = norm_term.sum()
    term2 = d_out / torch.tensor(logdet.shape).prod() * logdet.sum()
    loss = 0.5 * (term1 + term2 + mll_const)
    gs, gl = torch.autograd.grad(loss, [fgp.raw_scale, fgp.raw_lengthscales])
    del os.environ["FASTGP_FORCE_RECOMPILE"]
    out["norm_term"] = _np(norm_term)
    out["logdet"] = _np(logdet)
    out["loss"] = _np(loss)
    out["grad_raw_scale"] = _np(gs)
    out["grad_raw_lengthscales"] = _np(gl)
    xt = torch.rand((16, d), generator=torch.Generator().manual_seed(17))
    out["x_test"] = _np(xt)
    out["coeffs"] = _np(fgp.coeffs)
    out["pmean"] = _np(fgp.post_mean(xt))
    out["pvar"] = _np(fgp.post_var(xt))
    out["pcov"] = _np(fgp.post_cov(xt[:4], xt[4:9]))
    out["pcmean"] = _np(fgp.post_cubature_mean())
    out["pcvar"] = _np(fgp.post_cubature_var())
    out["pvar_2n"] = _np(fgp.post_var(xt, n=2 * n))
    out["pcvar_2n"] = _np(fgp.post_cubature_var(n=2 * n))
    data = fgp.fit(iterations=fit_its, store_hists=True, verbose=0, stop_crit_wait_iterations=fit_its + 5)
    out["fit_iterations"] = np.array(data["iterations"])
    out["fit_loss_hist"] = _np(data["loss_hist"])
    out["fit_scale_hist"] = _np(data["scale_hist"])
    out["fit_lengthscales_hist"] = _np(data["lengthscales_hist"])
    out["fit_raw_scale"] = _np(fgp.raw_scale)
    out["fit_raw_lengthscales"] = _np(fgp.raw_lengthscales)
    out["fit_pmean"] = _np(fgp.post_mean(xt))
    out["fit_pvar"] = _np(fgp.post_var(xt))
    # further fits, each on a fresh GP
    name = case_name(c)
    if name == "net_m8_d12_a1_b0":
        for metric in ("GCV", "CV"):
            gp = build(fg, qmcpy, c)
            data = gp.fit(loss_metric=metric, iterations=ALT_ITS, store_hists=True, verbose=0,
                          stop_crit_wait_iterations=ALT_ITS + 5)
            extra_fit(out, metric.lower(), gp, data, xt)
    if name == "lattice_m8_d12_a2_b0":
        gp = build(fg, qmcpy, c)
        opt = torch.optim.Adam(gp.parameters(), lr=0.05)
        data = gp.fit(optimizer=opt, iterations=3, store_hists=True, verbose=0, stop_crit_wait_iterations=8)
        extra_fit(out, "adam", gp, data, xt)
    if B > 0:
        gp = build(fg, qmcpy, c)
        mask = [[0, 2]]
        data = gp.fit(iterations=3, store_hists=True, verbose=0, stop_crit_wait_iterations=8, masks=torch.tensor(mask))
        out["mask"] = np.array(mask)
        extra_fit(out, "mask", gp, data, xt)
    return out


def extra_fit(out, key, gp, data, xt):
    out[key + "_loss_hist"] = _np(data["loss_hist"])
    out[key + "_scale_hist"] = _np(data["scale_hist"])
    out[key + "_lengthscales_hist"] = _np(data["lengthscales_hist"])
    out[key + "_raw_scale"] = _np(gp.raw_scale)
    out[key + "_raw_lengthscales"] = _np(gp.raw_lengthscales)
    out[key + "_pmean"] = _np(gp.post_mean(xt))


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for c in CASES:
        name = case_name(c)
        if only and name not in only:
            continue
        out = gen_case(fg, qmcpy, c)
        fn = os.path.join(OUT, name + ".npz")
        np.savez_compressed(fn, **out)
        # K(x, x) = scale prod_j (1 + l_j part_j(0)): the parts of point 0 against itself
        kxx = np.max(np.prod(1 + out["lengthscales"] * out["k1parts"][0, 0, 0, :], -1))
        print("wrote %s (%d KB) loss=%.10e  K(x,x)=%.3g  min|lam|=%.3g" % (
            name, os.path.getsize(fn) // 1024, float(out["loss"]), kxx, np.abs(out["lam"]).min()))


if __name__ == "__main__":
    main()
