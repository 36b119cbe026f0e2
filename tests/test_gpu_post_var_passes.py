"""GPBatch.post_var through the quadratic-form passes (csrc/fgp_predict.hip: k_qf_rows_r2c + k_qf_cols_r2c for
lattices at n >= 2^17, k_qf_rows + k_qf_cols below and for nets) at the smallest sizes that reach each form of the
column pass, and the spectra build's pass pair (csrc/fgp_nll.hip spec_basis_r2c):

  * against the CPU oracle at the posterior-variance tolerance of tests/test_gpu_configs.py (1e-8 K(x, x));
  * bit for bit the same value for a (problem, test point) row whichever launch, row of the launch or workgroup
    order computed it: the test points permuted, one per launch, all in one launch.  Every row has a column tile
    0, whose pair-column 0 holds the self-mirrored frequencies (0, n/2, n/4, 3n/4), so every point checks them;
  * the part-product spectra with work space for all 2^d subsets at once and for one subset per launch pair.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from fastgaussianprocesses_amd.fit_engine import LatticePartsGen, spec_chunks
from oracle import fgp_oracle as O
from tests.gpu_fixtures import DEV

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

# (family, log2 n, d, problems P, test points N): k_qf_cols_r2c<4> (2^17), <5> (2^18), <7> (2^20, the benchmark's
# instance); d = 1 and d = 5; P N = 15, no multiple of a power of two; the full-length net form at 2^13
CASES = [("lattice", 17, 1, 2, 3), ("lattice", 17, 5, 3, 5), ("lattice", 18, 5, 2, 3), ("lattice", 20, 5, 2, 3),
         ("net", 13, 3, 2, 5)]
IDS = ["%s-m%d-d%d-P%d-N%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def build(family, m, d, P, Nt):
    """(batch, its GPs, their points and observations on the host, shared test points [Nt, d] on the host)"""
    n = 2 ** m
    gps, xs, ys = [], [], []
    for seed in range(1000, 1000 + P):
        if family == "lattice":
            gp = F.FastGPLattice(F.Lattice(d, seed=seed, randomize="SHIFT"), device=DEV)
        else:
            gp = F.FastGPDigitalNetB2(F.DigitalNetB2(d, seed=seed), device=DEV)
        x = gp.get_x_next(n)
        y = O.f_ackley(x.cpu())
        gp.add_y_next(y.to(DEV))
        gps.append(gp)
        xs.append(x.cpu())
        ys.append(y)
    xt = torch.rand((Nt, d), generator=torch.Generator().manual_seed(100 * m + d))
    return F.GPBatch(gps), gps, xs, ys, xt


@functools.lru_cache(maxsize=None)
def post_var_once(case):
    batch, _, _, _, xt = build(*case)
    return batch.post_var(xt.to(DEV)).cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_post_var_matches_oracle(case):
    family, m, d, P, Nt = case
    _, gps, xs, ys, xt = build(*case)
    pv = post_var_once(case)
    assert pv.shape == (P, Nt)
    for p, gp in enumerate(gps):
        o = O.OracleFastGP(family, xs[p], gp.get_xb().cpu() if family == "net" else None, ys[p], alpha=gp._alphas[0],
                           t=getattr(gp, "t", None))
        opv = o.post_var(xt).detach()
        kxx = float(o.kernel(xt, xt).detach().abs().max())
        err = float((pv[p] - opv).abs().max())
        print("%s problem %d: |post_var - oracle| = %.3e, bound %.3e" % (case, p, err, 1e-8 * kxx))
        assert err <= 1e-8 * kxx


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_post_var_row_independent_of_launch_composition(case):
    family, m, d, P, Nt = case
    batch, _, _, _, xt = build(*case)
    base = post_var_once(case)
    perm = torch.randperm(Nt, generator=torch.Generator().manual_seed(m + Nt))
    inv = torch.argsort(perm)
    permuted = batch.post_var(xt[perm].to(DEV)).cpu()[:, inv]
    assert torch.equal(permuted, base)
    assert torch.equal(batch.post_var(xt.to(DEV), chunk=1).cpu(), base)
    assert torch.equal(batch.post_var(xt.to(DEV), chunk=16).cpu(), base)


def _spec_basis(name, head, m, d, wbytes):
    out = torch.empty((spec_chunks(0, 2 ** m), 2 ** d, 64), dtype=torch.float64, device=DEV)
    work = torch.empty((wbytes,), dtype=torch.uint8, device=DEV)
    N.call(name, *head, N.ptr(out), N.ptr(work), wbytes, N.stream_ptr(torch.device(DEV, 0)))
    return out.cpu()


def test_spectra_independent_of_subsets_per_launch():
    """fgp_spec_basis (and fgp_spec_basis_gen, the benchmark's row kernel) at n = 2^17, d = 2: work space for all 4
    subsets (one row / column launch pair) and for one subset (four pairs) give the same spectra bit for bit."""
    m, d, alpha = 17, 2, 2
    n = 2 ** m
    rng = np.random.default_rng(5)
    z = [int(v) for v in (2 * rng.integers(1, 2 ** (m - 1), size=d) + 1)]
    shift = torch.rand((1, d), generator=torch.Generator().manual_seed(3)).to(DEV)
    gen = LatticePartsGen(z, [alpha] * d, shift)
    parts = ops.lattice_parts_gen(gen.z, gen.shift[0], gen.alphas, n).contiguous()
    total = ctypes.c_int64(0)
    N.call("fgp_spec_basis_work", 0, m, d, ctypes.byref(total))
    one = total.value >> d
    from fastgaussianprocesses_amd.fit_engine import lattice_coefficient
    heads = {"fgp_spec_basis": (0, N.ptr(parts), d * n, 1, m, d),
             "fgp_spec_basis_gen": (N.int64_array(gen.z), m, d, 2 * alpha,
                                    N.double_array([lattice_coefficient(a) for a in gen.alphas]))}
    got = {}
    for name, head in heads.items():
        got[name] = _spec_basis(name, head, m, d, total.value)
        assert bool(torch.isfinite(got[name]).all())
        assert torch.equal(_spec_basis(name, head, m, d, one), got[name])
    assert torch.equal(got["fgp_spec_basis"], got["fgp_spec_basis_gen"])
