"""Posterior variance of wide GPs (9 <= d <= 64) by the Parseval form on the GPU: fgp_wide_post_var_qf (k_wide_qf_rows +
k_qf_cols) and the post_var / GPBatch.post_var paths over it.  Bound everywhere: 1e-8 K(x, x).

1. Every fixture of tests/golden/make_golden_wide_pvar.py (the REAL reference), post_var(x) and post_var(x, n=2n), with
   the switch on (the new entry, no kernel rows) and off (the rows, no new entry).
2. Every row-pass instance against rows-and-solve in one process.
3. Chunking and batching change no bit.
4. Per-output hyper-parameters.
5. GPBatch.post_var against each GP's own.
6. Peak memory is the chunk's scratch.
7. Routing stays put.
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

import fastgaussianprocesses_amd as F
from fastgaussianprocesses_amd import _native, ops
from oracle.fgp_oracle import f_ackley
from tests.gpu_fixtures import DEV, abs_err
from tests.test_gpu_wide import net_matrices
from tests.test_gpu_wide_fit import _replica

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

PVAR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_pvar")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PVAR_DIR, "*.npz")))
ENTRY, ROWS = "fgp_wide_post_var_qf", "fgp_wide_kernel_rows"
_LOADED = {}


def load_pvar(name):
    if name not in _LOADED:
        with np.load(os.path.join(PVAR_DIR, name + ".npz"), allow_pickle=False) as f:
            _LOADED[name] = {k: f[k] for k in f.files}
    return _LOADED[name]


def fixture_gp(g):
    """The product GP of a fixture: its explicit point set, lengthscales and observations."""
    fam, d, B = str(g["family"]), int(g["d"]), int(g["B"])
    kw = dict(lengthscales=torch.from_numpy(g["lengthscales"]).to(DEV))
    if B > 0:
        kw["shape_batch"] = [B]
    if bool(g["per_output"]):
        kw["shape_scale"] = [B, 1]
        kw["shape_lengthscales"] = [B, d]
    if fam == "lattice":
        seq = F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shift"])
        gp = F.FastGPLattice(seq, alpha=int(g["alpha"]), device=DEV, **kw)
    else:
        seq = F.DigitalNetB2(d, randomize="DS", generating_matrices=g["C"].astype(np.uint64), t=int(g["t"]),
                             shift=g["shift"].astype(np.uint64))
        gp = F.FastGPDigitalNetB2(seq, alpha=int(g["alpha"]), device=DEV, **kw)
    x = gp.get_x_next(2 ** int(g["m"])).cpu().numpy()
    assert np.array_equal(x[:8], g["x_head"]) and np.array_equal(x[-8:], g["x_tail"]), \
        "point generation differs from the reference fixture"
    gp.add_y_next(torch.from_numpy(g["y"]).to(DEV))
    return gp


def spy(monkeypatch):
    names = []
    orig = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    return names


def corner_gp(family, d, alpha, n, seed=3, **kw):
    """A GP on n points with the lengthscales of the wide fixtures (K(x, x) stays O(10))."""
    kw.setdefault("lengthscales", (torch.linspace(0.01, 0.05, d) if d == 64 else torch.linspace(0.05, 0.3, d)).to(DEV))
    if family == "lattice":
        gp = F.FastGPLattice(F.Lattice(d, seed=seed), alpha=alpha, device=DEV, **kw)
    else:
        seq = F.DigitalNetB2(d, seed=seed, generating_matrices=net_matrices(d, seed))
        gp = F.FastGPDigitalNetB2(seq, alpha=alpha, device=DEV, **kw)
    x = gp.get_x_next(n)
    y = f_ackley(x)
    B = kw.get("shape_batch")
    if B:
        y = torch.stack([y * (1 + 0.1 * b) for b in range(B[0])])
    gp.add_y_next(y)
    return gp


def make_test_points(gp, N, seed=2):
    """N test points: row 0 starts with the coordinates 0.0, 1.0 and 0.5, row 1 is training point 5."""
    xt = torch.rand((N, gp.d), generator=torch.Generator().manual_seed(seed)).to(DEV)
    xt[0, 0], xt[0, 1], xt[0, 2] = 0.0, 1.0, 0.5
    if N > 1:
        xt[1] = gp.get_x(0)[5]
    return xt


def both_paths(gp, xt, monkeypatch, **kw):
    """(post_var with the switch on, with it off, K(x, x)), checking which entry points each took."""
    names = spy(monkeypatch)
    monkeypatch.setenv("FGP_WIDE_POST_VAR_QF", "1")
    on = gp.post_var(xt, **kw)
    assert ENTRY in names and ROWS not in names, names
    del names[:]
    monkeypatch.setenv("FGP_WIDE_POST_VAR_QF", "0")
    off = gp.post_var(xt, **kw)
    assert ROWS in names and ENTRY not in names, names
    with torch.no_grad():
        kxx = float(gp._kdiag(xt).abs().max())
    return on, off, kxx


# ---------------------------------------------------------------------------------------------- 1. fixtures
def test_fixtures_present():
    assert len(NAMES) == 6


@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_post_var_matches_reference(name, switch, monkeypatch):
    """Measured on the MI355X (err / K, switch on): see DESIGN.md section 3.5."""
    g = load_pvar(name)
    gp = fixture_gp(g)
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    n = 2 ** int(g["m"])
    K = float(np.abs(g["kxx"]).max())
    with torch.no_grad():
        assert abs_err(gp._kdiag(xt).expand(g["kxx"].shape), g["kxx"]) <= 1e-13 * K
    monkeypatch.setenv("FGP_WIDE_POST_VAR_QF", switch)
    want, banned = (ENTRY, ROWS) if switch == "1" else (ROWS, ENTRY)
    names = spy(monkeypatch)
    for key, kw in (("pvar", {}), ("pvar_2n", dict(n=2 * n))):
        del names[:]
        pv = gp.post_var(xt, **kw)
        assert pv.shape == g[key].shape
        err = abs_err(pv, g[key])
        print(name, "switch", switch, key, "err / K = %.3g" % (err / K))
        assert want in names and banned not in names, names
        assert err <= 1e-8 * K


# ---------------------------------------------------------------------------------------------- 2. instances
INSTANCES = [(fam, alpha, d, m) for fam, alpha in (("lattice", 2), ("lattice", 3), ("net", 1)) for d in (9, 13, 64)
             for m in (13, 14, 15, 16)] + [(fam, alpha, 9, 17) for fam, alpha in (("lattice", 2), ("lattice", 3), ("net", 1))]


@pytest.mark.parametrize("family,alpha,d,m", INSTANCES)
def test_row_pass_instance_against_rows_and_solve(family, alpha, d, m, monkeypatch):
    """k_wide_qf_rows<P2, T, ORD> for P2 = 9..12 (m = 13..16; m = 17: P2 = 12 with a 32-row column pass, where a narrow
    lattice goes half-length), T = double2 / double, ORD = 4 (lattice alpha = 2) / 0, N = 5 test points with the
    boundary row and a training point."""
    gp = corner_gp(family, d, alpha, 2 ** m)
    xt = make_test_points(gp, 5)
    on, off, kxx = both_paths(gp, xt, monkeypatch)
    err = abs_err(on, off)
    print("instance", family, alpha, d, m, "err / K = %.3g" % (err / kxx), "pvar at the training point / K = %.3g" %
          (float(on[1]) / kxx))
    assert on.shape == off.shape == (5,)
    assert err <= 1e-8 * kxx
    # at a training point the variance is at most the noise (1e-8 lattice, 1e-16 net), up to the bound above
    assert float(on[1]) <= 1e-8 + 1e-8 * kxx


# ---------------------------------------------------------------------------------------------- 3. no bit changes
@pytest.mark.parametrize("family,alpha", [("lattice", 2), ("net", 1)])
def test_chunking_changes_no_bit(family, alpha, monkeypatch):
    gp = corner_gp(family, 9, alpha, 2 ** 13)
    xt = make_test_points(gp, 37)                      # three chunks of 16
    names = spy(monkeypatch)
    full = gp.post_var(xt)
    assert names.count(ENTRY) == 3 and ROWS not in names
    head = gp.post_var(xt[:5])
    assert torch.equal(full[:5], head)
    assert torch.equal(gp.post_var(xt), full)


@pytest.mark.parametrize("shared_x", [True, False])
@pytest.mark.parametrize("shared_z", [True, False])
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_stacked_problems_equal_single_calls(family, shared_z, shared_x):
    """The entry with P = 3 stacked problems (own hyper-parameters and weights; shared or own z and test points)
    against three P = 1 calls: torch.equal."""
    d, n, Nt, P = 13, 2 ** 13, 5, 3
    gen = torch.Generator().manual_seed(41)
    fam = ops.LATTICE if family == "lattice" else ops.NET
    if family == "lattice":
        z = torch.rand((P, d, n), generator=gen).to(DEV)
        alphas, tbits = [3] * d, 0
    else:
        z = torch.randint(0, 2 ** 32, (P, d, n), generator=gen).to(DEV)
        alphas, tbits = [1] * d, 32
    xt = torch.rand((P, Nt, d), generator=gen).to(DEV)
    xt[0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    hyp = torch.cat([0.5 + torch.rand((P, 1), generator=gen), 0.05 + 0.25 * torch.rand((P, d), generator=gen)], 1).to(DEV)
    wa = (0.1 + torch.rand((P, n), generator=gen)).to(DEV)
    zz = z[0] if shared_z else z
    xx = xt[0] if shared_x else xt
    stacked = ops.wide_post_var_quadform(fam, xx, zz, hyp, wa, alphas=alphas, tbits=tbits)
    assert stacked.shape == (P, Nt) and bool(torch.isfinite(stacked).all()) and float(stacked.min()) > 0
    for p in range(P):
        one = ops.wide_post_var_quadform(fam, xx if shared_x else xx[p], zz if shared_z else zz[p], hyp[p], wa[p],
                                         alphas=alphas, tbits=tbits)
        assert one.shape == (1, Nt)
        assert torch.equal(stacked[p], one[0]), (p, float((stacked[p] - one[0]).abs().max()))
    if not shared_z:
        assert not torch.equal(stacked[0], stacked[1])


# ---------------------------------------------------------------------------------------------- 4. per-output
def test_per_output_fixture_against_rows_and_solve(monkeypatch):
    g = load_pvar("lattice_m13_d12_a2_b3_po")
    gp = fixture_gp(g)
    xt = torch.from_numpy(g["x_test"]).to(DEV)
    on, off, kxx = both_paths(gp, xt, monkeypatch)
    print("per-output fixture err / K = %.3g" % (abs_err(on, off) / kxx))
    assert on.shape == off.shape == (3, 16) and abs_err(on, off) <= 1e-8 * kxx


@pytest.mark.parametrize("family,alpha", [("lattice", 2), ("net", 1)])
def test_per_output_scale_with_shared_lengthscales(family, alpha, monkeypatch):
    gp = corner_gp(family, 12, alpha, 2 ** 13, shape_batch=[3], shape_scale=[3, 1],
                   scale=torch.tensor([[0.5], [1.0], [2.0]]).to(DEV))
    xt = make_test_points(gp, 7)
    on, off, kxx = both_paths(gp, xt, monkeypatch)
    print("per-output scale", family, "err / K = %.3g" % (abs_err(on, off) / kxx))
    assert on.shape == off.shape == (3, 7) and abs_err(on, off) <= 1e-8 * kxx
    assert not torch.equal(on[0], on[1])


# ---------------------------------------------------------------------------------------------- 5. GPBatch
@pytest.mark.parametrize("family", ["lattice", "net"])
def test_gpbatch_post_var_matches_each_gp(family, monkeypatch):
    d, n, P, Nt = 12, 2 ** 13, 3, 37
    gps = [_replica(family, d, n, p, lengthscales=0.05 * (1 + p)) for p in range(P)]
    b = F.GPBatch(gps)
    b.set_data(torch.stack([gp._y[0] for gp in gps]).clone())
    gen = torch.Generator().manual_seed(5)
    shared = torch.rand((Nt, d), generator=gen).to(DEV)
    own = torch.rand((P, Nt, d), generator=gen).to(DEV)
    b.coeffs()
    for xt in (shared, own):
        names = spy(monkeypatch)
        pv = b.post_var(xt)
        assert pv.shape == (P, Nt)
        assert names.count(ENTRY) == math.ceil(Nt / 16) and ROWS not in names, names
        monkeypatch.undo()
        for p, gp in enumerate(gps):
            xp = xt if xt.ndim == 2 else xt[p]
            with torch.no_grad():
                kxx = float(gp._kdiag(xp).abs().max())
            err = abs_err(pv[p], gp.post_var(xp)) / kxx
            print("GPBatch", family, "shared" if xt.ndim == 2 else "own", p, "err / K = %.3g" % err)
            assert err <= 1e-8
    assert float(pv.min()) >= 0.0


# ---------------------------------------------------------------------------------------------- 6. memory
@pytest.mark.parametrize("family,alpha", [("lattice", 2), ("net", 1)])
def test_peak_memory_is_the_chunk_scratch(family, alpha, monkeypatch):
    """n = 2^15, d = 9, N = 64.  On: at most 2 x (work of 16 test points + their partials + out), the chunk's scratch
    with a factor 2 for the allocator's rounding of blocks.  Off: more than the N x n float64 kernel rows."""
    n, Nt = 2 ** 15, 64
    gp = corner_gp(family, 9, alpha, n)
    xt = make_test_points(gp, Nt)
    size_t = 16 if family == "lattice" else 8
    bound = 2 * (16 * n * size_t + 16 * (n >> 12) * 8 + Nt * 8)
    peaks = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("FGP_WIDE_POST_VAR_QF", switch)
        gp.post_var(xt)                              # warm: points, eigenvalues and tables are cached
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pv = gp.post_var(xt)
        torch.cuda.synchronize()
        peaks[switch] = torch.cuda.max_memory_allocated() - base
        del pv
    print("peak bytes", family, peaks, "bound", bound, "rows", Nt * n * 8)
    assert peaks["1"] <= bound
    assert peaks["0"] > Nt * n * 8


# ---------------------------------------------------------------------------------------------- 7. routing
def test_small_n_keeps_the_rows(monkeypatch):
    gp = corner_gp("lattice", 12, 2, 2 ** 12)
    names = spy(monkeypatch)
    gp.post_var(make_test_points(gp, 5))
    assert ROWS in names and ENTRY not in names


def test_graph_mode_keeps_the_rows(monkeypatch):
    gp = corner_gp("lattice", 12, 2, 2 ** 13)
    assert any(p.requires_grad for p in gp.parameters())
    names = spy(monkeypatch)
    with torch.enable_grad():
        pv = gp.post_var(make_test_points(gp, 5), eval=False)
    assert ROWS in names and ENTRY not in names
    assert pv.requires_grad
    del names[:]
    gp.post_var(make_test_points(gp, 5))
    assert ENTRY in names and ROWS not in names


@pytest.mark.parametrize("family,alpha", [("lattice", 2), ("net", 1)])
def test_narrow_gp_never_reaches_the_wide_entries(family, alpha, monkeypatch):
    n = 2 ** 13
    if family == "lattice":
        gp = F.FastGPLattice(F.Lattice(8, seed=3), alpha=alpha, device=DEV, lengthscales=0.1)
    else:
        gp = F.FastGPDigitalNetB2(F.DigitalNetB2(8, seed=3), alpha=alpha, device=DEV, lengthscales=0.1)
    gp.add_y_next(f_ackley(gp.get_x_next(n)))
    names = spy(monkeypatch)
    xt = torch.rand((5, 8), generator=torch.Generator().manual_seed(2)).to(DEV)
    gp.post_var(xt), gp.post_var(xt, n=2 * n)
    assert "fgp_post_var_qf" in names and not [nm for nm in names if nm.startswith("fgp_wide_")], names
