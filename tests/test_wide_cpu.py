"""Wide inputs (9 <= d <= 64), the part that needs no GPU:

  * the CPU oracle (oracle/fgp_oracle.py, generic in d) against the wide fixtures of the REAL reference
    (tests/golden/make_golden_wide.py -> tests/golden/wide/*.npz), with the bounds of tests/test_oracle_golden.py;
  * every fgp_wide_* entry point validates its arguments before any HIP call: d = 8, d = 65, a null pointer and a
    negative size are refused with a message on a machine without a device;
  * ABI 19, and every fgp_wide_* name of include/fgp_hip.h is bound in _native._SIGNATURES.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from oracle import fgp_oracle as O
from tests.test_oracle_golden import rel_close

torch.set_default_dtype(torch.float64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_DIR = os.path.join(ROOT, "tests", "golden", "wide")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WIDE_DIR, "*.npz")))


def load_wide(name):
    with np.load(os.path.join(WIDE_DIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def build_oracle(g):
    fam = str(g["family"])
    B, d = int(g["B"]), int(g["d"])
    y = torch.from_numpy(g["y"])
    ls = torch.from_numpy(g["lengthscales"])
    kw = dict(lengthscales=ls, shape_lengthscales=tuple(ls.shape))
    if bool(g["per_output"]):
        kw["shape_scale"] = (B, 1)
    if fam == "lattice":
        return O.OracleFastGP("lattice", torch.from_numpy(g["x"]), None, y, alpha=int(g["alpha"]), **kw)
    return O.OracleFastGP("net", torch.from_numpy(g["x"]), torch.from_numpy(g["xb"]), y, alpha=int(g["alpha"]),
                          t=int(g["t"]), **kw)


def test_the_eight_wide_fixtures_exist():
    assert NAMES == sorted(["lattice_m8_d12_a2_b0", "lattice_m6_d9_a3_b0", "lattice_m7_d64_a2_b0",
                            "lattice_m8_d12_a2_b3_po", "net_m8_d12_a1_b0", "net_m7_d13_a2_b0", "net_m6_d64_a1_b0",
                            "net_m8_d12_a1_b3"])
    for name in NAMES:
        g = load_wide(name)
        assert 9 <= int(g["d"]) <= 64 and g["lengthscales"].shape[-1] == int(g["d"])
        ls = g["lengthscales"].reshape(-1, int(g["d"]))
        assert all(len(set(r.tolist())) == int(g["d"]) for r in ls), "pairwise different lengthscales"


@pytest.mark.parametrize("name", NAMES)
def test_wide_points_regenerate_bit_exact(name):
    g = load_wide(name)
    n = 2 ** int(g["m"])
    if str(g["family"]) == "lattice":
        assert np.array_equal(O.lattice_points(g["z"], g["shift"], 0, n), g["x"])
        # the generating vector is DEFAULT_LATTICE_Z extended by seqs.Lattice's rule
        import fastgaussianprocesses_amd as F
        assert np.array_equal(F.Lattice(int(g["d"]), shift=g["shift"]).z, g["z"])
        assert np.array_equal(F.Lattice(int(g["d"]), shift=g["shift"])(0, n), g["x"])
    else:
        xb = O.net_points_binary(g["C"], g["shift"], 0, n)
        assert np.array_equal(xb, g["xb"])
        assert np.array_equal(xb * 2.0 ** (-int(g["t"])), g["x"])


@pytest.mark.parametrize("name", NAMES)
def test_wide_oracle_caches_and_mll(name):
    g = load_wide(name)
    o = build_oracle(g)
    rel_close(o.k1parts().numpy(), g["k1parts"][:, 0, 0, :], 1e-14)
    rel_close(o.lam().detach().numpy(), g["lam"], 1e-13)
    rel_close(o.ytilde().numpy(), g["ytilde"], 1e-13)
    norm, logdet = o.norm_logdet()
    rel_close(norm.detach().numpy(), g["norm_term"], 5e-8)
    rel_close(logdet.detach().numpy(), g["logdet"], 1e-9)
    loss, _, _ = o.mll_loss()
    rel_close(loss.item(), g["loss"], 5e-8)
    gs, gl = torch.autograd.grad(loss, [o.raw_scale, o.raw_lengthscales])
    rel_close(gs.numpy(), g["grad_raw_scale"], 2e-7)
    rel_close(gl.numpy(), g["grad_raw_lengthscales"], 2e-7)


@pytest.mark.parametrize("name", NAMES)
def test_wide_oracle_posteriors(name):
    g = load_wide(name)
    o = build_oracle(g)
    xt = torch.from_numpy(g["x_test"])
    rel_close(o.coeffs().detach().numpy(), g["coeffs"], 1e-7)
    rel_close(o.post_mean(xt).numpy(), g["pmean"], 1e-9)
    kxx = o.kernel(xt, xt).detach().numpy()
    assert np.max(np.abs(o.post_var(xt).numpy() - g["pvar"])) <= 1e-9 * np.max(np.abs(kxx))
    assert np.max(np.abs(o.post_cov(xt[:4], xt[4:9]).numpy() - g["pcov"])) <= 1e-9 * np.max(np.abs(kxx))
    rel_close(o.post_cubature_mean().numpy(), g["pcmean"], 1e-10)
    assert np.max(np.abs(o.post_cubature_var().numpy() - g["pcvar"])) <= 1e-9 * float(o.scale.max())


@pytest.mark.parametrize("name", NAMES)
def test_wide_oracle_fit_trajectory(name):
    g = load_wide(name)
    o = build_oracle(g)
    its = int(g["fit_iterations"])
    data = o.fit(iterations=its, stop_crit_wait_iterations=its + 5)
    assert data["iterations"] == its
    rel_close(data["loss_hist"].numpy(), g["fit_loss_hist"], 1e-9)
    rel_close(data["scale_hist"].numpy(), g["fit_scale_hist"], 1e-12)
    rel_close(data["lengthscales_hist"].numpy(), g["fit_lengthscales_hist"], 1e-12)
    rel_close(o.raw_scale.detach().numpy(), g["fit_raw_scale"], 1e-12)
    rel_close(o.raw_lengthscales.detach().numpy(), g["fit_raw_lengthscales"], 1e-12)


# ------------------------------------------------------------------------------------------ C ABI
def header_wide_functions():
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(fgp_wide_\w+)\s*\(", src, flags=re.M)))


def test_abi_19_and_wide_symbols_bound():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20 and N.WIDE_MAX_D == 64
    names = header_wide_functions()
    assert {"fgp_wide_lattice_points", "fgp_wide_lattice_parts", "fgp_wide_net_parts", "fgp_wide_k1", "fgp_wide_k1_bwd",
            "fgp_wide_kernel_rows", "fgp_wide_post_mean"} <= set(names)
    for name in names:
        assert name in N._SIGNATURES, "ctypes binding misses %s" % name
        assert hasattr(lib, name), "libfgp_hip.so does not export %s" % name
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    assert re.search(r"#define\s+FGP_WIDE_MAX_D\s+64\b", src) and re.search(r"#define\s+FGP_MAX_D\s+8\b", src)


# host buffers standing in for device memory: a call that fails validation never reads them
_BUF = (ctypes.c_double * 4096)()


def _p(null=False):
    return ctypes.c_void_p(None if null else ctypes.addressof(_BUF))


def _wide_calls(d, null=False, neg=False):
    """(name, args) of every fgp_wide_* entry point with dimension d; `null` nulls one required pointer, `neg` makes
    one size negative -- everything else valid."""
    dd = max(1, min(d, 64))
    order_l, order_n = N.int_array([4] * dd), N.int_array([1] * dd)
    coef, z64 = N.double_array([1.0] * dd), N.int64_array([1] * dd)
    n = -1 if neg else 16
    out = ctypes.c_int64(0)
    return [
        ("fgp_wide_lattice_points", (None if null else z64, _p(), 0, -1 if neg else 16, d, _p(), None)),
        ("fgp_wide_lattice_parts", (_p(), d, _p(null), n, d, order_l, coef, _p(), None)),
        ("fgp_wide_net_parts", (_p(), d, _p(), n, d, 32, order_n, _p(null), None)),
        ("fgp_wide_k1", (_p(), n, d, _p(), _p(null), 1, _p(), None)),
        ("fgp_wide_k1_bwd", (_p(), n, d, _p(), _p(), 1, _p(), _p(), _p(null), _p(), None)),
        ("fgp_wide_k1_bwd_work", (n, d, 1, None if null else ctypes.pointer(out))),
        ("fgp_wide_kernel_rows", (0, _p(), -1 if neg else 2, _p(), 16, d, 0, order_l, coef, _p(null), 1, _p(), None)),
        ("fgp_wide_post_mean", (0, _p(), -1 if neg else 2, _p(), 16, d, 0, order_l, coef, _p(), 1, _p(null), 16, 1, _p(), 2,
                                _p(), 16, None)),
    ]


@pytest.mark.parametrize("why,kw", [("d = 8", dict(d=8)), ("d = 65", dict(d=65)), ("null pointer", dict(d=12, null=True)),
                                    ("negative size", dict(d=12, neg=True))])
def test_wide_entry_points_validate_before_any_hip_call(why, kw):
    lib = N.lib()
    calls = _wide_calls(**kw)
    assert sorted(c[0] for c in calls) == header_wide_functions(), "every fgp_wide_* entry point is exercised"
    for name, args in calls:
        lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
        before = lib.fgp_last_error()
        rc = getattr(lib, name)(*args)
        msg = lib.fgp_last_error()
        assert rc == -1, "%s accepted %s (rc = %d)" % (name, why, rc)
        assert msg and msg != before and name.encode() in msg, (name, why, msg)


def test_wide_python_dispatch_limits():
    """ops routes by d: d <= 8 keeps the narrow entry points, d > 8 takes the wide ones."""
    from fastgaussianprocesses_amd import ops
    assert not ops._wide(1) and not ops._wide(8) and ops._wide(9) and ops._wide(64)
