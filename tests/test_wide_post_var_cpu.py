"""Posterior variance of wide GPs (9 <= d <= 64) by the Parseval form, the part that needs no GPU:

  * fgp_wide_post_var_qf is exported, declared `extern int` in include/fgp_hip.h and bound at ABI 20;
  * it refuses bad arguments before any HIP call, with the status fgp_post_var_qf / fgp_post_var_batched return for the
    same mistake and its own name in fgp_last_error();
  * the CPU oracle's post_var agrees with the fixtures of the REAL reference (tests/golden/make_golden_wide_pvar.py ->
    tests/golden/wide_pvar/*.npz) at 1e-9 K(x, x), at n and at 2n (the oracle over the first 2n points: the posterior
    variance does not depend on the observations);
  * ops.wide_post_var_qf() parses FGP_WIDE_POST_VAR_QF.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from oracle import fgp_oracle as O

torch.set_default_dtype(torch.float64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVAR_DIR = os.path.join(ROOT, "tests", "golden", "wide_pvar")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PVAR_DIR, "*.npz")))
EXPECTED = sorted(["lattice_m13_d64_a2_b0", "lattice_m13_d9_a3_b0", "lattice_m13_d12_a2_b3_po", "net_m13_d9_a1_b0",
                   "net_m13_d13_a2_b0", "net_m14_d64_a1_b0"])
ENTRY = "fgp_wide_post_var_qf"


def load_pvar(name):
    with np.load(os.path.join(PVAR_DIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def points(g, n):
    """(x, xb) of the fixture's first n points, regenerated (the fixtures store x[:8] and x[-8:] only)."""
    if str(g["family"]) == "lattice":
        return O.lattice_points(g["z"], g["shift"], 0, n), None
    xb = O.net_points_binary(g["C"], g["shift"], 0, n)
    return xb * 2.0 ** (-int(g["t"])), xb


def build_oracle(g, n):
    """The oracle GP of a fixture over its first n points (n = 2^m: the fixture's observations; n = 2^(m+1): zeros)."""
    fam = str(g["family"])
    B = int(g["B"])
    y = torch.from_numpy(g["y"])
    if n != y.shape[-1]:
        y = torch.zeros(tuple(y.shape[:-1]) + (n,))
    ls = torch.from_numpy(g["lengthscales"])
    kw = dict(lengthscales=ls, shape_lengthscales=tuple(ls.shape))
    if bool(g["per_output"]):
        kw["shape_scale"] = (B, 1)
    x, xb = points(g, n)
    if fam == "lattice":
        return O.OracleFastGP("lattice", torch.from_numpy(x), None, y, alpha=int(g["alpha"]), **kw)
    return O.OracleFastGP("net", torch.from_numpy(x), torch.from_numpy(xb), y, alpha=int(g["alpha"]), t=int(g["t"]), **kw)


def test_the_six_fixtures_exist_and_are_small():
    assert NAMES == EXPECTED
    for name in NAMES:
        assert os.path.getsize(os.path.join(PVAR_DIR, name + ".npz")) < 300 * 1024
        g = load_pvar(name)
        d, n = int(g["d"]), 2 ** int(g["m"])
        assert "x" not in g and "xb" not in g
        assert g["x_test"].shape == (16, d) and g["y"].shape[-1] == n
        assert list(g["x_test"][0, :3]) == [0.0, 1.0, 0.5]
        x, _ = points(g, n)
        assert np.array_equal(x[:8], g["x_head"]) and np.array_equal(x[-8:], g["x_tail"])
        assert np.array_equal(g["x_test"][1], x[5]), "row 1 of x_test is training point 5"
        assert g["pvar"].shape == g["pvar_2n"].shape == g["kxx"].shape


@pytest.mark.parametrize("name", EXPECTED)
def test_oracle_post_var_matches_fixture(name):
    g = load_pvar(name)
    xt = torch.from_numpy(g["x_test"])
    K = float(np.max(np.abs(g["kxx"])))
    n = 2 ** int(g["m"])
    for key, nn in (("pvar", n), ("pvar_2n", 2 * n)):
        o = build_oracle(g, nn)
        if key == "pvar":
            assert np.max(np.abs(o.kernel(xt, xt).detach().numpy() - g["kxx"])) <= 1e-13 * K
        err = float(np.max(np.abs(o.post_var(xt).numpy() - g[key])))
        print(name, key, "oracle err / K = %.3g" % (err / K))
        assert err <= 1e-9 * K


# ------------------------------------------------------------------------------------------ C ABI
def test_symbol_exported_declared_extern_and_bound_at_abi_20():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    assert hasattr(lib, ENTRY), "libfgp_hip.so does not export %s" % ENTRY
    assert ENTRY in N._SIGNATURES and len(N._SIGNATURES[ENTRY]) == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"^extern\s+int\s+%s\s*\(" % ENTRY, src, flags=re.M)
    assert not re.search(r"^\s*int\s+%s\s*\(" % ENTRY, src, flags=re.M)
    assert re.search(r"#define\s+FGP_ABI_VERSION\s+20\b", src)


# host buffers standing in for device memory: a call that fails validation never reads them
_BUF = (ctypes.c_double * 4096)()
FGP_ERR_INVALID, FGP_ERR_UNSUPPORTED = -1, -2


def _args(family=0, xt=True, N_=2, z=True, log2n=13, d=12, order="ok", coef=True, hyp=True, wa=True, P=1, work=True,
          partial=True, out=True):
    def p(ok):
        return ctypes.c_void_p(ctypes.addressof(_BUF) if ok else None)
    dd = max(1, min(d, 64))
    if order == "ok":
        order_a = N.int_array([4 if family == 0 else 1] * dd)
    elif order is None:
        order_a = None
    else:
        order_a = N.int_array([order] * dd)
    coef_a = N.double_array([1.0] * dd) if coef else None
    return (family, p(xt), 0, N_, p(z), 0, log2n, d, 32 if family == 1 else 0, order_a, coef_a, p(hyp), 0, p(wa), 0, P,
            p(work), p(partial), p(out), None)


REFUSALS = [
    ("d = 8", dict(d=8), FGP_ERR_INVALID),
    ("d = 65", dict(d=65), FGP_ERR_INVALID),
    ("log2n = 12", dict(log2n=12), FGP_ERR_INVALID),
    ("log2n = 25", dict(log2n=25), FGP_ERR_INVALID),
    ("N < 0", dict(N_=-1), FGP_ERR_INVALID),
    ("P = 0", dict(P=0), FGP_ERR_INVALID),
    ("P = 65536", dict(P=65536), FGP_ERR_INVALID),
    ("null xt", dict(xt=False), FGP_ERR_INVALID),
    ("null z", dict(z=False), FGP_ERR_INVALID),
    ("null hyp", dict(hyp=False), FGP_ERR_INVALID),
    ("null wa", dict(wa=False), FGP_ERR_INVALID),
    ("null work", dict(work=False), FGP_ERR_INVALID),
    ("null partial", dict(partial=False), FGP_ERR_INVALID),
    ("null out", dict(out=False), FGP_ERR_INVALID),
    ("null lattice order", dict(order=None), FGP_ERR_INVALID),
    ("null lattice coef", dict(coef=False), FGP_ERR_INVALID),
    ("bad family", dict(family=7), FGP_ERR_INVALID),
    ("odd Bernoulli order", dict(order=5), FGP_ERR_UNSUPPORTED),
    ("Bernoulli order 10", dict(order=10), FGP_ERR_UNSUPPORTED),
    ("Walsh order 5", dict(family=1, order=5), FGP_ERR_UNSUPPORTED),
    ("P N 2^(log2n-12) = 2^31", dict(P=2 ** 7, N_=2 ** 12, log2n=24), FGP_ERR_UNSUPPORTED),
    ("P N 2^(log2n-12) = 2^31, N large", dict(P=1, N_=2 ** 30, log2n=13), FGP_ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("why,kw,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_hip_call(why, kw, status):
    lib = N.lib()
    fn = getattr(lib, ENTRY)
    fn.argtypes = N._SIGNATURES[ENTRY]
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = fn(*_args(**kw))
    msg = lib.fgp_last_error()
    assert rc == status, "%s: rc = %d, %r" % (why, rc, msg)
    assert msg and msg != before and ENTRY.encode() in msg, (why, msg)


def test_same_status_as_the_narrow_entry():
    """The narrow entry's statuses for the same mistakes (fgp_post_var_qf: sizes and null pointers FGP_ERR_INVALID, too
    many workgroups and a bad order FGP_ERR_UNSUPPORTED)."""
    lib = N.lib()
    fn = lib.fgp_post_var_qf
    fn.argtypes = N._SIGNATURES["fgp_post_var_qf"]
    p = ctypes.c_void_p(ctypes.addressof(_BUF))
    o4, o5, c = N.int_array([4] * 3), N.int_array([5] * 3), N.double_array([1.0] * 3)
    assert fn(0, p, 2, p, 12, 3, 0, o4, c, p, p, p, p, p, None) == FGP_ERR_INVALID
    assert fn(0, p, -1, p, 13, 3, 0, o4, c, p, p, p, p, p, None) == FGP_ERR_INVALID
    assert fn(0, p, 2, p, 13, 3, 0, o4, c, p, None, p, p, p, None) == FGP_ERR_INVALID
    assert fn(0, p, 2, p, 13, 3, 0, o5, c, p, p, p, p, p, None) == FGP_ERR_UNSUPPORTED
    assert fn(0, p, 2 ** 30, p, 13, 3, 0, o4, c, p, p, p, p, p, None) == FGP_ERR_UNSUPPORTED


def test_no_test_points_is_ok_without_a_device():
    lib = N.lib()
    fn = getattr(lib, ENTRY)
    fn.argtypes = N._SIGNATURES[ENTRY]
    assert fn(*_args(N_=0)) == 0
    assert fn(*_args(N_=0, xt=False, work=False)) == 0         # (as fgp_post_var_qf: N = 0 returns before the pointers)


@pytest.mark.parametrize("value,on", [(None, True), ("1", True), ("0", False), ("", True), ("00", False), ("on", True),
                                      ("01", False)])
def test_switch_parsing(value, on, monkeypatch):
    """As ops.wide_fused(): unset or anything not starting with '0' is on."""
    if value is None:
        monkeypatch.delenv("FGP_WIDE_POST_VAR_QF", raising=False)
    else:
        monkeypatch.setenv("FGP_WIDE_POST_VAR_QF", value)
    assert ops.wide_post_var_qf() is on
    monkeypatch.setenv("FGP_WIDE_FUSED", "0")                  # (another switch does not leak into this one)
    assert ops.wide_post_var_qf() is on
