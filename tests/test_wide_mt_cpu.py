"""Multitask / derivative-informed GPs on wide inputs (9 <= d <= 64), the part that needs no GPU:

  * the CPU oracle (oracle/fgp_oracle_mt.py, generic in d) against the wide multitask fixtures of the REAL reference
    (tests/golden/make_golden_wide_mt.py -> tests/golden/wide_mt/*.npz), with the tolerances of
    tests/test_oracle_multitask.py;
  * every fgp_wide_mt_* entry point validates its arguments before any HIP call: d = 8, d = 65, P = 0, P = 17, a null
    pointer, a negative size, a bad order and a bad tbits are refused with a message naming the entry point, on a machine
    without a device;
  * the entry points are declared in include/fgp_hip.h, bound in _native._SIGNATURES and exported, at ABI 20.
"""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from oracle.fgp_oracle_mt import OracleMultiTaskFastGP
from tests.test_oracle_multitask import rel

torch.set_default_dtype(torch.float64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_MT_DIR = os.path.join(ROOT, "tests", "golden", "wide_mt")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(WIDE_MT_DIR, "*.npz")))
ENTRY_POINTS = ["fgp_wide_mt_k1", "fgp_wide_mt_k1_bwd", "fgp_wide_mt_k1_bwd_work", "fgp_wide_mt_parts", "fgp_wide_mt_rows"]


def load_wide_mt(name):
    with np.load(os.path.join(WIDE_MT_DIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_derivatives(g):
    """(derivatives, derivatives_coeffs) lists over the tasks, or (None, None) for a plain multitask fixture."""
    if str(g["kind"]) != "deriv":
        return None, None
    T = len(g["ns"])
    return ([torch.from_numpy(g["derivatives_%d" % l]) for l in range(T)],
            [torch.from_numpy(g["derivatives_coeffs_%d" % l]) for l in range(T)])


def make_oracle(g):
    """The oracle at the fixture's initial lengthscales (its constructor starts from 1)."""
    T = len(g["ns"])
    ys = [torch.from_numpy(g["y_%d" % l]) for l in range(T)]
    derivs, dcoeffs = fixture_derivatives(g)
    if str(g["family"]) == "lattice":
        o = OracleMultiTaskFastGP("lattice", g["z"], g["shifts"], ys, alpha=int(g["alpha"]), derivatives=derivs,
                                  derivatives_coeffs=dcoeffs)
    else:
        o = OracleMultiTaskFastGP("net", g["C"], g["shifts"], ys, alpha=int(g["alpha"]), t=int(g["t"]), derivatives=derivs,
                                  derivatives_coeffs=dcoeffs)
    with torch.no_grad():
        o.raw_lengthscales.copy_(torch.log(torch.from_numpy(g["lengthscales"])))
    return o


def kxx_scale(g):
    return max(1.0, float(np.max(np.abs(g["pvar"]))), float(np.max(np.abs(g["pcvar"])))) * 10


def test_the_five_wide_multitask_fixtures_exist():
    assert NAMES == sorted(["mt_lattice_d12_a2_T3", "deriv_lattice_d12_a2", "deriv_net_d12_a4", "mt_net_d9_a2_T2_b2",
                            "deriv_lattice_d17_a3_c2"])
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    for name in NAMES:
        g = load_wide_mt(name)
        assert 9 <= int(g["d"]) <= 64 and g["lengthscales"].shape == (int(g["d"]),)
        assert len(set(g["lengthscales"].tolist())) == int(g["d"]), "pairwise different lengthscales"
        assert float(g["lengthscales"].max()) <= 0.3
        assert os.path.getsize(os.path.join(WIDE_MT_DIR, name + ".npz")) <= min(biggest, 1 << 20)
    g = load_wide_mt("deriv_lattice_d17_a3_c2")
    assert g["derivatives_1"].shape == (2, 17) and g["derivatives_coeffs_1"].tolist() == [0.5, -1.5]
    assert load_wide_mt("mt_net_d9_a2_T2_b2")["y_0"].shape == (2, 32)


@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_oracle_matches_reference(name):
    g = load_wide_mt(name)
    o = make_oracle(g)
    T = o.T
    for l in range(T):
        x, xb = o.points(l, int(g["ns"][l]))
        assert np.array_equal(x.numpy(), g["x_%d" % l])
        assert np.array_equal(xb.numpy(), g["xb_%d" % l])
    for a in range(T):
        for b in range(a, T):
            n = max(int(g["ns"][a]), int(g["ns"][b]))
            assert rel(o.k1parts(a, b, n).numpy(), g["k1parts_%d%d" % (a, b)]) < 1e-13
            assert rel(o.lam(a, b, n).detach().numpy(), g["lam_%d%d" % (a, b)]) < 1e-12
        assert rel(o.ytilde(a).numpy(), g["ytilde_%d" % a]) < 1e-12
    assert rel(o.gram_matrix_tasks.detach().numpy(), g["gram_matrix_tasks"]) == 0.0
    A, logdet, to, nsrt, nmin = o.inv_logdet()
    inv_ref = g["inv"]
    assert A.shape == inv_ref.shape
    assert rel(A.detach().numpy() if np.iscomplexobj(inv_ref) else A.detach().real.numpy(), inv_ref) < 1e-6
    ld_ref = g["logdet"].reshape(-1)
    assert np.max(np.abs(logdet.detach().numpy().reshape(-1) - ld_ref)) <= 1e-8 * np.max(np.abs(ld_ref)) + 1e-8
    norm, _ = o.norm_logdet()
    assert rel(norm.detach().numpy().reshape(-1), g["norm_term"].reshape(-1)) < 1e-7
    loss = o.mll_loss()
    assert abs(loss.item() - float(g["loss"])) <= 2e-7 * abs(float(g["loss"]))
    params = dict(raw_scale=o.raw_scale, raw_lengthscales=o.raw_lengthscales, raw_noise=o.raw_noise,
                  raw_factor_task_kernel=o.raw_factor_task_kernel, raw_noise_task_kernel=o.raw_noise_task_kernel)
    names = [str(s) for s in g["grad_names"]]
    grads = torch.autograd.grad(loss, [params[nm] for nm in names])
    for nm, gr in zip(names, grads):
        assert rel(gr.numpy(), g["grad_" + nm]) < 2e-6, nm
    xt = torch.from_numpy(g["x_test"])
    assert rel(o.coeffs().detach().numpy(), g["coeffs"]) < 1e-5
    assert rel(o.post_mean(xt).numpy(), g["pmean"]) < 1e-7
    kxx = kxx_scale(g)
    assert np.max(np.abs(o.post_var(xt).numpy() - g["pvar"])) <= 1e-8 * kxx
    assert np.max(np.abs(o.post_cov(xt[:4], xt[4:9]).numpy() - g["pcov"])) <= 1e-7 * kxx
    assert rel(o.post_cubature_mean().numpy(), g["pcmean"]) < 1e-8
    assert np.max(np.abs(o.post_cubature_var().numpy() - g["pcvar"])) <= 1e-8 * kxx
    assert np.max(np.abs(o.post_cubature_cov().numpy() - g["pccov"])) <= 1e-8 * kxx
    n_new = [int(v) for v in g["n_new"]]
    tol_new = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
    assert np.max(np.abs(o.post_var(xt, n_new).numpy() - g["pvar_new"])) <= tol_new
    assert np.max(np.abs(o.post_cubature_var(n_new).numpy() - g["pcvar_new"])) <= 1e-8 * kxx


@pytest.mark.parametrize("name", NAMES)
def test_wide_multitask_oracle_fit_trajectory(name):
    g = load_wide_mt(name)
    o = make_oracle(g)
    its = int(g["fit_iterations"])
    data = o.fit(iterations=its, stop_crit_wait_iterations=its + 5)
    assert data["iterations"] == its
    assert rel(data["loss_hist"].numpy(), g["fit_loss_hist"]) < 2e-7
    assert rel(data["lengthscales_hist"].numpy(), g["fit_lengthscales_hist"]) < 1e-10
    assert rel(data["scale_hist"].numpy(), g["fit_scale_hist"]) < 1e-10
    assert rel(data["task_kernel_hist"].numpy(), g["fit_task_kernel_hist"]) < 1e-10
    assert rel(o.post_mean(torch.from_numpy(g["x_test"])).numpy(), g["fit_pmean"]) < 1e-7


# ------------------------------------------------------------------------------------------ C ABI
def header_wide_mt_functions():
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*extern\s+int\s+(fgp_wide_mt_\w+)\s*\(", src, flags=re.M)))


def test_wide_mt_symbols_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20 and N.WIDE_MT_MAX_P == 16
    assert header_wide_mt_functions() == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert name in N._SIGNATURES, "ctypes binding misses %s" % name
        assert hasattr(lib, name), "libfgp_hip.so does not export %s" % name
        assert name in N.exported_symbols()
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    assert re.search(r"#define\s+FGP_WIDE_MT_MAX_P\s+16\b", src)


# host buffers standing in for device memory: a call that fails validation never reads them
_BUF = (ctypes.c_double * 4096)()


def _p(null=False):
    return ctypes.c_void_p(None if null else ctypes.addressof(_BUF))


def _calls(d=12, P=2, null=False, neg=False, order=4, tbits=32, family=0):
    """(name, args) of every fgp_wide_mt_* entry point; `null` nulls one required pointer, `neg` makes one size
    negative, `order` / `tbits` / `family` reach the entry points that take them -- everything else valid."""
    dd, PP = max(1, min(d, 64)), max(1, min(P, 17))
    o = N.int_array([order] * (PP * dd))
    ind = N.int_array([1] * (PP * dd))
    coef, add, cc = N.double_array([1.0] * (PP * dd)), N.double_array([0.0] * (PP * dd)), N.double_array([1.0] * PP)
    n = -1 if neg else 16
    out = ctypes.c_int64(0)
    return [
        ("fgp_wide_mt_parts", (family, _p(), d, n, _p(), d, 1, 0, d, P, o, coef, add, tbits, _p(null), None)),
        ("fgp_wide_mt_k1", (_p(), n, d, P, ind, cc, _p(), _p(null), 1, _p(), None)),
        ("fgp_wide_mt_k1_bwd_work", (n, d, P, 1, None if null else ctypes.pointer(out))),
        ("fgp_wide_mt_k1_bwd", (_p(), n, d, P, ind, cc, _p(), _p(), 1, _p(), _p(), _p(null), _p(), None)),
        ("fgp_wide_mt_rows", (family, _p(), -1 if neg else 2, _p(), 16, 0, d, P, o, coef, add, ind, cc, tbits, _p(null), 1,
                              _p(), None)),
    ]


def _refused(name, args, why, codes=(-1,)):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = getattr(lib, name)(*args)
    msg = lib.fgp_last_error()
    assert rc in codes, "%s accepted %s (rc = %d)" % (name, why, rc)
    assert msg and msg != before and name.encode() in msg, (name, why, msg)
    return msg


@pytest.mark.parametrize("why,kw,codes", [
    ("d = 8", dict(d=8), (-1,)), ("d = 65", dict(d=65), (-1,)), ("P = 0", dict(P=0), (-1,)),
    ("P = 17", dict(P=17), (-2,)),                           # FGP_ERR_UNSUPPORTED: the torch formulation covers it
    ("null pointer", dict(null=True), (-1,)), ("negative size", dict(neg=True), (-1,))])
def test_wide_mt_entry_points_validate_before_any_hip_call(why, kw, codes):
    calls = _calls(**kw)
    assert sorted(c[0] for c in calls) == ENTRY_POINTS, "every fgp_wide_mt_* entry point is exercised"
    for name, args in calls:
        msg = _refused(name, args, why, codes)
        if why.startswith("d ="):
            assert b"d=" in msg
        if why.startswith("P ="):
            assert b"P=" in msg


@pytest.mark.parametrize("why,kw,codes,word", [
    ("Bernoulli order 0", dict(order=0), (-2,), b"order"), ("Bernoulli order 9", dict(order=9), (-2,), b"order"),
    ("Walsh order 5", dict(order=5, family=1), (-2,), b"order"), ("tbits = 0", dict(order=2, family=1, tbits=0), (-1,), b"tbits"),
    ("tbits = 64", dict(order=2, family=1, tbits=64), (-1,), b"tbits"), ("family = 2", dict(family=2), (-1,), b"family")])
def test_wide_mt_spec_tables_are_validated(why, kw, codes, word):
    for name, args in _calls(**kw):
        if name in ("fgp_wide_mt_parts", "fgp_wide_mt_rows"):
            assert word in _refused(name, args, why, codes)


def test_wide_mt_ind_entries_are_validated():
    d, P = 12, 2
    bad = N.int_array([1] * (P * d - 1) + [2])
    cc = N.double_array([1.0] * P)
    assert b"ind" in _refused("fgp_wide_mt_k1", (_p(), 16, d, P, bad, cc, _p(), _p(), 1, _p(), None), "ind = 2")
    assert b"ind" in _refused("fgp_wide_mt_k1", (_p(), 16, d, P, None, cc, _p(), _p(), 1, _p(), None), "ind null")


def test_wide_mt_k1_bwd_work_length():
    out = ctypes.c_int64(0)
    assert N.lib().fgp_wide_mt_k1_bwd_work(66048, 17, 3, 5, ctypes.pointer(out)) == 0
    assert out.value == 5 * 18 * 258
