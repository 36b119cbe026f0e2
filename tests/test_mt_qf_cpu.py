"""The multitask posterior variance's quadratic form (fgp_mt_quadform), the part that needs no GPU:

  * the entry point is declared in include/fgp_hip.h, bound in _native._SIGNATURES and exported, at ABI 20;
  * it validates its arguments before any HIP call, on a machine without a device;
  * the longdouble reference (tests/mt_qf_reference.py) on a factor computed on the CPU -- the LDL^H recurrence applied to
    OracleMultiTaskFastGP.blocks -- reproduces the reference's pvar and pvar_new on the five wide fixtures and on the
    d <= 8 multitask fixtures, at tests/test_oracle_multitask.py's own tolerances;
  * the host rule of the route (ops.mt_post_var_qf).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from golden_util import load_golden
from tests import mt_qf_reference as R
from tests import test_oracle_multitask as OM
from tests import test_wide_mt_cpu as WM

torch.set_default_dtype(torch.float64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fgp_mt_quadform"


# ------------------------------------------------------------------------------------------ C ABI
def test_mt_quadform_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgp_hip.h")).read(), flags=re.S)
    assert re.search(r"^\s*extern\s+int\s+%s\s*\(" % NAME, src, flags=re.M)
    assert NAME in N._SIGNATURES and len(N._SIGNATURES[NAME]) == 10
    assert hasattr(lib, NAME) and NAME in N.exported_symbols()
    assert callable(ops.mt_quadform)


_BUF = (ctypes.c_double * 4096)()       # stands in for device memory: a call that fails validation never reads it


def _p(null=False):
    return ctypes.c_void_p(None if null else ctypes.addressof(_BUF))


def _lay(ns):
    lay = N.MtLayout()
    lay.T = len(ns)
    for k, v in enumerate(ns[:N.MT_MAX_TASKS]):
        lay.n[k] = v
    return lay


def _call(ns=(8, 8), layout=True, G=1, B=2, stride=None, real=0, fac=False, v=False, partial=False, out=False, T=None):
    lay = _lay(list(ns))
    if T is not None:
        lay.T = T
    stride = sum(ns) if stride is None else stride
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = getattr(lib, NAME)(ctypes.byref(lay) if layout else None, _p(fac), G, _p(v), stride, B, real, _p(partial),
                            _p(out), None)
    msg = lib.fgp_last_error()
    return rc, (msg if msg != before else b"")


@pytest.mark.parametrize("why,kw,word", [
    ("null layout", dict(layout=False), b"layout"),
    ("T = 0", dict(T=0), b"T"), ("T = 17", dict(T=17), b"T"),
    ("n not a power of two", dict(ns=(12, 4)), b"n["), ("n ascending", dict(ns=(4, 8)), b"n["),
    ("n = 0", dict(ns=(8, 0)), b"empty"),
    ("G = 0", dict(G=0), b"G"), ("B < 0", dict(B=-1), b"B"), ("B not a multiple of G", dict(G=2, B=3), b"B"),
    ("v_is_real = 2", dict(real=2), b"v_is_real"),
    ("null factor", dict(fac=True), b"null"), ("null v", dict(v=True), b"null"),
    ("null partial", dict(partial=True), b"null"), ("null out", dict(out=True), b"null"),
    ("stride < R nmin", dict(stride=15), b"v_row_stride")])
def test_mt_quadform_refuses_invalid_arguments_before_any_hip_call(why, kw, word):
    rc, msg = _call(**kw)
    assert rc == -1, "%s accepted (rc = %d)" % (why, rc)
    assert msg and word in msg, (why, msg)
    if not why.startswith("n"):
        assert NAME.encode() in msg, (why, msg)


@pytest.mark.parametrize("why,kw", [
    ("R > FGP_MT_MAX_ROWS", dict(ns=(1 << 25, 1), stride=(1 << 25) + 1)),
    ("2^31 partials", dict(ns=(512, 512), B=1 << 30, stride=1024))])
def test_mt_quadform_unsupported_sizes(why, kw):
    rc, msg = _call(**kw)
    assert rc == -2 and msg, (why, rc, msg)


def test_mt_quadform_of_no_vectors_is_ok_without_a_device():
    assert _call(B=0, fac=True, v=True, partial=True, out=True)[0] == 0
    assert _call(B=0, G=3)[0] == 0


# ------------------------------------------------------------------------------------------ host rule
def test_route_rule(monkeypatch):
    monkeypatch.delenv("FGP_MT_POST_VAR_QF", raising=False)
    assert ops.mt_post_var_qf([4096, 4096]) and ops.mt_post_var_qf([8192]) and ops.mt_post_var_qf([1 << 16] * 3)
    assert not ops.mt_post_var_qf([2048, 2048]) and not ops.mt_post_var_qf([8192, 128])
    assert not ops.mt_post_var_qf([256, 64, 8]), "the largest multitask post_var of the earlier tests keeps its route"
    # ... and all test points of a requested task in one chunk (asked only when the sizes pass)
    assert ops.mt_post_var_qf([4096, 4096], lambda: True) and not ops.mt_post_var_qf([4096, 4096], lambda: False)
    assert not ops.mt_post_var_qf([2048, 2048], lambda: 1 / 0)
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "1")
    assert ops.mt_post_var_qf([8, 4]) and ops.mt_post_var_qf([8, 4], lambda: False)
    monkeypatch.setenv("FGP_MT_POST_VAR_QF", "0")
    assert not ops.mt_post_var_qf([1 << 16] * 3)


# ------------------------------------------------------------------------------------------ reference vs oracle
def qf_post_var(o, xt, ns):
    """post_var [T, N] of oracle o at sizes ns through the CPU factor and the longdouble quadratic form."""
    with torch.no_grad():
        Lam, to, nsrt, nmin, _ = o.blocks(ns)
        act = [i for i in range(len(to)) if nsrt[i] > 0]
        nact = [nsrt[i] for i in act]
        fac = R.ldl_factor(R.pack_blocks(Lam.numpy(), nact), nact)
        kmat = o._kmat(xt, range(o.T), ns)                       # [T, N, sum n], task order
        segs = kmat.split(list(ns), -1)
        v = torch.cat([o.ft(segs[to[i]]) for i in act], -1)      # sorted active tasks
        v = v.reshape(-1, v.shape[-1]).numpy()
        q, _ = R.quadform_ref(fac, nact, v)
        Kt = o.gram_matrix_tasks
        knew = torch.stack([Kt[t, t] * o.kernel(xt, xt, t, t) for t in range(o.T)], 0).numpy()
    return np.maximum(knew - q.astype(np.float64).reshape(knew.shape), 0.0)


@pytest.mark.parametrize("name", WM.NAMES)
def test_reference_form_reproduces_the_wide_fixtures(name):
    g = WM.load_wide_mt(name)
    o = WM.make_oracle(g)
    xt = torch.from_numpy(g["x_test"])
    kxx = WM.kxx_scale(g)
    err = float(np.max(np.abs(qf_post_var(o, xt, list(o.ns)) - g["pvar"])))
    n_new = [int(v) for v in g["n_new"]]
    err_new = float(np.max(np.abs(qf_post_var(o, xt, n_new) - g["pvar_new"])))
    tol_new = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
    print("%s: pvar %.3g (tol %.3g), pvar_new %.3g (tol %.3g)" % (name, err, 1e-8 * kxx, err_new, tol_new))
    assert err <= 1e-8 * kxx
    assert err_new <= tol_new


# the fixtures of which tests/test_oracle_multitask.py compares a posterior variance (not the one whose reference inverse
# is inaccurate, nor the one whose posterior fp64 does not pin)
D8_NAMES = [n for n in OM.MT_NAMES if n not in OM.REF_INVERSE_ERROR and OM.pred_tol(n, "predictions", True)]


@pytest.mark.parametrize("name", D8_NAMES)
def test_reference_form_reproduces_the_multitask_fixtures(name):
    """tests/test_oracle_multitask.py's comparisons of pvar and pvar_new, with its tolerances."""
    g = load_golden(name)
    o = OM.make_oracle(g)
    xt = torch.from_numpy(g["x_test"])
    kxx = max(float(o.scale.detach()), float(np.max(np.abs(g["pvar"]))), float(np.max(np.abs(g["pcvar"])))) * 10
    err = float(np.max(np.abs(qf_post_var(o, xt, list(o.ns)) - g["pvar"])))
    print("%s: pvar %.3g (tol %.3g)" % (name, err, OM.pred_tol(name, "pvar", 1e-8) * kxx))
    assert err <= OM.pred_tol(name, "pvar", 1e-8) * kxx
    if OM.pred_tol(name, "pvar_new", 0.0) is not None:
        n_new = [int(v) for v in g["n_new"]]
        tol_new = 2e-2 * float(np.max(np.abs(g["pvar_new"]))) if str(g["kind"]) == "deriv" else 1e-8 * kxx
        err_new = float(np.max(np.abs(qf_post_var(o, xt, n_new) - g["pvar_new"])))
        print("%s: pvar_new %.3g (tol %.3g)" % (name, err_new, tol_new))
        assert err_new <= tol_new


def test_reference_form_equals_the_dense_inverse_on_seeded_blocks():
    """quadform_ref(ldl_factor(lams)) = v^H Lambda^-1 v of the dense class blocks, lattice and net, unequal n."""
    from tests.mt_qf_cases import make_lams, make_vectors
    for family in ("lattice", "net"):
        ns = [16, 8, 2]
        lay = R.Layout(ns)
        lams = make_lams(ns, 1, family, 1.0, 5)[0]
        v = make_vectors(ns, 3, family, 5)
        q, bq = R.quadform_ref(R.ldl_factor(lams, ns), ns, v)
        dense = np.zeros((lay.nmin, lay.R, lay.R), dtype=np.complex128)
        for (k, l) in lay.off:
            s = lay.seg(lams, k, l)
            for qq in range(lay.q[k]):
                r, c = lay.rs[k] + qq, lay.rs[l] + qq % lay.q[l]
                dense[:, r, c] = s[qq]
                if k != l:
                    dense[:, c, r] = np.conj(s[qq])
        vv = v.reshape(3, lay.R, lay.nmin).astype(np.complex128)
        want = np.einsum("brj,jrc,bcj->b", vv.conj(), np.linalg.inv(dense), vv).real
        assert np.max(np.abs(q.astype(np.float64) - want)) <= 1e-12 * float(np.max(bq))
        assert (bq >= q).all()
