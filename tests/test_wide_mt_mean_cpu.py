"""The matrix-free multitask posterior mean of wide inputs (fgp_mt_wide_post_mean), the part that needs no GPU:

  * both entry points are declared in include/fgp_hip.h as plain `extern int`, bound in _native._SIGNATURES and exported,
    at ABI 20;
  * the work length for two hand-computed sizes;
  * every refusal reaches fgp_last_error() before any HIP call (a machine without a device): d = 8 and 65, P = 0 and 17,
    null pointers by field name, beta = 2, Gk outside {1, B}, a bad ind entry, an out-of-range order, a bad chunk;
  * the 80-bit reference (tests/wide_mt_mean_reference.py) agrees with a plain float64 rows @ c on every case of
    tests/wide_mt_mean_cases.py to the bound, and every case meets its non-vacuity cap: the assertion of
    tests/test_gpu_wide_mt_mean_exact.py cannot hide a defect;
  * a deliberately wrong accumulation -- the last training point of a chunk dropped, two coefficient rows swapped -- is
    rejected by the bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from fastgaussianprocesses_amd import _native as N
from tests import predict_reference as PR
from tests import wide_mt_mean_cases as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, WORK = "fgp_mt_wide_post_mean", "fgp_mt_wide_post_mean_work"
U = PR.EPS53


# ------------------------------------------------------------------------------------------ C ABI
def test_mt_wide_post_mean_symbols_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^\s*extern\s+int\s+(fgp_mt_wide_post_mean\w*)\s*\(", src, flags=re.M))
    assert declared == {ENTRY, WORK}
    for name, nargs in ((ENTRY, 25), (WORK, 5)):
        assert name in N._SIGNATURES and len(N._SIGNATURES[name]) == nargs
        assert hasattr(lib, name), "libfgp_hip.so does not export %s" % name
        assert name in N.exported_symbols()
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]


def test_mt_wide_post_mean_work_length():
    out = ctypes.c_int64(0)
    lib = N.lib()
    # B min(N, 65535) ceil(n / chunk): 5 x 300 x ceil(66048 / 1024 = 64.5); 2 x 65535 x ceil(1000 / 256)
    assert lib.fgp_mt_wide_post_mean_work(300, 66048, 5, 0, ctypes.pointer(out)) == 0 and out.value == 5 * 300 * 65
    assert lib.fgp_mt_wide_post_mean_work(100000, 1000, 2, 256, ctypes.pointer(out)) == 0 and out.value == 2 * 65535 * 4
    assert lib.fgp_mt_wide_post_mean_work(0, 1, 1, 0, ctypes.pointer(out)) == 0 and out.value == 1
    for case in MM.CASES:
        assert lib.fgp_mt_wide_post_mean_work(case.N, case.n, case.B, case.chunk, ctypes.pointer(out)) == 0
        assert out.value == MM.work_len(case)


# host buffers standing in for device memory: a call that fails validation never reads them
_BUF = (ctypes.c_double * 4096)()
_PTRS = ("xt", "z", "hyp", "coeffs", "out", "work")


def _p(null=False):
    return ctypes.c_void_p(None if null else ctypes.addressof(_BUF))


def _args(d=12, P=2, null=None, order=4, tbits=32, family=0, N_=2, n=16, B=3, Gk=3, beta=1, chunk=0, ind_bad=False,
          cstride=None, ostride=None, tables=("order", "coef", "add", "ind", "cc")):
    dd, PP = max(1, min(d, 64)), max(1, min(P, 17))
    o = N.int_array([order] * (PP * dd)) if "order" in tables else None
    ind = N.int_array([1] * (PP * dd - 1) + [2 if ind_bad else 1]) if "ind" in tables else None
    coef = N.double_array([1.0] * (PP * dd)) if "coef" in tables else None
    add = N.double_array([0.0] * (PP * dd)) if "add" in tables else None
    cc = N.double_array([1.0] * PP) if "cc" in tables else None
    p = {k: _p(null == k) for k in _PTRS}
    return (family, p["xt"], N_, p["z"], n, d, P, o, coef, add, ind, cc, tbits, p["hyp"], Gk, p["coeffs"],
            n + 3 if cstride is None else cstride, B, None, beta, p["out"], N_ if ostride is None else ostride, p["work"],
            chunk, None)


def _refused(name, args, why, codes=(-1,)):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = getattr(lib, name)(*args)
    msg = lib.fgp_last_error()
    assert rc in codes, "%s accepted %s (rc = %d)" % (name, why, rc)
    assert msg and msg != before and name.encode() in msg, (name, why, msg)
    return msg


@pytest.mark.parametrize("why,kw,codes,word", [
    ("d = 8", dict(d=8), (-1,), b"d="), ("d = 65", dict(d=65), (-1,), b"d="), ("P = 0", dict(P=0), (-1,), b"P="),
    ("P = 17", dict(P=17), (-2,), b"P="),                    # FGP_ERR_UNSUPPORTED: the rows path covers it
    ("beta = 2", dict(beta=2), (-1,), b"beta"), ("beta = -1", dict(beta=-1), (-1,), b"beta"),
    ("Gk = 2, B = 3", dict(Gk=2), (-1,), b"Gk"), ("Gk = 0", dict(Gk=0), (-1,), b"Gk"),
    ("N < 0", dict(N_=-1), (-1,), b"N="), ("n = 0", dict(n=0), (-1,), b"n="), ("B = 0", dict(B=0, Gk=1), (-1,), b"B="),
    ("chunk = 100", dict(chunk=100), (-1,), b"chunk"), ("chunk < 0", dict(chunk=-256), (-1,), b"chunk"),
    ("coeff_stride < n", dict(cstride=8), (-1,), b"coeff_stride"), ("out_stride < N", dict(ostride=1), (-1,), b"out_stride"),
    ("ind = 2", dict(ind_bad=True), (-1,), b"ind"), ("ind null", dict(tables=("order", "coef", "add", "cc")), (-1,), b"ind"),
    ("cc null", dict(tables=("order", "coef", "add", "ind")), (-1,), b"cc"),
    ("order null", dict(tables=("coef", "add", "ind", "cc")), (-1,), b"order"),
    ("Bernoulli order 0", dict(order=0), (-2,), b"order"), ("Bernoulli order 9", dict(order=9), (-2,), b"order"),
    ("Walsh order 5", dict(order=5, family=1), (-2,), b"order"), ("tbits = 0", dict(order=2, family=1, tbits=0), (-1,), b"tbits"),
    ("tbits = 64", dict(order=2, family=1, tbits=64), (-1,), b"tbits"), ("family = 2", dict(family=2), (-1,), b"family"),
    ("net, add null", dict(order=2, family=1, tables=("order", "coef", "ind", "cc")), (-1,), b"add")])
def test_mt_wide_post_mean_validates_before_any_hip_call(why, kw, codes, word):
    assert word in _refused(ENTRY, _args(**kw), why, codes)


@pytest.mark.parametrize("field", _PTRS)
def test_mt_wide_post_mean_names_the_null_pointer(field):
    msg = _refused(ENTRY, _args(null=field), "null " + field)
    assert b"null pointer (%s)" % field.encode() in msg


def test_mt_wide_post_mean_work_validates():
    out = ctypes.c_int64(0)
    for args, word in (((-1, 16, 1, 0, ctypes.pointer(out)), b"N="), ((1, 0, 1, 0, ctypes.pointer(out)), b"n="),
                       ((1, 16, 0, 0, ctypes.pointer(out)), b"B="), ((1, 16, 1, 255, ctypes.pointer(out)), b"chunk"),
                       ((1, 16, 1, 0, None), b"len")):
        assert word in _refused(WORK, args, word.decode())


def test_no_test_points_is_no_launch():
    """N = 0 returns FGP_OK after the validation, without a HIP call (a machine without a device)."""
    assert N.lib().fgp_mt_wide_post_mean(*_args(N_=0)) == 0


# ------------------------------------------------------------------------------------------ the reference and its bound
def _f64_mean(inp, K, case, drop=None, swap=False):
    """A plain float64 rows @ c, w and beta as the kernel applies them; drop: a training point left out; swap: rows 0
    and 1 of the coefficients exchanged."""
    K64 = PR.to_f64(K)
    c = np.array(inp["coeffs"], dtype=np.float64)
    if swap:
        c[[0, 1]] = c[[1, 0]]
    if drop is not None:
        c[:, drop] = 0.0
    out = np.empty((case.B, case.N))
    for b in range(case.B):
        s = K64[b if case.Gk == case.B else 0] @ c[b]
        v = s if inp["w"] is None else inp["w"][b] * s
        out[b] = v if inp["out0"] is None else inp["out0"][b] + v
    return out


def _ratio(dev, ref, bnd):
    err = abs(PR._x(dev) - ref)
    return float(PR.to_f64(np.where(bnd > 0, err / np.where(bnd > 0, U * bnd, 1), np.where(err > 0, np.inf, 0))).max())


def cap_ok(case, q, Bq):
    """The non-vacuity cap of wide_mt_mean_cases on the arrays used."""
    q, B = np.abs(PR.to_f64(q)), PR.to_f64(Bq)
    if case.kind == "regular":
        return bool((MM.c_mean(case) * U * B <= MM.CAP * q).all())
    return bool(B.max() <= 8 * case.d * q.max())


@pytest.mark.parametrize("name", [c.name for c in MM.CASES])
def test_reference_matches_float64_and_meets_its_cap(name):
    case = MM.BY_NAME[name]
    inp, q, Bq, K, BK = MM.reference(name)
    assert q.shape == (case.B, case.N) and (PR.to_f64(Bq) >= 0).all()
    if case.beta:
        assert (inp["out0"] != 0).all()
    assert cap_ok(case, q, Bq), (name, "cap")
    C = MM.c_mean(case)
    r = _ratio(_f64_mean(inp, K, case), q, Bq)
    print("%-70s float64 err / (2^-53 B) = %6.2f   C = %d" % (name, r, C))
    assert r <= C


def test_c_of_the_default_case():
    assert MM.c_mean(MM.CASES[0]) == 39 and MM.CASES[0].fam == MM.LAT and MM.CASES[0].n == 257


@pytest.mark.parametrize("name", [MM.CASES[0].name, [c.name for c in MM.CASES if c.n == 600][0],
                                  [c.name for c in MM.CASES if c.fam == MM.NET and c.B == 5 and c.Gk == 5][0]])
def test_wrong_accumulations_are_rejected(name):
    case = MM.BY_NAME[name]
    inp, q, Bq, K, BK = MM.reference(name)
    C = MM.c_mean(case)
    last = min(case.n, MM.chunk_of(case)) - 1                  # the last training point of chunk 0
    assert _ratio(_f64_mean(inp, K, case, drop=last), q, Bq) > C
    assert _ratio(_f64_mean(inp, K, case, swap=True), q, Bq) > C
