"""The d <= 8 multitask prediction kernels (fgp_mt_rows, fgp_mt_post_mean_work, fgp_mt_post_mean; csrc/fgp_mt_pred.hip),
the part that needs no GPU:

  * the three entry points are declared in include/fgp_hip.h as plain `extern int`, bound in _native._SIGNATURES and
    exported, at ABI 20;
  * the work length for hand-computed sizes and for every case;
  * every refusal reaches fgp_last_error() before any HIP call (a machine without a device) and names the argument: d = 0
    and 9, P = 0 and 17, negative sizes, null pointers by field name, tbits outside 1 .. 63 for nets, an ind entry of 2,
    Gk outside {1, B}, beta outside {0, 1}, a bad chunk, a row stride below its row, an order outside its range; N = 0
    is no launch;
  * the rounding counts of tests/mt_pred_cases.py for hand-computed cases, and both non-vacuity caps on every case: the
    reference agrees with a plain float64 evaluation to the bound, and a deliberately wrong evaluation is rejected;
  * host routing with the library stubbed: a task-pair block at d <= 8 takes the fused rows by default and the parts +
    torch formulation under FGP_MT_FUSED_ROWS=0, under an autograd graph, with more than 16 multi-index pairs and for
    integer net inputs; _wide_pair_spec stays None at d <= 8 (the first column and the fit are the wide routes' own).
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from fastgaussianprocesses_amd.multitask import MultiTaskFastGP
from tests import mt_pred_cases as NC
from tests import predict_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, MEAN, WORK = "fgp_mt_rows", "fgp_mt_post_mean", "fgp_mt_post_mean_work"


# ------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^\s*extern\s+int\s+(fgp_mt_rows|fgp_mt_post_mean\w*)\s*\(", src, flags=re.M))
    assert declared == {ROWS, MEAN, WORK}
    for name, nargs in ((ROWS, 18), (MEAN, 25), (WORK, 5)):
        assert name in N._SIGNATURES and len(N._SIGNATURES[name]) == nargs
        assert hasattr(lib, name), "libfgp_hip.so does not export %s" % name
        assert name in N.exported_symbols()
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]
    # the same argument lists as the wide counterparts
    assert N._SIGNATURES[ROWS] == N._SIGNATURES["fgp_wide_mt_rows"]
    assert N._SIGNATURES[MEAN] == N._SIGNATURES["fgp_mt_wide_post_mean"]
    assert N._SIGNATURES[WORK] == N._SIGNATURES["fgp_mt_wide_post_mean_work"]


def test_work_length():
    out = ctypes.c_int64(0)
    lib = N.lib()
    # B min(N, 65535) ceil(n / chunk): 5 x 300 x ceil(66048 / 1024 = 64.5); 2 x 65535 x ceil(1000 / 256)
    assert lib.fgp_mt_post_mean_work(300, 66048, 5, 0, ctypes.pointer(out)) == 0 and out.value == 5 * 300 * 65
    assert lib.fgp_mt_post_mean_work(100000, 1000, 2, 256, ctypes.pointer(out)) == 0 and out.value == 2 * 65535 * 4
    assert lib.fgp_mt_post_mean_work(0, 1, 1, 0, ctypes.pointer(out)) == 0 and out.value == 1
    for case in NC.PM_CASES:
        assert lib.fgp_mt_post_mean_work(case.N, case.n, case.B, case.chunk, ctypes.pointer(out)) == 0
        assert out.value == NC.work_len(case)


# host buffers standing in for device memory: a call that fails validation never reads them
_BUF = (ctypes.c_double * 4096)()
_MEAN_PTRS = ("xt", "z", "hyp", "coeffs", "out", "work")
_ROWS_PTRS = ("xt", "z", "hyp", "rows")


def _p(null=False):
    return ctypes.c_void_p(None if null else ctypes.addressof(_BUF))


def _tables(d, P, order, ind_bad, tables):
    dd, PP = max(1, min(d, 8)), max(1, min(P, 17))
    o = N.int_array([order] * (PP * dd)) if "order" in tables else None
    ind = N.int_array([1] * (PP * dd - 1) + [2 if ind_bad else 1]) if "ind" in tables else None
    coef = N.double_array([1.0] * (PP * dd)) if "coef" in tables else None
    add = N.double_array([0.0] * (PP * dd)) if "add" in tables else None
    cc = N.double_array([1.0] * PP) if "cc" in tables else None
    return o, coef, add, ind, cc


_ALL = ("order", "coef", "add", "ind", "cc")


def _mean_args(d=3, P=2, null=None, order=4, tbits=32, family=0, N_=2, n=16, B=3, Gk=3, beta=1, chunk=0, ind_bad=False,
               cstride=None, ostride=None, tables=_ALL):
    o, coef, add, ind, cc = _tables(d, P, order, ind_bad, tables)
    p = {k: _p(null == k) for k in _MEAN_PTRS}
    return (family, p["xt"], N_, p["z"], n, d, P, o, coef, add, ind, cc, tbits, p["hyp"], Gk, p["coeffs"],
            n + 3 if cstride is None else cstride, B, None, beta, p["out"], N_ if ostride is None else ostride, p["work"],
            chunk, None)


def _rows_args(d=3, P=2, null=None, order=4, tbits=32, family=0, N_=2, n=16, zip_=0, Gk=3, ind_bad=False, tables=_ALL):
    o, coef, add, ind, cc = _tables(d, P, order, ind_bad, tables)
    p = {k: _p(null == k) for k in _ROWS_PTRS}
    return (family, p["xt"], N_, p["z"], n, zip_, d, P, o, coef, add, ind, cc, tbits, p["hyp"], Gk, p["rows"], None)


def _refused(name, args, why, codes=(-1,)):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = getattr(lib, name)(*args)
    msg = lib.fgp_last_error()
    assert rc in codes, "%s accepted %s (rc = %d)" % (name, why, rc)
    assert msg and msg != before and name.encode() in msg, (name, why, msg)
    return msg


_SHARED = [
    ("d = 0", dict(d=0), (-1,), b"d="), ("d = 9", dict(d=9), (-1,), b"d="), ("P = 0", dict(P=0), (-1,), b"P="),
    ("P = 17", dict(P=17), (-2,), b"P="),                    # FGP_ERR_UNSUPPORTED: the torch formulation covers it
    ("N < 0", dict(N_=-1), (-1,), b"N="), ("n = 0", dict(n=0), (-1,), b"n="), ("Gk = 0", dict(Gk=0), (-1,), b"Gk"),
    ("ind = 2", dict(ind_bad=True), (-1,), b"ind"), ("ind null", dict(tables=("order", "coef", "add", "cc")), (-1,), b"(ind)"),
    ("cc null", dict(tables=("order", "coef", "add", "ind")), (-1,), b"(cc)"),
    ("order null", dict(tables=("coef", "add", "ind", "cc")), (-1,), b"(order)"),
    ("coef null", dict(tables=("order", "add", "ind", "cc")), (-1,), b"(coef)"),
    ("Bernoulli order 0", dict(order=0), (-2,), b"order"), ("Bernoulli order 9", dict(order=9), (-2,), b"order"),
    ("Walsh order 5", dict(order=5, family=1), (-2,), b"order"), ("tbits = 0", dict(order=2, family=1, tbits=0), (-1,), b"tbits"),
    ("tbits = 64", dict(order=2, family=1, tbits=64), (-1,), b"tbits"), ("family = 2", dict(family=2), (-1,), b"family"),
    ("net, add null", dict(order=2, family=1, tables=("order", "coef", "ind", "cc")), (-1,), b"(add)")]


@pytest.mark.parametrize("why,kw,codes,word", _SHARED + [
    ("beta = 2", dict(beta=2), (-1,), b"beta"), ("beta = -1", dict(beta=-1), (-1,), b"beta"),
    ("Gk = 2, B = 3", dict(Gk=2), (-1,), b"Gk"), ("B = 0", dict(B=0, Gk=1), (-1,), b"B="),
    ("chunk = 100", dict(chunk=100), (-1,), b"chunk"), ("chunk < 0", dict(chunk=-256), (-1,), b"chunk"),
    ("coeff_stride < n", dict(cstride=8), (-1,), b"coeff_stride"), ("out_stride < N", dict(ostride=1), (-1,), b"out_stride")])
def test_post_mean_validates_before_any_hip_call(why, kw, codes, word):
    assert word in _refused(MEAN, _mean_args(**kw), why, codes)


@pytest.mark.parametrize("why,kw,codes,word", _SHARED + [
    ("N = 65536", dict(N_=65536), (-1,), b"N="), ("zip, N != n", dict(zip_=1, N_=3), (-1,), b"zip")])
def test_rows_validate_before_any_hip_call(why, kw, codes, word):
    assert word in _refused(ROWS, _rows_args(**kw), why, codes)


@pytest.mark.parametrize("field", _MEAN_PTRS)
def test_post_mean_names_the_null_pointer(field):
    assert b"null pointer (%s)" % field.encode() in _refused(MEAN, _mean_args(null=field), "null " + field)


@pytest.mark.parametrize("field", _ROWS_PTRS)
def test_rows_name_the_null_pointer(field):
    assert b"null pointer (%s)" % field.encode() in _refused(ROWS, _rows_args(null=field), "null " + field)


def test_work_validates():
    out = ctypes.c_int64(0)
    for args, word in (((-1, 16, 1, 0, ctypes.pointer(out)), b"N="), ((1, 0, 1, 0, ctypes.pointer(out)), b"n="),
                       ((1, 16, 0, 0, ctypes.pointer(out)), b"B="), ((1, 16, 1, 255, ctypes.pointer(out)), b"chunk"),
                       ((1, 16, 1, 0, None), b"len")):
        assert word in _refused(WORK, args, word.decode())


def test_no_test_points_is_no_launch():
    """N = 0 returns FGP_OK after the validation, without a HIP call (a machine without a device)."""
    assert N.lib().fgp_mt_post_mean(*_mean_args(N_=0)) == 0
    assert N.lib().fgp_mt_rows(*_rows_args(N_=0)) == 0
    for d in range(1, 9):                                            # (every d of the range passes the check of d)
        assert N.lib().fgp_mt_rows(*_rows_args(d=d, N_=0)) == 0 and N.lib().fgp_mt_post_mean(*_mean_args(d=d, N_=0)) == 0


# ------------------------------------------------------------------------------------------ counts and caps
def test_rounding_counts():
    rw = {c.name: c for c in NC.RW_CASES}
    lat = lambda d, P: [c for c in NC.RW_CASES if c.fam == NC.LAT and c.d == d and c.P == P and c.kind == "regular"][0]
    assert NC.c_rows(lat(1, 16)) == 10 + 2 + 17 and NC.c_rows(lat(8, 3)) == 10 + 2 + 1 and NC.c_rows(lat(1, 3)) == 10 + 2 + 4
    assert NC.c_rows(lat(3, 1)) == 10 + 2 + 1 and NC.c_rows(lat(2, 3)) == 10 + 2 + 2
    net63 = [c for c in NC.RW_CASES if c.fam == NC.NET and c.tbits == 63 and c.orders == (4,)][0]
    assert NC.c_rows(net63) == (63 + 4 + 2) + 2 + 1                  # omega_4 at t = 63: t + 4, add, coef
    first = NC.PM_CASES[0]                                           # lattice, d = 1, P = 3, n = 257, the default chunk
    assert (first.fam, first.d, first.P, first.n) == (NC.LAT, 1, 3, 257)
    assert NC.c_mean(first) == 16 + 1 + 2 + 9 + 1 + 9 + 2
    wrap = [c for c in NC.PM_CASES if c.n == 258 * 256][0]
    assert NC.nchunks_of(wrap) == 258 and NC.c_mean(wrap) == NC.c_rows(wrap) + 1 + 1 + 9 + 2 + 9 + 2
    assert len(rw) == len(NC.RW_CASES)


def _f64_rows(case, inp):
    """A plain float64 evaluation of the rows in the kernel's order (ascending j, ascending p, then the scale)."""
    from tests import wide_mt_reference as MR
    xt = inp["xt"]
    x = xt if case.fam == NC.LAT else PR.net_bits(xt, case.tbits).astype(np.int64)
    z = np.ascontiguousarray(np.asarray(inp["z"]).T)
    parts, _ = MR.mt_parts(case.fam, x, z, inp["order"], inp["coef"], inp["add"], case.tbits, case.zip)
    parts = PR.to_f64(parts)                                           # [P, d, E]
    hyp = np.asarray(inp["hyp"])
    out = []
    for g in range(hyp.shape[0]):
        acc = 0.0
        for p in range(case.P):
            pr = 1.0
            for j in range(case.d):
                pr = pr * (inp["ind"][p][j] + hyp[g, 1 + j] * parts[p, j])
            acc = acc + inp["cc"][p] * pr
        out.append(hyp[g, 0] * acc)
    out = np.stack(out)
    return out if case.zip else out.reshape(hyp.shape[0], case.N, case.n)


@pytest.mark.parametrize("name", [c.name for c in NC.RW_CASES])
def test_rows_reference_meets_its_cap_and_matches_float64(name):
    case = NC.RW_BY_NAME[name]
    inp, K, B = NC.rows_reference(name)
    C = NC.c_rows(case)
    fig = NC.cap_figure(case.kind, C, K, B)
    print("%-72s C = %3d   cap figure %.3g" % (name, C, fig))
    assert NC.cap_ok(case.kind, C, K, B), (name, "cap", fig)
    assert NC.ratio(_f64_rows(case, inp), K, B) <= C


def _f64_mean(inp, K, case, drop=None, swap=False):
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


@pytest.mark.parametrize("name", [c.name for c in NC.PM_CASES])
def test_mean_reference_meets_its_cap_and_matches_float64(name):
    case = NC.PM_BY_NAME[name]
    inp, q, Bq, K, BK = NC.mean_reference(name)
    assert q.shape == (case.B, case.N) and (PR.to_f64(Bq) >= 0).all()
    if case.beta:
        assert (inp["out0"] != 0).all()
    C = NC.c_mean(case)
    fig = NC.cap_figure(case.kind, C, q, Bq)
    print("%-72s C = %3d   cap figure %.3g" % (name, C, fig))
    assert NC.cap_ok(case.kind, C, q, Bq), (name, "cap", fig)
    assert NC.ratio(_f64_mean(inp, K, case), q, Bq) <= C


def test_pinned_points_lie_on_training_points():
    """Test points 0 (all 0.0) and 1 (all 1.0) lie on training point 7 (the origin), test point 2 on training point 5."""
    for name in (NC.RW_CASES[2].name, [c.name for c in NC.RW_CASES if c.fam == NC.NET][2]):
        case = NC.RW_BY_NAME[name]
        inp = NC.rows_inputs(case)
        z = np.asarray(inp["z"])
        assert (z[:, 7] == 0).all() and (inp["xt"][0] == 0.0).all() and (inp["xt"][1] == 1.0).all()
        z5 = z[:, 5] if case.fam == NC.LAT else z[:, 5].astype(np.float64) * 2.0 ** -case.tbits
        assert (inp["xt"][2] == z5).all()


@pytest.mark.parametrize("name", [NC.PM_CASES[2].name, [c.name for c in NC.PM_CASES if c.fam == NC.NET and c.B == 5 and c.Gk == 5][0]])
def test_wrong_accumulations_are_rejected(name):
    case = NC.PM_BY_NAME[name]
    inp, q, Bq, K, BK = NC.mean_reference(name)
    C = NC.c_mean(case)
    last = min(case.n, NC.chunk_of(case)) - 1                  # the last training point of chunk 0
    assert NC.ratio(_f64_mean(inp, K, case, drop=last), q, Bq) > C
    assert NC.ratio(_f64_mean(inp, K, case, swap=True), q, Bq) > C


# ------------------------------------------------------------------------------------------ host routing, library stubbed
def test_switch_parsing(monkeypatch):
    monkeypatch.delenv("FGP_MT_FUSED_ROWS", raising=False)
    monkeypatch.setenv("FGP_WIDE_FUSED", "0")                  # (the wide switch does not reach d <= 8, nor this one d > 8)
    assert ops.mt_fused_rows() and ops.mt_pair_fused(3) and not ops.mt_pair_fused(9)
    monkeypatch.delenv("FGP_WIDE_FUSED")
    for value, on in (("0", False), ("1", True), ("", True), ("00", False)):
        monkeypatch.setenv("FGP_MT_FUSED_ROWS", value)
        assert ops.mt_fused_rows() == on and ops.mt_pair_fused(8) == on and ops.mt_pair_fused(9)


class _StandIn(types.SimpleNamespace):
    pass


def _stand_in(d=3, family=ops.LATTICE, derivs=None, requires_grad=False):
    """What _kmat_block reads of a GP, on the CPU: two tasks (f and its first partial derivative by default)."""
    if derivs is None:
        derivs = [torch.zeros((1, d), dtype=torch.int64), torch.eye(d, dtype=torch.int64)[:1]]
    raw = lambda *s: torch.zeros(s, dtype=torch.float64, requires_grad=requires_grad)
    gp = _StandIn(d=d, device=torch.device("cpu"), _FAMILY=family, _alphas=[4] * d, t=32, num_tasks=len(derivs),
                  _derivs_h=derivs, derivatives=derivs, derivatives_coeffs=[torch.ones(len(v), dtype=torch.float64) for v in derivs],
                  raw_scale=raw(1), raw_lengthscales=raw(d), raw_noise=raw(1), raw_factor_task_kernel=raw(2, 1),
                  raw_noise_task_kernel=raw(2), calls=[])
    gp.scale, gp.lengthscales = torch.exp(gp.raw_scale), torch.exp(gp.raw_lengthscales)
    gp._tbits = lambda: 0 if family == ops.LATTICE else 32
    for name in ("_kmat_block", "_fused_pair_spec", "_wide_pair_spec", "_wide_mt_spec", "_pair_spec", "_pair_spec_eval",
                 "_wide_hyp_rows", "_wide_param_rows", "_gradmode", "_hparams", "_kargs"):
        setattr(gp, name, types.MethodType(getattr(MultiTaskFastGP, name), gp))

    def parts_pairs(x, z, b0, b1, zip_pairs=False, check=True):
        gp.calls.append("parts")
        return torch.zeros((x.shape[0], z.shape[0], len(b0), len(b1), d), dtype=torch.float64)

    gp._parts_pairs = parts_pairs
    gp._kernel_from_parts = lambda p, bd0, bd1, c0, c1: p.sum((-1, -2, -3))
    return gp


@pytest.fixture
def stub_rows(monkeypatch):
    seen = []

    def rows(spec, xt, z_dn, hyp, zip_pairs=False):
        seen.append((spec, tuple(xt.shape), tuple(z_dn.shape), tuple(hyp.shape), zip_pairs))
        return torch.zeros((hyp.shape[0], xt.shape[0]) + (() if zip_pairs else (z_dn.shape[1],)), dtype=torch.float64)

    monkeypatch.setattr(ops, "mt_pair_rows", rows)
    monkeypatch.delenv("FGP_MT_FUSED_ROWS", raising=False)
    return seen


def test_block_takes_the_fused_rows_by_default(stub_rows):
    gp = _stand_in()
    x, z = torch.rand(5, 3, dtype=torch.float64), torch.rand(7, 3, dtype=torch.float64)
    with torch.no_grad():
        k = gp._kmat_block(x, z, 0, 1)
    assert k.shape == (5, 7) and gp.calls == [] and len(stub_rows) == 1
    spec, xs, zs, hs, zp = stub_rows[0]
    assert (xs, zs, hs, zp) == ((5, 3), (3, 7), (1, 4), False)         # z dimension-major, hyp [1, 1 + d]
    assert (spec.P, spec.d, spec.family) == (1, 3, ops.LATTICE) and spec.fused
    assert gp._fused_pair_spec(0, 1) is spec and gp._wide_pair_spec(0, 1) is None
    with torch.no_grad():
        assert gp._kmat_block(x, x, 1, 1, zip_pairs=True).shape == (5,) and stub_rows[-1][-1] is True


def test_block_falls_back_to_the_parts(stub_rows, monkeypatch):
    x, z = torch.rand(5, 3, dtype=torch.float64), torch.rand(7, 3, dtype=torch.float64)
    # the switch
    monkeypatch.setenv("FGP_MT_FUSED_ROWS", "0")
    gp = _stand_in()
    with torch.no_grad():
        gp._kmat_block(x, z, 0, 1)
    assert gp.calls == ["parts"] and stub_rows == [] and gp._fused_pair_spec(0, 1) is None
    monkeypatch.delenv("FGP_MT_FUSED_ROWS")
    # an autograd graph: parameters that require gradients, and gradients enabled
    gp = _stand_in(requires_grad=True)
    gp._kmat_block(x, z, 0, 1)
    assert gp.calls == ["parts"] and stub_rows == []
    with torch.no_grad():
        gp._kmat_block(x, z, 0, 1)
    assert gp.calls == ["parts"] and len(stub_rows) == 1
    del stub_rows[:]
    # more than 16 multi-index pairs: 5 x 4 = 20
    many = [torch.zeros((5, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int64)]
    gp = _stand_in(derivs=many)
    with torch.no_grad():
        gp._kmat_block(x, z, 0, 1)
        assert gp.calls == ["parts"] and stub_rows == [] and gp._fused_pair_spec(0, 1) is None
        gp._kmat_block(x, z, 1, 1)                                     # 4 x 4 = 16 pairs: fused
    assert gp.calls == ["parts"] and len(stub_rows) == 1 and stub_rows[0][0].P == 16
    del stub_rows[:]
    # integer (already binary) net inputs
    gp = _stand_in(family=ops.NET)
    xi = torch.randint(0, 2 ** 32, (5, 3), dtype=torch.int64)
    with torch.no_grad():
        gp._kmat_block(xi, z, 0, 1)
        assert gp.calls == ["parts"] and stub_rows == []
        gp._kmat_block(x, xi, 0, 1)                                    # float test points against integer points: fused
    assert gp.calls == ["parts"] and len(stub_rows) == 1 and stub_rows[0][0].tbits == 32
    # an empty task
    with torch.no_grad():
        gp._kmat_block(x, z[:0], 0, 1)
    assert len(stub_rows) == 1


def test_entry_point_follows_d(monkeypatch):
    """ops.mt_pair_rows / mt_pair_post_mean pick fgp_mt_* at d <= 8 and fgp_wide_mt_* above."""
    seen = []
    monkeypatch.setattr(ops, "mt_rows", lambda *a, **k: seen.append("mt_rows"))
    monkeypatch.setattr(ops, "wide_mt_rows", lambda *a, **k: seen.append("wide_mt_rows"))
    monkeypatch.setattr(ops, "mt_post_mean", lambda *a, **k: seen.append("mt_post_mean"))
    monkeypatch.setattr(ops, "mt_wide_post_mean", lambda *a, **k: seen.append("mt_wide_post_mean"))
    for d in (1, 8, 9):
        spec = types.SimpleNamespace(d=d)
        ops.mt_pair_rows(spec, None, None, None)
        ops.mt_pair_post_mean(spec, None, None, None, None, None, None, 0)
    assert seen == ["mt_rows", "mt_post_mean"] * 2 + ["wide_mt_rows", "mt_wide_post_mean"]
