"""fgp_wide_mt_fit_work / fgp_wide_mt_fit_run (the device-resident fit loop of multitask / derivative-informed GPs on
wide inputs, an addition to ABI 20), the part that needs no GPU: the symbols are exported and bound, fgp_wide_mt_fit_desc
and fgp_wide_mt_pair have the layout of their ctypes mirrors, and every argument error is refused with its status and a
message naming the field before any HIP call."""
import ctypes
import os
import shutil
import subprocess

import pytest

from fastgaussianprocesses_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FGP_ERR_INVALID, FGP_ERR_UNSUPPORTED = -1, -2          # include/fgp_hip.h

_BUF = (ctypes.c_double * 4096)()    # host memory standing in for device memory: a refused call never reads it
_IND = (ctypes.c_int * (16 * 64))(*([1] * (16 * 64)))
_CC = (ctypes.c_double * 16)(*([1.0] * 16))


def _ptr():
    addr = ctypes.addressof(_BUF)
    return addr + (-addr) % 16


def _make(ns=(64, 8, 8), pair_kw=None, T=None, **kw):
    """A valid descriptor of len(ns) sorted tasks (every pair P = 1), with the given fields / pair fields replaced."""
    p = _ptr()
    vals = dict(family=0, d=12, B=1, T_all=len(ns), rank=1, dl=12, y=p, raw=p, vtask_exp=0, rg_scale=1, rg_ls=1,
                rg_noise=0, rg_factor=1, rg_vtask=1, rprop_prev=p, rprop_step=p, lr=0.1, eta_minus=0.5, eta_plus=1.2,
                step_min=1e-6, step_max=50.0, logdet_weight=1.0, mll_const=0.0, loss_hist=p, raw_hist=p, grad_out=p, work=p)
    vals.update(kw)
    desc = N.WideMtFitDesc(**vals)
    desc.layout.T = len(ns) if T is None else T
    for k, v in enumerate(ns):
        desc.layout.n[k] = v
        desc.task[k] = k
    for q in range(len(ns) * (len(ns) + 1) // 2):
        pr = desc.pair[q]
        pr.parts, pr.ind, pr.cc, pr.P, pr.conj = p, ctypes.addressof(_IND), ctypes.addressof(_CC), 1, 0
        for name, val in (pair_kw or {}).get(q, {}).items():
            setattr(pr, name, val)
    return desc


def test_symbols_exported_and_bound_and_abi_still_20():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    for name in ("fgp_wide_mt_fit_work", "fgp_wide_mt_fit_run"):
        assert hasattr(ctypes.CDLL(N.LIB_PATH), name), "libfgp_hip.so does not export %s" % name
        assert name in N._SIGNATURES and name in N.exported_symbols()
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]
        assert ("extern int (%s)(" % name) in src, "include/fgp_hip.h does not declare %s extern" % name
    assert "typedef struct fgp_wide_mt_fit_desc" in src and "typedef struct fgp_wide_mt_pair" in src


@pytest.mark.parametrize("cname,mirror", [("fgp_wide_mt_fit_desc", "WideMtFitDesc"), ("fgp_wide_mt_pair", "WideMtPair")])
def test_struct_layouts_match_header(tmp_path, cname, mirror):
    """sizeof / offsetof from a gcc probe against the ctypes mirror."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = getattr(N, mirror)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgp_hip.h"', "int main(void) {",
             'printf("%%zu\\n", sizeof(%s));' % cname]
    expect = [ctypes.sizeof(cls)]
    for fname, _ in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
        expect.append(getattr(cls, fname).offset)
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == expect
    assert len(N.WideMtFitDesc().pair) == 16 * 17 // 2


_POINTERS = ["y", "raw", "rprop_prev", "rprop_step", "loss_hist", "raw_hist", "grad_out", "work"]

_CASES = [
    ("d", FGP_ERR_INVALID, dict(d=8, dl=8), 1), ("d", FGP_ERR_INVALID, dict(d=65, dl=65), 1),
    ("T", FGP_ERR_INVALID, dict(T=0), 1), ("T", FGP_ERR_INVALID, dict(T=17), 1),
    ("n[1]", FGP_ERR_INVALID, dict(ns=(64, 24, 8)), 1),                     # not a power of two
    ("n[2]", FGP_ERR_INVALID, dict(ns=(64, 8, 16)), 1),                     # not descending
    ("n[0]", FGP_ERR_INVALID, dict(ns=(0,)), 1),
    ("B", FGP_ERR_INVALID, dict(B=0), 1),
    ("dl", FGP_ERR_INVALID, dict(dl=2), 1), ("dl", FGP_ERR_INVALID, dict(dl=0), 1),
    ("rank", FGP_ERR_INVALID, dict(rank=-1), 1),
    ("iters", FGP_ERR_INVALID, dict(), -1),
    ("pair[4].P", FGP_ERR_UNSUPPORTED, dict(pair_kw={4: dict(P=17)}), 1),
    ("pair[1].parts", FGP_ERR_INVALID, dict(pair_kw={1: dict(parts=None)}), 1),
    ("pair[2].ind", FGP_ERR_INVALID, dict(pair_kw={2: dict(ind=None)}), 1),
    ("pair[5].cc", FGP_ERR_INVALID, dict(pair_kw={5: dict(cc=None)}), 1),
] + [(name, FGP_ERR_INVALID, {name: None}, 1) for name in _POINTERS]


@pytest.mark.parametrize("field,status,kw,iters", _CASES)
def test_run_validates_before_any_hip_call(field, status, kw, iters):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = lib.fgp_wide_mt_fit_run(ctypes.byref(_make(**kw)), 0, iters, 0, None)
    msg = lib.fgp_last_error()
    assert rc == status, (field, rc, msg)
    assert msg != before and b"fgp_wide_mt_fit_run" in msg and field.encode() in msg, (field, msg)


@pytest.mark.parametrize("field,status,kw", [(f, s, k) for f, s, k, it in _CASES[:11] + _CASES[12:13]])
def test_work_validates_sizes(field, status, kw):
    lib = N.lib()
    out = ctypes.c_int64(-1)
    rc = lib.fgp_wide_mt_fit_work(ctypes.byref(_make(**kw)), ctypes.byref(out))
    assert rc == status and b"fgp_wide_mt_fit_work" in lib.fgp_last_error() and field.encode() in lib.fgp_last_error()
    assert lib.fgp_wide_mt_fit_work(ctypes.byref(_make()), None) == FGP_ERR_INVALID
    assert lib.fgp_wide_mt_fit_work(None, ctypes.byref(out)) == FGP_ERR_INVALID


def test_work_bytes_cover_every_buffer():
    """k1 / u [L], lambda / g~ [L] (complex for lattices) and the lattice transforms' scratch, the four packed complex
    arrays of the block kernels, the B solutions, the classes' logdet, the contraction's partials, fgp_wide_mt_k1_bwd's
    partials and per-pair results, the natural row and the constant gradient rows."""
    lib = N.lib()
    for fam in (0, 1):
        for ns, B, d in (((64, 8, 8), 1, 12), ((4096, 4096), 2, 9), ((1 << 17, 256, 1), 1, 64)):
            T = len(ns)
            npairs = T * (T + 1) // 2
            L = sum(ns[k] * (T - k) for k in range(T))
            nbx = (ns[0] + 255) // 256
            out, bwd = ctypes.c_int64(0), ctypes.c_int64(0)
            assert lib.fgp_wide_mt_fit_work(ctypes.byref(_make(ns=ns, family=fam, B=B, d=d, dl=d)), ctypes.byref(out)) == 0
            assert lib.fgp_wide_mt_k1_bwd_work(ns[0], d, 1, 1, ctypes.byref(bwd)) == 0
            need = 8 * L * (1 + (2 if fam == 0 else 1) + (2 if fam == 0 else 0)) + 4 * 16 * L + 16 * B * sum(ns) \
                + 8 * ns[-1] + 8 * 2 * (npairs + 1) * nbx + 8 * bwd.value + 8 * npairs * (1 + d) + 8 * (1 + d) + 8 * (B + 1) + 4
            assert need <= out.value <= need + 15 * 256, (fam, ns, out.value, need)


def test_zero_iterations_is_a_no_op_without_a_device():
    assert N.lib().fgp_wide_mt_fit_run(ctypes.byref(_make()), 0, 0, 0, None) == 0
