"""fgp_wide_fit_work / fgp_wide_fit_run (the device-resident fit loop of wide GPs, an addition to ABI 20), the part
that needs no GPU: the symbols are exported and bound, fgp_wide_fit_desc has the layout of its ctypes mirror, and every
argument error is refused with FGP_ERR_INVALID and a message naming the field before any HIP call."""
import ctypes
import os
import shutil
import subprocess

import pytest

from fastgaussianprocesses_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FGP_ERR_INVALID = -1          # include/fgp_hip.h

_BUF = (ctypes.c_double * 4096)()    # host memory standing in for device memory: a refused call never reads it


def _ptr():
    addr = ctypes.addressof(_BUF)
    return addr + (-addr) % 16


def _desc(**kw):
    p = _ptr()
    vals = dict(family=0, log2n=4, d=12, G=2, parts=p, parts_stride=0, ysq=p, raw=p, dl=12, scale_rg=1, ls_rg=1,
                noise_rg=0, logdet_weight=1.0, mll_const=0.0, rprop_prev=p, rprop_step=p, lr=0.1, eta_minus=0.5,
                eta_plus=1.2, step_min=1e-6, step_max=50.0, loss_hist=p, raw_hist=p, grad_out=p, work=p)
    vals.update(kw)
    return N.WideFitDesc(**vals)


def test_symbols_exported_and_bound_and_abi_still_20():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    for name in ("fgp_wide_fit_work", "fgp_wide_fit_run"):
        assert hasattr(ctypes.CDLL(N.LIB_PATH), name), "libfgp_hip.so does not export %s" % name
        assert name in N._SIGNATURES and name in N.exported_symbols()
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]
        assert ("int %s(" % name) in src, "include/fgp_hip.h does not declare %s" % name
    assert "typedef struct fgp_wide_fit_desc" in src


def test_wide_fit_desc_layout_matches_header(tmp_path):
    """sizeof / offsetof of fgp_wide_fit_desc from a gcc probe against the ctypes mirror."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgp_hip.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(fgp_wide_fit_desc));']
    expect = [ctypes.sizeof(N.WideFitDesc)]
    for fname, _ in N.WideFitDesc._fields_:
        lines.append('printf("%%zu\\n", offsetof(fgp_wide_fit_desc, %s));' % fname)
        expect.append(getattr(N.WideFitDesc, fname).offset)
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == expect


_POINTERS = ["parts", "ysq", "raw", "rprop_prev", "rprop_step", "loss_hist", "raw_hist", "grad_out", "work"]


@pytest.mark.parametrize("field,kw,iters", [
    ("d", dict(d=8, dl=8), 1), ("d", dict(d=65, dl=65), 1), ("log2n", dict(log2n=-1), 1), ("log2n", dict(log2n=25), 1),
    ("G", dict(G=0), 1), ("dl", dict(dl=2), 1), ("dl", dict(dl=0), 1), ("iters", dict(), -1)]
    + [(name, {name: None}, 1) for name in _POINTERS])
def test_run_validates_before_any_hip_call(field, kw, iters):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    rc = lib.fgp_wide_fit_run(ctypes.byref(_desc(**kw)), 0, iters, 0, None)
    msg = lib.fgp_last_error()
    assert rc == FGP_ERR_INVALID, (field, rc)
    assert msg != before and b"fgp_wide_fit_run" in msg and field.encode() in msg, (field, msg)


@pytest.mark.parametrize("field,kw", [("d", dict(d=8, dl=8)), ("d", dict(d=65, dl=65)), ("log2n", dict(log2n=25)),
                                      ("G", dict(G=0)), ("dl", dict(dl=3))])
def test_work_validates_sizes(field, kw):
    lib = N.lib()
    out = ctypes.c_int64(-1)
    rc = lib.fgp_wide_fit_work(ctypes.byref(_desc(**kw)), ctypes.byref(out))
    assert rc == FGP_ERR_INVALID and b"fgp_wide_fit_work" in lib.fgp_last_error() and \
        field.encode() in lib.fgp_last_error()
    assert lib.fgp_wide_fit_work(ctypes.byref(_desc()), None) == FGP_ERR_INVALID
    assert lib.fgp_wide_fit_work(None, ctypes.byref(out)) == FGP_ERR_INVALID


def test_work_length_covers_every_buffer():
    """k1 / u [G, n], lambda / g~ [G, n] (complex for lattices) and the lattice transforms' scratch, the natural and
    gradient rows, the partials of the eigenvalue-terms kernel and of fgp_wide_k1_bwd."""
    lib = N.lib()
    for fam, cplx in ((0, 2), (1, 1)):
        for m, G, d in ((4, 1, 9), (13, 5, 12), (17, 2, 64)):
            n = 1 << m
            out, bwd = ctypes.c_int64(0), ctypes.c_int64(0)
            assert lib.fgp_wide_fit_work(ctypes.byref(_desc(family=fam, log2n=m, G=G, d=d, dl=d)), ctypes.byref(out)) == 0
            assert lib.fgp_wide_k1_bwd_work(n, d, G, ctypes.byref(bwd)) == 0
            need = G * n * (1 + cplx + (2 if fam == 0 else 0)) + 2 * G * (1 + d) + 3 * G * ((n + 2047) // 2048) + bwd.value
            assert need <= out.value <= need + 16, (fam, m, G, d, out.value, need)


def test_zero_iterations_is_a_no_op_without_a_device():
    assert N.lib().fgp_wide_fit_run(ctypes.byref(_desc()), 0, 0, 0, None) == 0
