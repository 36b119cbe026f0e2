"""Parameter batches of the wide multitask fit loop (fgp_wide_mt_fit_batch_desc = fgp_wide_mt_fit_desc followed by G / rows
/ nrows, and the fgp_wide_mt_fit_batch_* entry points, additions to ABI 20), the part that needs no GPU: the descriptor
is mirrored and the one-problem descriptor is untouched, every refusal comes with its status and the field named before
any HIP call, a batch desc with G <= 1 has the work bytes and the 15 offsets of its one-problem descriptor, the G-fold
layout is ascending in 256-byte steps, and fgp_wide_mt_fit_batch_layout places the per-problem totals at its end."""
import ctypes
import os
import re
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


def _make(ns=(64, 8, 8), nrows=None, G=0, **kw):
    """A valid batch descriptor of len(ns) sorted tasks (every pair P = 1), with the given fields replaced."""
    one = _one(ns, **kw)
    bd = N.WideMtFitBatchDesc(one=one, G=G)
    for q, v in enumerate(nrows or ()):
        bd.nrows[q] = v
    return bd


def _one(ns=(64, 8, 8), **kw):
    p = _ptr()
    vals = dict(family=0, d=12, B=1, T_all=len(ns), rank=1, dl=12, y=p, raw=p, vtask_exp=0, rg_scale=1, rg_ls=1,
                rg_noise=0, rg_factor=1, rg_vtask=1, rprop_prev=p, rprop_step=p, lr=0.1, eta_minus=0.5, eta_plus=1.2,
                step_min=1e-6, step_max=50.0, logdet_weight=1.0, mll_const=0.0, loss_hist=p, raw_hist=p, grad_out=p, work=p)
    vals.update(kw)
    desc = N.WideMtFitDesc(**vals)
    desc.layout.T = len(ns)
    for k, v in enumerate(ns):
        desc.layout.n[k] = v
        desc.task[k] = k
    for q in range(len(ns) * (len(ns) + 1) // 2):
        pr = desc.pair[q]
        pr.parts, pr.ind, pr.cc, pr.P, pr.conj = p, ctypes.addressof(_IND), ctypes.addressof(_CC), 1, 0
    return desc


ENTRIES = ["fgp_wide_mt_fit_batch_run", "fgp_wide_mt_fit_batch_work", "fgp_wide_mt_fit_batch_work_layout",
           "fgp_wide_mt_fit_batch_layout", "fgp_wide_mt_fit_batch_stage"]


def test_batch_descriptor_is_mirrored_and_the_entry_points_are_bound():
    assert [f for f, _ in N.WideMtFitBatchDesc._fields_] == ["one", "G", "rows", "nrows"]
    assert N.WideMtFitBatchDesc._fields_[0][1] is N.WideMtFitDesc
    assert "G" not in [f for f, _ in N.WideMtFitDesc._fields_]          # the one-problem descriptor keeps its layout
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    assert "typedef struct fgp_wide_mt_fit_batch_desc" in src
    for name in ENTRIES:
        assert hasattr(ctypes.CDLL(N.LIB_PATH), name), name
        assert name in N._SIGNATURES and getattr(lib, name).argtypes == N._SIGNATURES[name]
        assert ("extern int (%s)(const fgp_wide_mt_fit_batch_desc*" % name) in src
    # the header declares no new unparenthesised name of the task-pair kernel's fixed set
    assert sorted(re.findall(r"extern int (fgp_wide_mt_\w+)\(", src)) == [
        "fgp_wide_mt_k1", "fgp_wide_mt_k1_bwd", "fgp_wide_mt_k1_bwd_work", "fgp_wide_mt_parts", "fgp_wide_mt_rows"]


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof from a gcc probe against the ctypes mirror."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls, cname = N.WideMtFitBatchDesc, "fgp_wide_mt_fit_batch_desc"
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


def test_null_descriptor_and_null_outputs():
    lib = N.lib()
    out = (ctypes.c_int64 * 15)()
    for name in ("fgp_wide_mt_fit_batch_work", "fgp_wide_mt_fit_batch_work_layout", "fgp_wide_mt_fit_batch_layout"):
        assert getattr(lib, name)(None, out) == FGP_ERR_INVALID and name.encode() in lib.fgp_last_error()
        assert getattr(lib, name)(ctypes.byref(_make(G=3)), None) == FGP_ERR_INVALID
    assert lib.fgp_wide_mt_fit_batch_run(None, 0, 1, 0, None) == FGP_ERR_INVALID
    assert lib.fgp_wide_mt_fit_batch_stage(None, 0, 1, 0, None) == FGP_ERR_INVALID
    assert lib.fgp_wide_mt_fit_batch_run(ctypes.byref(_make(G=3)), 0, 0, 0, None) == 0       # no iterations: a no-op


_REFUSALS = [
    ("G", FGP_ERR_INVALID, dict(G=-1)),
    ("nrows[3]", FGP_ERR_INVALID, dict(G=3, nrows=(1, 1, 1, -2, 1))),
    ("nrows[0]", FGP_ERR_INVALID, dict(G=2, nrows=(-1, 1, 1, 1, 1))),
    ("B", FGP_ERR_UNSUPPORTED, dict(G=3, B=2)),
    ("loss_metric", FGP_ERR_UNSUPPORTED, dict(G=3, ns=(64, 64, 64), loss_metric=N.LOSS_GCV)),
    ("loss_metric", FGP_ERR_UNSUPPORTED, dict(G=3, ns=(64, 64, 64), loss_metric=N.LOSS_CV, cv_weight=1.0)),
    ("G", FGP_ERR_UNSUPPORTED, dict(G=4097)),
    ("n_params", FGP_ERR_UNSUPPORTED, dict(G=700, nrows=(1, 700, 1, 1, 1))),          # 700 x 12 lengthscales
    ("nrows[1]", FGP_ERR_INVALID, dict(G=1, nrows=(1, 2, 1, 1, 1))),                  # one problem, two rows
]


@pytest.mark.parametrize("field,status,kw", _REFUSALS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_name_the_field_before_any_hip_call(entry, field, status, kw):
    lib = N.lib()
    lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
    before = lib.fgp_last_error()
    desc = _make(**kw)
    out = (ctypes.c_int64 * 15)()
    if entry == "fgp_wide_mt_fit_batch_run":
        rc = lib.fgp_wide_mt_fit_batch_run(ctypes.byref(desc), 0, 1, 0, None)
    elif entry == "fgp_wide_mt_fit_batch_stage":
        rc = lib.fgp_wide_mt_fit_batch_stage(ctypes.byref(desc), 0, 1, 0, None)
    else:
        rc = getattr(lib, entry)(ctypes.byref(desc), out)
    msg = lib.fgp_last_error()
    assert rc == status, (field, rc, msg)
    assert msg != before and entry.encode() in msg and field.encode() in msg, (field, msg)


def test_caps_are_inclusive():
    lib = N.lib()
    out = ctypes.c_int64(0)
    assert lib.fgp_wide_mt_fit_batch_work(ctypes.byref(_make(ns=(8, 8), G=4096)), ctypes.byref(out)) == 0
    # 8192 raw elements exactly: 682 lengthscale rows of 12, and the other blocks make up the rest
    d = _make(ns=(8, 8), G=682, nrows=(1, 682, 3, 1, 1))
    assert 1 + 682 * 12 + 3 + 2 + 2 == 8192
    assert lib.fgp_wide_mt_fit_batch_work(ctypes.byref(d), ctypes.byref(out)) == 0
    d.nrows[2] = 4
    assert lib.fgp_wide_mt_fit_batch_work(ctypes.byref(d), ctypes.byref(out)) == FGP_ERR_UNSUPPORTED


def _layout(desc):
    lib = N.lib()
    tot, offs, bl, ll = ctypes.c_int64(0), (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
    assert lib.fgp_wide_mt_fit_batch_work(ctypes.byref(desc), ctypes.byref(tot)) == 0
    assert lib.fgp_wide_mt_fit_batch_work_layout(ctypes.byref(desc), offs) == 0
    assert lib.fgp_wide_mt_fit_batch_layout(ctypes.byref(desc), bl) == 0
    return tot.value, list(offs), list(bl)


def _layout_one(desc):
    """The one-problem entry points on a one-problem descriptor."""
    lib = N.lib()
    tot, offs, ll = ctypes.c_int64(0), (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 2)()
    assert lib.fgp_wide_mt_fit_work(ctypes.byref(desc), ctypes.byref(tot)) == 0
    assert lib.fgp_wide_mt_fit_work_layout(ctypes.byref(desc), offs) == 0
    assert lib.fgp_wide_mt_fit_loss_layout(ctypes.byref(desc), ll) == 0
    return tot.value, list(offs), list(ll)


@pytest.mark.parametrize("fam", [0, 1])
@pytest.mark.parametrize("ns,B,d,dl,loss", [((64, 8, 8), 1, 12, 12, 0), ((4096, 4096), 2, 9, 1, 0),
                                            ((256, 256), 3, 9, 9, N.LOSS_GCV), ((256, 256), 1, 9, 9, N.LOSS_CV)])
def test_one_problem_keeps_its_bytes_and_offsets(fam, ns, B, d, dl, loss):
    """G = 0 and G = 1 (with and without explicit single rows) are the one-problem descriptor through its own entry points
    (any B, any loss)."""
    kw = dict(ns=ns, family=fam, B=B, d=d, dl=dl, loss_metric=loss, cv_weight=1.0)
    tot, offs, _ = _layout_one(_one(**kw))
    for G, nrows in ((0, None), (1, None), (1, (1, 1, 1, 1, 1)), (0, (0, 1, 0, 1, 0))):
        got = _layout(_make(G=G, nrows=nrows, **kw))
        assert got == (tot, offs, [tot, 0]), (G, nrows)             # no totals: an empty place at the end


@pytest.mark.parametrize("fam", [0, 1])
def test_three_problems_layout(fam):
    ns, d, dl, G, T, rank = (512, 256), 9, 9, 3, 2, 2
    desc = _make(ns=ns, family=fam, d=d, dl=dl, rank=rank, G=G, nrows=(3, 1, 3, 1, 1))
    tot, offs, bl = _layout(desc)
    assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs == sorted(offs)
    npairs, L, nbx = 3, 512 * 2 + 256, 2
    esz = 16 if fam == 0 else 8
    al = lambda b: (b + 255) // 256 * 256
    sizes = [8 * G * (1 + d), 8 * 2 * G, 4, 8 * npairs * G * (1 + d), 8 * G * L, esz * G * L, 16 * G * L if fam == 0 else 0,
             16 * G * L, 16 * G * L, 16 * G * L, 16 * G * L, 16 * G * sum(ns), 8 * G * ns[-1], 8 * G * (npairs + 1) * 2 * nbx,
             8 * G * (1 + d) * nbx]
    expect = [0]
    for b in sizes:
        expect.append(expect[-1] + al(b))
    assert offs == expect[:15]
    P1 = 2 + dl + T * rank + T
    assert bl == [expect[15], 8 * G * (2 + P1)]
    assert al(bl[0] + bl[1]) == tot
    assert tot > 2 * _layout_one(_one(ns=ns, family=fam, d=d, dl=dl, rank=rank))[0]
