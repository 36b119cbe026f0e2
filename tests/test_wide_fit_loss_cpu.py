"""fgp_wide_fit_desc.loss_metric / cv_weight (the GCV and CV losses of the device-resident fit loop of wide GPs, still
ABI 20), the part that needs no GPU: the two trailing fields sit where a gcc probe of the header puts them, a
loss_metric outside the three and a non-finite cv_weight under CV are refused by both entry points with the field named
before any HIP call, the GCV / CV workspace holds the extra partials and the MLL's is the one of a zeroed field."""
import ctypes
import math
import os
import shutil
import subprocess

import pytest

from fastgaussianprocesses_amd import _native as N
from tests.test_wide_fit_cpu import FGP_ERR_INVALID, ROOT, _desc


def test_abi_is_still_20_and_the_loss_constants_match_the_header():
    assert N.lib().fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    for name, val in (("FGP_LOSS_MLL", N.LOSS_MLL), ("FGP_LOSS_GCV", N.LOSS_GCV), ("FGP_LOSS_CV", N.LOSS_CV)):
        assert ("#define %s %d" % (name, val)) in src
    assert N.LOSS_MLL == 0, "a zeroed loss_metric must mean the MLL"


def test_new_fields_trail_the_desc_at_the_header_offsets(tmp_path):
    names = [f for f, _ in N.WideFitDesc._fields_]
    assert names[-2:] == ["loss_metric", "cv_weight"] and names[-3] == "work"
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgp_hip.h"', "int main(void) {",
             'printf("%zu %zu %zu %zu\\n", sizeof(fgp_wide_fit_desc), offsetof(fgp_wide_fit_desc, work),',
             '       offsetof(fgp_wide_fit_desc, loss_metric), offsetof(fgp_wide_fit_desc, cv_weight));',
             "return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = N.WideFitDesc
    assert got == [ctypes.sizeof(D), D.work.offset, D.loss_metric.offset, D.cv_weight.offset]
    assert D.work.offset < D.loss_metric.offset < D.cv_weight.offset


@pytest.mark.parametrize("field,kw", [
    ("loss_metric", dict(loss_metric=3)), ("loss_metric", dict(loss_metric=-1)),
    ("cv_weight", dict(loss_metric=N.LOSS_CV, cv_weight=math.nan)),
    ("cv_weight", dict(loss_metric=N.LOSS_CV, cv_weight=math.inf))])
def test_both_entry_points_refuse_and_name_the_field(field, kw):
    lib = N.lib()
    out = ctypes.c_int64(-1)
    for fn, call in (("fgp_wide_fit_work", lambda d: lib.fgp_wide_fit_work(ctypes.byref(d), ctypes.byref(out))),
                     ("fgp_wide_fit_run", lambda d: lib.fgp_wide_fit_run(ctypes.byref(d), 0, 1, 0, None))):
        lib.fgp_wall_clock_khz(0, None)                      # (leaves another message behind)
        before = lib.fgp_last_error()
        rc = call(_desc(**kw))
        msg = lib.fgp_last_error()
        assert rc == FGP_ERR_INVALID, (fn, field, rc)
        assert msg != before and fn.encode() in msg and field.encode() in msg, (fn, field, msg)
    assert out.value == -1


def test_cv_weight_is_only_looked_at_under_cv():
    lib = N.lib()
    out = ctypes.c_int64(-1)
    for metric in (N.LOSS_MLL, N.LOSS_GCV):
        assert lib.fgp_wide_fit_work(ctypes.byref(_desc(loss_metric=metric, cv_weight=math.nan)), ctypes.byref(out)) == 0
    assert lib.fgp_wide_fit_run(ctypes.byref(_desc(loss_metric=N.LOSS_CV, cv_weight=0.5)), 0, 0, 0, None) == 0


def _work(**kw):
    out = ctypes.c_int64(-1)
    assert N.lib().fgp_wide_fit_work(ctypes.byref(_desc(**kw)), ctypes.byref(out)) == 0
    return out.value


def test_work_lengths():
    """MLL: the length of a desc whose new fields are left at zero (a caller from before them).  GCV / CV: at least the
    MLL's plus the four rows of partials (N1, T, S1, S2) per problem and 2048-frequency workgroup."""
    for fam in (0, 1):
        for m, G, d in ((4, 1, 9), (13, 5, 12), (17, 2, 64), (20, 1, 16)):
            geo = dict(family=fam, log2n=m, G=G, d=d, dl=d)
            zeroed = N.WideFitDesc()
            for name, _ in N.WideFitDesc._fields_[:-2]:
                setattr(zeroed, name, getattr(_desc(**geo), name))
            assert zeroed.loss_metric == 0 and zeroed.cv_weight == 0.0
            out = ctypes.c_int64(-1)
            assert N.lib().fgp_wide_fit_work(ctypes.byref(zeroed), ctypes.byref(out)) == 0
            mll = _work(loss_metric=N.LOSS_MLL, cv_weight=1.0, **geo)
            assert mll == out.value
            extra = 4 * G * (((1 << m) + 2047) // 2048)
            for metric in (N.LOSS_GCV, N.LOSS_CV):
                got = _work(loss_metric=metric, cv_weight=0.5, **geo)
                assert mll + extra <= got <= mll + extra + 2, (fam, m, G, d, metric, got, mll, extra)
