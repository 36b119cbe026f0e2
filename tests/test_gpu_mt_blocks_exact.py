"""The block entry points on the device -- fgp_mt_factor (k_mt_ldl), fgp_mt_solve, fgp_mt_selinv, fgp_mt_mll_grad --
against the extended-precision reference within the derived bound (tests/mt_block_reference.py: every rounding of the
kernels counted into the bound, nothing fitted), stage by stage: each stage's reference takes the previous stage's
output as the device produced it.  Lattice (complex blocks) and net (real blocks)."""
import functools

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from tests import mt_block_reference as R
from tests.gpu_fixtures import DEV
from tests.mt_block_cases import CASE_IDS, CASES, case_inputs
from tests.mt_qf_cases import FAMILIES, make_lams, make_vectors

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)


def mll_grad(lay, zinv, z, gn, gl):
    """fgp_mt_mll_grad: zinv [G, L], z [B, R nmin], gn [B], gl [G] on the device -> glp [G, L]."""
    glp = torch.empty_like(zinv)
    N.call("fgp_mt_mll_grad", N.byref_layout(lay), N.ptr(zinv), N.ptr(z), N.ptr(gn), N.ptr(gl), z.shape[0], zinv.shape[0],
           N.ptr(glp), N.stream_ptr(zinv.device))
    return glp


def diag_mask(ns):
    lay = R.Layout(ns)
    m = np.zeros(lay.L, dtype=bool)
    for k in range(lay.T):
        m[lay.off[k, k]:lay.off[k, k] + lay.ns[k]] = True
    return m


def device_stages(ns, lams, v, gn, gl):
    """Every stage on the device, as numpy: fac, logdet, info, z, zinv, glp."""
    lay = ops.mt_layout(ns)
    fac, ld, info = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
    z = ops.mt_solve(lay, fac, torch.from_numpy(v).to(DEV))
    zinv = ops.mt_selinv(lay, fac)
    glp = mll_grad(lay, zinv, z, torch.from_numpy(gn).to(DEV), torch.from_numpy(gl).to(DEV))
    return {"fac": fac.cpu().numpy(), "logdet": ld.cpu().numpy(), "info": int(info.item()), "z": z.cpu().numpy(),
            "zinv": zinv.cpu().numpy(), "glp": glp.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def _run(name, family):
    """The device's stages, max err / bound per stage and the factor's reference: computed once, shared by the tests."""
    case = CASES[CASE_IDS.index(name)]
    _, ns, G, B, _ = case
    lams, v, gn, gl = case_inputs(case, family)
    dev = device_stages(ns, lams, v, gn, gl)
    rs, f = R.block_stage_ratios(dev, lams, v, gn, gl, ns, G)
    return dev, rs, f


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", CASE_IDS)
def test_every_stage_within_its_derived_bound(name, family):
    dev, rs, f = _run(name, family)
    _, ns, G, B, _ = CASES[CASE_IDS.index(name)]
    print("%s/%s: max err / bound: %s" % (name, family, ", ".join("%s %.3g" % kv for kv in rs.items())))
    for st in ("fac", "logdet", "z", "zinv", "glp"):
        assert np.isfinite(dev[st]).all(), st
    assert dev["info"] == 0 and f["info"] == 0
    dm = diag_mask(ns)
    for st in ("fac", "zinv", "glp"):
        assert (dev[st].reshape(G, -1)[:, dm].imag == 0).all(), "%s: a diagonal entry with an imaginary part" % st
    for st, r in rs.items():
        assert r <= 1.0, (st, r)


def test_the_pivots_of_the_scaled_case_are_tiny():
    dev, _, _ = _run("tiny_pivots", "lattice")
    ns = CASES[CASE_IDS.index("tiny_pivots")][1]
    assert float(np.max(np.abs(dev["fac"][0][diag_mask(ns)]))) < 2.0 ** -30


@pytest.mark.parametrize("family", FAMILIES)
def test_solve_with_a_padded_row_stride(family):
    """v_row_stride = R nmin + 3, the padding NaN: the bits of the unpadded call."""
    ns = [256, 64, 8]
    lay = ops.mt_layout(ns)
    lams = make_lams(ns, 1, family, 1.0, 91)
    v = torch.from_numpy(make_vectors(ns, 3, family, 92).astype(np.complex128)).to(DEV)
    fac, _, _ = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
    big = torch.full((3, v.shape[1] + 3), float("nan"), dtype=torch.complex128, device=DEV)
    big[:, :v.shape[1]] = v
    view = big[:, :v.shape[1]]
    assert view.stride(0) == v.shape[1] + 3
    z_pad = ops.mt_solve(lay, fac, view)
    z = ops.mt_solve(lay, fac, v)
    assert torch.isfinite(torch.view_as_real(z_pad)).all()
    assert torch.equal(torch.view_as_real(z_pad), torch.view_as_real(z))
    ref = R.solve_ref(fac.cpu().numpy(), ns, v.cpu().numpy(), 1)
    r = R.complex_ratio(z_pad.cpu().numpy(), ref, R.counts(ns)["solve"])
    print("stride_pad/%s: max err / bound: z %.3g" % (family, r))
    assert r <= 1.0


def test_solve_of_no_vectors_is_ok_and_writes_nothing():
    ns = [256, 64, 8]
    lay = ops.mt_layout(ns)
    fac, _, _ = ops.mt_factor(lay, torch.from_numpy(make_lams(ns, 1, "lattice", 1.0, 93)).to(DEV))
    v = torch.from_numpy(make_vectors(ns, 1, "lattice", 94)).to(DEV)
    out = torch.full_like(v, 7.0)
    rc = N.lib().fgp_mt_solve(N.byref_layout(lay), N.ptr(fac), 1, N.ptr(v), v.shape[1], 0, N.ptr(out), N.stream_ptr(v.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out == 7.0).all())


def test_a_negative_pivot_is_flagged_and_its_class_alone_changes():
    """The diagonal of the last task negative in one class: info == 1, that class's logdet the sum of log|pivot|, every
    other class bit for bit as without the edit.  An ordinary input: nothing faults."""
    ns, j0 = [256, 64, 8], 5
    layr = R.Layout(ns)
    lay = ops.mt_layout(ns)
    lams = make_lams(ns, 1, "lattice", 1.0, 95)
    edited = lams.copy()
    edited[0, layr.off[2, 2] + j0] = -3.0
    fac0, ld0, info0 = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
    fac1, ld1, info1 = ops.mt_factor(lay, torch.from_numpy(edited).to(DEV))
    assert int(info0.item()) == 0 and int(info1.item()) == 1
    f = R.factor_ref(edited, ns, 1)
    assert f["info"] == 1 and f["bad"][0, j0] and f["bad"].sum() == 1
    C = R.counts(ns)["factor"]
    ld1 = ld1.cpu().numpy()
    assert np.isfinite(ld1).all()
    r = R.ratio(ld1[0, j0], f["logdet"][0, j0], f["logdet_e"][0, j0], C)
    rf = R.complex_ratio(fac1.cpu().numpy(), (f["fac_x"], f["fac_y"], f["ex"], f["ey"]), C)
    print("negative_pivot: max err / bound: logdet %.3g, fac %.3g" % (r, rf))
    assert r <= 1.0 and rf <= 1.0
    others = np.arange(layr.nmin) != j0
    assert np.array_equal(ld1[0, others], ld0.cpu().numpy()[0, others])
    rows = lambda t: t.cpu().numpy().reshape(-1, layr.nmin)      # noqa: E731  (a class is a column)
    assert np.array_equal(rows(fac1)[:, others], rows(fac0)[:, others])
    assert not np.array_equal(rows(fac1)[:, j0], rows(fac0)[:, j0])
