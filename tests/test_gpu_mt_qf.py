"""fgp_mt_quadform on the device: the kernel against the longdouble reference within the derived bound (tests/
mt_qf_reference.py: C counted from the kernel's roundings, never fitted), against Re(v^H fgp_mt_solve(v)), and the bits
of a vector's result whatever else the call holds.  Lattice (complex128 vectors) and net (float64 vectors)."""
import functools

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import ops
from tests import mt_qf_reference as R
from tests.gpu_fixtures import DEV
from tests.mt_qf_cases import CASE_IDS, CASES, FAMILIES, case_inputs, make_lams, make_vectors

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)


def _device_vectors(v, pad):
    """v on the device in rows of R nmin + pad elements (the kernel's v_row_stride)."""
    t = torch.from_numpy(v).to(DEV)
    if pad == 0:
        return t
    big = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _run(name, family):
    """(device q, reference q, B_q, Re(v^H solve(v))) of a case: computed once, shared by the tests."""
    case = CASES[CASE_IDS.index(name)]
    _, ns, G, B, pad, _ = case
    lams, v = case_inputs(case, family)
    lay = ops.mt_layout(ns)
    fac, _, info = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
    assert int(info.item()) == 0, "the seeded blocks are positive definite"
    vd = _device_vectors(v, pad)
    vc = torch.from_numpy(v).to(DEV).to(torch.complex128)
    z = ops.mt_solve(lay, fac, vc)
    qs = (vc.conj() * z).real.sum(-1).cpu().numpy()
    q = ops.mt_quadform(lay, fac, vd)
    assert q.shape == (B,) and q.dtype == torch.float64
    ref, bq = R.quadform_ref(fac.cpu().numpy(), ns, v, G)
    return q.cpu().numpy(), ref, bq, qs


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", CASE_IDS)
def test_quadform_within_the_derived_bound(name, family):
    q, ref, bq, _ = _run(name, family)
    ns = CASES[CASE_IDS.index(name)][1]
    err = np.abs(q.astype(R.LD) - ref)
    bnd = R.bound(ns, bq)
    print("%s/%s: C = %d, max err / B_q = %.3g, bound / B_q = %.3g, q / B_q = %.3g" % (
        name, family, R.bound_count(ns), float(np.max(err / bq)), float(np.max(bnd / bq)), float(np.max(ref / bq))))
    assert np.isfinite(q).all() and (q > 0).all()
    assert (err <= bnd).all(), (err, bnd)


def test_the_bound_is_relative_to_the_pivot_scale():
    """tiny_pivots: the lams scaled by 2^-40 scale q and B_q by 2^40 -- the absolute error with them."""
    q, ref, bq, _ = _run("tiny_pivots", "lattice")
    assert float(np.min(ref)) > 2.0 ** 30 and float(np.min(bq)) > 2.0 ** 30


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", CASE_IDS)
def test_quadform_equals_the_solve(name, family):
    q, _, bq, qs = _run(name, family)
    err = np.abs(q - qs)
    print("%s/%s: max |q - Re(v^H solve(v))| / B_q = %.3g" % (name, family, float(np.max(err / bq.astype(np.float64)))))
    assert (err <= 1e-12 * bq.astype(np.float64)).all()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ns", [[512, 512, 512], [256, 64, 8], [16] * 16], ids=["equal", "unequal", "sixteen"])
def test_a_vector_has_the_same_bits_whatever_else_is_in_the_call(ns, family):
    """Alone, first of 7, last of 64, and twice in one call."""
    lams = make_lams(ns, 1, family, 1.0, 77)
    lay = ops.mt_layout(ns)
    fac, _, _ = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
    others = torch.from_numpy(make_vectors(ns, 64, family, 78)).to(DEV)
    x = torch.from_numpy(make_vectors(ns, 1, family, 79)).to(DEV)

    def run(rows):
        return ops.mt_quadform(lay, fac, torch.cat(rows, 0).contiguous())

    alone = run([x])[0]
    assert run([x, others[:6]])[0] == alone
    assert run([others[:63], x])[63] == alone
    twice = run([x, x])
    assert twice[0] == alone and twice[1] == alone
    assert run([others[:2], x, others[2:5]])[2] == alone


def test_unequal_layouts_overwrite_v_and_equal_ones_do_not():
    for ns, overwritten in (([256, 256], False), ([256, 64], True)):
        lams = make_lams(ns, 1, "lattice", 1.0, 5)
        lay = ops.mt_layout(ns)
        fac, _, _ = ops.mt_factor(lay, torch.from_numpy(lams).to(DEV))
        v = torch.from_numpy(make_vectors(ns, 3, "lattice", 6)).to(DEV)
        keep = v.clone()
        ops.mt_quadform(lay, fac, v)
        assert bool((v != keep).any()) == overwritten
