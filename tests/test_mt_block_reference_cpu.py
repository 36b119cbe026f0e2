"""The extended-precision reference of the multitask block kernels and of fgp_mt_fit_run's stages (tests/
mt_block_reference.py), the part that needs no GPU:

  * the reference is right: factor / selected inverse / solve against numpy's dense slogdet / inv / solve of the class
    blocks, the gradient against a central difference in extended precision, the chained fit stages against a central
    difference of their loss over every raw parameter;
  * the bound is neither vacuous nor too tight: a float64 restatement stays inside every bound on every case, and each of
    three seeded defects breaks one;
  * the seeded fit problems are strictly diagonally dominant (so info == 0 by construction) and the case meant to take
    both Rprop branches takes them;
  * fgp_mt_fit_work_layout is declared, bound, exported and consistent with fgp_mt_fit_work, without a device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from fastgaussianprocesses_amd import _native as N
from tests import mt_block_reference as R
from tests import mt_fit_cases as C
from tests.mt_block_cases import CASE_IDS, CASES, case_inputs
from tests.mt_qf_cases import FAMILIES
from tests.mt_qf_reference import ldl_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fgp_mt_fit_work_layout"
BLOCK_PARAMS = [(n, f) for n in CASE_IDS for f in FAMILIES]
LD = np.longdouble
CLD = np.clongdouble


def _case(name):
    return CASES[CASE_IDS.index(name)]


# ------------------------------------------------------------------------------------------ the reference is right
@pytest.mark.parametrize("name,family", BLOCK_PARAMS)
def test_factor_selinv_and_solve_equal_dense_linear_algebra(name, family):
    case = _case(name)
    _, ns, G, B, scale = case
    lams, v, _, _ = case_inputs(case, family)
    lay = R.Layout(ns)
    f = R.factor_ref(lams, ns, G)
    assert f["info"] == 0
    zx, zy, _, _ = R.selinv_ref(f["fac"], ns, G)
    sx, sy, _, _ = R.solve_ref(f["fac"], ns, v, G)
    pattern = R.dense_blocks(np.ones(lay.L) + 0j, ns) != 0
    for g in range(G):
        dense = R.dense_blocks(lams[g], ns)
        sign, ld = np.linalg.slogdet(dense)
        assert (sign.real > 0).all()
        assert np.max(np.abs(ld - f["logdet"][g].astype(np.float64))) <= 1e-12 * lay.R * max(1.0, float(np.max(np.abs(ld))))
        inv = np.linalg.inv(dense)
        got = R.dense_blocks((zx[g] + 1j * zy[g]).astype(np.complex128), ns)
        assert np.max(np.abs((got - inv)[pattern])) <= 1e-12 * float(np.max(np.abs(inv)))
        for b in range(g, B, G):
            want = np.linalg.solve(dense, v[b].reshape(lay.R, lay.nmin).T[..., None])[..., 0].T
            z = (sx[b] + 1j * sy[b]).astype(np.complex128).reshape(lay.R, lay.nmin)
            assert np.max(np.abs(z - want)) <= 1e-12 * float(np.max(np.abs(want)))


def _mll(lams, v, gn, gl, ns, G):
    """f = sum_b gn_b Re(y_b^H A y_b) + sum_g gl_g logdet_g in extended precision (every stage handed on unrounded)."""
    f = R.factor_ref(lams, ns, G)
    fac = f["fac_x"].astype(CLD) + 1j * f["fac_y"].astype(CLD)
    sx, sy, _, _ = R.solve_ref(fac, ns, v, G)
    norm = (v.real.astype(LD) * sx + v.imag.astype(LD) * sy).sum(-1)
    return (gn.astype(LD) * norm).sum() + (gl.astype(LD) * f["logdet"].sum(-1)).sum(), f, (sx, sy)


@pytest.mark.parametrize("name,family", [("three_levels", "lattice"), ("repeated_sizes", "lattice"), ("g3_b6", "lattice"),
                                         ("g3_b6", "net"), ("sixteen_16", "lattice")])
def test_gradient_equals_a_central_difference(name, family):
    case = _case(name)
    _, ns, G, B, _ = case
    lams, v, gn, gl = case_inputs(case, family)
    lay = R.Layout(ns)
    _, f, (sx, sy) = _mll(lams, v, gn, gl, ns, G)
    fac = f["fac_x"].astype(CLD) + 1j * f["fac_y"].astype(CLD)
    zx, zy, _, _ = R.selinv_ref(fac, ns, G)
    gx, gy, _, _ = R.grad_ref(zx.astype(CLD) + 1j * zy.astype(CLD), sx.astype(CLD) + 1j * sy.astype(CLD), gn, gl, ns, B, G)
    diag = np.zeros(lay.L, dtype=bool)
    for k in range(lay.T):
        diag[lay.off[k, k]:lay.off[k, k] + lay.ns[k]] = True
    rng = np.random.default_rng(11)
    h = LD(2.0) ** -22
    scale = float(np.max(np.abs(gx))) + float(np.max(np.abs(gy)))
    for e in rng.choice(lay.L, 12, replace=False):
        g = int(rng.integers(G))
        for part in ((1.0,) if diag[e] or family == "net" else (1.0, 1j)):
            up, dn = lams.astype(CLD), lams.astype(CLD)
            up[g, e] += part * h
            dn[g, e] -= part * h
            fd = (_mll(up, v, gn, gl, ns, G)[0] - _mll(dn, v, gn, gl, ns, G)[0]) / (2 * h)
            got = gx[g, e] if part == 1.0 else gy[g, e]
            assert abs(float(fd - got)) <= 1e-9 * scale, (e, g, part, float(fd), float(got))
    assert (gy[:, diag] == 0).all()


def _fit_loss(fs, raw):
    """The loss of fgp_mt_fit_run at raw, every stage handed on in extended precision."""
    lx, ly, _, _ = R.fit_lams_ref(fs, raw)
    f = R.factor_ref(lx.astype(CLD) + 1j * ly.astype(CLD), fs.ns, fs.G)
    v = np.asarray(fs.y).transpose(1, 0, 2).reshape(fs.B * fs.G, -1)
    sx, sy, _, _ = R.solve_ref(f["fac_x"].astype(CLD) + 1j * f["fac_y"].astype(CLD), fs.ns, v, fs.G)
    norm = (v.real.astype(LD) * sx + v.imag.astype(LD) * sy).sum()
    return (norm + LD(fs.logdet_weight) * f["logdet"].sum() + LD(fs.mll_const)) / 2


@pytest.mark.parametrize("name", C.FD_CASES)
def test_fit_gradient_equals_a_central_difference_of_the_loss(name):
    fs, raw, c = C.make_fit(name)
    o = R.fit_chain(fs, raw)
    loss, _, grad, _ = o["step"]
    assert abs(float(loss[0] - _fit_loss(fs, raw))) <= 1e-13 * abs(float(loss[0]))
    h = 2.0 ** -20
    scale = float(np.max(np.abs(grad)))
    for x in range(fs.n_params):
        up, dn = raw.copy(), raw.copy()
        up[x] += h
        dn[x] -= h
        fd = (_fit_loss(fs, up) - _fit_loss(fs, dn)) / (up[x] - dn[x])
        assert abs(float(fd - grad[x])) <= 1e-8 * scale, (x, float(fd), float(grad[x]))


# ------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("name,family", BLOCK_PARAMS)
def test_float64_restatement_of_the_blocks_stays_inside_every_bound(name, family):
    case = _case(name)
    _, ns, G, B, _ = case
    lams, v, gn, gl = case_inputs(case, family)
    dev = R.block_stages(lams, v, gn, gl, ns, G)
    rs, _ = R.block_stage_ratios(dev, lams, v, gn, gl, ns, G)
    # ... and the division-based recurrence of tests/mt_qf_reference.py for the factor
    f = R.factor_ref(lams, ns, G)
    plain = np.stack([ldl_factor(lams[g], ns) for g in range(G)])
    rs["ldl_factor"] = R.complex_ratio(plain, (f["fac_x"], f["fac_y"], f["ex"], f["ey"]), R.counts(ns, B, G)["factor"])
    print("%s/%s: float64 max err / bound: %s" % (name, family, ", ".join("%s %.3g" % kv for kv in rs.items())))
    assert all(r <= 1.0 for r in rs.values()), rs
    # not vacuous: the restatement's rounding is within two orders of magnitude of the bound
    if len(ns) > 1:
        assert min(rs["fac"], rs["z"], rs["zinv"], rs["glp"]) >= 0.01, rs


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_float64_restatement_of_the_fit_stages_stays_inside_every_bound(name):
    fs, raw, c = C.make_fit(name)
    rs = R.fit_stage_ratios(fs, raw, R.fit_stages_f64(fs, raw))
    print("%s: float64 max err / bound: %s" % (name, ", ".join("%s %.3g" % kv for kv in rs.items())))
    assert all(r <= 1.0 for r in rs.values()), rs
    assert min(rs.values()) >= 0.001, rs


@pytest.mark.parametrize("mutate,stage", [("noconj", "fac"), ("qmod", "fac"), ("nofac2", "glp")])
def test_a_seeded_defect_breaks_a_bound(mutate, stage):
    broken = []
    for name, family in BLOCK_PARAMS:
        case = _case(name)
        _, ns, G, B, _ = case
        if len(ns) == 1 or ns == [1024, 1]:
            continue
        lams, v, gn, gl = case_inputs(case, family)
        rs, _ = R.block_stage_ratios(R.block_stages(lams, v, gn, gl, ns, G, mutate=mutate), lams, v, gn, gl, ns, G)
        if rs[stage] > 1.0:
            broken.append((name, family))
    print("%s breaks the %s bound on %s" % (mutate, stage, broken))
    assert broken
    # the missing conjugate shows on every complex case with a coupling, the row index on every case with unequal
    # sizes, the missing factor on every case with a coupling
    want = {"noconj": [(n, f) for n, f in BLOCK_PARAMS if f == "lattice" and len(_case(n)[1]) > 1 and _case(n)[1] != [1024, 1]],
            "qmod": [(n, f) for n, f in BLOCK_PARAMS if len(set(_case(n)[1])) > 1 and len(_case(n)[1]) > 2],
            "nofac2": [(n, f) for n, f in BLOCK_PARAMS if len(_case(n)[1]) > 1 and _case(n)[1] != [1024, 1]]}[mutate]
    assert broken == want


@pytest.mark.parametrize("mutate,stage", [("noconj", "sums"), ("qmod", "sums"), ("nofac2", "sums")])
def test_a_seeded_defect_moves_the_fit_s_totals_far_outside_the_bound(mutate, stage):
    """The same defects in the chained fit stages: the totals of the defective chain against the sound chain's bound."""
    fs, raw, _ = C.make_fit("three_levels")
    good, bad = R.fit_chain(fs, raw), R.fit_chain(fs, raw, np.float64, mutate)
    assert R.ratio(np.asarray(bad["sums"][0], dtype=np.float64), good["sums"][0], good["sums"][1], fs.counts()["contract"]) > 1e6


# ------------------------------------------------------------------------------------------ the cases
def _dominance(lams, ns):
    """min over the rows of every class block of |diagonal| - sum |couplings|, relative to the diagonal."""
    lay = R.Layout(ns)
    G = lams.shape[0]
    a = np.abs(lams).reshape(G, lay.L // lay.nmin, lay.nmin)
    o = {kl: v // lay.nmin for kl, v in lay.off.items()}
    off = np.zeros((G, lay.R, lay.nmin))
    dg = np.zeros((G, lay.R, lay.nmin))
    for (k, l), ok in o.items():
        for q in range(lay.q[k]):
            if k == l:
                dg[:, lay.rs[k] + q] = lams.reshape(a.shape)[:, ok + q].real
            else:
                off[:, lay.rs[k] + q] += a[:, ok + q]
                off[:, lay.rs[l] + q % lay.q[l]] += a[:, ok + q]
    return float(np.min((dg - off) / dg)), float(np.min(dg))


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_seeded_fit_problems_are_strictly_diagonally_dominant(name):
    fs, raw, c = C.make_fit(name)
    lx, ly, _, _ = R.fit_lams_ref(fs, raw)
    margin, dmin = _dominance((lx + 1j * ly).astype(np.complex128), fs.ns)
    print("%s: min (|d| - sum |c|) / d = %.3g" % (name, margin))
    assert dmin > 0 and margin > 0.05
    assert np.all(np.abs(raw) <= 0.5)


def test_the_branch_case_takes_both_rprop_branches_at_its_second_iteration():
    fs, raw, c = C.make_fit(C.BRANCH_CASE)
    mask = C.rg_mask(fs, c["rg"])
    g0 = R.fit_stages_f64(fs, raw)["grad"]
    raw1, prev1, step1, prod0 = R.rprop_f64(g0, raw, np.zeros_like(raw), np.full_like(raw, c["lr"]), mask, *C.ETAS, *C.STEPS)
    assert (prod0 == 0).all() and np.array_equal(prev1, g0) and np.array_equal(raw1, raw - np.sign(g0) * c["lr"])
    g1 = R.fit_stages_f64(fs, raw1)["grad"]
    raw2, prev2, step2, prod1 = R.rprop_f64(g1, raw1, prev1, step1, mask, *C.ETAS, *C.STEPS)
    assert (prod1 < 0).any() and (prod1 > 0).any()
    # torch.optim.Rprop: a sign change halves the step, zeroes the stored gradient and does not move the parameter
    flip = prod1 < 0
    assert np.array_equal(step2[flip], step1[flip] * 0.5) and (prev2[flip] == 0).all() and np.array_equal(raw2[flip], raw1[flip])
    assert np.array_equal(step2[~flip], step1[~flip] * 1.2)


def test_the_no_stage_case_is_the_batch_case_with_unused_scale_rows():
    fs0, raw0, _ = C.make_fit("batch_g3")
    fs1, raw1, _ = C.make_fit("nostage")
    assert fs1.n_params == fs0.n_params + 4198 <= 8192
    assert 2 * 8 * fs1.n_params + 8 * fs1.G * (R.KMTGQ + fs1.P) + 20 * fs1.G > 65536
    assert np.array_equal(np.concatenate([raw1[:2], raw1[4200:]]), raw0)
    assert set(int(v) for v in fs1.rows[0]) == {0, 1}


# ------------------------------------------------------------------------------------------ the new query
def test_work_layout_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgp_hip.h")).read(), flags=re.S)
    assert re.search(r"^\s*extern\s+int\s+%s\s*\(" % NAME, src, flags=re.M)
    assert NAME in N._SIGNATURES and len(N._SIGNATURES[NAME]) == 2
    assert hasattr(lib, NAME) and NAME in N.exported_symbols()


def test_work_layout_refuses_what_the_work_query_refuses():
    lib = N.lib()
    fs, raw, c = C.make_fit("d2")
    offs = (ctypes.c_int64 * 10)()
    assert lib.fgp_mt_fit_work_layout(ctypes.byref(C.fill_desc(fs, c)), None) == -1
    assert b"fgp_mt_fit_work_layout" in lib.fgp_last_error() and b"offsets" in lib.fgp_last_error()
    assert lib.fgp_mt_fit_work_layout(None, offs) == -1
    wb = ctypes.c_int64(0)
    for field, value in (("d", 7), ("B", 0), ("dl", 3), ("rank", -1), ("T_all", 1)):
        desc = C.fill_desc(fs, c)
        setattr(desc, field, value)
        rc = lib.fgp_mt_fit_work_layout(ctypes.byref(desc), offs)
        assert rc != 0 and rc == lib.fgp_mt_fit_work(ctypes.byref(desc), ctypes.byref(wb)), field
    desc = C.fill_desc(fs, c)
    desc.nrows[0] = 9000
    assert lib.fgp_mt_fit_work_layout(ctypes.byref(desc), offs) == -2


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_work_layout_is_ascending_aligned_and_ends_at_the_work_size(name):
    lib = N.lib()
    fs, raw, c = C.make_fit(name)
    desc = C.fill_desc(fs, c)
    rows = np.ascontiguousarray(fs.rows, dtype=np.int32)        # (a parameter batch must name its rows; not read here)
    desc.rows = rows.ctypes.data if fs.G > 1 else None
    offs = (ctypes.c_int64 * 10)()
    wb = ctypes.c_int64(0)
    npar = ctypes.c_int(0)
    assert lib.fgp_mt_fit_work_layout(ctypes.byref(desc), offs) == 0
    assert lib.fgp_mt_fit_work(ctypes.byref(desc), ctypes.byref(wb)) == 0
    assert lib.fgp_mt_fit_nparams(ctypes.byref(desc), ctypes.byref(npar)) == 0 and npar.value == fs.n_params
    o = list(offs)
    assert o[0] == 0 and all(b > a for a, b in zip(o, o[1:])) and all(v % 256 == 0 for v in o)
    assert o[-1] + 256 == wb.value
    lay, G = fs.lay, fs.G
    sizes = [16 * G * lay.L] * 4 + [16 * G * fs.B * lay.R * lay.nmin, 8 * G * lay.nmin, 8 * G * lay.L,
                                    8 * G * fs.nblk * R.KMTGQ, 8 * G * (R.KMTGQ + fs.P)]
    assert all(b - a >= s and b - a < s + 256 for a, b, s in zip(o, o[1:], sizes)), (o, sizes)
