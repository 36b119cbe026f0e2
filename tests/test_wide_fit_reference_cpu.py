"""The reference of the wide fit loops' own kernels (tests/wide_fit_reference.py), the part that needs no GPU.

  1. The reference is right: for one small case per loss and family the stages composed in extended precision (k1 and
     its adjoint from predict_reference / wide_mt_reference, the transforms from transform_reference, the block stages
     from mt_block_reference) reproduce the loss and the raw gradient of the CPU oracle (oracle/fgp_oracle.py; GCV and
     CV from the oracle's own eigenvalues, coefficients and autograd; oracle/fgp_oracle_mt.py) to 2e-7.
  2. A plain float64 restatement of every stage stays inside its bound.
  3. Each seeded defect breaks a bound.
  4. Non-vacuity: for every case and compared array ||u e||_1 <= 100 2^-53 C ||value||_1, no twin infinite or NaN.
  5. The four hooks are declared, bound and exported, validate without a device, and their offsets are ascending and
     consistent with fgp_wide_fit_work / fgp_wide_mt_fit_work."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from oracle import fgp_oracle as O
from oracle.fgp_oracle_mt import OracleMultiTaskFastGP
from tests import mt_block_reference as MB
from tests import predict_reference as PR
from tests import transform_reference as TR
from tests import wide_fit_cases as C
from tests import wide_fit_reference as R
from tests import wide_mt_reference as WMR
from tests.test_wide_fit_cpu import FGP_ERR_INVALID, ROOT, _desc

torch.set_default_dtype(torch.float64)
F64 = np.float64
TOL = 2e-7


def f64(a):
    return np.asarray(a, dtype=np.float64) if not isinstance(a, R.Tr) else R._f64(a)


# ------------------------------------------------------------------------------------------------ single task: chain
def wf_lambda(parts, raw, G, d, dl, fam):
    """(nat_scale, nat_ls, lambda real parts [G, n]) of the reference chain, rounded to double."""
    ns, nl = R.nat_ref(raw, G, d, dl)
    ns, nl = f64(ns), f64(nl)
    if parts.ndim == 3:
        k1 = np.concatenate([PR.k1(parts[g], ns[g:g + 1], nl[g:g + 1])[0] for g in range(G)])
    else:
        k1 = PR.k1(parts, ns, nl)[0]
    k1 = PR.to_f64(k1)
    lam = TR.fftbr(k1)[0] if fam == C.LAT else TR.fwht(k1)
    return ns, nl, PR.to_f64(lam)


def wf_adjoint(gt, fam):
    return PR.to_f64(TR.ifftbr(gt.astype(np.complex128))[0] if fam == C.LAT else TR.fwht(gt))


def wf_k1_bwd(parts, ns, nl, u, G):
    if parts.ndim == 3:
        out = [PR.k1_bwd(parts[g], ns[g:g + 1], nl[g:g + 1], u[g:g + 1]) for g in range(G)]
        return np.concatenate([PR.to_f64(o[0]) for o in out]), np.concatenate([PR.to_f64(o[2]) for o in out])
    ds, _, dls, _ = PR.k1_bwd(parts, ns, nl, u)
    return PR.to_f64(ds), PR.to_f64(dls)


def wf_chain(parts, ysq, raw, fam, m, d, G, dl, loss, w, cvw, mll_const, xt=R.XT, mutate=None):
    """One evaluation with the stages of the loop in `xt` arithmetic, every stage fed the one before rounded to double:
    dict of the stages' tracked outputs and the arrays handed on."""
    n = 1 << m
    ns, nl, lam = wf_lambda(parts, raw, G, d, dl, fam)
    raw_noise = np.asarray(raw)[G * (1 + dl):]
    out = {"lam": lam, "nat": (ns, nl)}
    if loss == C.MLL:
        e = R.eig_ref(lam, ysq, raw_noise, n, w, xt, mutate)
        out["gt"], out["pe"] = e["gt"], e["pe"]
    else:
        cv = loss == C.CV
        out["pe"] = R.loss_sums_ref(lam, ysq, raw_noise, n, cv, xt, mutate)
        pl = np.full((G, 4, R.nbe_of(n)), np.nan)
        pl[:, :out["pe"].v.shape[1]] = f64(out["pe"])
        out["gt"] = R.loss_grad_ref(lam, ysq, raw_noise, pl, n, cvw, cv, xt, mutate)
    u = wf_adjoint(f64(out["gt"]), fam)
    out["dscale"], out["dls"] = wf_k1_bwd(parts, ns, nl, u, G)
    pe = f64(out["pe"])
    out["step"] = R.step_ref(loss, pe, out["dscale"], out["dls"], ns, nl, raw, G, d, dl, n, w, mll_const, cvw, xt)
    return out


def wf_case_chain(name, xt=R.XT, mutate=None):
    c = C.WF_BY_NAME[name]
    inp = C.wf_inputs(name)
    return c, inp, wf_chain(inp["parts"], inp["ysq"], inp["raw"], c.fam, c.m, c.d, c.G, c.dl, c.loss, C.LOGDET_WEIGHT,
                            C.CV_WEIGHT, C.MLL_CONST, xt, mutate)


def wf_stage_ratios(name, mutate=None):
    """max err / bound of the float64 restatement (with `mutate`) of every stage against the extended reference on the
    SAME inputs (the restatement's own stage inputs), and the non-vacuity figures of the reference's arrays."""
    c, inp, dev = wf_case_chain(name, F64, mutate)
    n, G = 1 << c.m, c.G
    Cn = R.counts(n, c.d)
    raw_noise = inp["raw"][G * (1 + c.dl):]
    lam, (ns, nl) = dev["lam"], dev["nat"]
    ratios, vac = {}, {}

    def put(key, t, got, cn):
        ratios[key] = R.rel(got, t, cn)
        vac[key] = R.vacuity(t, cn)

    # the natural rows (prologue, step): the float64 exp against the extended one
    rs, rl = R.nat_ref(inp["raw"], G, c.d, c.dl)
    ps, pl_ = R.nat_ref(inp["raw"], G, c.d, c.dl, F64)
    put("nat_scale", rs, f64(ps), 2 * R.ULP_LIBM + 1)
    put("nat_ls", rl, f64(pl_), 2 * R.ULP_LIBM + 1)
    if c.loss == C.MLL:
        ref = R.eig_ref(lam, inp["ysq"], raw_noise, n, C.LOGDET_WEIGHT)
        put("gt", ref["gt"], f64(dev["gt"]), Cn["terms"])
        put("pe", ref["pe"], f64(dev["pe"]), Cn["terms"])
    else:
        cv = c.loss == C.CV
        put("pe", R.loss_sums_ref(lam, inp["ysq"], raw_noise, n, cv), f64(dev["pe"]), Cn["sums"])
        pl = np.full((G, 4, R.nbe_of(n)), np.nan)
        pl[:, :dev["pe"].v.shape[1]] = f64(dev["pe"])
        put("gt", R.loss_grad_ref(lam, inp["ysq"], raw_noise, pl, n, C.CV_WEIGHT, cv), f64(dev["gt"]), Cn["grad"])
    ref = R.step_ref(c.loss, f64(dev["pe"]), dev["dscale"], dev["dls"], ns, nl, inp["raw"], G, c.d, c.dl, n, C.LOGDET_WEIGHT,
                     C.MLL_CONST, C.CV_WEIGHT)
    put("loss", ref["loss"], f64(dev["step"]["loss"]), Cn["step"])
    put("grad", ref["grad"], f64(dev["step"]["grad"]), Cn["step"])
    return ratios, vac


# ------------------------------------------------------------------------------------------------ 1. the oracle
def _oracle_problem(fam, m=6, d=9, seed=5):
    import fastgaussianprocesses_amd as F
    n = 1 << m
    g = np.random.default_rng([41, fam, m, d, seed])
    if fam == C.LAT:
        x = torch.from_numpy(F.Lattice(d, seed=seed)(0, n))
        xb, t = None, None
    else:
        from tests.wide_cases import net_sequence
        seq = net_sequence(d, seed)
        xb, t = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64)), seq.t
        x = xb.to(torch.float64) * 2.0 ** -t
    y = O.f_ackley(x) + 0.1 * torch.from_numpy(g.standard_normal(n))
    ls = torch.from_numpy(g.uniform(0.1, 0.3, d))
    o = O.OracleFastGP("lattice" if fam == C.LAT else "net", x, xb, y[None, :], alpha=2 if fam == C.LAT else 1, t=t,
                       scale=float(g.uniform(0.7, 1.3)), lengthscales=ls, noise=1e-2, requires_grad_noise=True)
    return o


def _oracle_loss(o, loss, cvw):
    if loss == C.MLL:
        return o.mll_loss()[0]
    A, _ = o.inv_logdet()
    yt = o.ytilde()
    if loss == C.GCV:
        z = yt * A
        return ((z.conj() * z).real.sum() / (A.real.sum() / o.n) ** 2)
    inv_diag = (1 / (o.lam() * math.sqrt(o.n))).real.mean()
    return ((o.coeffs().real / inv_diag) ** 2 * cvw).sum()


@pytest.mark.parametrize("loss", [C.MLL, C.GCV, C.CV])
@pytest.mark.parametrize("fam", [C.LAT, C.NET])
def test_composed_stages_reproduce_the_oracle(fam, loss):
    o = _oracle_problem(fam)
    n, d, m = o.n, o.d, 6
    want = _oracle_loss(o, loss, C.CV_WEIGHT)
    gs = torch.autograd.grad(want, [o.raw_scale, o.raw_lengthscales, o.raw_noise])
    gref = np.concatenate([g.detach().numpy().reshape(-1) for g in gs])
    parts = np.ascontiguousarray(o.k1parts().numpy().T)
    yt = TR.fftbr(o.y.numpy()) if fam == C.LAT else (TR.fwht(o.y.numpy()), 0)
    ysq = PR.to_f64(yt[0] * yt[0] + yt[1] * yt[1]).reshape(1, n)
    raw = np.concatenate([p.detach().numpy().reshape(-1) for p in (o.raw_scale, o.raw_lengthscales, o.raw_noise)])
    mll_const = 0.5 * n * math.log(2 * math.pi)
    out = wf_chain(parts, ysq, raw, fam, m, d, 1, d, loss, 1.0, C.CV_WEIGHT, mll_const)
    got_loss = float(out["step"]["loss"].v[0, 0])
    got = f64(out["step"]["grad"])
    el = abs(got_loss - float(want)) / abs(float(want))
    eg = float(np.abs(got - gref).max() / np.abs(gref).max())
    print("oracle", fam, loss, "loss rel err %.3g, gradient rel err %.3g" % (el, eg))
    assert el <= TOL and eg <= TOL


# ------------------------------------------------------------------------------------------------ 2 - 4. single task
@functools.lru_cache(maxsize=None)
def _wf_plain(name):
    return wf_stage_ratios(name)


@pytest.mark.parametrize("name", C.WF_CPU)
def test_plain_float64_restatement_stays_inside_the_bound(name):
    ratios, _ = _wf_plain(name)
    print(name, ", ".join("%s %.3g" % kv for kv in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", C.WF_CPU)
def test_bounds_are_not_vacuous(name):
    _, vac = _wf_plain(name)
    for k, (v, fin) in vac.items():
        assert fin and v <= 1.0, (name, k, v, fin)


@pytest.mark.parametrize("mutate,name,key", [
    ("hs", "lat-m9", "gt"), ("hs", "net-m12", "gt"),
    ("pair", "lat-m9", "pe"), ("pair", "net-m1", "pe"), ("pair", "lat-gcv-m9", "pe"),
    ("cv_w2", "lat-cv-m9", "gt"), ("cv_w2", "net-cv-m12", "gt")])
def test_seeded_defects_break_a_bound(mutate, name, key):
    ratios, _ = wf_stage_ratios(name, mutate)
    print(mutate, name, ratios)
    assert ratios[key] > 1.0, (mutate, name, ratios)


# ------------------------------------------------------------------------------------------------ multitask: chain
def mt_chain(sp, pairs, y, raw, xt=R.XT, mutate=None):
    """One evaluation of fgp_wide_mt_fit_run's loss and gradient, every stage in `xt` arithmetic on the stage before
    rounded to double."""
    lay, d = sp.lay, sp.d
    nat = f64(R.mt_nat_ref(sp, raw))
    lat = sp.family == C.LAT
    lam = np.zeros(lay.L, dtype=np.complex128 if lat else np.float64)
    for p, (k, l) in enumerate(sp.pairs):
        parts, ind, cc = pairs[p]
        k1 = PR.to_f64(WMR.mt_k1(parts, ind, cc, nat[:1], nat[None, 1:])[0])
        sl = slice(lay.off[k, l], lay.off[k, l] + lay.ns[k])
        if lat:
            re, im = TR.fftbr(k1)
            lam[sl] = PR.to_f64(re)[0] + 1j * PR.to_f64(im)[0]
        else:
            lam[sl] = PR.to_f64(TR.fwht(k1))[0]
    out = {"lam": lam, "nat": nat}
    out["lams"] = R.mt_lams_ref(sp, raw, lam, xt, mutate)
    lams = f64(out["lams"][0]) + 1j * f64(out["lams"][1])
    f = MB.factor_ref(lams[None], sp.ns, 1, xt)
    z = MB.solve_ref(f["fac"], sp.ns, y, 1, xt)
    z = np.asarray(z[0], dtype=F64) + 1j * np.asarray(z[1], dtype=F64)
    zi = MB.selinv_ref(f["fac"], sp.ns, 1, xt)
    zi = np.asarray(zi[0], dtype=F64) + 1j * np.asarray(zi[1], dtype=F64)
    gl = MB.grad_ref(zi, z, np.full(sp.B, 0.5), np.array([0.5 * sp.logdet_weight]), sp.ns, sp.B, 1, xt)
    out["glp"] = (np.asarray(gl[0], dtype=F64) + 1j * np.asarray(gl[1], dtype=F64))[0]
    out["z"], out["logdet"], out["info"] = z, np.asarray(f["logdet"], dtype=F64)[0], f["info"]
    out["contract"] = cr = R.mt_contract_ref(sp, raw, out["glp"], lam, y, z, out["logdet"], xt, mutate)
    gt = f64(cr["gx"]) + 1j * f64(cr["gy"])
    dsl = np.zeros((sp.np, 1 + d))
    for p, (k, l) in enumerate(sp.pairs):
        parts, ind, cc = pairs[p]
        sl = slice(lay.off[k, l], lay.off[k, l] + lay.ns[k])
        u = PR.to_f64(TR.ifftbr(gt[sl])[0] if lat else TR.fwht(gt[sl].real))
        ds, _, dls, _ = WMR.mt_k1_bwd(parts, ind, cc, nat[:1], nat[None, 1:], u.reshape(1, -1))
        dsl[p, 0], dsl[p, 1:] = PR.to_f64(ds)[0], PR.to_f64(dls)[0]
    out["dsl"] = dsl
    out["part"] = f64(cr["part"])
    out["step"] = R.mt_step_ref(sp, raw, out["part"], dsl, nat, xt, mutate)
    return out


def mt_stage_ratios(name, mutate=None):
    c = C.MT_BY_NAME[name]
    sp, inp = C.mt_spec(c), C.mt_inputs(name)
    dev = mt_chain(sp, inp["pairs"], inp["y"], inp["raw"], F64, mutate)
    assert dev["info"] == 0
    Cn = sp.counts()
    ratios, vac = {}, {}

    def put(key, t, got, cn):
        ratios[key] = R.rel(got, t, cn)
        vac[key] = R.vacuity(t, cn)

    put("nat", R.mt_nat_ref(sp, inp["raw"]), f64(R.mt_nat_ref(sp, inp["raw"], F64)), 2 * R.ULP_LIBM + 1)
    X, Y = R.mt_lams_ref(sp, inp["raw"], dev["lam"])
    put("lams_x", X, f64(dev["lams"][0]), Cn["lams"])
    if sp.family == C.LAT:
        put("lams_y", Y, f64(dev["lams"][1]), Cn["lams"])
    cr = R.mt_contract_ref(sp, inp["raw"], dev["glp"], dev["lam"], inp["y"], dev["z"], dev["logdet"])
    put("gt_x", cr["gx"], f64(dev["contract"]["gx"]), Cn["contract"])
    if sp.family == C.LAT:
        put("gt_y", cr["gy"], f64(dev["contract"]["gy"]), Cn["contract"])
    put("part", cr["part"], dev["part"], Cn["contract"])
    st = R.mt_step_ref(sp, inp["raw"], dev["part"], dev["dsl"], dev["nat"])
    put("loss", st["loss"], f64(dev["step"]["loss"]), Cn["step"])
    put("grad", st["grad"], f64(dev["step"]["grad"]), Cn["step"])
    return ratios, vac


@functools.lru_cache(maxsize=None)
def _mt_plain(name):
    return mt_stage_ratios(name)


@pytest.mark.parametrize("name", C.MT_CPU)
def test_mt_plain_float64_restatement_stays_inside_the_bound(name):
    ratios, _ = _mt_plain(name)
    print(name, ", ".join("%s %.3g" % kv for kv in ratios.items()))
    for k, r in ratios.items():
        assert r <= 1.0, (name, k, r)


@pytest.mark.parametrize("name", C.MT_CPU)
def test_mt_bounds_are_not_vacuous(name):
    _, vac = _mt_plain(name)
    for k, (v, fin) in vac.items():
        assert fin and v <= 1.0, (name, k, v, fin)


@pytest.mark.parametrize("mutate,name,key", [
    ("nk", "lat-T3", "lams_x"), ("nk", "net-T3", "lams_x"),
    ("nocj", "lat-T3", "gt_y"), ("nocj", "lat-tall4", "gt_y"),
    ("tot", "lat-T3", "grad"), ("tot", "net-tall4", "grad")])
def test_mt_seeded_defects_break_a_bound(mutate, name, key):
    ratios, _ = mt_stage_ratios(name, mutate)
    print(mutate, name, ratios)
    assert ratios[key] > 1.0, (mutate, name, ratios)


@pytest.mark.parametrize("fam,ns", [(C.LAT, [16, 8]), (C.LAT, [8, 16]), (C.NET, [16, 8])])
def test_mt_composed_stages_reproduce_the_oracle(fam, ns):
    """[8, 16]: the sorted order is (task 1, task 0), the coupling pair's lambda enters conjugated."""
    import fastgaussianprocesses_amd as F
    d, T = 9, 2
    g = np.random.default_rng([43, fam] + ns)
    if fam == C.LAT:
        gen, shifts, t = [int(v) for v in F.Lattice(d).z], g.uniform(0, 1, (T, d)), 32
    else:
        from tests.test_gpu_wide import net_matrices
        gen, shifts, t = net_matrices(d, 3), g.integers(0, 1 << 32, (T, d), dtype=np.int64), 32
    o = OracleMultiTaskFastGP("lattice" if fam == C.LAT else "net", gen, shifts, [torch.zeros(n) for n in ns],
                              alpha=2 if fam == C.LAT else 1, t=t, noise=1e-2)
    o.ys = [torch.sin(3 * o.points(l, ns[l])[0]).mean(1) + 0.1 * l + 0.05 * torch.from_numpy(g.standard_normal(ns[l]))
            for l in range(T)]
    with torch.no_grad():
        o.raw_scale.copy_(torch.tensor([float(g.uniform(-0.3, 0.3))]))
        o.raw_lengthscales.copy_(torch.log(torch.from_numpy(g.uniform(0.1, 0.3, d))))
        o.raw_factor_task_kernel.copy_(torch.from_numpy(g.uniform(0.3, 0.9, (T, 1))))
        o.raw_noise_task_kernel.copy_(torch.from_numpy(g.uniform(-0.2, 0.2, T)))
    o.raw_noise.requires_grad_(True)
    want = o.mll_loss()
    gs = torch.autograd.grad(want, o.parameters())
    gref = np.concatenate([v.detach().numpy().reshape(-1) for v in gs])
    to = o.order(ns).tolist()
    nsrt = [ns[i] for i in to]
    pairs, conj = [], []
    for k in range(T):
        for l in range(k, T):
            a, b = to[k], to[l]
            p = o.k1parts(min(a, b), max(a, b), nsrt[k]).numpy()               # [n, 1, 1, d]
            pairs.append((np.ascontiguousarray(p.reshape(nsrt[k], d).T[None]), np.ones((1, d), dtype=np.int32), np.ones(1)))
            conj.append(int(a > b))
    sp = R.MtSpec(ns=nsrt, d=d, dl=d, B=1, family=fam, task=to, T_all=T, rank=1, vtask_exp=1, conj=conj, logdet_weight=1.0,
                  mll_const=0.5 * sum(ns) * math.log(2 * math.pi))
    yts = []
    for i in to:
        yv = o.ys[i].numpy()
        if fam == C.LAT:
            re, im = TR.fftbr(yv)
            yts.append(PR.to_f64(re)[0] + 1j * PR.to_f64(im)[0])
        else:
            yts.append(PR.to_f64(TR.fwht(yv))[0].astype(np.complex128))
    y = np.concatenate(yts)[None]
    raw = np.concatenate([v.detach().numpy().reshape(-1) for v in o.parameters()])
    out = mt_chain(sp, pairs, y, raw)
    got_loss, got = float(out["step"]["loss"].v[0]), f64(out["step"]["grad"])
    el = abs(got_loss - float(want)) / abs(float(want))
    eg = float(np.abs(got - gref).max() / np.abs(gref).max())
    print("mt oracle", fam, ns, "loss rel err %.3g, gradient rel err %.3g" % (el, eg))
    assert el <= TOL and eg <= TOL


# ------------------------------------------------------------------------------------------------ 5. the hooks
HOOKS = ("fgp_wide_fit_work_layout", "fgp_wide_fit_stage", "fgp_wide_mt_fit_work_layout", "fgp_wide_mt_fit_stage")


def test_hooks_declared_bound_and_exported():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in HOOKS:
        decl = ("extern int (%s)(" if "_mt_" in name else "extern int %s(") % name
        assert decl in src, "include/fgp_hip.h does not declare %s" % name
        assert name in N._SIGNATURES and name in N.exported_symbols()
        assert hasattr(ctypes.CDLL(N.LIB_PATH), name), "libfgp_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == N._SIGNATURES[name]


def _offsets(desc):
    offs = (ctypes.c_int64 * 10)()
    assert N.lib().fgp_wide_fit_work_layout(ctypes.byref(desc), offs) == 0
    return list(offs)


@pytest.mark.parametrize("fam", [0, 1])
@pytest.mark.parametrize("m,G,d", [(0, 1, 9), (4, 3, 12), (13, 5, 12), (17, 2, 64), (20, 1, 9)])
@pytest.mark.parametrize("metric", [N.LOSS_MLL, N.LOSS_GCV, N.LOSS_CV])
def test_wide_fit_offsets_are_ascending_and_consistent_with_the_work_length(fam, m, G, d, metric):
    desc = _desc(family=fam, log2n=m, G=G, d=d, dl=d, loss_metric=metric, cv_weight=0.5)
    o = _offsets(desc)
    n, nbe = 1 << m, ((1 << m) + 2047) // 2048
    ln = ctypes.c_int64(-1)
    assert N.lib().fgp_wide_fit_work(ctypes.byref(desc), ctypes.byref(ln)) == 0
    sizes = [G, G * d, G, G * d, G * n, G * n * (2 if fam == 0 else 1), 2 * G * n if fam == 0 else 0, 3 * G * nbe,
             G * (1 + d) * ((n + 255) // 256), 0 if metric == N.LOSS_MLL else 4 * G * nbe]
    assert o[0] == 0 and all(v % 2 == 0 for v in o)
    for i in range(10):
        end = o[i + 1] if i < 9 else ln.value
        assert o[i] + sizes[i] <= end <= o[i] + sizes[i] + 1, (i, o, sizes, ln.value)


def test_wide_fit_hooks_validate_without_a_device():
    lib = N.lib()
    offs = (ctypes.c_int64 * 10)()
    assert lib.fgp_wide_fit_work_layout(ctypes.byref(_desc()), None) == FGP_ERR_INVALID
    assert lib.fgp_wide_fit_work_layout(None, offs) == FGP_ERR_INVALID
    for field, kw in (("d", dict(d=8, dl=8)), ("log2n", dict(log2n=25)), ("G", dict(G=0)), ("dl", dict(dl=3)),
                      ("loss_metric", dict(loss_metric=3))):
        assert lib.fgp_wide_fit_work_layout(ctypes.byref(_desc(**kw)), offs) == FGP_ERR_INVALID
        msg = lib.fgp_last_error()
        assert b"fgp_wide_fit_work_layout" in msg and field.encode() in msg, msg
        assert lib.fgp_wide_fit_stage(ctypes.byref(_desc(**kw)), 0, 1, 0, None) == FGP_ERR_INVALID
        assert b"fgp_wide_fit_stage" in lib.fgp_last_error() and field.encode() in lib.fgp_last_error()
    # every (stage, mode) outside the table, before any HIP call (no device here: a launch would fail differently)
    bad = [(-1, 0), (8, 0), (0, 2), (0, -1), (7, 0), (7, 3), (4, 0)] + [(s, 1) for s in (1, 2, 3, 5, 6)]
    for stage, mode in bad:
        rc = lib.fgp_wide_fit_stage(ctypes.byref(_desc()), 0, stage, mode, None)
        msg = lib.fgp_last_error()
        assert rc == FGP_ERR_INVALID and b"fgp_wide_fit_stage" in msg and (b"stage" in msg or b"mode" in msg), (stage, mode, msg)
    assert lib.fgp_wide_fit_stage(ctypes.byref(_desc(lr=0.0)), 0, 0, 1, None) == FGP_ERR_INVALID and b"lr" in lib.fgp_last_error()
    assert lib.fgp_wide_fit_stage(ctypes.byref(_desc()), -1, 1, 0, None) == FGP_ERR_INVALID and b"iter" in lib.fgp_last_error()
    assert lib.fgp_wide_fit_stage(ctypes.byref(_desc(work=None)), 0, 1, 0, None) == FGP_ERR_INVALID
    assert b"work" in lib.fgp_last_error()
    assert lib.fgp_wide_fit_stage(None, 0, 1, 0, None) == FGP_ERR_INVALID


_IND = N.int_array([1] * 64)
_CC = N.double_array([1.0])


def _mt_desc(ns=(64, 16), fam=0, d=12, B=2, rank=2, T_all=None, **kw):
    from tests.test_wide_fit_cpu import _ptr
    p = _ptr()
    T = len(ns)
    desc = N.WideMtFitDesc(family=fam, d=d, B=B, T_all=T if T_all is None else T_all, rank=rank, dl=d, y=p, raw=p,
                           vtask_exp=1, rg_scale=1, rg_ls=1, rg_noise=1, rg_factor=1, rg_vtask=1, rprop_prev=p, rprop_step=p,
                           lr=0.1, eta_minus=0.5, eta_plus=1.2, step_min=1e-6, step_max=50.0, logdet_weight=1.0, mll_const=0.0,
                           loss_hist=p, raw_hist=p, grad_out=p, work=p)
    desc.layout.T = T
    for k, n in enumerate(ns):
        desc.layout.n[k] = n
        desc.task[k] = k
    for q in range(T * (T + 1) // 2):
        desc.pair[q].parts = p
        desc.pair[q].ind = ctypes.cast(_IND, ctypes.c_void_p)
        desc.pair[q].cc = ctypes.cast(_CC, ctypes.c_void_p)
        desc.pair[q].P = 1
    for k, v in kw.items():
        setattr(desc, k, v)
    return desc


@pytest.mark.parametrize("fam", [0, 1])
@pytest.mark.parametrize("ns,B,d", [((64,), 1, 9), ((64, 64, 16), 3, 12), ((4, 1), 1, 9), ((1 << 17, 1 << 9), 1, 9)])
def test_wide_mt_fit_offsets_are_ascending_and_consistent_with_the_work_length(fam, ns, B, d):
    lib = N.lib()
    desc = _mt_desc(ns, fam, d, B)
    offs = (ctypes.c_int64 * 15)()
    assert lib.fgp_wide_mt_fit_work_layout(ctypes.byref(desc), offs) == 0
    nb = ctypes.c_int64(-1)
    assert lib.fgp_wide_mt_fit_work(ctypes.byref(desc), ctypes.byref(nb)) == 0
    o = list(offs)
    T = len(ns)
    npairs, L, rn, nbx = T * (T + 1) // 2, sum(n * (T - k) for k, n in enumerate(ns)), sum(ns), (ns[0] + 255) // 256
    sizes = [8 * (1 + d), 8 * (B + 1), 4, 8 * npairs * (1 + d), 8 * L, (16 if fam == 0 else 8) * L, 16 * L if fam == 0 else 0,
             16 * L, 16 * L, 16 * L, 16 * L, 16 * B * rn, 8 * ns[-1], 8 * (npairs + 1) * 2 * nbx, 8 * (1 + d) * nbx]
    assert o[0] == 0 and all(v % 256 == 0 for v in o) and nb.value % 256 == 0
    for i in range(15):
        end = o[i + 1] if i < 14 else nb.value
        assert o[i] + sizes[i] <= end < o[i] + sizes[i] + 512, (i, o, sizes, nb.value)


def test_wide_mt_fit_hooks_validate_without_a_device():
    lib = N.lib()
    offs = (ctypes.c_int64 * 15)()
    assert lib.fgp_wide_mt_fit_work_layout(ctypes.byref(_mt_desc()), None) == FGP_ERR_INVALID
    assert lib.fgp_wide_mt_fit_work_layout(None, offs) == FGP_ERR_INVALID
    for field, kw in (("d", dict(d=8, dl=8)), ("B", dict(B=0)), ("dl", dict(dl=3)), ("rank", dict(rank=-1))):
        assert lib.fgp_wide_mt_fit_work_layout(ctypes.byref(_mt_desc(**kw)), offs) == FGP_ERR_INVALID
        msg = lib.fgp_last_error()
        assert b"fgp_wide_mt_fit_work_layout" in msg and field.encode() in msg, msg
        assert lib.fgp_wide_mt_fit_stage(ctypes.byref(_mt_desc(**kw)), 0, 1, 0, None) == FGP_ERR_INVALID
        assert b"fgp_wide_mt_fit_stage" in lib.fgp_last_error()
    bad = [(-1, 0), (9, 0), (0, 2), (0, -1), (8, 0), (8, 3)] + [(s, 1) for s in range(1, 8)]
    for stage, mode in bad:
        rc = lib.fgp_wide_mt_fit_stage(ctypes.byref(_mt_desc()), 0, stage, mode, None)
        msg = lib.fgp_last_error()
        assert rc == FGP_ERR_INVALID and b"fgp_wide_mt_fit_stage" in msg and (b"stage" in msg or b"mode" in msg), (stage, mode, msg)
    assert lib.fgp_wide_mt_fit_stage(ctypes.byref(_mt_desc(lr=-1.0)), 0, 0, 1, None) == FGP_ERR_INVALID
    assert b"lr" in lib.fgp_last_error()
    assert lib.fgp_wide_mt_fit_stage(ctypes.byref(_mt_desc()), -1, 1, 0, None) == FGP_ERR_INVALID and b"iter" in lib.fgp_last_error()
    assert lib.fgp_wide_mt_fit_stage(ctypes.byref(_mt_desc(work=None)), 0, 1, 0, None) == FGP_ERR_INVALID
    assert b"work" in lib.fgp_last_error()
