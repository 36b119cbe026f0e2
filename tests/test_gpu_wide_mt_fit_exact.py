"""fgp_wide_mt_fit_run on the device, stage by stage (fgp_wide_mt_fit_stage, fgp_wide_mt_fit_work_layout).

Per case: the work buffer filled with 0xFF bytes, the histories and grad_out with NaN; two iterations issued one stage
at a time, every stage checked on the bits the device produced for the stage before:

  prologue   nat = exp(raw) within the bound, gn = 1/2, gl = 1/2 w and info = 0 exactly, a new fit's Rprop state;
  k1, forward, blocks, adjoint, k1_bwd   the work buffer against the stand-alone entry points (fgp_wide_mt_k1 per pair,
             the transforms batched over the T - k rows of sorted task k -- the half-length ones from n_k = 2^17 --,
             fgp_mt_factor / _solve / _selinv / _mll_grad, fgp_wide_mt_k1_bwd per pair) with the same arguments, BIT FOR BIT;
  lams       k_wide_mt_lams against mt_lams_ref within the bound;
  contract   g~ over lambda and the workgroup partials against mt_contract_ref; a workgroup past its pair's n_k writes
             nothing (the fill stays: in `big`, 510 of the 512 partials of each row of the shorter task's pairs);
  step       the loss row and every raw gradient against mt_step_ref (which reads only the first ceil(n_k / 256)
             partials of a pair: a read of the unwritten NaN tail would show), Rprop bit for bit, the new natural row;
every compared output finite, every bound inside the non-vacuity cap, every stage re-issued on the same inputs giving
the same bits; then fgp_wide_mt_fit_run itself (iters = 2, fresh copies) bit for bit the staged sequence."""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import wide_fit_cases as C
from tests import wide_fit_reference as R
from tests.gpu_fixtures import DEV, uses_r2c
from tests.gpu_fixtures import raw_stream as _stream
from tests.gpu_fixtures import same_bits as _same
from tests.gpu_fixtures import to_dev as _dev
from tests.gpu_fixtures import to_np as _np

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

PROLOGUE, K1, FORWARD, LAMS, BLOCKS, CONTRACT, ADJOINT, K1BWD, STEP = range(9)
NAMES = ("nat", "gn", "info", "dsl", "A", "B", "W", "lams", "fac", "zinv", "glp", "z", "logdet", "part", "pb")
WORST = {}


def _note(stage, fam, name, what, t, got, Cn):
    r = R.rel(got, t, Cn)
    vac, fin = R.vacuity(t, Cn)
    key = (stage, "lattice" if fam == C.LAT else "net")
    WORST[key] = max(WORST.get(key, 0.0), r)
    print("%-16s %-10s %-10s err / bound = %.3f   ||u e|| / cap = %.3g" % (name, stage, what, r, vac))
    assert fin and vac <= 1.0, (name, stage, what, "vacuous bound", vac)
    assert r <= 1.0, (name, stage, what, r)


def _bp(t, nbytes=0):
    return ctypes.c_void_p(t.data_ptr() + nbytes)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    """After the module's tests: the table of DESIGN.md section 3.5.1 (a report; every ratio is asserted where measured)."""
    yield
    print()
    for key in sorted(WORST):
        print("| `%s` | %s | %.3f |" % (key + (WORST[key],)))


class DeviceMt(object):
    def __init__(self, c, inp):
        self.c, self.sp = c, C.mt_spec(c)
        sp = self.sp
        self.lat = c.fam == C.LAT
        self.parts = [_dev(p[0]) for p in inp["pairs"]]
        self.ind = [N.int_array(p[1].reshape(-1)) for p in inp["pairs"]]
        self.cc = [N.double_array(p[2]) for p in inp["pairs"]]
        self.y, self.raw = _dev(inp["y"]), _dev(inp["raw"])
        n = sp.n_params
        self.prev = torch.full((n,), float("nan"), device=DEV)
        self.step = torch.full((n,), float("nan"), device=DEV)
        self.grad = torch.full((n,), float("nan"), device=DEV)
        self.loss_hist = torch.full((2, 3), float("nan"), device=DEV)
        self.raw_hist = torch.full((2, n), float("nan"), device=DEV)
        desc = N.WideMtFitDesc(family=c.fam, d=c.d, B=c.B, T_all=c.T_all, rank=c.rank, dl=c.dl, y=self.y.data_ptr(),
                               raw=self.raw.data_ptr(), vtask_exp=c.vexp, rg_scale=c.rg[0], rg_ls=c.rg[1], rg_noise=c.rg[2],
                               rg_factor=c.rg[3], rg_vtask=c.rg[4], rprop_prev=self.prev.data_ptr(),
                               rprop_step=self.step.data_ptr(), lr=c.lr, eta_minus=C.ETAS[0], eta_plus=C.ETAS[1],
                               step_min=C.STEPS[0], step_max=C.STEPS[1], logdet_weight=sp.logdet_weight, mll_const=sp.mll_const,
                               loss_hist=self.loss_hist.data_ptr(), raw_hist=self.raw_hist.data_ptr(),
                               grad_out=self.grad.data_ptr(), work=0)
        desc.layout.T = sp.T
        for k in range(sp.T):
            desc.layout.n[k] = sp.ns[k]
            desc.task[k] = c.task[k]
        for q in range(sp.np):
            desc.pair[q].parts = self.parts[q].data_ptr()
            desc.pair[q].ind = ctypes.cast(self.ind[q], ctypes.c_void_p)
            desc.pair[q].cc = ctypes.cast(self.cc[q], ctypes.c_void_p)
            desc.pair[q].P = c.P
            desc.pair[q].conj = c.conj[q]
        nb = ctypes.c_int64(0)
        N.call("fgp_wide_mt_fit_work", desc, ctypes.byref(nb))
        offs = (ctypes.c_int64 * 15)()
        N.call("fgp_wide_mt_fit_work_layout", desc, offs)
        self.off = dict(zip(NAMES, list(offs)))
        self.work = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
        self.work.fill_(255)
        desc.work = self.work.data_ptr()
        self.desc = desc
        self.mtlay = N.MtLayout()
        self.mtlay.T = sp.T
        for k in range(sp.T):
            self.mtlay.n[k] = sp.ns[k]
        L, d, B = sp.lay.L, c.d, c.B
        cd = torch.complex128
        self.shape = {"nat": (torch.float64, 1 + d), "gn": (torch.float64, B + 1), "info": (torch.int32, 1),
                      "dsl": (torch.float64, sp.np * (1 + d)), "A": (torch.float64, L),
                      "B": (cd if self.lat else torch.float64, L), "lams": (cd, L), "fac": (cd, L), "zinv": (cd, L),
                      "glp": (cd, L), "z": (cd, B * sp.rn), "logdet": (torch.float64, sp.lay.nmin),
                      "part": (torch.float64, (sp.np + 1) * 2 * sp.nbx)}

    def v(self, name):
        dt, cnt = self.shape[name]
        o = self.off[name]
        return self.work[o:o + cnt * torch.empty(0, dtype=dt).element_size()].view(dt)

    def state(self):
        return [t.clone() for t in (self.work, self.raw, self.prev, self.step, self.grad, self.loss_hist, self.raw_hist)]

    def restore(self, st):
        for t, s in zip((self.work, self.raw, self.prev, self.step, self.grad, self.loss_hist, self.raw_hist), st):
            t.copy_(s)

    def issue(self, it, stage, mode=0):
        N.call("fgp_wide_mt_fit_stage", self.desc, int(it), int(stage), int(mode), _stream())
        torch.cuda.synchronize()

    def issue_twice(self, it, stage, mode=0):
        before = self.state()
        self.issue(it, stage, mode)
        after = self.state()
        self.restore(before)
        self.issue(it, stage, mode)
        for a, b in zip(after, self.state()):
            assert _same(a, b), (self.c.name, "stage %d does not repeat" % stage)

    # ---- the stand-alone entry points on the buffer's own contents
    def k1_direct(self):
        sp, c = self.sp, self.c
        out = torch.full((sp.lay.L,), float("nan"), device=DEV)
        nat = self.v("nat").clone()
        for q, (k, l) in enumerate(sp.pairs):
            N.call("fgp_wide_mt_k1", N.ptr(self.parts[q]), sp.ns[k], c.d, c.P, self.ind[q], self.cc[q], _bp(nat), _bp(nat, 8), 1,
                   _bp(out, 8 * sp.lay.off[k, l]), _stream())
        return out

    def transform_direct(self, adjoint):
        sp = self.sp
        L = sp.lay.L
        src = (self.v("B") if adjoint else self.v("A")).clone()
        out = torch.full((L,), float("nan"), device=DEV, dtype=torch.float64 if adjoint or not self.lat else torch.complex128)
        W = torch.empty(2 * L, device=DEV)
        es_in, es_out = src.element_size(), out.element_size()
        for k in range(sp.T):
            n, rows, lg = sp.ns[k], sp.T - k, sp.ns[k].bit_length() - 1
            o = sp.lay.off[k, k]
            i_, o_ = _bp(src, es_in * o), _bp(out, es_out * o)
            r2c = uses_r2c(self.lat, lg)
            if not self.lat:
                N.call("fgp_fwht", i_, n, o_, rows, lg, 1, _stream())
            elif adjoint and r2c:
                N.call("fgp_ifftbr_real", i_, n, None, 0, o_, n, N.ptr(W), rows, lg, _stream())
            elif adjoint:
                N.call("fgp_ifftbr", i_, n, o_, 1, N.ptr(W), rows, lg, 1, _stream())
            elif r2c:
                N.call("fgp_fftbr_real", i_, n, o_, N.ptr(W), rows, lg, _stream())
            else:
                N.call("fgp_fftbr", i_, n, 1, o_, rows, lg, 1, _stream())
        return out

    def blocks_direct(self):
        sp, c = self.sp, self.c
        L = sp.lay.L
        lams, gn = self.v("lams").clone(), self.v("gn").clone()
        fac, zinv, glp = (torch.full((L,), float("nan"), device=DEV, dtype=torch.complex128) for _ in range(3))
        z = torch.full((c.B * sp.rn,), float("nan"), device=DEV, dtype=torch.complex128)
        ld = torch.full((sp.lay.nmin,), float("nan"), device=DEV)
        info = torch.zeros(1, dtype=torch.int32, device=DEV)
        lay = ctypes.byref(self.mtlay)
        N.call("fgp_mt_factor", lay, N.ptr(lams), 1, N.ptr(fac), N.ptr(ld), N.ptr(info), _stream())
        N.call("fgp_mt_solve", lay, N.ptr(fac), 1, N.ptr(self.y), sp.rn, c.B, N.ptr(z), _stream())
        N.call("fgp_mt_selinv", lay, N.ptr(fac), 1, N.ptr(zinv), _stream())
        N.call("fgp_mt_mll_grad", lay, N.ptr(zinv), N.ptr(z), _bp(gn), _bp(gn, 8 * c.B), c.B, 1, N.ptr(glp), _stream())
        return {"fac": fac, "logdet": ld, "z": z, "zinv": zinv, "glp": glp, "info": info}

    def k1_bwd_direct(self):
        sp, c = self.sp, self.c
        d = c.d
        dsl = torch.full((sp.np * (1 + d),), float("nan"), device=DEV)
        nat, u = self.v("nat").clone(), self.v("A").clone()
        for q, (k, l) in enumerate(sp.pairs):
            wl = ctypes.c_int64(0)
            N.call("fgp_wide_mt_k1_bwd_work", sp.ns[k], d, c.P, 1, ctypes.byref(wl))
            wk = torch.empty(max(1, wl.value), device=DEV)
            N.call("fgp_wide_mt_k1_bwd", N.ptr(self.parts[q]), sp.ns[k], d, c.P, self.ind[q], self.cc[q], _bp(nat), _bp(nat, 8), 1,
                   _bp(u, 8 * sp.lay.off[k, l]), _bp(dsl, 8 * q * (1 + d)), _bp(dsl, 8 * (q * (1 + d) + 1)), N.ptr(wk), _stream())
        return dsl


def check_nat(dm, stage, raw):
    c = dm.c
    _note(stage, c.fam, c.name, "nat", R.mt_nat_ref(dm.sp, raw), _np(dm.v("nat")), 2 * R.ULP_LIBM + 1)


def run_staged(c, inp):
    dm = DeviceMt(c, inp)
    sp = dm.sp
    Cn = sp.counts()
    mask = sp.rg_mask(c.rg)
    raw0 = inp["raw"]
    dm.issue_twice(0, PROLOGUE, 1)
    check_nat(dm, "prologue", raw0)
    gn = _np(dm.v("gn"))
    assert (gn[:c.B] == 0.5).all() and gn[c.B] == 0.5 * sp.logdet_weight and int(dm.v("info")[0]) == 0
    assert bool((dm.prev == 0).all()) and bool((dm.step == c.lr).all()) and _same(dm.raw, _dev(raw0))
    for it in (0, 1):
        raw = _np(dm.raw)
        dm.issue_twice(it, K1)
        assert _same(dm.v("A"), dm.k1_direct()), (c.name, it, "k1 is not fgp_wide_mt_k1's")
        dm.issue_twice(it, FORWARD)
        assert _same(dm.v("B"), dm.transform_direct(False)), (c.name, it, "lambda is not the stand-alone transforms'")
        lam = _np(dm.v("B"))
        assert np.isfinite(lam.view(np.float64)).all()
        dm.issue_twice(it, LAMS)
        assert _same(dm.v("B"), _dev(lam)), (c.name, "k_wide_mt_lams touched lambda")
        lams = _np(dm.v("lams"))
        X, Y = R.mt_lams_ref(sp, raw, lam)
        assert np.isfinite(lams.view(np.float64)).all()
        _note("lams", c.fam, c.name, "re", X, lams.real, Cn["lams"])
        _note("lams", c.fam, c.name, "im", Y, lams.imag, Cn["lams"])
        want = dm.blocks_direct()
        dm.issue_twice(it, BLOCKS)
        for k, t in want.items():
            assert _same(dm.v(k), t), (c.name, it, k, "the block stage is not the stand-alone entry point's")
            assert bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t.to(torch.float64)).all()), k
        assert int(dm.v("info")[0]) == 0
        glp, z, ld = _np(dm.v("glp")), _np(dm.v("z")), _np(dm.v("logdet"))
        dm.issue_twice(it, CONTRACT)
        cr = R.mt_contract_ref(sp, raw, glp, lam, inp["y"], z, ld)
        gt = _np(dm.v("B"))
        assert np.isfinite(gt.view(np.float64)).all()
        _note("contract", c.fam, c.name, "g~ re", cr["gx"], gt.real, Cn["contract"])
        if dm.lat:
            _note("contract", c.fam, c.name, "g~ im", cr["gy"], gt.imag, Cn["contract"])
        part = dm.v("part").view(sp.np + 1, 2, sp.nbx)
        wr = torch.from_numpy(cr["written"]).to(DEV)
        assert bool((part[~wr].contiguous().view(torch.uint8) == 255).all()), (c.name, "a workgroup past n_k wrote a partial")
        parth = _np(part)
        assert np.isfinite(parth[cr["written"]]).all()
        ph = np.where(cr["written"], parth, np.nan)
        _note("contract", c.fam, c.name, "partials", cr["part"], ph, Cn["contract"])
        want = dm.transform_direct(True)
        dm.issue_twice(it, ADJOINT)
        assert _same(dm.v("A"), want), (c.name, it, "u is not the stand-alone adjoint transforms'")
        want = dm.k1_bwd_direct()
        dm.issue_twice(it, K1BWD)
        assert _same(dm.v("dsl"), want), (c.name, it, "k1_bwd is not fgp_wide_mt_k1_bwd's")
        assert bool(torch.isfinite(want).all())
        before = {k: _np(getattr(dm, k)) for k in ("raw", "prev", "step")}
        dsl, nat = _np(dm.v("dsl")).reshape(sp.np, 1 + c.d), _np(dm.v("nat"))
        dm.issue_twice(it, STEP, 2)
        st = R.mt_step_ref(sp, raw, parth, dsl, nat)
        lh, grad = _np(dm.loss_hist[it]), _np(dm.grad)
        assert np.isfinite(lh).all() and np.isfinite(grad).all()
        _note("step", c.fam, c.name, "loss row", st["loss"], lh, Cn["step"])
        _note("step", c.fam, c.name, "grad_out", st["grad"], grad, Cn["step"])
        assert np.array_equal(_np(dm.raw_hist[it]), before["raw"])
        w_raw, w_prev, w_step, prod = R.rprop_f64(grad, before["raw"], before["prev"], before["step"], mask, *C.ETAS, *C.STEPS)
        for k, want in (("raw", w_raw), ("prev", w_prev), ("step", w_step)):
            got = _np(getattr(dm, k))
            assert np.array_equal(got, want) and np.isfinite(got).all(), (c.name, k)
            assert np.array_equal(got[~mask].view(np.int64), before[k][~mask].view(np.int64)), (c.name, k, "frozen moved")
        if it == 0:
            assert (prod == 0).all()
        check_nat(dm, "step", _np(dm.raw))
    return dm


@pytest.mark.parametrize("name", [c.name for c in C.MT_CASES])
def test_two_iterations_stage_by_stage(name):
    c = C.MT_BY_NAME[name]
    inp = C.mt_inputs(name)
    staged = run_staged(c, inp)
    whole = DeviceMt(c, inp)
    N.call("fgp_wide_mt_fit_run", whole.desc, 0, 2, 0, _stream())
    torch.cuda.synchronize()
    for k in ("loss_hist", "raw_hist", "raw", "grad", "prev", "step"):
        assert _same(getattr(staged, k), getattr(whole, k)), (name, k, "the run differs from the staged sequence")
    assert not _same(whole.raw, _dev(inp["raw"]))
