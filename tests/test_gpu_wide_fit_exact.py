"""fgp_wide_fit_run on the device, stage by stage (fgp_wide_fit_stage, fgp_wide_fit_work_layout).

Per case: the work buffer filled with 0xFF bytes, the histories and grad_out with NaN; two iterations issued one stage
at a time, every stage checked on the bits the device produced for the stage before:

  prologue   the natural rows against exp(raw) within the bound; a new fit's Rprop state (prev = 0, step = lr);
  k1, forward, adjoint, k1_bwd   the work buffer against the stand-alone entry point called with the same arguments, BIT
             FOR BIT (per problem under parts_stride != 0; the half-length transforms from n = 2^17);
  terms      k_wide_fit_eig: g~ and the three partials against eig_ref within the bound, the lattice's imaginary parts
             exactly 0, nothing written past n;  GCV / CV: k_wide_fit_loss_sums' partials (lambda untouched, CV's row 3
             still the fill) and k_wide_fit_loss_grad's g~;
  step       the loss row and grad_out against step_ref, the raw_hist row, Rprop bit for bit against its float64
             restatement on the device's own grad_out, the natural rows of the new parameters;
every compared output finite, every bound inside the non-vacuity cap, every stage re-issued on the same inputs giving
the same bits.  Then fgp_wide_fit_run itself (iters = 2, fresh copies): histories, raw, grad_out and the Rprop state bit
for bit those of the staged sequence; and for G > 1 every problem run alone (G = 1), bit for bit.
The bounds are those of tests/wide_fit_reference.py: counted from the kernels' roundings, never fitted."""
import ctypes

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import wide_fit_cases as C
from tests import wide_fit_reference as R
from tests.gpu_fixtures import DEV, uses_r2c
from tests.gpu_fixtures import bits as _bits
from tests.gpu_fixtures import raw_stream as _stream
from tests.gpu_fixtures import same_bits as _same
from tests.gpu_fixtures import to_dev as _dev
from tests.gpu_fixtures import to_np as _np

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

PROLOGUE, K1, FORWARD, TERMS, TERMS2, ADJOINT, K1BWD, STEP = range(8)
NAMES = ("nat_scale", "nat_ls", "dscale", "dls", "A", "B", "W", "pe", "pb", "pl")
WORST = {}          # (stage, family) -> worst err / bound


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 8 * off)


def _note(stage, fam, name, what, t, got, Cn):
    r = R.rel(got, t, Cn)
    vac, fin = R.vacuity(t, Cn)
    key = (stage, "lattice" if fam == C.LAT else "net")
    WORST[key] = max(WORST.get(key, 0.0), r)
    print("%-22s %-10s %-10s err / bound = %.3f   ||u e|| / cap = %.3g" % (name, stage, what, r, vac))
    assert fin and vac <= 1.0, (name, stage, what, "vacuous bound", vac)
    assert r <= 1.0, (name, stage, what, r)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    """After the module's tests: the table of DESIGN.md section 3.5.1 (a report; every ratio is asserted where measured)."""
    yield
    print()
    for key in sorted(WORST):
        print("| `%s` | %s | %.3f |" % (key + (WORST[key],)))


class DeviceFit(object):
    """A problem on the device: desc, buffers, views of the work buffer."""

    def __init__(self, c, parts, ysq, raw, prev=None, step=None):
        self.c = c
        self.n, self.G, self.d, self.dl = 1 << c.m, int(ysq.shape[0]), c.d, c.dl
        G, n, d = self.G, self.n, self.d
        self.own = parts.ndim == 3
        self.parts, self.ysq, self.raw = _dev(parts), _dev(ysq), _dev(raw)
        npar = self.npar = G * (2 + c.dl)
        self.prev = _dev(prev) if prev is not None else torch.full((npar,), float("nan"), device=DEV)
        self.step = _dev(step) if step is not None else torch.full((npar,), float("nan"), device=DEV)
        self.grad = torch.full((npar,), float("nan"), device=DEV)
        self.rows = c.iter0 + 2
        self.loss_hist = torch.full((self.rows, G, 3), float("nan"), device=DEV)
        self.raw_hist = torch.full((self.rows, npar), float("nan"), device=DEV)
        self.desc = desc = N.WideFitDesc(
            family=c.fam, log2n=c.m, d=d, G=G, parts=self.parts.data_ptr(), parts_stride=d * n if self.own else 0,
            ysq=self.ysq.data_ptr(), raw=self.raw.data_ptr(), dl=c.dl, scale_rg=c.rg[0], ls_rg=c.rg[1], noise_rg=c.rg[2],
            logdet_weight=C.LOGDET_WEIGHT, mll_const=C.MLL_CONST, rprop_prev=self.prev.data_ptr(),
            rprop_step=self.step.data_ptr(), lr=c.lr, eta_minus=C.ETAS[0], eta_plus=C.ETAS[1], step_min=C.STEPS[0],
            step_max=C.STEPS[1], loss_hist=self.loss_hist.data_ptr(), raw_hist=self.raw_hist.data_ptr(),
            grad_out=self.grad.data_ptr(), work=0, loss_metric=c.loss, cv_weight=C.CV_WEIGHT)
        wlen = ctypes.c_int64(0)
        N.call("fgp_wide_fit_work", desc, ctypes.byref(wlen))
        offs = (ctypes.c_int64 * 10)()
        N.call("fgp_wide_fit_work_layout", desc, offs)
        self.off = dict(zip(NAMES, list(offs)))
        self.off["end"] = wlen.value
        self.work = torch.empty(wlen.value, dtype=torch.float64, device=DEV)
        self.work.view(torch.uint8).fill_(255)
        desc.work = self.work.data_ptr()
        self.nbe = R.nbe_of(n)
        cx = 2 if c.fam == C.LAT else 1
        self.len = {"nat_scale": G, "nat_ls": G * d, "dscale": G, "dls": G * d, "A": G * n, "B": G * n * cx,
                    "pe": G * 3 * self.nbe, "pl": 0 if c.loss == C.MLL else G * 4 * self.nbe}

    def v(self, name):
        o = self.off[name]
        return self.work[o:o + self.len[name]]

    def lam_real(self):
        b = self.v("B")
        return (b.view(self.G, self.n, 2)[..., 0] if self.c.fam == C.LAT else b.view(self.G, self.n)).cpu().numpy().copy()

    def padding_untouched(self, name, nxt):
        """The doubles between the end of array `name` and the start of `nxt` still hold the 0xFF fill."""
        gap = self.work[self.off[name] + self.len[name]:self.off[nxt]]
        return bool((gap.view(torch.uint8) == 255).all())

    def state(self):
        return [t.clone() for t in (self.work, self.raw, self.prev, self.step, self.grad, self.loss_hist, self.raw_hist)]

    def restore(self, st):
        for t, s in zip((self.work, self.raw, self.prev, self.step, self.grad, self.loss_hist, self.raw_hist), st):
            t.copy_(s)

    def issue(self, it, stage, mode=0):
        N.call("fgp_wide_fit_stage", self.desc, int(it), int(stage), int(mode), _stream())
        torch.cuda.synchronize()

    def issue_twice(self, it, stage, mode=0):
        """The stage, then the stage again on the same inputs: the same bits everywhere (scratch included)."""
        before = self.state()
        self.issue(it, stage, mode)
        after = self.state()
        self.restore(before)
        self.issue(it, stage, mode)
        for a, b in zip(after, self.state()):
            assert _same(a, b), (self.c.name, "stage %d does not repeat" % stage)

    # ---- the stand-alone entry points on the buffer's own contents
    def k1_direct(self):
        G, n, d = self.G, self.n, self.d
        out = torch.full((G, n), float("nan"), device=DEV)
        sc, ls = self.v("nat_scale").clone(), self.v("nat_ls").clone()
        if not self.own:
            N.call("fgp_wide_k1", N.ptr(self.parts), n, d, N.ptr(sc), N.ptr(ls), G, N.ptr(out), _stream())
        else:
            for g in range(G):
                N.call("fgp_wide_k1", _vp(self.parts, g * d * n), n, d, _vp(sc, g), _vp(ls, g * d), 1, _vp(out, g * n), _stream())
        return out.reshape(-1)

    def transform_direct(self, adjoint):
        c, G, n, m = self.c, self.G, self.n, self.c.m
        lat, r2c = c.fam == C.LAT, uses_r2c(c.fam == C.LAT, m)
        src = (self.v("B") if adjoint else self.v("A")).clone()
        out = torch.full((G * n * (1 if adjoint or not lat else 2),), float("nan"), device=DEV)
        W = torch.empty(2 * G * n, device=DEV)
        if not lat:
            N.call("fgp_fwht", N.ptr(src), n, N.ptr(out), G, m, 1, _stream())
        elif adjoint and r2c:
            N.call("fgp_ifftbr_real", N.ptr(src), n, None, 0, N.ptr(out), n, N.ptr(W), G, m, _stream())
        elif adjoint:
            N.call("fgp_ifftbr", N.ptr(src), n, N.ptr(out), 1, N.ptr(W), G, m, 1, _stream())
        elif r2c:
            N.call("fgp_fftbr_real", N.ptr(src), n, N.ptr(out), N.ptr(W), G, m, _stream())
        else:
            N.call("fgp_fftbr", N.ptr(src), n, 1, N.ptr(out), G, m, 1, _stream())
        return out

    def k1_bwd_direct(self):
        G, n, d = self.G, self.n, self.d
        ds, dl = torch.full((G,), float("nan"), device=DEV), torch.full((G * d,), float("nan"), device=DEV)
        sc, ls, u = self.v("nat_scale").clone(), self.v("nat_ls").clone(), self.v("A").clone()
        wl = ctypes.c_int64(0)
        N.call("fgp_wide_k1_bwd_work", n, d, G, ctypes.byref(wl))
        wk = torch.empty(wl.value, device=DEV)
        if not self.own:
            N.call("fgp_wide_k1_bwd", N.ptr(self.parts), n, d, N.ptr(sc), N.ptr(ls), G, N.ptr(u), N.ptr(ds), N.ptr(dl), N.ptr(wk),
                   _stream())
        else:
            for g in range(G):
                N.call("fgp_wide_k1_bwd", _vp(self.parts, g * d * n), n, d, _vp(sc, g), _vp(ls, g * d), 1, _vp(u, g * n),
                       _vp(ds, g), _vp(dl, g * d), N.ptr(wk), _stream())
        return ds, dl


def check_nat(df, stage, raw):
    c = df.c
    ns, nl = R.nat_ref(raw, df.G, df.d, df.dl)
    Cn = 2 * R.ULP_LIBM + 1
    _note(stage, c.fam, c.name, "nat_scale", ns, _np(df.v("nat_scale")), Cn)
    _note(stage, c.fam, c.name, "nat_ls", nl, _np(df.v("nat_ls")), Cn)


def check_terms(df, it):
    """The terms stage(s) of iteration `it` from the lambda in the buffer."""
    c, G, n, nbe = df.c, df.G, df.n, df.nbe
    Cn = R.counts(n, df.d)
    lam = df.lam_real()
    lam_bits = df.v("B").clone()
    raw_noise = _np(df.raw)[G * (1 + df.dl):]
    Y = _np(df.ysq)
    lat = c.fam == C.LAT

    def g_tilde():
        b = df.v("B")
        if lat:
            b = b.view(G, n, 2)
            assert bool((_bits(b[..., 1]) == 0).all()), (c.name, "the imaginary part of g~ is not +0")
            b = b[..., 0]
        assert df.padding_untouched("B", "W"), (c.name, "written past n")
        return _np(b).reshape(G, n)

    if c.loss == C.MLL:
        df.issue_twice(it, TERMS)
        ref = R.eig_ref(lam, Y, raw_noise, n, C.LOGDET_WEIGHT)
        gt, pe = g_tilde(), _np(df.v("pe")).reshape(G, 3, nbe)
        assert np.isfinite(gt).all() and np.isfinite(pe).all()
        _note("eig", c.fam, c.name, "g~", ref["gt"], gt, Cn["terms"])
        _note("eig", c.fam, c.name, "partials", ref["pe"], pe, Cn["terms"])
        assert df.padding_untouched("pe", "pb")
        return
    cv = c.loss == C.CV
    df.issue_twice(it, TERMS)
    assert _same(df.v("B"), lam_bits), (c.name, "k_wide_fit_loss_sums touched lambda")
    pl = df.v("pl").view(G, 4, nbe)
    ref = R.loss_sums_ref(lam, Y, raw_noise, n, cv)
    got = _np(pl[:, :3 if cv else 4])
    assert np.isfinite(got).all()
    _note("loss_sums", c.fam, c.name, "partials", ref, got, Cn["sums"])
    if cv:
        assert bool((_bits(pl[:, 3]) == 255).all()), (c.name, "CV wrote partial row 3")
    df.issue_twice(it, TERMS2)
    plh = _np(pl)
    ref = R.loss_grad_ref(lam, Y, raw_noise, plh, n, C.CV_WEIGHT, cv)
    gt = g_tilde()
    assert np.isfinite(gt).all()
    _note("loss_grad", c.fam, c.name, "g~", ref, gt, Cn["grad"])
    assert _same(df.v("pl"), _dev(plh.reshape(-1))), (c.name, "k_wide_fit_loss_grad touched the partials")
    if cv:
        assert bool((_bits(pl[:, 3]) == 255).all()), (c.name, "CV row 3 after pass 2")


def check_step(df, it, row, mode, mask):
    """The step of history row `row`: returns Rprop's products over the updated parameters."""
    c, G, n, d, dl = df.c, df.G, df.n, df.d, df.dl
    Cn = R.counts(n, d)
    before = {k: _np(getattr(df, k)) for k in ("raw", "prev", "step")}
    nat_before = (df.v("nat_scale").clone(), df.v("nat_ls").clone())
    pe = _np(df.v("pe" if c.loss == C.MLL else "pl")).reshape(G, 3 if c.loss == C.MLL else 4, df.nbe)
    dscale, dls = _np(df.v("dscale")), _np(df.v("dls"))
    ns, nl = _np(nat_before[0]), _np(nat_before[1])
    df.issue_twice(row, STEP, mode)
    ref = R.step_ref(c.loss, pe, dscale, dls, ns, nl, before["raw"], G, d, dl, n, C.LOGDET_WEIGHT, C.MLL_CONST, C.CV_WEIGHT)
    lh, grad = _np(df.loss_hist[row]), _np(df.grad)
    assert np.isfinite(grad).all()
    if c.loss == C.CV:
        assert np.isfinite(lh[:, 0]).all() and np.isnan(lh[:, 1:]).all()
    else:
        assert np.isfinite(lh).all()
    _note("step", c.fam, c.name, "loss row", ref["loss"], lh, Cn["step"])
    _note("step", c.fam, c.name, "grad_out", ref["grad"], grad, Cn["step"])
    assert np.array_equal(_np(df.raw_hist[row]), before["raw"])
    after = {k: _np(getattr(df, k)) for k in ("raw", "prev", "step")}
    if mode == 1:
        for k in after:
            assert np.array_equal(after[k].view(np.int64), before[k].view(np.int64)), (c.name, k, "moved without an update")
        assert _same(df.v("nat_scale"), nat_before[0]) and _same(df.v("nat_ls"), nat_before[1])
        return np.zeros(0)
    raw, prev, step, prod = R.rprop_f64(grad, before["raw"], before["prev"], before["step"], mask, *C.ETAS, *C.STEPS)
    for k, want in (("raw", raw), ("prev", prev), ("step", step)):
        assert np.array_equal(after[k], want), (c.name, k)
        assert np.array_equal(after[k][~mask].view(np.int64), before[k][~mask].view(np.int64)), (c.name, k, "frozen moved")
        assert np.isfinite(after[k]).all()
    check_nat(df, "step", after["raw"])
    return prod[mask]


def run_staged(c, inp):
    """Two iterations stage by stage; returns the DeviceFit and the caller state it used (None: the device's own)."""
    df = DeviceFit(c, inp["parts"], inp["ysq"], inp["raw"])
    mask = R.rg_mask(df.G, df.dl, c.rg)
    caller = None
    init = c.iter0 == 0 and c.lr > 0
    if not init and c.lr > 0:                    # a continued fit: the state of the iterations before
        caller = (np.linspace(-0.5, 0.5, df.npar), np.full(df.npar, 0.1))
        df.prev.copy_(_dev(caller[0]))
        df.step.copy_(_dev(caller[1]))
    df.issue_twice(0, PROLOGUE, int(init))
    check_nat(df, "prologue", inp["raw"])
    if init:
        assert bool((df.prev == 0).all()) and bool((df.step == c.lr).all())
    assert _same(df.raw, _dev(inp["raw"]))
    for it in (0, 1):
        row = c.iter0 + it
        df.issue_twice(row, K1)
        assert _same(df.v("A"), df.k1_direct()), (c.name, it, "k1 is not fgp_wide_k1's")
        assert bool(torch.isfinite(df.v("A")).all())
        df.issue_twice(row, FORWARD)
        assert _same(df.v("B"), df.transform_direct(False)), (c.name, it, "lambda is not the stand-alone transform's")
        assert bool(torch.isfinite(df.v("B")).all())
        check_terms(df, row)
        want = df.transform_direct(True)
        df.issue_twice(row, ADJOINT)
        assert _same(df.v("A"), want), (c.name, it, "u is not the stand-alone adjoint transform's")
        ds, dl = df.k1_bwd_direct()
        df.issue_twice(row, K1BWD)
        assert _same(df.v("dscale"), ds) and _same(df.v("dls"), dl), (c.name, it, "k1_bwd is not fgp_wide_k1_bwd's")
        assert bool(torch.isfinite(df.v("dscale")).all()) and bool(torch.isfinite(df.v("dls")).all())
        mode = 1 if (it == 1 and c.fnu) else 2
        if it == 0 and c.lr <= 0:                # the caller's state, built from the gradient of an evaluation
            df.issue(row, STEP, 1)
            caller = C.caller_state(_np(df.grad), mask)
            df.prev.copy_(_dev(caller[0]))
            df.step.copy_(_dev(caller[1]))
        prod = check_step(df, it, row, mode, mask)
        if it == 0 and init:
            assert (prod == 0).all()
        if it == 0 and c.lr <= 0:
            st = _np(df.step)[mask]
            assert (prod > 0).any() and (prod < 0).any() and (prod == 0).any(), prod
            assert (st == C.STEPS[0]).any() and (st == C.STEPS[1]).any(), st
            assert ((st > C.STEPS[0]) & (st < C.STEPS[1])).any()
    return df, caller


def run_entry(c, parts, ysq, raw, caller, sel=None):
    """fgp_wide_fit_run, iters = 2, on fresh copies (sel: the parameter indices of one problem of a larger run)."""
    prev, step = (None, None) if caller is None else ((caller[0], caller[1]) if sel is None else (caller[0][sel], caller[1][sel]))
    df = DeviceFit(c, parts, ysq, raw, prev, step)
    N.call("fgp_wide_fit_run", df.desc, c.iter0, 2, int(c.fnu), _stream())
    torch.cuda.synchronize()
    return df


@pytest.mark.parametrize("name", [c.name for c in C.WF_CASES])
def test_two_iterations_stage_by_stage(name):
    c = C.WF_BY_NAME[name]
    inp = C.wf_inputs(name)
    staged, caller = run_staged(c, inp)
    whole = run_entry(c, inp["parts"], inp["ysq"], inp["raw"], caller)
    for k in ("loss_hist", "raw_hist", "raw", "grad", "prev", "step"):
        assert _same(getattr(staged, k), getattr(whole, k)), (name, k, "the run differs from the staged sequence")
    assert bool(torch.isnan(whole.loss_hist[:c.iter0]).all()) and bool(torch.isnan(whole.raw_hist[:c.iter0]).all())
    G, dl = c.G, c.dl
    for g in range(G if G > 1 else 0):
        sel = np.concatenate([[g], G + g * dl + np.arange(dl), [G + G * dl + g]])
        parts = inp["parts"][g] if c.own else inp["parts"]
        alone = run_entry(c, parts, inp["ysq"][g:g + 1], inp["raw"][sel], caller, sel)
        tsel = torch.from_numpy(sel).to(DEV)
        assert _same(alone.loss_hist[:, 0], whole.loss_hist[:, g]), (name, g, "loss_hist depends on G")
        assert _same(alone.raw_hist, whole.raw_hist[:, tsel]), (name, g, "raw_hist depends on G")
        for k in ("raw", "grad", "prev", "step"):
            assert _same(getattr(alone, k), getattr(whole, k)[tsel]), (name, g, k, "depends on G")
