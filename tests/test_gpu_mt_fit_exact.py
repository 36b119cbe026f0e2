"""fgp_mt_fit_run on the device, stage by stage.  One iteration leaves every intermediate in the work buffer
(fgp_mt_fit_work_layout says where); the test reads them and checks

  lams      k_mtg_lams against fit_lams_ref(spectra, raw) within the derived bound;
  blocks    fac, logdet, z, zinv, glp in the work buffer against the stand-alone entry points (fgp_mt_factor, fgp_mt_solve,
            fgp_mt_selinv, fgp_mt_mll_grad) applied to the device lams: BIT FOR BIT, under the thread-per-class kernel
            (fgp_set_mt_class_kernel(1)) and the wave-per-class kernel (2) -- the promise of the comment above
            k_mtg_class.  The wave-per-class kernel keeps the factor and the selected inverse in LDS and never stores
            them: under it logdet, z, glp and info are compared (z is a function of the whole factor, glp of the whole
            selected inverse on the pattern), and fac / zinv in the work buffer are asserted untouched.
            tests/test_gpu_mt_blocks_exact.py carries the accuracy of those entry points;
  contract  the totals sums[g][q] against fit_contract_ref(device glp, z, logdet, spectra, raw) within the bound, all
            4 + d + P of them;
  step      the loss row and grad_out against fit_step_ref(device sums, raw) within the bound; raw, rprop_prev and
            rprop_step against the float64 restatement of torch.optim.Rprop from the device's grad_out, bit for bit; the
            raw_hist row equal to the parameters the iteration started from;
and then a second iteration (iter0 = 1) the same way.  The bounds are those of tests/mt_block_reference.py: counted from
the kernels' roundings, never fitted to what the device returns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd import ops
from tests import mt_block_reference as R
from tests import mt_fit_cases as C
from tests.gpu_fixtures import DEV
from tests.test_gpu_mt_blocks_exact import mll_grad

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

WORK_NAMES = ("lams", "fac", "zinv", "glp", "z", "logdet", "dkt", "part", "sums", "info")


class DeviceFit(object):
    """A case on the device: the desc, its buffers, and views of the work buffer's arrays."""

    def __init__(self, name):
        self.fs, self.raw0, self.c = fs, raw0, c = C.make_fit(name)
        lay = fs.lay
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        self.spec = dev(np.concatenate([s.reshape(-1) for s in fs.spectra]))
        self.y = dev(fs.y)
        self.raw = dev(raw0)
        n = fs.n_params
        self.prev = torch.zeros(n, device=DEV)
        self.step = torch.full((n,), float(c["lr"]), device=DEV)
        self.grad = torch.full((n,), float("nan"), device=DEV)
        self.loss_hist = torch.full((2, 3), float("nan"), device=DEV)
        self.raw_hist = torch.full((2, n), float("nan"), device=DEV)
        self.rows = dev(fs.rows.astype(np.int32)) if fs.G > 1 else None
        self.nug = dev(fs.nug_coef.astype(np.complex128)) if fs.nug_coef is not None else None
        desc = C.fill_desc(fs, c)
        desc.spectra, desc.y, desc.raw = self.spec.data_ptr(), self.y.data_ptr(), self.raw.data_ptr()
        desc.rprop_prev, desc.rprop_step, desc.grad_out = self.prev.data_ptr(), self.step.data_ptr(), self.grad.data_ptr()
        desc.loss_hist, desc.raw_hist = self.loss_hist.data_ptr(), self.raw_hist.data_ptr()
        desc.rows = self.rows.data_ptr() if self.rows is not None else None
        desc.nugget_coef = self.nug.data_ptr() if self.nug is not None else None
        wb = ctypes.c_int64(0)
        N.call("fgp_mt_fit_work", desc, ctypes.byref(wb))
        offs = (ctypes.c_int64 * 10)()
        N.call("fgp_mt_fit_work_layout", desc, offs)
        npar = ctypes.c_int(0)
        N.call("fgp_mt_fit_nparams", desc, ctypes.byref(npar))
        assert npar.value == n
        self.work = torch.zeros(wb.value, dtype=torch.uint8, device=DEV)
        desc.work = self.work.data_ptr()
        self.desc = desc
        G, L, B, rn = fs.G, lay.L, fs.B, lay.R * lay.nmin
        NQ = R.KMTGQ + fs.P
        shapes = {"lams": (torch.complex128, (G, L)), "fac": (torch.complex128, (G, L)), "zinv": (torch.complex128, (G, L)),
                  "glp": (torch.complex128, (G, L)), "z": (torch.complex128, (G, B, rn)), "logdet": (torch.float64, (G, lay.nmin)),
                  "dkt": (torch.float64, (G, L)), "part": (torch.float64, (G, fs.nblk, R.KMTGQ)),
                  "sums": (torch.float64, (G, NQ)), "info": (torch.int32, (1,))}
        self.view = {}
        for nm, o in zip(WORK_NAMES, list(offs)):
            dt, shp = shapes[nm]
            nbytes = int(np.prod(shp)) * torch.empty(0, dtype=dt).element_size()
            self.view[nm] = self.work[o:o + nbytes].view(dt).reshape(shp)

    def iterate(self, it):
        """Iteration `it` (with its update): the state before it, and everything it left, as numpy."""
        before = {k: getattr(self, k).cpu().numpy().copy() for k in ("raw", "prev", "step")}
        N.call("fgp_mt_fit_run", self.desc, int(it), 1, 0, N.stream_ptr(self.raw.device))
        torch.cuda.synchronize()
        fs = self.fs
        snap = {k: v.cpu().numpy().copy() for k, v in self.view.items()}
        # (a row holds 4 + FGP_MAX_D + P; the pairs' totals follow the 4 + d block totals directly: q = 4 + D + p)
        snap["sums"] = snap["sums"][:, :4 + fs.d + fs.P]
        snap["loss"] = self.loss_hist[it].cpu().numpy().copy()
        snap["raw_hist"] = self.raw_hist[it].cpu().numpy().copy()
        snap["grad"] = self.grad.cpu().numpy().copy()
        for k in ("raw", "prev", "step"):
            snap[k + "_after"] = getattr(self, k).cpu().numpy().copy()
        return before, snap

    def entry_points(self):
        """The stand-alone entry points on the work buffer's lams (device tensors): fac, logdet, z [G, B, R nmin], zinv,
        glp, info."""
        fs = self.fs
        G, B = fs.G, fs.B
        lay = ops.mt_layout(fs.ns)
        fac, ld, info = ops.mt_factor(lay, self.view["lams"].clone())
        # problem g's B vectors are together in the fit; the entry points take vector b against problem b mod G
        v = self.y.permute(1, 0, 2).reshape(B * G, -1).contiguous()
        z = ops.mt_solve(lay, fac, v)
        zinv = ops.mt_selinv(lay, fac)
        gn = torch.full((B * G,), fs.grad_norm, device=DEV)
        gl = torch.full((G,), fs.grad_logdet, device=DEV)
        glp = mll_grad(lay, zinv, z, gn, gl)
        return {"fac": fac, "logdet": ld, "z": z.reshape(B, G, -1).permute(1, 0, 2).contiguous(), "zinv": zinv, "glp": glp,
                "info": info}


def same_bits(a, b):
    a = torch.view_as_real(a) if a.is_complex() else a
    b = torch.view_as_real(b) if b.is_complex() else b
    return a.shape == b.shape and bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())


def run_case(name, mode):
    """Two iterations of a case under class-kernel mode `mode`: per iteration (before, snap, blocks_equal) with
    blocks_equal = {array: the work buffer's equals the entry point's, bit for bit}."""
    N.call("fgp_set_mt_class_kernel", mode)
    try:
        df = DeviceFit(name)
        out = []
        for it in (0, 1):
            before, snap = df.iterate(it)
            ep = df.entry_points()
            wave = mode == 2 and df.fs.class_lds() > 0
            eq = {k: same_bits(df.view[k], ep[k]) for k in (("logdet", "z", "glp") if wave else ("fac", "logdet", "z", "zinv", "glp"))}
            eq["info"] = int(ep["info"].item()) == int(snap["info"][0])
            if wave:           # not stored by this kernel: as the buffer was allocated
                eq["fac untouched"] = not snap["fac"].any()
                eq["zinv untouched"] = not snap["zinv"].any()
            out.append((before, snap, eq))
        return df.fs, df.c, out
    finally:
        N.call("fgp_set_mt_class_kernel", 0)


@functools.lru_cache(maxsize=None)
def thread_run(name):
    return run_case(name, 1)


def check_iteration(name, it, fs, c, before, snap):
    """The accuracy of the non-block stages and the exact restatement of the update."""
    rs = R.fit_stage_ratios(fs, before["raw"], snap)
    print("%s iteration %d: max err / bound: %s" % (name, it, ", ".join("%s %.3g" % kv for kv in rs.items())))
    assert int(snap["info"][0]) == 0
    for k in ("lams", "fac", "zinv", "glp", "z", "logdet", "sums", "loss", "grad", "raw_after", "prev_after", "step_after"):
        assert np.isfinite(snap[k]).all(), k
    for st, r in rs.items():
        assert r <= 1.0, (st, r)
    assert np.array_equal(snap["raw_hist"], before["raw"])
    mask = C.rg_mask(fs, c["rg"])
    raw, prev, step, prod = R.rprop_f64(snap["grad"], before["raw"], before["prev"], before["step"], mask, *C.ETAS, *C.STEPS)
    for k, want in (("raw", raw), ("prev", prev), ("step", step)):
        assert np.array_equal(snap[k + "_after"], want), k
        # a parameter whose requires_grad is cleared keeps its state (its gradient is still written: checked above)
        assert np.array_equal(snap[k + "_after"][~mask], before[k][~mask]), k
    return prod[mask]


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_two_iterations_stage_by_stage(name):
    fs, c, its = thread_run(name)
    for it, (before, snap, eq) in enumerate(its):
        assert all(eq.values()), "iteration %d, thread per class: the work buffer differs from the entry points: %s" % (it, eq)
        prod = check_iteration(name, it, fs, c, before, snap)
        if it == 0:
            assert (prod == 0).all()
        elif name == C.BRANCH_CASE:
            assert (prod < 0).any() and (prod > 0).any(), "both Rprop branches must occur: %s" % prod
    assert not np.array_equal(its[0][1]["raw_after"], its[0][0]["raw"])


@pytest.mark.parametrize("name", [n for n in C.CASE_IDS if n != "nblk_cap"])
def test_the_wave_per_class_kernel_gives_the_same_bits(name):
    """Mode 2 (class_512_b3: the class does not fit LDS and the launch falls back to the thread per class): the entry
    points' bits again, and with them every later stage's of the thread-per-class run."""
    _, _, want = thread_run(name)
    _, _, got = run_case(name, 2)
    for it in (0, 1):
        (_, sw, _), (_, sg, eq) = want[it], got[it]
        assert all(eq.values()), "iteration %d, wave per class: the work buffer differs from the entry points: %s" % (it, eq)
        for k in sw:
            if k in ("fac", "zinv") and not np.array_equal(sw[k], sg[k]):
                assert not sg[k].any() and C.make_fit(name)[0].class_lds() > 0, (it, k)
                continue
            assert np.array_equal(sw[k].view(np.int64) if sw[k].dtype == np.float64 else sw[k],
                                  sg[k].view(np.int64) if sg[k].dtype == np.float64 else sg[k]), (it, k)


def test_unstaged_step_kernel_gives_the_staged_one_s_bits():
    """nostage = batch_g3 with 4198 more scale rows that no problem uses (n_params = 4217: the step kernel's LDS copies
    no longer fit and it reads global memory, STAGE == false).  The used parameters: the bits of batch_g3; the unused
    rows: gradient 0, raw / prev / step unchanged."""
    fs0, _, small = thread_run("batch_g3")
    fs1, _, big = thread_run("nostage")
    assert 2 * 8 * fs1.n_params + 8 * fs1.G * (R.KMTGQ + fs1.P) + 20 * fs1.G > 65536 >= 8 * fs1.n_params
    extra = fs1.l_off - fs0.l_off
    used = np.concatenate([np.arange(fs0.l_off), fs1.l_off + np.arange(fs0.n_params - fs0.l_off)])
    unused = fs0.l_off + np.arange(extra)
    for it in (0, 1):
        (_, s0, _), (b1, s1, _) = small[it], big[it]
        for k in ("lams", "fac", "z", "zinv", "glp", "logdet", "sums", "loss"):
            assert np.array_equal(s0[k], s1[k]), (it, k)
        for k in ("grad", "raw_after", "prev_after", "step_after", "raw_hist"):
            assert np.array_equal(s0[k], s1[k][used]), (it, k)
        assert (s1["grad"][unused] == 0).all()
        for k in ("raw", "prev", "step"):
            assert np.array_equal(s1[k + "_after"][unused], b1[k][unused]), (it, k)


def test_the_capped_contraction_takes_a_second_stride():
    fs, _, _ = thread_run("nblk_cap")
    assert fs.nblk == 1024 and fs.lay.L > 1024 * 256 and fs.G * fs.lay.nmin > 8192
