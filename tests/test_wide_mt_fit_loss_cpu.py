"""GCV / CV in fgp_wide_mt_fit_run (fgp_wide_mt_fit_desc.loss_metric / cv_weight, an addition to ABI 20), the part that
needs no GPU:

  * the argument refusals, each with its status and the field named in fgp_last_error, before any HIP call;
  * an MLL descriptor's work bytes do not depend on cv_weight, and fgp_wide_mt_fit_loss_layout is consistent with
    fgp_wide_mt_fit_work (the partials follow pb, only under GCV / CV);
  * the header declares the new hook in the parenthesised form and the ABI number is still 20;
  * the long-double restatement of the two kernels (tests/wide_mt_loss_reference.py) reproduces torch autograd through a
    torch restatement of the reference's losses (util.py:371-394, abstract_gp.py:242-273) on random Hermitian
    positive-definite blocks -- the closed forms and the glp convention (dL/dRe + i dL/dIm of the packed upper triangle);
  * the host's routing predicate on a stand-in GP object.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from fastgaussianprocesses_amd.multitask import MultiTaskFastGP
from tests import wide_mt_loss_reference as LR
from tests.test_wide_mt_fit_cpu import FGP_ERR_INVALID, FGP_ERR_UNSUPPORTED, ROOT, _make

MLL, GCV, CV = N.LOSS_MLL, N.LOSS_GCV, N.LOSS_CV
EQ = (64, 64, 64)


# ---------------------------------------------------------------------------------------------- refusals
_REFUSED = [
    ("loss_metric", FGP_ERR_INVALID, dict(ns=EQ, loss_metric=3)),
    ("loss_metric", FGP_ERR_INVALID, dict(ns=EQ, loss_metric=-1)),
    ("cv_weight", FGP_ERR_INVALID, dict(ns=EQ, loss_metric=CV, cv_weight=float("nan"))),
    ("cv_weight", FGP_ERR_INVALID, dict(ns=EQ, loss_metric=CV, cv_weight=float("inf"))),
    ("n[", FGP_ERR_UNSUPPORTED, dict(ns=(64, 8, 8), loss_metric=GCV)),
    ("n[", FGP_ERR_UNSUPPORTED, dict(ns=(64, 64, 32), loss_metric=CV, cv_weight=1.0)),
    ("T=1", FGP_ERR_UNSUPPORTED, dict(ns=(64,), loss_metric=CV, cv_weight=1.0)),
]


@pytest.mark.parametrize("field,status,kw", _REFUSED)
def test_refused_before_any_hip_call(field, status, kw):
    lib = N.lib()
    out, offs = ctypes.c_int64(-1), (ctypes.c_int64 * 2)()
    for fn, call in (("fgp_wide_mt_fit_run", lambda d: lib.fgp_wide_mt_fit_run(d, 0, 1, 0, None)),
                     ("fgp_wide_mt_fit_stage", lambda d: lib.fgp_wide_mt_fit_stage(d, 0, 4, 0, None)),
                     ("fgp_wide_mt_fit_work", lambda d: lib.fgp_wide_mt_fit_work(d, ctypes.byref(out))),
                     ("fgp_wide_mt_fit_loss_layout", lambda d: lib.fgp_wide_mt_fit_loss_layout(d, offs))):
        lib.fgp_wall_clock_khz(0, None)                          # (leaves another message behind)
        before = lib.fgp_last_error()
        rc = call(ctypes.byref(_make(**kw)))
        msg = lib.fgp_last_error()
        assert rc == status, (fn, field, rc, msg)
        assert msg != before and fn.encode() in msg and field.encode() in msg, (fn, field, msg)


def test_what_the_refusals_leave_alone():
    """A garbage cv_weight is unread outside CV; GCV accepts one task; equal n passes both."""
    lib = N.lib()
    out = ctypes.c_int64(-1)
    for kw in (dict(ns=(64, 8, 8), cv_weight=float("nan")), dict(ns=EQ, loss_metric=GCV, cv_weight=float("nan")),
               dict(ns=(64,), loss_metric=GCV), dict(ns=EQ, loss_metric=CV, cv_weight=-2.5)):
        assert lib.fgp_wide_mt_fit_work(ctypes.byref(_make(**kw)), ctypes.byref(out)) == 0, (kw, lib.fgp_last_error())
        assert lib.fgp_wide_mt_fit_run(ctypes.byref(_make(**kw)), 0, 0, 0, None) == 0


# ---------------------------------------------------------------------------------------------- work bytes, layout
def _bytes(**kw):
    out = ctypes.c_int64(-1)
    assert N.lib().fgp_wide_mt_fit_work(ctypes.byref(_make(**kw)), ctypes.byref(out)) == 0
    return out.value


def _layouts(**kw):
    o15, o2 = (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 2)()
    assert N.lib().fgp_wide_mt_fit_work_layout(ctypes.byref(_make(**kw)), o15) == 0
    assert N.lib().fgp_wide_mt_fit_loss_layout(ctypes.byref(_make(**kw)), o2) == 0
    return list(o15), list(o2)


@pytest.mark.parametrize("ns,B,d,fam", [((64, 8, 8), 1, 12, 0), ((4096, 4096), 2, 9, 1), ((1 << 17, 256, 1), 1, 64, 0)])
def test_mll_bytes_do_not_depend_on_cv_weight(ns, B, d, fam):
    kw = dict(ns=ns, B=B, d=d, dl=d, family=fam)
    ref = _bytes(**kw)
    for w in (0.0, 1.0, float("nan"), float("inf"), -3e300):
        assert _bytes(cv_weight=w, **kw) == ref
    o15, o2 = _layouts(cv_weight=float("nan"), **kw)
    assert o2 == [ref, 0] and o15 == _layouts(**kw)[0]


@pytest.mark.parametrize("ns,B,d,fam", [((64, 64, 64), 1, 12, 0), ((512, 512), 2, 9, 1), ((4, 4), 1, 9, 0),
                                        ((1 << 17,) * 5, 3, 64, 1), ((8,) * 16, 1, 12, 0)])
def test_loss_layout_is_consistent_with_work(ns, B, d, fam):
    """The partials follow pb: the 15 offsets and everything before them are the MLL's; bytes = offset + length rounded up
    to 256; length = 8 * 2 * NT * ceil(n / 256) with NT = 1 (GCV) or T (CV)."""
    kw = dict(ns=ns, B=B, d=d, dl=d, family=fam)
    mll = _bytes(**kw)
    o15_mll = _layouts(**kw)[0]
    nbx = -(-ns[0] // 256)
    for loss, nt in ((GCV, 1), (CV, len(ns))):
        o15, (off, length) = _layouts(loss_metric=loss, cv_weight=0.75, **kw)
        assert o15 == o15_mll
        assert off == mll and off % 256 == 0 and off > o15[14]
        assert length == 8 * 2 * nt * nbx
        assert _bytes(loss_metric=loss, cv_weight=0.75, **kw) == off + (length + 255) // 256 * 256
    assert N.lib().fgp_wide_mt_fit_loss_layout(ctypes.byref(_make(**kw)), None) == FGP_ERR_INVALID
    assert N.lib().fgp_wide_mt_fit_loss_layout(None, (ctypes.c_int64 * 2)()) == FGP_ERR_INVALID


def test_hook_declared_in_the_parenthesised_form_and_abi_still_20():
    lib = N.lib()
    assert lib.fgp_abi_version() == 20 and N.ABI_VERSION == 20
    src = open(os.path.join(ROOT, "include", "fgp_hip.h")).read()
    assert "#define FGP_ABI_VERSION 20" in src
    name = "fgp_wide_mt_fit_loss_layout"
    assert ("extern int (%s)(const fgp_wide_mt_fit_desc*" % name) in src
    assert ("extern int %s(" % name) not in src
    assert hasattr(ctypes.CDLL(N.LIB_PATH), name) and name in N._SIGNATURES
    fields = [f for f, _ in N.WideMtFitDesc._fields_]
    assert fields[-2:] == ["loss_metric", "cv_weight"] and fields[-3] == "work"
    assert N.WideMtFitDesc().loss_metric == MLL


# ---------------------------------------------------------------------------------------------- closed forms
def _blocks(T, n, B, seed):
    """Random Hermitian positive-definite blocks lam [n, T, T] and data ytilde [B, T, n] of a REAL problem: every entry
    the unitary DFT of a real sequence (lam_{-j} = conj(lam_j)), as the transform of a real symmetric Gram matrix is, so
    that the real-space coefficients and K^-1 the reference's CV reads are real."""
    rng = np.random.default_rng(seed)
    M = np.fft.fft(rng.standard_normal((T, T, n)), axis=-1)                  # M_j[t, s]
    lam = np.einsum("trj,srj->jts", M, M.conj()) / n + 0.5 * np.eye(T)[None]
    y = np.fft.fft(rng.standard_normal((B, T, n)), axis=-1, norm="ortho")
    return lam, y


def _torch_losses(lam, y, cv, w):
    """util.py:371-394 / abstract_gp.py:242-273 in torch, differentiable in the packed upper triangle of the blocks (a
    complex leaf: autograd returns dL/dRe + i dL/dIm).  ft = the unitary DFT.  GCV: numer / denom summed over the data
    batch; CV: coeffs = K^-1 y in real space, inv_diag = diag K^-1 by solving the identity, sum (coeffs / inv_diag)^2 w."""
    n, T = lam.shape[0], lam.shape[-1]
    B = y.shape[0]
    iu = [(k, l) for k in range(T) for l in range(k, T)]
    leaf = torch.tensor(np.stack([lam[:, k, l] for k, l in iu]), dtype=torch.complex128, requires_grad=True)   # [np, n]
    rows = []
    for t in range(T):
        row = []
        for s in range(T):
            if t == s:
                row.append(leaf[iu.index((t, t))].real.to(torch.complex128))
            elif t < s:
                row.append(leaf[iu.index((t, s))])
            else:
                row.append(leaf[iu.index((s, t))].conj())
        rows.append(torch.stack(row))
    L = torch.stack(rows).permute(2, 0, 1)                                  # [n, T, T]
    A = torch.linalg.inv(L)

    def solve_tilde(v):                                                     # v [..., T, n] -> A v
        return torch.einsum("nts,...sn->...tn", A, v)

    yt = torch.tensor(y, dtype=torch.complex128)
    if not cv:
        z = solve_tilde(yt)
        numer = (z.conj() * z).real.sum((-1, -2))                            # [B]
        idx = torch.arange(T)
        tr = A[:, idx, idx].real.sum()
        denom = (tr / (T * n)) ** 2
        loss = (numer / denom).sum()
    else:
        ft = lambda v: torch.fft.fft(v, dim=-1, norm="ortho")                # noqa: E731
        ift = lambda v: torch.fft.ifft(v, dim=-1, norm="ortho")              # noqa: E731
        coeffs = ift(solve_tilde(yt)).real.reshape(B, T * n)
        eye = torch.eye(T * n, dtype=torch.complex128).reshape(T * n, T, n)
        kinv = ift(solve_tilde(ft(eye))).real.reshape(T * n, T * n)
        inv_diag = torch.diagonal(kinv)
        loss = (((coeffs / inv_diag) ** 2) * w).sum()
    loss.backward()
    return float(loss.detach()), leaf.grad.detach().numpy().reshape(-1)


@pytest.mark.parametrize("cv", [False, True], ids=["GCV", "CV"])
def test_restated_kernels_reproduce_autograd(cv):
    """T = 3, n = 8, B = 2: loss to 1e-13 relative, every dL/dlams entry to 1e-11 of the largest; the seeded defect (the
    c2 term dropped) is far outside."""
    T, n, B, w = 3, 8, 2, 0.75
    lam, y = _blocks(T, n, B, seed=5)
    assert np.allclose(lam, lam.conj().transpose(0, 2, 1)) and (np.linalg.eigvalsh(lam) > 0.4).all()
    loss_t, grad_t = _torch_losses(lam, y, cv, w)
    loss, gx, gy = LR.closed_forms(lam, y, cv, w)
    el = abs(float(loss) - loss_t) / abs(loss_t)
    g = gx.astype(np.float64) + 1j * gy.astype(np.float64)
    eg = float(np.max(np.abs(g - grad_t)) / np.max(np.abs(grad_t)))
    print("closed forms", "CV" if cv else "GCV", "loss rel err %.3g" % el, "gradient err / max %.3g" % eg)
    assert el < 1e-13 and eg < 1e-11
    # the diagonal entries' imaginary parts do not enter a Hermitian block
    diag = np.concatenate([np.arange(o, o + n) for o in LR.offk(T, n)])
    assert (grad_t.imag[diag] == 0).all() and (gy[diag] == 0).all()
    _, bx, by = LR.closed_forms(lam, y, cv, w, mutate="noc2")
    bad = bx.astype(np.float64) + 1j * by.astype(np.float64)
    assert float(np.max(np.abs(bad - grad_t)) / np.max(np.abs(grad_t))) > 1e-3


def test_float64_restatement_stays_inside_its_bound():
    """The restatement run in plain float64 against the tracked long-double one: inside the counted bound, and the seeded
    defect outside it (what the GPU test asserts of the device, on the CPU)."""
    from tests.mt_block_reference import ratio
    T, n, B, w = 3, 64, 2, 0.75
    lam, y = _blocks(T, n, B, seed=9)
    A = np.linalg.inv(lam)
    zinv = LR.pack_upper(A)
    z = np.einsum("nts,bsn->btn", A, y).reshape(B, T * n)
    Cn = LR.counts(T, n, B)
    for cv in (False, True):
        pl = LR.loss_sums_ref(T, n, B, zinv, z, cv)
        pl64 = LR.loss_sums_ref(T, n, B, zinv, z, cv, np.float64)
        assert ratio(pl64.v, pl.v, pl.e, Cn["sums"]) <= 1.0
        plv = np.asarray(pl64.v, dtype=np.float64)
        gx, gy = LR.loss_grad_ref(T, n, B, zinv, z, plv, cv, w)
        for mutate, inside in ((None, True), ("noc2", False)):
            hx, hy = LR.loss_grad_ref(T, n, B, zinv, z, plv, cv, w, np.float64, mutate)
            r = max(ratio(hx.v, gx.v, gx.e, Cn["grad"]), ratio(hy.v, gy.v, gy.e, Cn["grad"]))
            assert (r <= 1.0) == inside, (cv, mutate, r)
        row, row64 = LR.loss_row_ref(T, n, plv, cv, w), LR.loss_row_ref(T, n, plv, cv, w, np.float64)
        keep = ~np.isnan(np.asarray(row.v, dtype=np.float64))
        assert np.array_equal(keep, [True, not cv, not cv])
        assert ratio(row64.v[keep], row.v[keep], row.e[keep], Cn["row"]) <= 1.0


# ---------------------------------------------------------------------------------------------- routing predicate
def _stand_in(d=12, ns=(64, 64, 64), wide_ok=True, num_tasks=None):
    gp = types.SimpleNamespace(d=d, _ns=list(ns), num_tasks=len(ns) if num_tasks is None else num_tasks,
                               _mt_fused_ok=lambda: False, _mt_learn_ok=lambda: False, _mt_general_ok=lambda: False,
                               _mt_wide_ok=lambda: wide_ok)
    gp._mt_wide_alt_ok = types.MethodType(MultiTaskFastGP._mt_wide_alt_ok, gp)
    gp._device_fit_args = types.MethodType(MultiTaskFastGP._device_fit_args, gp)
    return gp


def test_routing_predicate(monkeypatch):
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "1")
    monkeypatch.delenv("FGP_ALT_LOSS_DEVICE", raising=False)
    gp = _stand_in()
    assert gp._device_fit_args("GCV", None, None, 1) == dict(loss_metric="GCV", cv_weight=1.0)
    assert gp._device_fit_args("CV", None, None, 0.75) == dict(loss_metric="CV", cv_weight=0.75)
    assert gp._device_fit_args("CV", None, None, torch.tensor([0.5])) == dict(loss_metric="CV", cv_weight=0.5)
    assert gp._device_fit_args("MLL", None, None, 1) == {}
    # outside: a per-point weight, masks, an optimizer, unequal n, an empty task, one task under CV, outside _mt_wide_ok
    assert gp._device_fit_args("CV", None, None, torch.ones(192)) is None
    assert gp._device_fit_args("GCV", None, [torch.tensor([0])], 1) is None
    assert gp._device_fit_args("GCV", object(), None, 1) is None
    assert _stand_in(ns=(64, 8, 256))._device_fit_args("GCV", None, None, 1) is None
    assert _stand_in(ns=(64, 64, 0))._device_fit_args("GCV", None, None, 1) is None
    assert _stand_in(ns=(64,))._device_fit_args("CV", None, None, 1) is None
    assert _stand_in(ns=(64,))._device_fit_args("GCV", None, None, 1) == dict(loss_metric="GCV", cv_weight=1.0)
    assert _stand_in(wide_ok=False)._device_fit_args("GCV", None, None, 1) is None
    assert _stand_in(d=6)._device_fit_args("GCV", None, None, 1) is None
    # the two switches
    monkeypatch.setenv("FGP_ALT_LOSS_DEVICE", "0")
    assert gp._device_fit_args("GCV", None, None, 1) is None and gp._device_fit_args("MLL", None, None, 1) == {}
    monkeypatch.delenv("FGP_ALT_LOSS_DEVICE")
    monkeypatch.setenv("FGP_WIDE_FIT_DEVICE", "0")
    assert gp._device_fit_args("GCV", None, None, 1) is None and gp._device_fit_args("CV", None, None, 1) is None
    monkeypatch.delenv("FGP_WIDE_FIT_DEVICE")
    assert gp._device_fit_args("GCV", None, None, 1) is None
