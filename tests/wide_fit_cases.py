"""Seeded problems of the stage-by-stage tests of fgp_wide_fit_run (WF) and fgp_wide_mt_fit_run (MT): the smallest
shapes that reach each branch of the loops' own kernels.

Parameters chosen so that the reference alone stays inside the non-vacuity cap (||u e||_1 <= 100 2^-53 C ||value||_1):

  * synthetic parts [d, n]: part_j[0] in [1, 2], part_j[1] = 0.6 part_j[0], part_j[i > 1] = uniform(-1, 1) / sqrt(n).
    Then k1[0] >= scale (1 + l)^d > k1[1] and k1[i > 1] = scale (1 + O(l sqrt(d / n))), and element 1 enters both
    transforms with the sign (-1)^k, so the eigenvalues sqrt(n) lambda_k are (k1[0] - scale) +- (k1[1] - scale) + scale
    O(l sqrt(d)) > 0 (k != 0) or about n scale (k = 0): lambda' is positive (CV's 1 / lambda' has no pole), ev =
    sqrt(n) lambda + noise has no cancellation, and the spectrum has two well separated levels (on a flat one the GCV
    loss N1 / D does not depend on the level and its gradient is a cancelling difference);
  * noise = exp(raw_noise) with raw_noise in [-2, -1] up to n = 2^13 and log(2e-6 n) + [0, 1] above: never below 1e-6
    of the largest eigenvalue (about n scale, scale <= e^0.3);
  * lengthscales in [0.1, 0.3] (d <= 16) or [0.03, 0.06] (d = 64), raw scale in [-0.3, 0.3], Y in [0.1, 2.1];
  * "real" cases: the first-column parts of a rank-1 lattice (alpha 2) / a digital net (alpha 1) from the CPU oracle,
    whose kernel matrices are positive definite.

WF cases (d = 9, G = 1, dl = d, MLL, every flag set, lr = 0.1 unless the name says otherwise):
  m0, m1           the lone-element tail; one pair
  m9               lanes past n;  m11: exactly one full k_wide_fit_eig workgroup;  m12: nbe = 2
  m13              sqrt(n) inexact, two-pass transforms;  lat-m17: the half-length route
  lat-m20-mll, net-m20-gcv   nbe = 512 > 256: the second-level loops take a second trip
  G3-own           parts_stride = d n;  G5-shared;  dl1;  d64
  rg-scale / rg-ls / rg-noise   that flag cleared
  state, state-gcv lr <= 0 with a caller-supplied Rprop state built from the evaluated gradient: the eta_plus, eta_minus
                   and zero-product branches and both clamps in ONE update
  iter3-fnu        iter0 = 3 and final_no_update
  gcv / cv at m9 and m12, lat-cv-m1, net-gcv-m1-G3 (cv_weight = 0.75);  real: oracle parts
Every case exists in both families except m17 (the half-length route is the lattice's), the two n = 2^20 cases (one
per family), cv-m1 / gcv-m1-G3 and the two `real` shapes.
"""
import collections
import functools
import math

import numpy as np

LAT, NET = 0, 1
MLL, GCV, CV = 0, 1, 2
ETAS = (0.5, 1.2)
STEPS = (1e-6, 50.0)
CV_WEIGHT = 0.75
MLL_CONST = 3.25               # any constant: the step adds it to the loss as given
LOGDET_WEIGHT = 1.5            # not a power of two: its product rounds

WF = collections.namedtuple("WF", "name fam m d G dl own loss rg lr iter0 fnu src")


def _wf(tag, fam, m, d=9, G=1, dl=None, own=False, loss=MLL, rg=(1, 1, 1), lr=0.1, iter0=0, fnu=False, src="syn"):
    return WF("%s-%s" % ("lat" if fam == LAT else "net", tag), fam, m, d, G, d if dl is None else dl, own, loss, tuple(rg),
              lr, iter0, fnu, src)


def _wf_cases():
    out = []
    for fam in (LAT, NET):
        out += [_wf("m%d" % m, fam, m) for m in (0, 1, 9, 11, 12, 13)]
        out += [_wf("G3-own", fam, 9, G=3, own=True), _wf("G5-shared-dl1", fam, 9, G=5, dl=1), _wf("dl1", fam, 9, dl=1),
                _wf("d64", fam, 9, d=64), _wf("gcv-m9", fam, 9, loss=GCV), _wf("cv-m9", fam, 9, loss=CV)]
        out += [_wf("rg-scale", fam, 9, rg=(0, 1, 1)), _wf("rg-ls", fam, 9, rg=(1, 0, 1)), _wf("rg-noise", fam, 9, rg=(1, 1, 0))]
        out += [_wf("state", fam, 9, G=2, lr=-1.0), _wf("state-gcv", fam, 9, G=2, lr=0.0, loss=GCV)]
        out += [_wf("iter3-fnu", fam, 9, iter0=3, fnu=True), _wf("iter3-fnu-cv", fam, 9, iter0=3, fnu=True, loss=CV)]
        out += [_wf("gcv-m12", fam, 12, loss=GCV), _wf("cv-m12", fam, 12, loss=CV)]
    out += [_wf("m17", LAT, 17), _wf("m20-mll", LAT, 20), _wf("m20-gcv", NET, 20, loss=GCV)]
    out += [_wf("cv-m1", LAT, 1, loss=CV), _wf("gcv-m1-G3", NET, 1, loss=GCV, G=3, own=True)]
    out += [_wf("real-m9", LAT, 9, src="real"), _wf("real-m9", NET, 9, src="real", G=2, dl=1)]
    return out


WF_CASES = _wf_cases()
WF_BY_NAME = {c.name: c for c in WF_CASES}
assert len(WF_BY_NAME) == len(WF_CASES)
# the CPU tests run every stage of every case
WF_CPU = [c.name for c in WF_CASES]


def _seed(c):
    return [31, c.fam, c.m, c.d, c.G, c.dl, int(c.own), c.loss, sum(c.rg), WF_CASES.index(c)]


def _real_parts(fam, m, d):
    import torch

    import fastgaussianprocesses_amd as F
    from oracle import fgp_oracle as O
    n = 1 << m
    if fam == LAT:
        x = torch.from_numpy(F.Lattice(d, seed=11)(0, n))
        p = O.lattice_k1parts(x, [2] * d)
    else:
        from tests.wide_cases import net_sequence
        seq = net_sequence(d, 11)
        xb = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64))
        p = O.net_k1parts(xb, seq.t, [1] * d)
    return np.ascontiguousarray(p.to(torch.float64).numpy().T)           # [n, d] -> [d, n]


@functools.lru_cache(maxsize=4)
def wf_inputs(name):
    """dict: parts [d, n] or [G, d, n], ysq [G, n], raw [G (2 + dl)]."""
    c = WF_BY_NAME[name]
    g = np.random.default_rng(_seed(c))
    n, d, G = 1 << c.m, c.d, c.G
    if c.src == "real":
        parts = _real_parts(c.fam, c.m, d)
    else:
        shape = (G, d, n) if c.own else (d, n)
        parts = g.uniform(-1.0, 1.0, shape) / math.sqrt(n)
        parts[..., 0] = g.uniform(1.0, 2.0, shape[:-1])
        if n > 1:
            parts[..., 1] = 0.6 * parts[..., 0]
    ysq = g.uniform(0.1, 2.1, (G, n))
    lo, hi = (0.03, 0.06) if d > 16 else (0.1, 0.3)
    noise = g.uniform(-2.0, -1.0, G) if c.m <= 13 else math.log(2e-6 * n) + g.uniform(0.0, 1.0, G)
    raw = np.concatenate([g.uniform(-0.3, 0.3, G), np.log(g.uniform(lo, hi, G * c.dl)), noise])
    return dict(parts=np.ascontiguousarray(parts), ysq=ysq, raw=raw)


def caller_state(grad, rg_mask):
    """The caller-supplied Rprop state of the `state` cases from the evaluated raw gradient: over the parameters in
    turn, a previous gradient of the same sign with a step eta_plus pushes past step_max, one of the opposite sign with
    a step eta_minus pushes below step_min, zero, and then the same three with steps that stay inside the clamps."""
    grad = np.asarray(grad, dtype=np.float64)
    prev, step = np.zeros_like(grad), np.full_like(grad, 0.1)
    for i in range(grad.size):
        k = i % 6
        prev[i] = (grad[i], -grad[i], 0.0)[k % 3]
        step[i] = (49.0, 1.5e-6, 0.3, 0.2, 0.4, 0.05)[k]
    return prev, step


# ------------------------------------------------------------------------------------------------ multitask
MT = collections.namedtuple("MT", "name fam ns d dl B task T_all rank vexp conj P rg lr src")


def _mt(tag, fam, ns, d=9, dl=None, B=1, task=None, T_all=None, rank=None, vexp=1, conj=None, P=1, rg=(1, 1, 1, 1, 1),
        lr=0.1, src="syn"):
    T = len(ns)
    T_all = T if T_all is None else T_all
    npairs = T * (T + 1) // 2
    return MT("%s-%s" % ("lat" if fam == LAT else "net", tag), fam, tuple(ns), d, d if dl is None else dl, B,
              tuple(range(T)) if task is None else tuple(task), T_all, 2 if rank is None else rank, vexp,
              tuple([0] * npairs) if conj is None else tuple(conj), P, tuple(rg), lr, src)


def _mt_cases():
    out = []
    for fam in (LAT, NET):
        out += [_mt("T1", fam, [64], rank=0),
                _mt("T3", fam, [64, 64, 16], B=3, conj=(0, 1, 0, 0, 1, 0)),
                _mt("n4-1", fam, [4, 1], dl=1, vexp=0, rank=0),
                _mt("big", fam, [1 << 17, 1 << 9], conj=(0, 1, 0)),
                _mt("tall4", fam, [64, 64, 8], task=[2, 0, 3], T_all=4, conj=(0, 1, 0, 0, 0, 0), vexp=0),
                _mt("deriv", fam, [64, 16], P=3, dl=1, B=3, d=12)]
    for i, nm in enumerate(("scale", "ls", "noise", "factor", "vtask")):
        rg = [1] * 5
        rg[i] = 0
        out += [_mt("rg-" + nm, fam, [64, 16], rg=rg, conj=(0, 1, 0)) for fam in (LAT, NET)]
    return out


MT_CASES = _mt_cases()
MT_BY_NAME = {c.name: c for c in MT_CASES}
assert len(MT_BY_NAME) == len(MT_CASES)
MT_CPU = [c.name for c in MT_CASES]
# what `big` is the smallest shape for, from the spec alone: the contraction's grid is 512 workgroups wide, the shorter
# task's pairs fill 2 of them (the other 510 partials of each row stay unwritten and must stay unread), and the longer
# task takes the half-length transforms
_BIG = [c for c in MT_CASES if c.name.endswith("-big")]
assert _BIG and all(-(-c.ns[0] // 256) == 512 and -(-c.ns[1] // 256) == 2 and c.ns[0] >= 1 << 17 for c in _BIG)


def mt_spec(c):
    from tests.wide_fit_reference import MtSpec
    return MtSpec(ns=list(c.ns), d=c.d, dl=c.dl, B=c.B, family=c.fam, task=list(c.task), T_all=c.T_all, rank=c.rank,
                  vtask_exp=c.vexp, conj=list(c.conj), logdet_weight=float(c.B) * 0.75,
                  mll_const=0.5 * c.B * sum(c.ns) * math.log(2 * math.pi))


@functools.lru_cache(maxsize=4)
def mt_inputs(name):
    """dict: pairs = [(parts [P, d, n_k], ind [P, d] int, cc [P])] per sorted pair, y [B, R nmin] complex128, raw.
    The diagonal pairs as the WF parts (a dominant first element: positive, well separated eigenvalues); the coupling
    pairs smaller by a factor 4 T, so every class block is strictly diagonally dominant (info stays 0).  Pairs with P > 1
    have their terms' indicators mixed (the derivative form) and cc in [0.5, 1]."""
    c = MT_BY_NAME[name]
    g = np.random.default_rng([37, c.fam, len(c.ns), c.d, c.dl, c.B, c.rank, c.P, MT_CASES.index(c)])
    T = len(c.ns)
    pairs = []
    for k in range(T):
        for l in range(k, T):
            n = c.ns[k]
            parts = g.uniform(-1.0, 1.0, (c.P, c.d, n)) / math.sqrt(n)
            parts[..., 0] = g.uniform(1.0, 2.0, (c.P, c.d))
            if k != l:
                parts /= 4.0 * T * c.P
            ind = np.ones((c.P, c.d), dtype=np.int32)
            if c.P > 1:
                ind[1:] = g.integers(0, 2, (c.P - 1, c.d))
                ind[1:, 0] = 1
            cc = np.ones(c.P) if c.P == 1 else g.uniform(0.5, 1.0, c.P) / c.P
            if k != l:
                cc = cc / (4.0 * T)
            pairs.append((np.ascontiguousarray(parts), ind, cc))
    R_nmin = sum(c.ns)
    y = g.uniform(-1, 1, (c.B, R_nmin)) + (0 if c.fam == NET else 1j) * g.uniform(-1, 1, (c.B, R_nmin))
    sp = mt_spec(c)
    raw = g.uniform(-0.3, 0.3, sp.n_params)
    lo, hi = (0.03, 0.06) if c.d > 16 else (0.1, 0.3)
    raw[1:1 + c.dl] = np.log(g.uniform(lo, hi, c.dl))
    raw[sp.noise_off] = g.uniform(-2.0, -1.0) if c.ns[0] <= (1 << 13) else math.log(2e-6 * c.ns[0]) + g.uniform(0, 1)
    raw[sp.f_off:sp.v_off] = g.uniform(-0.3, 0.3, sp.v_off - sp.f_off)
    raw[sp.v_off:] = g.uniform(0.0, 0.3, c.T_all) if c.vexp else g.uniform(1.0, 1.4, c.T_all)
    return dict(pairs=pairs, y=y.astype(np.complex128), raw=raw)
