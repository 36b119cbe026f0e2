"""Seeded problems of the stage-by-stage tests of fgp_mt_fit_run: a FitSpec (tests/mt_block_reference.py) built from
synthetic data the way multitask.MtGeneralEngine builds its fgp_mt_fit_desc from a GP.

  * pair spectra [2^d][n_k] per sorted pair: the diagonal pairs real with a dominant S = 0 term (8 R + [0, 1)), every
    other term of modulus at most 2^-d / 4; nets real throughout;
  * data y [G][B][R nmin] of mixed magnitude;
  * raw parameters in [-0.5, 0.5] (the task noise in [0.3, 0.5] where it enters untransformed, vtask_exp = 0: a
    negative one would make K_task indefinite).
With these every class block of the lams is strictly diagonally dominant (tests/test_mt_block_reference_cpu.py asserts
it on the reference's lams), so info == 0 by construction.

A case names the path it is the smallest shape for:
  d1 .. d6             d = 1, 2, 3, 4 (dl = 1 and dl = d), 6 on [64, 64]: d >= 4 takes the `sh` bits of mtg_poly
  rank0 / rank1 / vraw the task kernel: no factor, one column, T_all columns (the default); vtask_exp = 0
  tall4                T_all = 4 with T = 3 active, task = [2, 0, 3]
  rg_*                 one requires_grad flag cleared
  three_levels, sixteen_16, nmin_1
  class_512_b2         [512, 1], B = 2: the largest class that fits k_mtg_class's LDS, 513 rows in the first task
  class_512_b3         [512, 1], B = 3: it does not fit; the wave-per-class mode falls back to the thread per class
  b3_repeated          B = 3 on [64, 64, 8, 8]
  batch_g3             G = 3, shared parameter rows; batch_g3_vraw: the same with vtask_exp = 0 and rank = 0
  nostage              the same with 4200 scale rows: the step kernel's STAGE == false instantiation
  nugget               the adaptive nugget, d = 3, [64, 16], nugget_ref = 1
  nblk_cap             [2^17, 2^17]: nblk = 1024 and a second stride in k_mtg_contract
"""
import math

import numpy as np

from tests.mt_block_reference import FitSpec, Layout

ETAS = (0.5, 1.2)
STEPS = (1e-6, 50.0)
G3_ROWS = [[0, 0, 1], [0, 1, 1], [0, 0, 0], [0, 1, 0], [1, 1, 0]]
G3_NROWS = [2, 2, 1, 2, 2]


def _case(ns, d=2, dl=None, B=1, G=1, family="lattice", rank=None, T_all=None, task=None, vtask_exp=1, rows=None,
          nrows=None, nugget=False, nugget_ref=0, rg=(1, 1, 1, 1, 1), lr=0.1):
    T = len(ns)
    T_all = T if T_all is None else T_all
    return dict(ns=list(ns), d=d, dl=d if dl is None else dl, B=B, G=G, family=family, rank=T_all if rank is None else rank,
                T_all=T_all, task=list(range(T)) if task is None else list(task), vtask_exp=vtask_exp,
                rows=rows if rows is not None else [[0] * G] * 5, nrows=nrows if nrows is not None else [1] * 5,
                nugget=nugget, nugget_ref=nugget_ref, rg=tuple(rg), lr=lr)


CASES = {
    "d1": _case([64, 64], d=1),
    "d2": _case([64, 64], d=2, lr=0.4),
    "d3": _case([64, 64], d=3, family="net"),
    "d4_dl1": _case([64, 64], d=4, dl=1),
    "d4_dl4": _case([64, 64], d=4, dl=4),
    "d6": _case([64, 64], d=6),
    "rank0": _case([64, 64], rank=0),
    "rank1": _case([64, 64], rank=1),
    "vraw": _case([64, 64], vtask_exp=0, family="net"),
    "tall4": _case([64, 64, 8], T_all=4, task=[2, 0, 3], rank=2),
    "rg_scale": _case([64, 16], rg=(0, 1, 1, 1, 1)),
    "rg_ls": _case([64, 16], rg=(1, 0, 1, 1, 1)),
    "rg_noise": _case([64, 16], rg=(1, 1, 0, 1, 1)),
    "rg_factor": _case([64, 16], rg=(1, 1, 1, 0, 1)),
    "rg_vtask": _case([64, 16], rg=(1, 1, 1, 1, 0)),
    "three_levels": _case([256, 64, 8], B=2),
    "sixteen_16": _case([16] * 16, d=1, rank=2),
    "nmin_1": _case([64, 1]),
    "class_512_b2": _case([512, 1], d=1, B=2),
    "class_512_b3": _case([512, 1], d=1, B=3),
    "b3_repeated": _case([64, 64, 8, 8], B=3, rank=1),
    "batch_g3": _case([64, 16], G=3, rows=G3_ROWS, nrows=G3_NROWS),
    "batch_g3_vraw": _case([64, 16], G=3, rows=G3_ROWS, nrows=G3_NROWS, vtask_exp=0, rank=0),
    "nostage": dict(_case([64, 16], G=3, rows=G3_ROWS, nrows=[4200, 2, 1, 2, 2]), like="batch_g3"),
    "nugget": _case([64, 16], d=3, nugget=True, nugget_ref=1),
    "nblk_cap": _case([1 << 17, 1 << 17], d=1),
}
CASE_IDS = list(CASES)
# a loss whose gradient the CPU tests difference over every raw parameter
FD_CASES = ["nugget", "tall4", "batch_g3"]
# both Rprop branches (prod < 0, prod > 0) must occur at the second iteration of this one
BRANCH_CASE = "d2"


def make_fit(name):
    """(FitSpec, raw [n_params], case dict) of a case; seeded by the case's position."""
    c = CASES[name]
    if c.get("like"):
        # the data and the used parameters of another case, with scale rows no problem uses after its own
        fs0, raw0, c0 = make_fit(c["like"])
        kw = dict(fs0.__dict__)
        for key in ("lay", "P", "l_off", "n_off", "f_off", "v_off", "n_params", "nblk", "pairs"):
            kw.pop(key)
        kw["nrows"] = list(c["nrows"])
        fs = FitSpec(**kw)
        extra = fs.l_off - fs0.l_off
        rng = np.random.default_rng(7000 + CASE_IDS.index(name))
        return fs, np.concatenate([raw0[:fs0.l_off], rng.uniform(-0.5, 0.5, extra), raw0[fs0.l_off:]]), c
    rng = np.random.default_rng(7000 + CASE_IDS.index(name))
    lay = Layout(c["ns"])
    d, NS, real = c["d"], 1 << c["d"], c["family"] == "net"
    spectra = []
    for k in range(lay.T):
        for l in range(k, lay.T):
            n = lay.ns[k]
            mod = rng.uniform(0, 1, (NS, n)) * 2.0 ** -d / 4
            if k == l or real:
                s = (mod * rng.choice([-1.0, 1.0], (NS, n))).astype(np.complex128)
            else:
                s = mod * np.exp(2j * np.pi * rng.uniform(0, 1, (NS, n)))
            if k == l:
                s[0] = 8 * lay.R + rng.uniform(0, 1, n)
            spectra.append(np.ascontiguousarray(s))
    G, B = c["G"], c["B"]
    shape = (G, B, lay.R * lay.nmin)
    mag = 10.0 ** rng.uniform(-1, 1, shape)
    y = mag * (rng.uniform(-1, 1, shape) + (0 if real else 1j) * rng.uniform(-1, 1, shape))
    nug = None
    if c["nugget"]:
        # as MtGeneralEngine: sqrt(n_k) sum_i Phi^{kk}_S[i] of every sorted task
        nug = np.stack([spectra[k * lay.T - k * (k - 1) // 2].sum(-1) * math.sqrt(lay.ns[k]) for k in range(lay.T)])
    w = 1.0 if G > 1 else float(B)
    fs = FitSpec(ns=c["ns"], d=d, dl=c["dl"], B=B, G=G, task=c["task"], T_all=c["T_all"], rank=c["rank"],
                 vtask_exp=c["vtask_exp"], rows=np.array(c["rows"], dtype=np.int32), nrows=list(c["nrows"]),
                 spectra=spectra, y=y.astype(np.complex128), nug_coef=nug, nug_ref=c["nugget_ref"],
                 grad_norm=0.5, grad_logdet=0.5 * w, logdet_weight=w,
                 mll_const=float(B * G) * sum(c["ns"]) * math.log(2 * math.pi), family=0 if not real else 1)
    raw = rng.uniform(-0.5, 0.5, fs.n_params)
    if not c["vtask_exp"]:
        raw[fs.v_off:] = rng.uniform(0.3, 0.5, fs.n_params - fs.v_off)
    return fs, raw, c


def rg_mask(fs, rg):
    """requires_grad of every raw element."""
    m = np.zeros(fs.n_params, dtype=bool)
    for flag, lo, hi in zip(rg, (0, fs.l_off, fs.n_off, fs.f_off, fs.v_off),
                            (fs.l_off, fs.n_off, fs.f_off, fs.v_off, fs.n_params)):
        m[lo:hi] = bool(flag)
    return m


def fill_desc(fs, c):
    """fgp_mt_fit_desc of a case without its pointers (the caller sets spectra, y, raw, the Rprop state, the histories,
    rows and work): what fgp_mt_fit_work / fgp_mt_fit_work_layout validate."""
    from fastgaussianprocesses_amd import _native as N
    desc = N.MtFitDesc()
    desc.family, desc.d, desc.B = int(fs.family), int(fs.d), int(fs.B)
    desc.G = int(fs.G)
    for q in range(5):
        desc.nrows[q] = int(fs.nrows[q])
    desc.layout.T = fs.lay.T
    for k, n in enumerate(fs.lay.ns):
        desc.layout.n[k] = n
        desc.task[k] = int(fs.task[k])
    desc.T_all, desc.rank, desc.dl = int(fs.T_all), int(fs.rank), int(fs.dl)
    o = 0
    for p, s in enumerate(fs.spectra):
        desc.spec_off[p] = o
        o += s.size
    desc.vtask_exp = int(fs.vtask_exp)
    desc.rg_scale, desc.rg_ls, desc.rg_noise, desc.rg_factor, desc.rg_vtask = (int(v) for v in c["rg"])
    desc.grad_norm, desc.grad_logdet = fs.grad_norm, fs.grad_logdet
    desc.logdet_weight, desc.mll_const = fs.logdet_weight, fs.mll_const
    desc.eta_minus, desc.eta_plus = ETAS
    desc.step_min, desc.step_max = STEPS
    desc.nugget_ref = int(fs.nug_ref)
    return desc
