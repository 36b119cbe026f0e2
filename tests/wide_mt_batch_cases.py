"""Parameter-batched problems of fgp_wide_mt_fit_run (fgp_wide_mt_fit_batch_desc): the seeded cases of the
stage-by-stage test (tests/test_gpu_wide_mt_fit_batch_exact.py) and the loaders of the reference fixtures
(tests/golden/wide_batch_mt/*.npz) of tests/test_gpu_wide_mt_fit_batch.py.

Staged cases, all at d = 9 -- the smallest shapes that reach each index path of the G-fold layout:

  {lat,net}-G3     T = 2, n = [512, 256], G = 3, dl = d: two workgroups of partials for the long task and one for the short
                   (an untouched fill word stays behind the short pairs); scale and noise per problem, lengthscales,
                   factor and task noise shared
  lat-G6-dl1       T = 3, n = [256, 256, 64], G = 6 from shape_batch [2, 3], dl = 1: scale and factor rows [2, 3],
                   lengthscale and task-noise rows [3] (a trailing-dimension broadcast: row g mod 3), noise shared; one
                   pair conjugated
  net-deriv-G2     P = 3 multi-index pairs per task pair, n = [64, 16], G = 2, the task factor frozen
  lat-big-G2       T = 2, n = [2^17, 2^17], G = 2: 512 partials per row (the second level's lanes stride) and the
                   half-length transforms; every block per problem

The parts, the data and the parameter ranges are those of tests.wide_fit_cases.mt_inputs (positive, well separated
eigenvalues, strictly diagonally dominant class blocks), the parts shared by the problems, every parameter row drawn on
its own.  logdet_weight = 1/2: a power of two, so that a one-problem run's loss_hist[2] / w is exact.
"""
import collections
import functools
import glob
import math
import os

import numpy as np

from tests.wide_fit_cases import LAT, NET

BMT = collections.namedtuple("BMT", "name fam ns d dl G rowmap nrows task T_all rank vexp conj P rg lr")
LOGDET_WEIGHT = 0.5
WIDTH_NAMES = ("scale", "lengthscales", "noise", "factor", "vtask")


def _own(G):
    return list(range(G))


def _cases():
    out = []
    for fam in (LAT, NET):
        out.append(BMT("%s-G3" % ("lat" if fam == LAT else "net"), fam, (512, 256), 9, 9, 3,
                       (_own(3), [0] * 3, _own(3), [0] * 3, [0] * 3), (3, 1, 3, 1, 1), (0, 1), 2, 2, 1, (0, 0, 0), 1,
                       (1, 1, 1, 1, 1), 0.1))
    g6 = _own(6)
    m3 = [g % 3 for g in range(6)]
    out.append(BMT("lat-G6-dl1", LAT, (256, 256, 64), 9, 1, 6, (g6, m3, [0] * 6, g6, m3), (6, 3, 1, 6, 3), (0, 1, 2), 3, 2, 1,
                   (0, 1, 0, 0, 0, 0), 1, (1, 1, 1, 1, 1), 0.1))
    out.append(BMT("net-deriv-G2", NET, (64, 16), 9, 9, 2, (_own(2), _own(2), [0, 0], [0, 0], _own(2)), (2, 2, 1, 1, 2),
                   (0, 1), 2, 2, 0, (0, 0, 0), 3, (1, 1, 1, 0, 1), 0.1))
    out.append(BMT("lat-big-G2", LAT, (1 << 17, 1 << 17), 9, 9, 2, (_own(2),) * 5, (2,) * 5, (1, 0), 2, 1, 1, (0, 1, 0), 1,
                   (1, 1, 1, 1, 1), 0.1))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_BIG = BY_NAME["lat-big-G2"]
assert -(-_BIG.ns[0] // 256) == 512 and _BIG.ns[0] >= 1 << 17
for _c in CASES:
    assert all(len(r) == _c.G and 0 <= min(r) and max(r) < n for r, n in zip(_c.rowmap, _c.nrows))
    # every row of every block is some problem's
    assert all(sorted(set(r)) == list(range(n)) for r, n in zip(_c.rowmap, _c.nrows))


def widths(c):
    return (1, c.dl, 1, c.T_all * c.rank, c.T_all)


def block_offsets(c):
    """Raw offset of each block, and the raw length."""
    offs, o = [], 0
    for n, w in zip(c.nrows, widths(c)):
        offs.append(o)
        o += n * w
    return offs, o


def one_spec(c):
    """The MtSpec of ONE problem of the case (B = 1)."""
    from tests.wide_fit_reference import MtSpec
    return MtSpec(ns=list(c.ns), d=c.d, dl=c.dl, B=1, family=c.fam, task=list(c.task), T_all=c.T_all, rank=c.rank,
                  vtask_exp=c.vexp, conj=list(c.conj), logdet_weight=LOGDET_WEIGHT,
                  mll_const=0.5 * sum(c.ns) * math.log(2 * math.pi))


def gather(c, raw, g):
    """Problem g's rows of the batch raw vector as a one-problem raw vector."""
    offs, _ = block_offsets(c)
    return np.concatenate([raw[o + r[g] * w:o + (r[g] + 1) * w] for o, r, w in zip(offs, c.rowmap, widths(c))])


def columns(c):
    """For every raw element of the batch vector: (block q, row r, column in one problem's raw order)."""
    out = []
    col0 = np.cumsum((0,) + widths(c))[:5]
    for q, (n, w) in enumerate(zip(c.nrows, widths(c))):
        out += [(q, r, int(col0[q]) + e) for r in range(n) for e in range(w)]
    return out


def rg_mask(c):
    return np.concatenate([np.full(n * w, bool(f)) for n, w, f in zip(c.nrows, widths(c), c.rg)])


@functools.lru_cache(maxsize=2)
def inputs(name):
    """dict: pairs = [(parts [P, d, n_k], ind [P, d] int, cc [P])] per sorted pair (shared by the problems), y [G, R nmin]
    complex128, raw (the batch vector), rows [5, G] int32."""
    c = BY_NAME[name]
    g = np.random.default_rng([41, c.fam, len(c.ns), c.d, c.dl, c.G, c.rank, c.P, CASES.index(c)])
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
    rn = sum(c.ns)
    y = g.uniform(-1, 1, (c.G, rn)) + (0 if c.fam == NET else 1j) * g.uniform(-1, 1, (c.G, rn))
    nr = c.nrows
    noise = g.uniform(-2.0, -1.0, nr[2]) if c.ns[0] <= (1 << 13) else math.log(2e-6 * c.ns[0]) + g.uniform(0, 1, nr[2])
    raw = np.concatenate([g.uniform(-0.3, 0.3, nr[0]), np.log(g.uniform(0.1, 0.3, nr[1] * c.dl)), noise,
                          g.uniform(-0.3, 0.3, nr[3] * c.T_all * c.rank),
                          g.uniform(0.0, 0.3, nr[4] * c.T_all) if c.vexp else g.uniform(1.0, 1.4, nr[4] * c.T_all)])
    assert raw.size == block_offsets(c)[1]
    return dict(pairs=pairs, y=y.astype(np.complex128), raw=raw, rows=np.array(c.rowmap, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ reference fixtures
GDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_batch_mt")
GOLDEN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GDIR, "*.npz")))
PNAMES = ("raw_scale", "raw_lengthscales", "raw_noise", "raw_factor_task_kernel", "raw_noise_task_kernel")


def load_golden_batch(name):
    with np.load(os.path.join(GDIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def golden_gp(g, **kw):
    """The fixture's parameter-batched GP on the device, at the reference's initial parameters, with its data."""
    import torch

    import fastgaussianprocesses_amd as F
    from tests.gpu_fixtures import DEV
    fam, d, alpha, T = str(g["family"]), int(g["d"]), int(g["alpha"]), int(g["T"])
    sb = [int(v) for v in g["shape_batch"]]
    args = dict(alpha=alpha, num_tasks=T, shape_batch=sb, shape_scale=sb + [1], shape_lengthscales=sb[1:] + [d],
                shape_noise=sb[2:] + [1], shape_factor_task_kernel=sb + [T, T], shape_noise_task_kernel=sb[1:] + [T],
                device=DEV, **kw)
    if fam == "lattice":
        seqs = [F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shifts"][l]) for l in range(T)]
        gp = F.FastGPLattice(seqs, **args)
    else:
        seqs = [F.DigitalNetB2(d, randomize="DS", generating_matrices=g["C"].astype(np.uint64), t=int(g["t"]),
                               shift=g["shifts"][l].astype(np.uint64)) for l in range(T)]
        gp = F.FastGPDigitalNetB2(seqs, **args)
    with torch.no_grad():
        for nm in PNAMES:
            p = getattr(gp, nm)
            assert tuple(p.shape) == tuple(g["init_" + nm].shape), nm
            p.copy_(torch.from_numpy(g["init_" + nm]).to(DEV))
    ns = [int(v) for v in g["ns"]]
    xs = gp.get_x_next(n=torch.tensor(ns))
    for l in range(T):
        assert np.array_equal(xs[l].cpu().numpy(), g["x_%d" % l])
    gp.add_y_next([torch.from_numpy(g["y_%d" % l]).to(DEV) for l in range(T)])
    return gp
