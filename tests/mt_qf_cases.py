"""Seeded inputs of the fgp_mt_quadform tests: layouts, well-conditioned Hermitian positive-definite lams, vectors.

A case is (name, ns, G, B, pad, scale): sorted active task sizes, problems, vectors, extra elements per vector row
(v_row_stride = R nmin + pad) and the pivot scale the lams are multiplied by.  Every case runs for both families
(complex128 vectors / float64 vectors).  The shapes are the smallest that take each path of the kernel:

  one_task           [1024]             T = 1: no substitution, four class chunks
  two_256            [256, 256]         one workgroup of classes, register path
  three_512          [512, 512, 512]    two class chunks, B = 7: a group of four vectors and a group of three
  sixteen_16         16 tasks of 16     T = FGP_MT_MAX_TASKS, two vectors per thread, a partly filled workgroup
  unequal_41_rows    [256, 64, 8]       R = 41: the in-place path
  nmin_1             [1024, 1]          one class, R = 1025
  wrap_2p17          [2^17, 2^17]       512 partials per vector: the second-level sum wraps
  g3_b6 / g3_b12     G = 3              register path and in-place path
  stride_pad         v_row_stride > R nmin
  tiny_pivots        lams scaled by 2^-40: B_q and q grow by 2^40, the bound with them
"""
import numpy as np

from tests.mt_qf_reference import Layout

CASES = [
    ("one_task", [1024], 1, 3, 0, 1.0),
    ("two_256", [256, 256], 1, 5, 0, 1.0),
    ("three_512", [512, 512, 512], 1, 7, 0, 1.0),
    ("sixteen_16", [16] * 16, 1, 5, 0, 1.0),
    ("unequal_41_rows", [256, 64, 8], 1, 6, 0, 1.0),
    ("nmin_1", [1024, 1], 1, 3, 0, 1.0),
    ("wrap_2p17", [1 << 17, 1 << 17], 1, 2, 0, 1.0),
    ("g3_b6", [256, 256], 3, 6, 0, 1.0),
    ("g3_b12", [256, 256], 3, 12, 0, 1.0),
    ("g3_b6_unequal", [256, 64, 8], 3, 6, 0, 1.0),
    ("g3_b12_unequal", [256, 64, 8], 3, 12, 0, 1.0),
    ("stride_pad", [512, 512, 512], 1, 5, 6, 1.0),
    ("stride_pad_unequal", [256, 64, 8], 1, 5, 3, 1.0),
    ("tiny_pivots", [256, 256, 64], 1, 4, 0, 2.0 ** -40),
]
CASE_IDS = [c[0] for c in CASES]
FAMILIES = ["lattice", "net"]


def make_lams(ns, G, family, scale, seed):
    """[G, L] complex128 packed lams, every class block Hermitian and strictly diagonally dominant (couplings of modulus
    <= 1, diagonals in R + [1, 2]: a row has fewer than R couplings), times `scale`.  Nets: real."""
    lay = Layout(ns)
    rng = np.random.default_rng(seed)
    out = np.empty((G, lay.L), dtype=np.complex128)
    for g in range(G):
        for (k, l), o in lay.off.items():
            n = lay.ns[k]
            if k == l:
                out[g, o:o + n] = lay.R + 1.0 + rng.random(n)
            elif family == "net":
                out[g, o:o + n] = rng.uniform(-1, 1, n) / np.sqrt(2)
            else:
                out[g, o:o + n] = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)) / np.sqrt(2)
    return out * scale


def make_vectors(ns, B, family, seed):
    """[B, R nmin] complex128 (lattice) / float64 (net), entries of mixed magnitude."""
    lay = Layout(ns)
    rng = np.random.default_rng(seed + 1000)
    shape = (B, lay.R * lay.nmin)
    mag = 10.0 ** rng.uniform(-2, 2, shape)
    if family == "net":
        return mag * rng.uniform(-1, 1, shape)
    return mag * (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape))


def case_inputs(case, family):
    name, ns, G, B, pad, scale = case
    seed = CASE_IDS.index(name) * 2 + FAMILIES.index(family)
    return make_lams(ns, G, family, scale, seed), make_vectors(ns, B, family, seed)
