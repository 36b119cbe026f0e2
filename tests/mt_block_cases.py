"""Seeded inputs of the block entry points' tests (fgp_mt_factor, fgp_mt_solve, fgp_mt_selinv, fgp_mt_mll_grad): the
lams and vectors of tests/mt_qf_cases.py (diagonally dominant: small growth, info == 0) on the layouts below, each the
smallest shape that reaches its path.  A case is (name, ns, G, B, scale); every case runs for both families.

  one_task        [256]               T = 1
  equal_256       [256, 256]          equal n
  sixteen_16      16 tasks of 16      T = FGP_MT_MAX_TASKS, a partly filled workgroup
  three_levels    [256, 64, 8]        three size levels, R = 41
  repeated_sizes  [64, 64, 8, 8]      q mod q_l with equal and unequal partners
  nmin_1          [1024, 1]           one class, R = 1025
  two_workgroups  [512, 512, 512]     two workgroups of classes
  tiny_pivots     [256, 256, 64]      lams scaled by 2^-40
  g3_b6 / g3_b12  G = 3               vector b against problem b mod G
"""
import numpy as np

from tests.mt_qf_cases import FAMILIES, make_lams, make_vectors

CASES = [
    ("one_task", [256], 1, 2, 1.0),
    ("equal_256", [256, 256], 1, 2, 1.0),
    ("sixteen_16", [16] * 16, 1, 2, 1.0),
    ("three_levels", [256, 64, 8], 1, 3, 1.0),
    ("repeated_sizes", [64, 64, 8, 8], 1, 2, 1.0),
    ("nmin_1", [1024, 1], 1, 2, 1.0),
    ("two_workgroups", [512, 512, 512], 1, 2, 1.0),
    ("tiny_pivots", [256, 256, 64], 1, 2, 2.0 ** -40),
    ("g3_b6", [64, 64, 8, 8], 3, 6, 1.0),
    ("g3_b12", [256, 64, 8], 3, 12, 1.0),
]
CASE_IDS = [c[0] for c in CASES]


def case_inputs(case, family):
    """(lams [G, L] complex128, v [B, R nmin] complex128, grad_norm [B], grad_logdet [G]); the two weights differ per
    vector / problem and have mixed signs."""
    name, ns, G, B, scale = case
    seed = 500 + CASE_IDS.index(name) * 2 + FAMILIES.index(family)
    rng = np.random.default_rng(seed + 2000)
    gn = rng.uniform(0.25, 1.0, B) * np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    gl = rng.uniform(0.25, 1.0, G) * np.where(np.arange(G) % 2 == 0, -1.0, 1.0)
    return (make_lams(ns, G, family, scale, seed), make_vectors(ns, B, family, seed).astype(np.complex128), gn, gl)
