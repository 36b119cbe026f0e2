"""Golden posterior variances of wide GPs (9 <= d <= 64) at n >= 2^13 -- the sizes at which post_var takes the
Parseval quadratic form (fgp_wide_post_var_qf) -- from the REAL reference, into tests/golden/wide_pvar/*.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_pvar.py [fixture names...]

Point sets, lengthscales and observations are those of make_golden_wide.build.  The points themselves are not stored
(4 MB at d = 64): `x_head` = x[:8] and `x_tail` = x[-8:] pin the point generation instead.  Keys: the case fields,
z / C, t, shift, lengthscales, y, x_head, x_tail, x_test [16, d] (row 0 starts with the coordinates 0.0, 1.0 and 0.5,
row 1 is training point 5), pvar, pvar_2n (post_var(x_test, n=2n)) and kxx = K(x_test, x_test).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle.refshim.load_reference import import_reference  # noqa: E402
from make_golden import _np  # noqa: E402
from make_golden_wide import build, case_name  # noqa: E402

OUT = os.path.join(HERE, "wide_pvar")

CASES = [
    # family, m, d, alpha, B, per_output
    ("lattice", 13, 64, 2, 0, False),
    ("lattice", 13, 9, 3, 0, False),
    ("lattice", 13, 12, 2, 3, True),
    ("net", 13, 9, 1, 0, False),
    ("net", 13, 13, 2, 0, False),       # Walsh order 2: parity unpinned at the qmcpy boundary
    ("net", 14, 64, 1, 0, False),
]


def gen_case(fg, qmcpy, c):
    family, m, d, alpha, B, po = c
    n = 2 ** m
    out = {}
    gp = build(fg, qmcpy, c, out)
    x = out.pop("x")
    out.pop("xb")
    out["x_head"] = x[:8].copy()
    out["x_tail"] = x[-8:].copy()
    xt = torch.rand((16, d), generator=torch.Generator().manual_seed(23))
    xt[0, 0], xt[0, 1], xt[0, 2] = 0.0, 1.0, 0.5
    xt[1] = torch.from_numpy(x[5])
    out["x_test"] = _np(xt)
    out["pvar"] = _np(gp.post_var(xt))
    out["pvar_2n"] = _np(gp.post_var(xt, n=2 * n))
    out["kxx"] = _np(gp.kernel(xt, xt))
    return out


def main():
    torch.set_default_dtype(torch.float64)
    fg = import_reference()
    import qmcpy
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for c in CASES:
        name = case_name(c)
        if only and name not in only:
            continue
        out = gen_case(fg, qmcpy, c)
        fn = os.path.join(OUT, name + ".npz")
        np.savez_compressed(fn, **out)
        print("wrote %s (%d KB)  K(x,x)=%.4g  pvar in [%.3g, %.3g]  pvar_2n max %.3g" % (
            name, os.path.getsize(fn) // 1024, float(out["kxx"].max()), float(out["pvar"].min()),
            float(out["pvar"].max()), float(out["pvar_2n"].max())))


if __name__ == "__main__":
    main()
