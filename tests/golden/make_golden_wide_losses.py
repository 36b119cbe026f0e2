"""Golden GCV / CV fit trajectories of wide GPs (9 <= d <= 64) with a trained noise, from the REAL reference, into
tests/golden/wide_losses/*.npz (a directory of its own: tests/test_gpu_wide.py::test_fixtures_present counts the files of
tests/golden/wide/).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_losses.py [fixture names...]

Point sets, lengthscales, data and seeds are make_golden_wide.py's (its net_matrices, lengthscales_for, case_name and
make_y).  Digital nets only: the reference's lattice GCV / CV raise TypeError (make_golden_losses.py).

Every case is built with noise=1e-2 and requires_grad_noise=True and fitted twice from fresh GPs, by
fit(loss_metric="GCV") and by fit(loss_metric="CV", cv_weights=0.5), 4 iterations, stop_crit_wait_iterations=9.  With
the default 1e-16 nugget GCV and CV coincide to the printed digits and training the noise changes nothing; at 1e-2 the
losses fall monotonically and the noise moves by Rprop's full factor every step, so no sign fork is near.

Keys: the inputs of tests.gpu_fixtures.product_gp (family, m, d, alpha, B, per_output, C, t, shift, x, xb, y), the
`lengthscales` and `noise` the GP was built with, `x_test` [16, d], and per metric (prefix gcv_ / cv_) loss_hist,
scale_hist, lengthscales_hist, noise_hist, raw_scale, raw_lengthscales, raw_noise, pmean.
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
from make_golden_wide import case_name, lengthscales_for, make_y, net_matrices  # noqa: E402

OUT = os.path.join(HERE, "wide_losses")
ITS = 4
WAIT = 9
NOISE = 1e-2
CV_WEIGHT = 0.5

CASES = [
    # family, m, d, alpha, B, per_output
    ("net", 6, 64, 1, 3, False),       # three outputs, shared hyper-parameters
    ("net", 7, 13, 2, 0, False),
    ("net", 4, 9, 1, 0, False),        # n = 16, the device loop's smallest size
]


def build(fg, qmcpy, c, out=None, seed=7):
    """A fresh reference GP of case c (the nugget NOISE, trained) with its data; fills the inputs into `out`."""
    family, m, d, alpha, B, po = c
    assert family == "net" and not po
    n = 2 ** m
    ls = lengthscales_for(d, B, po)
    t = 32
    C = net_matrices(d, t=t)
    shift = np.random.default_rng(seed).integers(0, 2 ** t, size=d, dtype=np.uint64)
    seq = qmcpy.DigitalNetB2(d, randomize="DS", generating_matrices=C, t=t, shift=shift)
    gp = fg.FastGPDigitalNetB2(seq, alpha=alpha, shape_batch=[B] if B > 0 else [], lengthscales=ls.clone(),
                               noise=NOISE, requires_grad_noise=True)
    x = gp.get_x_next(n)
    y = make_y(x, B)
    gp.add_y_next(y)
    if out is not None:
        out.update({"family": np.array(family), "m": np.array(m), "d": np.array(d), "alpha": np.array(alpha),
                    "B": np.array(B), "per_output": np.array(po), "lengthscales": _np(ls), "noise": np.array(NOISE),
                    "C": C.astype(np.int64), "t": np.array(t), "shift": shift.astype(np.int64),
                    "x": _np(x), "xb": _np(gp.get_xb(0)), "y": _np(y)})
    return gp


def gen_case(fg, qmcpy, c):
    d = c[2]
    out = {}
    build(fg, qmcpy, c, out)
    xt = torch.rand((16, d), generator=torch.Generator().manual_seed(17))
    out["x_test"] = _np(xt)
    out["cv_weight"] = np.array(CV_WEIGHT)
    for metric, kw in (("GCV", {}), ("CV", {"cv_weights": CV_WEIGHT})):
        gp = build(fg, qmcpy, c)
        data = gp.fit(loss_metric=metric, iterations=ITS, store_hists=True, verbose=0, stop_crit_wait_iterations=WAIT,
                      **kw)
        assert data["iterations"] == ITS
        key = metric.lower()
        out[key + "_loss_hist"] = _np(data["loss_hist"])
        out[key + "_scale_hist"] = _np(data["scale_hist"])
        out[key + "_lengthscales_hist"] = _np(data["lengthscales_hist"])
        out[key + "_noise_hist"] = _np(data["noise_hist"])
        out[key + "_raw_scale"] = _np(gp.raw_scale)
        out[key + "_raw_lengthscales"] = _np(gp.raw_lengthscales)
        out[key + "_raw_noise"] = _np(gp.raw_noise)
        out[key + "_pmean"] = _np(gp.post_mean(xt))
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
        print("wrote %s (%d KB)" % (name, os.path.getsize(fn) // 1024))
        for key in ("gcv", "cv"):
            print("  %s loss %s noise %s" % (key, out[key + "_loss_hist"], out[key + "_noise_hist"].reshape(-1)))


if __name__ == "__main__":
    main()
