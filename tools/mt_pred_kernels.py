"""Launch only the d <= 8 multitask prediction kernels (csrc/fgp_mt_pred.hip) at a user's size, for a rocprofv3 counter
pass or kernel trace run on its own.

  python tools/mt_pred_kernels.py [--log2n 16] [--points 256] [--reps 3] [--dims 3 6]

Per d: a lattice GP with T = 3 tasks of n = 2^log2n points each (tools/prof_mt_narrow_pred.make_gp), and one
derivative-informed GP (f, d1 f, d2 f) at d = 4, n = 2^14; `--reps` calls of post_mean by the kernel rows
(FGP_WIDE_MT_POST_MEAN=0: k_mt_rows<0, D, 1, true>, 9 launches a call) and by the matrix-free sum (=1: k_mt_post_mean<0, D, 1,
1, true> + k_mt_post_mean_sum), and of post_var's prior term (k_mt_rows_zip).  What a post_mean call moves and computes
follows from the shapes and is printed per configuration: T T N n pairs (test point, training point); the rows route
stores 8 bytes a pair and reads the T n D training coordinates (8 bytes each, from cache after the first test point);
a lattice pair at alpha = 2 with P = 1 costs about 10 D FP64 instructions (per dimension: the difference, mod 1, B_4
in u = t (t - 1), the product with coef, the factor's fma, the running product).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

torch.set_default_dtype(torch.float64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--log2n", type=int, default=16)
    p.add_argument("--points", type=int, default=256)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--dims", type=int, nargs="*", default=[3, 6])
    a = p.parse_args()
    import prof_mt_narrow_pred as P
    if not torch.cuda.is_available():
        raise SystemExit("mt_pred_kernels: no GPU")
    names = []
    for d in a.dims:
        name = "mt_d%d_n%d_N%d" % (d, a.log2n, a.points)
        P.CONFIGS[name] = (d, a.log2n, a.points, False)
        names.append(name)
    names.append("grad_d4_n14_N256")
    os.environ["FGP_MT_FUSED_ROWS"] = "1"
    for name in names:
        gp = P.make_gp(name)
        x = torch.rand((P.CONFIGS[name][2], gp.d), generator=torch.Generator().manual_seed(1)).to("cuda")
        with torch.no_grad():
            gp.coeffs
        for _ in range(a.reps):
            for route in ("0", "1"):
                os.environ["FGP_WIDE_MT_POST_MEAN"] = route
                gp.post_mean(x)
            with torch.no_grad():
                for t in range(gp.num_tasks):
                    gp._kmat_block(x, x, t, t, zip_pairs=True)
        torch.cuda.synchronize()
        n, N, T = gp._ns[0], x.shape[0], gp.num_tasks
        print("%s: %d reps; per post_mean call %d pairs (test point, training point): rows store %d bytes, read %d bytes of "
              "training points" % (name, a.reps, T * T * N * n, 8 * T * T * N * n, 8 * T * n * gp.d))


if __name__ == "__main__":
    main()
