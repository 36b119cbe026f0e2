"""The case matrix of the prediction-kernel tests (tests/test_gpu_predict_exact.py on the device,
tests/test_predict_reference_cpu.py without one), the inputs of every case and the derived tolerance factors.

Inputs are synthetic, so the conditioning is chosen and not inherited from a fitted GP:
  'regular'  lengthscales in [0.02, 0.25], positive coefficients.  With |coef B| <= 19.74 / 6, 64.94 / 30, 85.46 / 42,
             60.24 / 30 (alpha 1..4: coef = (2 pi)^(2 alpha) / (2 alpha)!, max |B_2..B_8| = 1/6, 1/30, 1/42, 1/30) and
             Walsh parts in [-1/2, 3/2] every factor lies in about [0.17, 1.9] and no term of a mean cancels: the cap
             C 2^-53 B_q <= 1e-11 |q| holds for every output.
  'signed'   lengthscales in [0.02, 5] (factors cross zero), randn coefficients: max_q B_q <= 100 max_q |q|.
Test points: row 0 all 0, row 1 all 1, row 2 training point 5 (delta == 0, t == 0), the rest rand; training points rand
(lattice) / randint(0, 2^t) (net; at t = 63 point 5 keeps 52 bits, so it is a double).

Tolerance factors C of |device - reference| <= C 2^-53 B_q: the worst-case linear count of the kernel's roundings, per
term and per summation level, in units of the bound's terms (tests/predict_reference.py); u = 2^-53.

  a factor, FACTOR_COUNT (units of bf, the factor's term magnitudes):
    lattice 10   a = l coef (1 on every a-term); c = 1 +- a / k: constant, product, sum (3 on |a B(0)|, 1 on 1);
                 u = fma(t, t, -t) once, through the polynomial in u at most 2.5 (orders 2 / 4 / 6 / 8: 1 / 2 / 2.34 /
                 2.5 = the logarithmic derivative on u in [-1/4, 0]); the products and inner fmas 0 / 1 / 3 / 5; the
                 last fma 1 on |f| <= bf.  Order 8: (1 + 2.5 + 5) |a (B - B(0))| + 4 |a B(0)| + 1 + bf <= 9.5 bf.  The
                 folded order-4 factor a (u^2 + c'), c' = c / a: c' carries c's 4 and the division, the fma 1 -- less.
    net 1    2   1 + l, 3 l, the subtraction: (1 + l) + 3 l 2^(..) + |f| <= 2 bf.
    net 2    8   omega_2 = fma(-beta, x, 5/2 (1 - t1)) - 1: x's rounding at t > 53 (beta x <= 1), 1 - t1 and the
                 product (2 x 5/2), the fma (5/2), the last sum (3/2): 10 u = 6.7 W_2 u; the factor's own fma 1.
    net 3   28   omega_3's three terms have magnitudes <= 1, 5, 43/18 with 3 roundings each, the two fmas 7.4 and
                 2.4, the last sum 1.4: 36.4 u = 26.2 W_3 u; + 1.
    net 4  t+5   the recursion's t steps round E, e3, e2 (and e1 at t > 53) once each, and |E| + e1 + e2 + e3 <= W_4
                 throughout (it is omega_4(0) with every sign +): t W_4 u; the three last sums 3 W_4 u; + 1.
  rows (k_kernel_rows)       max_j FACTOR_COUNT + 2: the d - 1 products and the scale are d roundings of |K|, and
                             B_K >= d |K| (bf_j >= |f_j|), so they are at most 1 unit of B_K; 1 to spare.
  mean (k_post_mean + k_sum_chunks)   max_j FACTOR_COUNT + 3 + min(chunk, n) + ceil(nchunks / 256) + 9: the products,
                             the scale and (folded) the d factors a_j moved into it: (2 d) / d + 1; a term passes
                             through at most min(chunk, n) accumulating fmas of its thread; the chunk sums: a strided
                             thread sum, 6 shuffle levels and 3 wave sums.
  mean by GEMM               max_j FACTOR_COUNT + 2 + n: a dot product of n terms in whatever order the library takes.
  quadratic form             max(rows, 44): bin 0 has the mean re-added twice (4 on its term), |.|^2 / n wa is 5,
                             16 terms per thread, 6 + 3 levels of block_sum, the partials' sum 1 + 9; the transform's
                             error is in the bound with its own constant, the rows' error enters through ||B_r||_2.
  variance (k_qf_finish)     max(quadratic form, 2 d + 2): K(x, x) is d sums, d products, the scale; the subtraction.
"""
import collections
import functools
import math

import numpy as np

from tests import predict_reference as PR

LAT, NET = PR.LAT, PR.NET

RM = collections.namedtuple("RM", "name fam d n N B Gk chunk alphas tbits kind zero_ls tiny pad path seed")


def _rm(group, fam, d, n=257, N=5, B=1, Gk=None, chunk=32, alphas=None, tbits=32, kind="regular", zero_ls=False,
        tiny=False, pad=0, path="direct", seed=0):
    if Gk is None:
        Gk = B
    if alphas is None:
        alphas = [2] * d if fam == LAT else [1] * d
    alphas = [int(a) for a in alphas]
    name = "%s-%s-d%d-n%d-N%d-B%d-G%d-c%d-a%s" % (group, "lat" if fam == LAT else "net", d, n, N, B, Gk, chunk,
                                                  "".join(map(str, alphas)))
    if fam == NET:
        name += "-t%d" % tbits
    for flag, tag in ((kind == "signed", "signed"), (zero_ls, "ls0"), (tiny, "tiny"), (pad, "pad"), (path != "direct", path)):
        if flag:
            name += "-" + tag
    return RM(name, fam, d, n, N, B, Gk, chunk, tuple(alphas), tbits if fam == NET else 0, kind, zero_ls, tiny, pad, path, seed)


def _mixed(d):
    return [1 + j % 4 for j in range(d)]


def _rm_matrix():
    c = []
    for fam in (LAT, NET):
        # every D instantiation
        for d in range(1, 9):
            c.append(_rm("dim", fam, d))
    # every variant at d in {3, 8}, with one output (NB = 1 instances) and three (NB = 4, one dead lane)
    for d in (3, 8):
        for B in (1, 3):
            for a in (1, 2, 3, 4):
                c.append(_rm("var", LAT, d, B=B, alphas=[a] * d))               # 2: the fold; 1, 3, 4: ORD = 0
            c.append(_rm("var", LAT, d, B=B, alphas=_mixed(d)))                 # ORD = 0, per-dimension orders
            c.append(_rm("var", LAT, d, B=B, zero_ls=True))                     # the fold refused: a == 0
            c.append(_rm("var", NET, d, B=B, alphas=_mixed(d)))
            c.append(_rm("var", NET, d, B=B, tbits=63))
            c.append(_rm("var", NET, d, B=B, alphas=_mixed(d), tbits=63))
    # factors that cross zero, signed coefficients
    for d in (3, 8):
        c.append(_rm("sgn", LAT, d, n=33, B=3, kind="signed"))
        c.append(_rm("sgn", LAT, d, n=33, B=3, alphas=_mixed(d), kind="signed"))
        c.append(_rm("sgn", NET, d, n=33, B=3, alphas=_mixed(d), kind="signed"))
    c.append(_rm("sgn", NET, 3, n=33, B=1, kind="signed"))
    # shapes: n and N off the 256-point slab / 256-thread tile, both chunk sizes
    Ns = (1, 255, 257)
    i = 0
    for fam in (LAT, NET):
        for n in (1, 255, 256, 257, 1025):
            for chunk in (32, 1024):
                c.append(_rm("shape", fam, 2, n=n, N=Ns[i % 3], chunk=chunk))
                i += 1
        for N in Ns:
            c.append(_rm("shape", fam, 2, n=1025, N=N, B=2, chunk=32 if N == 255 else 1024))
    # outputs and hyper-parameter rows
    for fam in (LAT, NET):
        for B in (1, 2, 3, 4):
            for Gk in sorted(set((1, B))):
                c.append(_rm("out", fam, 3, n=300, B=B, Gk=Gk, path="ops"))
        c.append(_rm("out", fam, 3, n=300, B=4, Gk=2))                           # g = b mod Gk, 1 < Gk < B
        c.append(_rm("out", fam, 3, n=300, B=3, Gk=3))
        c.append(_rm("out", fam, 3, n=300, B=10, Gk=10))                         # block launch + remainder
        c.append(_rm("out", fam, 3, n=300, B=8, Gk=1, path="ops"))               # kernel rows + GEMM
        c.append(_rm("out", fam, 3, n=300, B=3, Gk=3, pad=8))                    # coeff_stride = n + 8
    # tiny lengthscales: prod a underflows and prod c' overflows in the folded form
    for d in (6, 8):
        for B in (1, 4):
            c.append(_rm("tiny", LAT, d, B=B, tiny=True))
    return c


RM_CASES = _rm_matrix()
assert len(set(c.name for c in RM_CASES)) == len(RM_CASES)
RM_BY_NAME = {c.name: c for c in RM_CASES}

BT = collections.namedtuple("BT", "name fam d n N P own_xt seed")
BT_CASES = [BT("batched-%s-xt%d" % ("lat" if fam == LAT else "net", own), fam, 3, 1025, 257, 3, own, 0)
            for fam in (LAT, NET) for own in (0, 1)]
BT_BY_NAME = {c.name: c for c in BT_CASES}

QF = collections.namedtuple("QF", "name fam m d alphas tbits r2c seed")


def _qf(fam, m, d, alphas, r2c=None, seed=0):
    name = "qf-%s-m%d-d%d-a%s%s" % ("lat" if fam == LAT else "net", m, d, "".join(map(str, alphas)),
                                    "-r2c0" if r2c == "0" else "")
    return QF(name, fam, m, d, tuple(alphas), 32 if fam == NET else 0, r2c, seed)


QF_CASES = [
    _qf(LAT, 13, 2, [2, 2]), _qf(LAT, 16, 3, [2, 1, 3]),                         # full length
    _qf(LAT, 17, 1, [2]), _qf(LAT, 17, 3, [1, 2, 3]), _qf(LAT, 17, 5, [2] * 5),  # half length (R2C): ORD = 0 and 4
    _qf(LAT, 17, 3, [1, 2, 3], r2c="0"),                                         # FGP_R2C=0: full length at 2^17
    _qf(NET, 13, 2, [1, 1]), _qf(NET, 13, 4, [1, 2, 3, 4]), _qf(NET, 17, 2, [1, 1]), _qf(NET, 17, 3, [2, 3, 4]),
]
QF_BY_NAME = {c.name: c for c in QF_CASES}
WA_KINDS = ("one", "unif", "gp")
QF_N, QF_P = 3, 2
GP_NOISE = 1e-4


# ------------------------------------------------------------------------------------------------ tolerance factors
def factor_count(fam, order, tbits):
    """Roundings of one factor in units of its term magnitudes bf (module docstring); order: alpha (lattice) /
    Walsh order (net)."""
    if fam == LAT:
        return 10
    return {1: 2, 2: 8, 3: 28}.get(int(order), int(tbits) + 5)


def c_factor(case):
    return max(factor_count(case.fam, a, case.tbits) for a in case.alphas)


def c_rows(case):
    return c_factor(case) + 2


def c_mean(case, chunk=None):
    if case.path == "ops" and case.Gk == 1 and case.B >= 8:
        return c_factor(case) + 2 + case.n
    chunk = case.chunk if chunk is None else chunk
    nchunks = (case.n + chunk - 1) // chunk
    return c_factor(case) + 3 + min(chunk, case.n) + (nchunks + 255) // 256 + 9


def c_batched(case):
    """fgp_post_mean_batched takes 512, 1024 or 2048 training points per workgroup (post_mean_chunk)."""
    return 10 + 3 + min(2048, case.n) + 1 + 9 if case.fam == LAT else 2 + 3 + min(2048, case.n) + 1 + 9


def c_quadform(case):
    return max(c_rows(case), 44)


def c_var(case):
    return max(c_quadform(case), 2 * case.d + 2)


# ------------------------------------------------------------------------------------------------ inputs
def lattice_coef(alpha):
    from fastgaussianprocesses_amd.ops import lattice_coefficient
    return lattice_coefficient(int(alpha))


def pred_args(fam, alphas):
    """(order [d], coef [d]) as the C entry points take them."""
    if fam == LAT:
        return [2 * a for a in alphas], [lattice_coef(a) for a in alphas]
    return list(alphas), [0.0] * len(alphas)


def part0(fam, alphas):
    """The parts at zero distance, coef B_2a(0) / walsh1(0) = 1 / omega_a(0), rounded to fp64 (k_qf_finish's input)."""
    if fam == LAT:
        return [lattice_coef(a) * float(PR.BERNOULLI[2 * a][-1]) for a in alphas]
    return [1.0 if a == 1 else float(PR.WALSH_W[a]) for a in alphas]


def _points(g, fam, d, n, N, tbits):
    """(xt [N, d], z [d, n])."""
    xt = g.random((N, d))
    if fam == LAT:
        z = g.random((d, n))
    else:
        z = g.integers(0, 2 ** tbits, (d, n), dtype=np.int64)
        if tbits > 52 and n > 5:
            z[:, 5] = (z[:, 5] >> (tbits - 52)) << (tbits - 52)
    xt[0] = 0.0
    if N > 1:
        xt[1] = 1.0
    if N > 2 and n > 5:
        xt[2] = z[:, 5] if fam == LAT else z[:, 5].astype(np.float64) * 2.0 ** -tbits
        if fam == NET:
            assert (PR.net_bits(xt[2], tbits) == z[:, 5].astype(np.uint64)).all()
    return xt, z


def _hyp(g, G, d, kind):
    hi = 5.0 if kind == "signed" else 0.25
    h = np.empty((G, 1 + d))
    h[:, 0] = 0.5 + 1.5 * g.random(G)
    h[:, 1:] = 0.02 + (hi - 0.02) * g.random((G, d))
    return h


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def rm_inputs(case):
    """dict: xt [N, d], z [d, n], hyp [Gk, 1 + d], coeffs [B, n] (a view of [B, n + pad]), order, coef."""
    g = _rng(11, case.fam, case.d, case.n, case.N, case.B, case.Gk, case.chunk, sum(case.alphas), case.tbits, case.seed)
    xt, z = _points(g, case.fam, case.d, case.n, case.N, case.tbits)
    hyp = _hyp(g, case.Gk, case.d, case.kind)
    if case.zero_ls:
        hyp[:, 1 + case.d // 2] = 0.0
    if case.tiny:
        hyp[:, 1:] = 1e-60
    full = g.standard_normal((case.B, case.n + case.pad)) if case.kind == "signed" else \
        0.1 + g.random((case.B, case.n + case.pad))
    order, coef = pred_args(case.fam, case.alphas)
    return dict(xt=xt, z=z, hyp=hyp, coeffs_full=full, coeffs=full[:, :case.n], order=order, coef=coef)


@functools.lru_cache(maxsize=4)
def rm_reference(name):
    """(inputs, K, B_K, mean, B_mean) of a rows-and-mean case, computed once."""
    case = RM_BY_NAME[name]
    inp = rm_inputs(case)
    K, BK = PR.kernel_rows(case.fam, inp["xt"], inp["z"], inp["hyp"], inp["order"], inp["coef"], case.tbits)
    mean, Bm = PR.post_mean(K, BK, inp["coeffs"])
    return inp, K, BK, mean, Bm


def bt_inputs(case):
    """P problems with their own points, hyper-parameters and coefficients: xt [P, N, d] (row 0 for all problems
    unless own_xt), z [P, d, n], hyp [P, 1 + d], coeffs [P, n]."""
    g = _rng(12, case.fam, case.d, case.n, case.N, case.P, case.seed)
    tb = 32 if case.fam == NET else 0
    pts = [_points(g, case.fam, case.d, case.n, case.N, tb) for _ in range(case.P)]
    xt = np.stack([p[0] for p in pts])
    if not case.own_xt:
        xt = xt[:1]
    alphas = [2] * case.d if case.fam == LAT else [1] * case.d
    order, coef = pred_args(case.fam, alphas)
    return dict(xt=xt, z=np.stack([p[1] for p in pts]), hyp=_hyp(g, case.P, case.d, "regular"),
                coeffs=0.1 + g.random((case.P, case.n)), order=order, coef=coef, tbits=tb, alphas=alphas)


@functools.lru_cache(maxsize=2)
def bt_reference(name):
    case = BT_BY_NAME[name]
    inp = bt_inputs(case)
    out, bnd = [], []
    for p in range(case.P):
        K, BK = PR.kernel_rows(case.fam, inp["xt"][p if case.own_xt else 0], inp["z"][p], inp["hyp"][p:p + 1],
                               inp["order"], inp["coef"], inp["tbits"])
        m, b = PR.post_mean(K, BK, inp["coeffs"][p:p + 1])
        out.append(m[0])
        bnd.append(b[0])
    return inp, np.stack(out), np.stack(bnd)


def gp_weights(fam, m, d, alphas, seed):
    """wa = Re(1 / ev) [n] of a real GP on n = 2^m points of a rank-1 lattice / digital net: ev = sqrt(n) ft(k1) +
    noise, noise 1e-4, the kernel's scale 1e-2 / n so that ev spans [1e-4, ~1e-2] -- the bound of the quadratic form
    carries sqrt(max |wa|) against sqrt(wa) of the frequencies that hold the row's energy, and a spectrum of ratio
    1e8, as a unit-scale kernel has at this noise, would make any bound of an fp64 transform vacuous."""
    import torch

    import fastgaussianprocesses_amd as F
    from oracle import fgp_oracle as O
    n = 1 << m
    ls = torch.full((d,), 0.2, dtype=torch.float64)
    sc = torch.tensor([1e-2 / n], dtype=torch.float64)
    if fam == LAT:
        x = torch.from_numpy(F.Lattice(d, seed=seed)(0, n))
        parts, tr = O.lattice_k1parts(x, list(alphas)), O.fftbr
    else:
        seq = F.DigitalNetB2(d, seed=seed)
        xb = torch.from_numpy(seq(0, n, return_binary=True).astype(np.int64))
        parts, tr = O.net_k1parts(xb, seq.t, list(alphas)), O.fwht
    k1 = O.kernel_from_parts(parts, sc, ls)
    ev = math.sqrt(n) * O.ft_stable(k1.to(torch.float64), tr) + GP_NOISE
    return np.ascontiguousarray((1.0 / ev).real.numpy() if torch.is_complex(ev) else (1.0 / ev).numpy())


def qf_inputs(case, gen_points=None):
    """dict: xt [N, d], z [d, n] (gen_points [P, n, d]: z [P, d, n], the materialised lattice of every problem, and
    row 2 of xt is point 5 of problem 0), hyp [P, 1 + d], wa {kind: [n]}, order, coef, part0."""
    n = 1 << case.m
    g = _rng(13, case.fam, case.m, case.d, sum(case.alphas), case.seed)
    xt, z = _points(g, case.fam, case.d, n, QF_N, case.tbits)
    if gen_points is not None:
        z = np.ascontiguousarray(np.swapaxes(np.asarray(gen_points, dtype=np.float64), 1, 2))
        xt[2] = z[0][:, 5]
    hyp = _hyp(g, QF_P, case.d, "regular")
    unif = 0.5 + g.random(n)
    if case.fam == LAT:                               # the weights of a Hermitian spectrum: wa[n - k] = wa[k]
        unif[n // 2 + 1:] = unif[1:n // 2][::-1]
    wa = dict(one=np.ones(n), unif=unif, gp=gp_weights(case.fam, case.m, case.d, case.alphas, 7 + case.seed))
    order, coef = pred_args(case.fam, case.alphas)
    return dict(xt=xt, z=z, hyp=hyp, wa=wa, order=order, coef=coef, part0=part0(case.fam, case.alphas))


def qf_gen(case):
    """(generating vector [d], shifts [P, d]) of the regenerated-lattice form of a lattice case."""
    import fastgaussianprocesses_amd as F
    seqs = [F.Lattice(case.d, seed=21 + p) for p in range(QF_P)]
    return [int(v) for v in seqs[0].z], np.stack([s.shift for s in seqs])


def qf_gen_points_cpu(case):
    """[P, n, d]: the lattices of qf_gen from the host generator (bit-identical to ops.lattice_points)."""
    import fastgaussianprocesses_amd as F
    zg, sh = qf_gen(case)
    return np.stack([F.Lattice(case.d, generating_vector=zg, shift=sh[p])(0, 1 << case.m) for p in range(QF_P)])


def qf_reference(case, inp, regenerated=False):
    """Rows [P, N, n] of the P hyper-parameter rows, their bounds and spectrum powers: what every weight shares."""
    rows, Br = [], []
    for p in range(QF_P):
        zp = inp["z"][p] if inp["z"].ndim == 3 else inp["z"]
        K, BK = PR.kernel_rows(case.fam, inp["xt"], zp, inp["hyp"][p:p + 1], inp["order"], inp["coef"], case.tbits,
                               regenerated=regenerated)
        rows.append(K[0])
        Br.append(BK[0])
    power = [PR.spectrum_power(case.fam, r) for r in rows]
    return rows, Br, power


def var_weights(k0, q, clamp):
    """The factor that scales a problem's weights so that its variances K(x, x) - q are all positive (clamp False:
    max q = 3/4 K(x, x)) or all clamped (min q = 3/2 K(x, x)): a power of two, so the scaled weights are exact."""
    q = PR.to_f64(q)
    f = (1.5 * float(k0) / q.min()) if clamp else (0.75 * float(k0) / q.max())
    return 2.0 ** math.floor(math.log2(f)) if not clamp else 2.0 ** math.ceil(math.log2(f))
