"""Cases, derived constants and the shared comparison of the transform tests (tests/test_transform_reference_cpu.py,
tests/test_gpu_transforms_exact.py) against tests/transform_reference.py.

Constants, counted from the code (csrc/fgp_common.h, fgp_transforms.hip, fgp_nll.hip), never from device output
-------------------------------------------------------------------------------------------------------------------
c, per butterfly stage, in units of u (2^-53; 2^-24 for the float / float2 instances):
  lattice 10   a stage is a +- w b (bfly_dit / bfly_dif / group_bfly_cx).  In a register pass with S > 0 the twiddle
               is a rounded table entry (|error| <= sqrt 2 u) times a rounded compile-time root (mul_root: sqrt 2 u
               for the constant, 2 u for its fma product), then cmul by the entry (2 u with fma) and the addition
               (1 u): 1.4 + 1.4 + 2 + 2 + 1 = 7.8; pass 0 has no table entry (4.4), the roots +-1, +-i are free (1).
               FFT_C[LAT] = 10 of tests/predict_reference.py (Higham Thm 24.2 with mu = 4.3) covers each.  The fp32
               instances round the same fp64 entries once more to fp32 (to_f2): the same count in units of 2^-24.
  net 2        one rounded addition per element and stage (FFT_C[NET]).
m_eff, the butterflies (or equally priced steps) on a path from an input to an output:
  stages                       m (full length), m - 1 (half length)
  inter-pass twiddle           lattice, m >= 13: inter_tw is the cmul of two table entries (1.4 + 1.4 + 2) and tw_mul
                               one more cmul (2): 1 step for N2 < 4096 (m = 13..15); the one-row-per-workgroup
                               form (N2 = 4096: m >= 16 and every half-length row pass) uses RowTwiddle::at, the cmul
                               of two inter_tw (4 entries, 3 products: 11.6) and tw_mul (2): 2 steps
  split / packing              half length: r2c pair_eval (S, D: 1; W = cmul of two entries: 4.8; cmul W D: 2; A: 1):
                               1 step; c2r herm + vpack (average 1, E 1, h0 - h1 1, W 4.8, cmulc 2, V 1 = 10.8):
                               2 steps, 1 for the Hermitian-input form (no average)
  fused product                pre_mul / xv: 1 step (a complex fma product 2 u, a real one 1 u)
  the "1 +"                    the subtraction of the means (1 u |data| per pass) and the final scaling (1 u, plus the
                               rounded 1/sqrt n: 1 u)
dcc, on the bins of the DC set only, relative to D = ||re-added means||_2: per centring pass the product mean * L and
  its addition to bin 0 (2), the final scaling (1): 3 (one pass), 5 (two passes); half-length forward 15 (the split's
  10 act on the column-0 bins and their mirror partners too); half-length inverse 5.

DC sets, read off the code per path (dc_kind):
  k_tiny, k_single                                      bin 0
  two-pass forward (fftbr, fwht; rows then columns)     k = 0 mod N2: the row pass re-adds N2 * mean(row u) at (u, 0),
                                                        column 0, and the column pass spreads column 0 over k1 N2
  two-pass adjoint (ifftbr; fwht with a fused factor:   i < N2: the column pass re-adds at row 0, (0, k2), whose
  columns then rows)                                    rounding the row pass of row 0 spreads over that row's outputs
  half-length forward                                   k = 0 mod 4096 (column 0 of the n/2-point transform and its
                                                        mirror partners n/2 - k, n - k, k + n/2: again multiples of 4096)
  half-length inverse                                   not separated (no large-DC case: dcc D on every bin)
A forward set holds n / N2 <= n / 2^9 bins (asserted: at most max(1, n / 2^8)).  The adjoint's set is row 0, n / N1
bins with N1 >= 16: it cannot meet n / 2^8 at any m (the design passes the re-added column means through the row
pass), so its cap is n / 2^4 and 15 / 16 of the outputs are held to the bound without a DC term.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

from tests import transform_reference as TR
from tests.transform_reference import LAT, NET, U32, U64

C_STAGE = {LAT: 10.0, NET: 2.0}
R2C = ("fftbr_real", "fftbr_real_half", "fftbr_real_half_f32")
C2R = ("ifftbr_real", "ifftbr_real_rf")
SINGLE = ("fftbr_c64", "ifftbr_c64", "fwht_f32")
ALL_BELOW = 18                    # up to this m every output is compared


def split_m2(m):
    return min(m - 4, 12)


def spec(entry, m, stable=1, fam=LAT, mul=False, single=False, f=None):
    """The derived constants of the kernel path an entry point takes at size m (module docstring)."""
    n = 1 << m
    net = entry in ("fwht", "fwht_f32") or (entry == "ifftbr_mul" and fam == NET)
    s = NS(entry=entry, m=m, n=n, net=net, c=C_STAGE[NET if net else LAT], stable=stable,
           u=U32 if (entry in SINGLE or single) else U64)
    if entry in R2C:
        s.m_eff, s.first, s.dc, s.dcc, s.stable = (m - 1) + 2 + 1, ("seg", 4096), ("mod", 4096), 15.0, 1
    elif entry in C2R:
        s.m_eff = (m - 1) + 2 + (1 if entry == "ifftbr_real_rf" else 2) + (1 if f else 0)
        s.first, s.dc, s.dcc, s.stable = None, ("all", 0), 5.0, 1
    else:
        two = m >= 13
        N2 = 1 << split_m2(m) if two else n
        s.m_eff = m + ((2 if N2 == 4096 else 1) if two and not net else 0) + (1 if mul else 0)
        cols_first = entry in ("ifftbr", "ifftbr_c64") or entry == "ifftbr_mul"
        if not stable:
            s.first, s.dc, s.dcc = None, ("none", 0), 0.0
        elif not two:
            s.first, s.dc, s.dcc = ("seg", n), ("zero", 0), 3.0
        elif cols_first:
            s.first, s.dc, s.dcc = ("col", N2), ("low", N2), 5.0
        else:
            s.first, s.dc, s.dcc = ("seg", N2), ("mod", N2), 5.0
    kind, L = s.dc
    s.dc_count = {"none": 0, "zero": 1, "mod": n // max(L, 1), "low": L, "all": n}[kind]
    return s


def dc_mask(s, idx):
    kind, L = s.dc
    idx = np.asarray(idx, dtype=np.int64)
    if kind == "none":
        return np.zeros(idx.shape, bool)
    if kind == "zero":
        return idx == 0
    if kind == "mod":
        return idx % L == 0
    if kind == "low":
        return idx < L
    return np.ones(idx.shape, bool)


def dc_cap(s):
    """The largest DC set a path may have (module docstring)."""
    return s.n // 16 if s.dc[0] == "low" else max(1, s.n >> 8)


def out_index(m, half=False, n_out=None):
    """The compared outputs: all up to m = 18; from m = 19 a fixed set of at most 2^16 -- the first and last 4096, the
    first 4096 multiples of N2, their mirror partners n/2 - k and n - k (half-length paths), 2^14 seeded random ones."""
    n = 1 << m
    n_out = n if n_out is None else n_out
    if m <= ALL_BELOW:
        return np.arange(n_out, dtype=np.int64)
    N2 = 1 << split_m2(m)
    col0 = np.arange(min(4096, n // N2), dtype=np.int64) * N2
    parts = [np.arange(4096), n - 1 - np.arange(4096), col0, np.random.default_rng(m).integers(0, n, 1 << 14)]
    if half:
        parts += [(n // 2 - col0) % n, (n - col0) % n, n // 2 + np.arange(-8, 9)]
    idx = np.unique(np.concatenate(parts).astype(np.int64))
    idx = idx[idx < n_out]
    assert idx.size <= 1 << 16
    return idx


# ------------------------------------------------------------------------------------------------ the case lists
def _case(table, entry, m, batch, **kw):
    kw.setdefault("stable", 1)
    kw.setdefault("pad", 0)
    c = NS(table=table, entry=entry, m=m, batch=batch, **kw)
    tag = "-".join("%s%s" % (k, v) for k, v in sorted(kw.items()) if k not in ("pad",) and v not in (None, False))
    c.name = "%s-%s-m%d-%s" % (table, entry, m, tag)
    return c


def _batch(m):
    return 3 if m <= 12 else 2


def dense_cases():
    out = []
    for m in list(range(0, 17)) + [17, 18]:
        for st in (0, 1):
            out += [_case("dense", "fftbr", m, _batch(m), stable=st, in_real=1, pad=8),
                    _case("dense", "fftbr", m, _batch(m), stable=st, in_real=0, pad=8),
                    _case("dense", "ifftbr", m, _batch(m), stable=st, out_real=0, pad=8),
                    _case("dense", "ifftbr", m, _batch(m), stable=st, out_real=1, pad=8),
                    _case("dense", "fwht", m, _batch(m), stable=st, pad=8)]
    return out


def half_cases():
    out = []
    for m in (17, 18):
        out += [_case("half", "fftbr_real", m, 2, pad=8), _case("half", "fftbr_real_half", m, 3, pad=2, opad=3),
                _case("half", "fftbr_real_half_f32", m, 2, pad=8, opad=0),
                _case("half", "ifftbr_real", m, 2, f=None, pad=4), _case("half", "ifftbr_real", m, 3, f="shared", pad=0),
                _case("half", "ifftbr_real", m, 2, f="per", pad=4),
                _case("half", "ifftbr_real_rf", m, 2, f="shared", rows="full", pad=0),
                _case("half", "ifftbr_real_rf", m, 3, f="per", rows="half", pad=2)]
    return out


def mul_cases():
    out = []
    for m in (3, 10, 13, 16):
        for fs in ("shared", "per"):
            out += [_case("mul", "ifftbr_mul", m, _batch(m), fam=LAT, f=fs, out_real=0),
                    _case("mul", "ifftbr_mul", m, _batch(m), fam=LAT, f=fs, out_real=1),
                    _case("mul", "ifftbr_mul", m, _batch(m), fam=NET, f=fs)]
    return out


def single_cases():
    out = []
    for m in (2, 10, 13, 16):
        out += [_case("single", "fftbr_c64", m, _batch(m), in_real=1, pad=4), _case("single", "fftbr_c64", m, _batch(m), in_real=0),
                _case("single", "ifftbr_c64", m, _batch(m), out_real=0), _case("single", "ifftbr_c64", m, _batch(m), out_real=1),
                _case("single", "fwht_f32", m, _batch(m), pad=4),
                _case("single", "ifftbr_mul", m, _batch(m), fam=LAT, f="per", out_real=1, single=1),
                _case("single", "ifftbr_mul", m, _batch(m), fam=NET, f="shared", single=1)]
    return out


def dc_cases():
    out = []
    for m in (3, 10, 13, 17):
        out += [_case("dc", "fftbr", m, 2, in_real=1, dc=1), _case("dc", "ifftbr", m, 2, out_real=0, dc=1),
                _case("dc", "fwht", m, 2, dc=1)]
    return out + [_case("dc", "fftbr_real", 17, 2, dc=1)]


def sparse_cases():
    """Which case reaches which instance: fgp_fftbr / fgp_ifftbr / fgp_fwht at m reach k_tiny<m> (m <= 3),
    k_single<m> (4..12), k_rows<min(m - 4, 12)> + k_cols<m - min(m - 4, 12)> (13..24: k_rows<9..12> at m = 13..16,
    k_cols<4> at 13..16 and k_cols<5..12> at m = 17..24) and twm[m]; the half-length entries at m reach
    k_fwd_rows_r2c_in<double | float>, k_fwd_cols_r2c<m - 13, 1> (fftbr_real) and <m - 13, 3> (fftbr_real_half),
    k_inv_cols_c2r<m - 13, false, false> (ifftbr_real), <m - 13, true, true> (ifftbr_real_rf), k_inv_rows_c2r, and
    the tables twm[m] (split twiddle) and twm[m - 1] (row twiddle)."""
    out = []
    for m in range(0, 25):
        b = 4 if m <= 20 else 1
        out += [_case("sparse", "fftbr", m, b, in_real=1), _case("sparse", "fftbr", m, b, in_real=0),
                _case("sparse", "ifftbr", m, b, out_real=0), _case("sparse", "ifftbr", m, b, out_real=1),
                _case("sparse", "fwht", m, b),
                _case("sparse", "ifftbr_mul", m, b, fam=LAT, f="shared", out_real=0),
                _case("sparse", "ifftbr_mul", m, b, fam=NET, f="shared")]
    for m in range(17, 25):
        b = 4 if m <= 20 else 1
        out += [_case("sparse", "fftbr_real", m, b), _case("sparse", "fftbr_real_half", m, b, opad=1),
                _case("sparse", "ifftbr_real", m, b, f=None), _case("sparse", "ifftbr_real", m, b, f="shared"),
                _case("sparse", "ifftbr_real_rf", m, b, f="shared", rows="half")]
    for m in (13, 17, 20):
        out += [_case("sparse", "fftbr_c64", m, 4, in_real=0), _case("sparse", "ifftbr_c64", m, 4, out_real=0),
                _case("sparse", "fwht_f32", m, 4),
                _case("sparse", "ifftbr_mul", m, 4, fam=LAT, f="shared", out_real=0, single=1)]
        if m >= 17:
            out.append(_case("sparse", "fftbr_real_half_f32", m, 4, opad=0))
    return out


def alias_cases():
    return [_case("alias", e, m, 2, **kw) for m in (10, 13, 17) for e, kw in (("fftbr", dict(in_real=0)), ("fwht", {}))]


TABLES = {"dense": dense_cases, "half": half_cases, "mul": mul_cases, "single": single_cases, "dc": dc_cases,
          "sparse": sparse_cases, "alias": alias_cases}


@functools.lru_cache(maxsize=None)
def cases(table):
    return tuple(TABLES[table]())


@functools.lru_cache(maxsize=None)
def by_name():
    allc = [c for t in TABLES for c in cases(t)]
    d = {c.name: c for c in allc}
    assert len(d) == len(allc), "case names must be unique"
    return d


def case_spec(c):
    return spec(c.entry, c.m, stable=c.stable, fam=getattr(c, "fam", LAT), mul=c.entry == "ifftbr_mul",
                single=getattr(c, "single", 0), f=getattr(c, "f", None))


# ------------------------------------------------------------------------------------------------ inputs
def _is_net(c):
    return c.entry in ("fwht", "fwht_f32") or getattr(c, "fam", LAT) == NET


def _real_in(c):
    return _is_net(c) or c.entry in R2C or getattr(c, "in_real", 0)


def _single(c):
    return c.entry in SINGLE or getattr(c, "single", 0) or c.entry == "fftbr_real_half_f32"


def factor_row(k, n, cx, even=False):
    """The shared factor row of the sparse cases, small dyadic values about 1 that any side can regenerate exactly."""
    k = np.asarray(k, dtype=np.int64)
    if even:
        k = np.minimum(k, n - k)
    f = 0.75 + (k % 7) / 8.0
    return f + 1j * ((k % 5) - 2) / 16.0 if cx else f


def _seed(c):
    return int.from_bytes(c.name.encode(), "little") % (2 ** 32)


@functools.lru_cache(maxsize=8)
def _dense_inputs(name):
    c = by_name()[name]
    n = 1 << c.m
    g = np.random.default_rng(_seed(NS(name="%s-%d-%d" % (c.entry, c.m, bool(_real_in(c))))))   # shared by stable 0 / 1
    cx = not _real_in(c)
    stride = n + c.pad
    dc = 65536.0 if getattr(c, "dc", 0) else 0.0
    if c.entry == "ifftbr_real_rf":                       # Hermitian rows: the transform of real data
        h = g.standard_normal((c.batch, n // 2 + 1)) + 1j * g.standard_normal((c.batch, n // 2 + 1))
        h[:, 0], h[:, -1] = h[:, 0].real, h[:, -1].real
        full = TR.hermitian_full(h, n)
        if c.rows == "half":
            x = np.zeros((c.batch, n // 2 + 1 + c.pad), np.complex128)
            x[:, :n // 2 + 1] = h
        else:
            x = full
        fr = g.uniform(0.5, 1.5, (1 if c.f == "shared" else c.batch, n // 2 + 1))
        f = np.concatenate([fr, fr[:, 1:n // 2][:, ::-1]], -1)       # even
        return dict(x=x, f=f, logical=full)
    x = np.zeros((c.batch, stride), np.complex128 if cx else np.float64)
    x[:, :n] = g.standard_normal((c.batch, n)) + dc
    if cx:
        x[:, :n] += 1j * g.standard_normal((c.batch, n))
    f = None
    if getattr(c, "f", None):
        rows = 1 if c.f == "shared" else c.batch
        f = g.uniform(0.5, 1.5, (rows, n)) + (0.25j * g.standard_normal((rows, n)) if cx else 0)
    if _single(c):
        x = x.astype(np.complex64 if cx else np.float32)
        f = None if f is None else f.astype(np.complex64 if cx else np.float32)
    return dict(x=x, f=f, logical=x[:, :n])          # (views of the arrays as cast: the kernel's very inputs)


def sparse_rows(c):
    """[(positions int64 [s], values [s])] per batch row: the structured positions {0, 1, N2 - 1, N2, n/2, n - 1}, a single
    bit in each half of the split, seeded random ones; values of magnitude 1..3, the second negative; fp32 cases:
    values that are floats, so that the comparison is of the fp32 twiddle path, not of an input rounding."""
    m, n = c.m, 1 << c.m
    m2 = split_m2(m) if m >= 13 else max(m // 2, 0)
    if c.entry in R2C + C2R:
        m2 = 12
    N2 = 1 << m2
    g = np.random.default_rng(_seed(c))
    rnd = [int(v) for v in g.integers(0, n, 32)]
    bits = [1 << (m2 // 2), 1 << max(m2 - 1, 0), 1 << (m2 + (m - m2) // 2), 1 << max(m - 1, 0)]
    struct = [0, 1, N2 - 1, N2, n // 2, n - 1]
    plan = {1: [N2, n - 1], 2: [1, n - 1, 0], 4: [0, N2 - 1, n // 2, bits[2], 1], 16: struct + bits}
    cx = not _real_in(c)
    rows = []
    for s in ((1, 2, 4, 16) if c.batch == 4 else (16,)):
        if c.entry == "ifftbr_real_rf":                  # conjugate pairs (k, n - k), k = 0 and k = n/2
            cand = [0, n // 2, 1, N2, N2 - 1, n // 4] + [v % (n // 2) for v in bits + rnd]
            start = {1: 0, 2: 2, 4: 1, 16: 0}[s]
            cand = cand[start:] + cand[:start]
            ks = list(dict.fromkeys(k for k in cand if 0 <= k <= n // 2))[:max(1, s // 2)]
            val = g.uniform(1, 3, len(ks)) + 1j * g.uniform(-1, 1, len(ks))
            val = np.where(np.isin(ks, (0, n // 2)), val.real, val)      # the self-mirrored bins are real
            val[min(1, len(ks) - 1)] *= -1
            rows.append((np.array(ks, np.int64), val))
            continue
        pos = list(dict.fromkeys(p for p in plan[s] + rnd if 0 <= p < n))[:s]
        val = g.uniform(1, 3, len(pos))
        if cx:
            val = val + 1j * g.uniform(-1, 1, len(pos))
        val[min(1, len(pos) - 1)] *= -1
        if _single(c):
            val = val.astype(np.complex64 if cx else np.float32).astype(np.complex128 if cx else np.float64)
        rows.append((np.array(pos, np.int64), val))
    return rows


def rf_full(pos, val, n):
    """The Hermitian completion (positions, values) of half-row non-zeros at k <= n/2."""
    mk = (pos > 0) & (pos < n // 2)
    return np.concatenate([pos, n - pos[mk]]), np.concatenate([val, np.conj(val[mk])])


def sparse_dense(c, rows, n_cols=None):
    """The dense input array of a sparse case (tests up to moderate m; the GPU test builds it on the device)."""
    n = 1 << c.m
    cx = not _real_in(c)
    x = np.zeros((len(rows), n if n_cols is None else n_cols), np.complex128 if cx else np.float64)
    for r, (p, v) in enumerate(rows):
        x[r, p] = v
    return x


# ------------------------------------------------------------------------------------------------ expectations
def _inverse(c):
    return c.entry in ("ifftbr", "ifftbr_c64", "ifftbr_mul") + C2R and not _is_net(c)


def _real_out(c):
    return _is_net(c) or c.entry in C2R or getattr(c, "out_real", 0)


def n_out(c):
    return (1 << c.m) // 2 + 1 if c.entry in ("fftbr_real_half", "fftbr_real_half_f32") else 1 << c.m


@functools.lru_cache(maxsize=8)
def _dense_reference(entry_kind, key_name):
    c = by_name()[key_name]
    inp = _dense_inputs(key_name)
    x = inp["logical"]
    f = inp["f"]
    pr, pi_ = TR.product(x, f) if f is not None else TR.widen(x)
    pi0 = pr * 0 if pi_ is None else pi_
    if _is_net(c):
        ref = (TR.transform(NET, pr, pr * 0)[0], None)
    else:
        ref = TR.transform(LAT, pr, pi0, adjoint=_inverse(c))
    return ref, (pr, pi0)


def dense_expected(name):
    """(ref_re, ref_im or None, out_idx, data_norm [batch], D [batch], xnorm [batch]) of a dense case."""
    c = by_name()[name]
    s = case_spec(c)
    key = [k for k in by_name() if _dense_key(by_name()[k]) == _dense_key(c)][0]
    (re, im), (pr, pi0) = _dense_reference(_dense_key(c), key)
    dn, D = TR.dense_brackets(pr, pi0, s.first)
    if s.dc[0] == "all":
        D = TR.norm2(pr, pi0)
    no = n_out(c)
    if _real_out(c):
        im = None
    return re[:, :no], None if im is None else im[:, :no], np.arange(no), dn, D, TR.norm2(pr, pi0)


def _dense_key(c):
    """Cases that share their input and reference (the stable flag, the real-output flag and the half spectrum do not
    change the operation)."""
    d = dict(vars(c))
    for k in ("name", "stable", "out_real", "opad"):
        d.pop(k, None)
    return tuple(sorted((k, str(v)) for k, v in d.items()))


def sparse_expected(c, rows):
    """(ref_re, ref_im or None [batch, n_idx], out_idx, B [batch], xnorm2 [batch]) by the closed form."""
    m, n = c.m, 1 << c.m
    idx = out_index(m, half=c.entry in R2C + C2R, n_out=n_out(c))
    cx_f = getattr(c, "f", None)
    RE, IM, B, X2 = [], [], [], []
    for pos, val in rows:
        if c.entry == "ifftbr_real_rf":
            pos, val = rf_full(pos, val, n)
        if cx_f:
            val = val * factor_row(pos, n, cx=not _is_net(c) and c.entry != "ifftbr_real_rf", even=c.entry == "ifftbr_real_rf")
        if _is_net(c):
            re, im = TR.sparse_fwht(pos, val, m, idx), None
        elif _inverse(c):
            re, im = TR.sparse_ifftbr(pos, val, m, idx)
        else:
            re, im = TR.sparse_fftbr(pos, val, m, idx)
        RE.append(re)
        IM.append(im)
        B.append(float(np.abs(val).sum()) / np.sqrt(n))
        X2.append(float(np.sqrt((np.abs(val) ** 2).sum())))
    im = None if (_real_out(c) or IM[0] is None) else np.stack(IM)
    return np.stack(RE), im, idx, np.array(B), np.array(X2)


# ------------------------------------------------------------------------------------------------ comparison
def _err(dev, re, im):
    dev = np.asarray(dev)
    er = TR._x(dev.real.astype(np.float64)) - re
    if im is None:
        return abs(er), er * er
    ei = TR._x(dev.imag.astype(np.float64)) - im
    e2 = er * er + ei * ei
    return TR._sqrt(e2), e2


def _ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 (an exact result against a zero bound) and x / 0 = inf."""
    err, bound = TR.to_f64(err), TR.to_f64(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def check_dense(c, dev, expected=None):
    """Worst ratio error / (u bound / c) of a dense case's device output dev [batch, n_out]; asserts the caps.  The
    caller asserts ratio <= c.  Returns (ratio over all bins, ratio over the bins outside the DC set, c)."""
    s = case_spec(c)
    re, im, idx, dn, D, xn = dense_expected(c.name) if expected is None else expected
    assert np.asarray(dev).shape == re.shape, (np.asarray(dev).shape, re.shape)
    assert np.isfinite(np.asarray(dev)).all(), (c.name, "not finite")
    _, e2 = _err(dev, re, im)
    mask = dc_mask(s, idx)
    assert s.dc[0] in ("none", "all") or mask.sum() <= dc_cap(s), (c.name, "DC set", int(mask.sum()))
    steps = 1 + s.m_eff
    br_all = steps * dn + (s.dcc / s.c) * D
    assert (TR.to_f64(s.c * br_all) <= 1e5 * TR.to_f64(xn)).all(), (c.name, "cap")
    r_all = _ratio(TR._sqrt(e2.sum(-1)), s.u * br_all)
    off = e2[:, ~mask].sum(-1) if (~mask).any() else e2.sum(-1) * 0
    r_off = _ratio(TR._sqrt(off), s.u * steps * dn)
    return r_all, r_off, s.c


def sparse_caps(c, rows, idx=None):
    """The sparse cap, c (1 + m_eff + dcc / c) B <= 1e5 ||x||_2 / sqrt n, on the case's own arrays (the DC term taken
    on every output when idx is None)."""
    s = case_spec(c)
    n = s.n
    for pos, val in rows:
        if c.entry == "ifftbr_real_rf":
            pos, val = rf_full(pos, val, n)
        if getattr(c, "f", None):
            val = val * factor_row(pos, n, cx=not _is_net(c) and c.entry != "ifftbr_real_rf", even=c.entry == "ifftbr_real_rf")
        B = (1 + s.stable) * float(np.abs(val).sum()) / np.sqrt(n)
        assert s.c * ((1 + s.m_eff) + s.dcc / s.c) * B <= 1e5 * float(np.sqrt((np.abs(val) ** 2).sum())) / np.sqrt(n), c.name


def check_sparse(c, dev, expected):
    """Worst per-output ratio of a sparse case's device values dev [batch, n_idx] at the compared outputs."""
    s = case_spec(c)
    re, im, idx, B, x2 = expected
    assert np.asarray(dev).shape == re.shape, (np.asarray(dev).shape, re.shape)
    assert np.isfinite(np.asarray(dev)).all(), (c.name, "not finite")
    e, _ = _err(dev, re, im)
    steps = (1 + s.m_eff) + (s.dcc / s.c) * dc_mask(s, idx)
    Bk = (1 + s.stable) * B[:, None] * steps[None, :]
    assert (s.c * Bk <= 1e5 * x2[:, None] / np.sqrt(s.n)).all(), (c.name, "cap")
    return _ratio(e, s.u * TR._x(Bk)), s.c


# ------------------------------------------------------------------------------------------------ element-wise
C_DOUBLE = {LAT: 10.0, NET: 4.0}
# k_double_cx: sincospi (1 ulp = 2 u per component: 2.9 on w), the product in plain operations (2 per component:
# 2.9), the addition (1), the rounded 1/sqrt 2 and its product (2): 8.8 -> 10, of (|prev| + |nxt|) / sqrt 2;
# k_double_re: addition, constant, product: 3 -> 4.
DOUBLE_CASES = [(fam, m) for fam in (LAT, NET) for m in (0, 1, 7, 13)]
SUMSQ_CASES = [(kind, G) for kind in range(4) for G in (1, 2, 3)]
SUMSQ_R, SUMSQ_N = 3, 777


def c_sum_sq(R, cx):
    """k_sum_sq: per term the square (1), the sum of the two squares (complex: 1), R accumulations."""
    return R + 1 + (1 if cx else 0)


def double_inputs(fam, m):
    g = np.random.default_rng(1000 + 10 * m + fam)
    n = 1 << m
    mk = (lambda: g.standard_normal((3, n + 3)) + 1j * g.standard_normal((3, n + 3))) if fam == LAT else \
        (lambda: g.standard_normal((3, n + 3)))
    return mk(), mk()


def sumsq_inputs(kind, G, n=SUMSQ_N, R=SUMSQ_R):
    g = np.random.default_rng(50 + kind * 4 + G)
    x = g.standard_normal((R * G, n + 5))
    if kind in (1, 3):
        x = x + 1j * g.standard_normal((R * G, n + 5))
    return x.astype({0: np.float64, 1: np.complex128, 2: np.float32, 3: np.complex64}[kind])
