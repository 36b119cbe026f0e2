"""The transform reference (tests/transform_reference.py) and the bounds of tests/transform_cases.py, without a device.

  * the reference itself: network against closed form on sparse rows (m = 0..20), against oracle.fgp_oracle at the
    fp64 level, Parseval and adjointness in 80-bit, the half-spectrum mirror, predict_reference.ft unchanged in value;
  * every cap of every case;
  * the bounds are not too tight: a plain radix-2 network in numpy (fp64; fp32 for the single-precision cases) and the
    library FFT behind oracle.fgp_oracle meet every dense and sparse bound of every case up to m = 18;
  * the bounds are not too loose: one twiddle scaled by 1 + 2^-40, one butterfly with its sign flipped and the
    uncentred transform of the large-DC input each exceed them.
"""
import numpy as np
import pytest
import torch

from oracle import fgp_oracle as O
from tests import predict_reference as PR
from tests import transform_cases as TC
from tests import transform_reference as TR
from tests.transform_reference import LAT, NET

EPS_X = 2.0 ** -64 if not PR.MP else 1e-38
MAX_M = 18


# ------------------------------------------------------------------------------------------------ fp models
def np_network(net, x, adjoint=False, dtype=np.float64, tw_fault=None, flip=None):
    """A plain radix-2 network in numpy arithmetic of `dtype` (twiddles from fp64 cos / sin, rounded to it).  tw_fault
    = (h, j): that twiddle of the stage of half-span h scaled by 1 + 2^-40; flip = (h, block, j): that butterfly's
    difference output negated."""
    cd = {np.float64: np.complex128, np.float32: np.complex64}[dtype]
    y = np.asarray(x).astype(dtype if net else cd)
    Rn, n = y.shape
    m = n.bit_length() - 1
    hs = [1 << s for s in range(m)]
    for h in (hs[::-1] if adjoint else hs):
        w = np.exp(-1j * np.pi * np.arange(h) / h)
        if tw_fault and tw_fault[0] == h:
            w[tw_fault[1]] *= 1 + 2.0 ** -40
        w = w.astype(cd)
        y = y.reshape(Rn, n // (2 * h), 2, h)
        a, b = y[:, :, 0, :], y[:, :, 1, :]
        if net:
            new = np.stack([a + b, a - b], 2)
        elif not adjoint:
            t = b * w
            new = np.stack([a + t, a - t], 2)
        else:
            new = np.stack([a + b, (a - b) * np.conj(w)], 2)
        if flip and flip[0] == h:
            new[:, flip[1], 1, flip[2]] *= -1
        y = new.reshape(Rn, n)
    return y * dtype(1.0 / np.sqrt(n))


def _stable(x, fn):
    """AbstractFastGP.ft's wrapper: centre the whole row, transform, re-add the mean to bin 0."""
    mean = x.mean(-1, dtype=x.dtype)
    y = fn(x - mean[:, None])
    y[:, 0] += mean * x.real.dtype.type(np.sqrt(x.shape[-1]))
    return y


def _finish(c, y):
    y = y[:, :TC.n_out(c)]
    return y.real if (TC._real_out(c) and np.iscomplexobj(y)) else y


def model(c, x, f=None, unstable=False, library=False, **fault):
    """The operation of case c on the logical rows x (and factor rows f) in floating point."""
    dt = np.float32 if TC._single(c) and c.entry != "fftbr_real_half_f32" else np.float64
    x = np.asarray(x)
    if f is not None:
        x = x * np.asarray(f)
    net, adj = TC._is_net(c), TC._inverse(c)
    if library:
        xt = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64 if net or not np.iscomplexobj(x) else np.complex128)))
        op = O.fwht if net else (O.ifftbr if adj else O.fftbr)
        if not net and not xt.is_complex():
            xt = xt.to(torch.complex128)
        return _finish(c, (op(xt) if unstable else O.ft_stable(xt, op)).numpy())
    x = x.astype(dt if not np.iscomplexobj(x) else {np.float64: np.complex128, np.float32: np.complex64}[dt])
    fn = lambda v: np_network(net, v, adjoint=adj, dtype=dt, **fault)      # noqa: E731
    if not net and not np.iscomplexobj(x):
        x = x.astype({np.float64: np.complex128, np.float32: np.complex64}[dt])
    return _finish(c, fn(x) if unstable else _stable(x, fn))


def _sparse_logical(c, rows):
    """(x [batch, n], f or None) of a sparse case as full logical rows."""
    n = 1 << c.m
    if c.entry == "ifftbr_real_rf":
        rows = [TC.rf_full(p, v, n) for p, v in rows]
    x = TC.sparse_dense(c, rows)
    f = None
    if getattr(c, "f", None):
        rf = c.entry == "ifftbr_real_rf"
        f = TC.factor_row(np.arange(n), n, cx=not TC._is_net(c) and not rf, even=rf)[None, :]
    return x, f


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("m", list(range(0, 21)))
def test_network_agrees_with_closed_form_on_sparse_rows(m):
    """Two independent evaluations in 80-bit: agreement to 10 (1 + m) roundings of the extended format on ||x||_1 /
    sqrt n (measured: 0.006 2^-53 ||x||_1 / sqrt n at m = 13..20)."""
    n = 1 << m
    c = TC._case("sparse", "fftbr", m, 1, in_real=0)
    pos, val = TC.sparse_rows(c)[0]
    x = np.zeros((1, n), np.complex128)
    x[0, pos] = val
    idx = np.arange(n) if m <= 14 else TC.out_index(19)[TC.out_index(19) < n]
    tol = 10 * (1 + m) * EPS_X * float(np.abs(val).sum()) / np.sqrt(n)
    for net_fn, closed in ((TR.fftbr, TR.sparse_fftbr), (TR.ifftbr, TR.sparse_ifftbr)):
        re, im = net_fn(x)
        cr, ci = closed(pos, val, m, idx)
        assert float(abs(re[0, idx] - cr).max()) <= tol and float(abs(im[0, idx] - ci).max()) <= tol
    w = TR.fwht(x.real)
    assert float(abs(w[0, idx] - TR.sparse_fwht(pos, val.real, m, idx)).max()) <= tol


@pytest.mark.parametrize("m", [0, 1, 2, 5, 9, 13])
def test_reference_agrees_with_the_oracle_at_fp64_level(m):
    n = 1 << m
    g = np.random.default_rng(m)
    x = g.standard_normal((2, n)) + 1j * g.standard_normal((2, n)) + 0.5
    xt = torch.from_numpy(x)
    tol = 10 * (1 + m) * 2.0 ** -53 * np.sqrt((np.abs(x) ** 2).sum(-1)).max() + 1e-300
    for ref, orc in ((TR.fftbr(x), O.fftbr(xt)), (TR.ifftbr(x), O.ifftbr(xt)), (TR.fftbr(x), O.ft_stable(xt, O.fftbr)),
                     (TR.ifftbr(x), O.ft_stable(xt, O.ifftbr)), (TR.fftbr(x.real), O.fftbr(xt.real.to(torch.complex128)))):
        d = (TR.to_f64(ref[0]) + 1j * TR.to_f64(ref[1])) - orc.numpy()
        assert np.sqrt((np.abs(d) ** 2).sum(-1)).max() <= tol
    for orc in (O.fwht(xt.real.contiguous()), O.ft_stable(xt.real.contiguous(), O.fwht)):
        d = TR.to_f64(TR.fwht(x.real)) - orc.numpy()
        assert np.sqrt((d ** 2).sum(-1)).max() <= tol


@pytest.mark.parametrize("m", [0, 3, 10])
def test_parseval_and_adjointness_in_extended_precision(m):
    n = 1 << m
    g = np.random.default_rng(70 + m)
    x = g.standard_normal((1, n)) + 1j * g.standard_normal((1, n))
    y = g.standard_normal((1, n)) + 1j * g.standard_normal((1, n))
    tol = 10 * (1 + m) * EPS_X * float(np.sqrt((np.abs(x) ** 2).sum() * (np.abs(y) ** 2).sum()))
    ar, ai = TR.fftbr(x)
    hr, hi = TR.ifftbr(y)
    xr, xi = TR.widen(x)
    yr, yi = TR.widen(y)
    assert float(abs((ar * ar + ai * ai).sum() - (xr * xr + xi * xi).sum())) <= tol * 4
    # <A x, y> = <x, A^H y>, <u, v> = sum u conj v
    lhs = ((ar * yr + ai * yi).sum(), (ai * yr - ar * yi).sum())
    rhs = ((xr * hr + xi * hi).sum(), (xi * hr - xr * hi).sum())
    assert float(abs(lhs[0] - rhs[0])) <= tol and float(abs(lhs[1] - rhs[1])) <= tol
    w = TR.fwht(x.real)
    assert float(abs((w * w).sum() - (xr * xr).sum())) <= tol * 4
    assert float(abs((w * yr).sum() - (xr * TR.fwht(y.real)).sum())) <= tol
    br, bi = TR.ifftbr(TR.to_f64(ar) + 1j * TR.to_f64(ai))                      # round trip at the fp64 rounding of A x
    assert float(abs(br - xr).max()) <= 4 * 2.0 ** -53 * float(np.abs(x).max()) * np.sqrt(n)


def test_half_spectrum_mirror_and_sum_sq():
    n = 64
    g = np.random.default_rng(5)
    x = g.standard_normal((4, n))
    re, im = TR.fftbr(x)
    k = np.arange(1, n)
    tol = 10 * 7 * EPS_X * 8
    assert float(abs(re[:, n - k] - re[:, k]).max()) <= tol and float(abs(im[:, n - k] + im[:, k]).max()) <= tol
    spec = TR.to_f64(re) + 1j * TR.to_f64(im)
    half = spec[:, :n // 2 + 1].copy()
    half[:, 0], half[:, -1] = half[:, 0].real, half[:, -1].real
    full = TR.hermitian_full(half, n)
    assert np.abs(full - spec).max() <= 1e-14
    for G in (1, 2):
        assert np.array_equal(TR.sum_sq_half(half, n, G), TR.sum_sq(full, G))
    pr, pi_ = TR.product(full, x[:1])
    assert np.array_equal(TR.to_f64(pr), full.real * x[:1]) and np.array_equal(TR.to_f64(pi_), full.imag * x[:1])


@pytest.mark.parametrize("m", [0, 1, 6, 12])
def test_predict_reference_ft_is_unchanged_in_value(m):
    rows = PR._x(np.random.default_rng(m).standard_normal((2, 1 << m)) + 0.25)
    for fam in (LAT, NET):
        for a, b in zip(TR.ft(fam, rows), PR.ft(fam, rows)):
            assert np.array_equal(a, b)


def test_double_update_reference_is_the_transform_of_both_halves():
    g = np.random.default_rng(11)
    n = 64
    x = g.standard_normal((2, 2 * n))
    for fam, ftf in ((LAT, TR.fftbr), (NET, lambda v: (TR.fwht(v), None))):
        cat = lambda t: TR.to_f64(t[0]) + (0 if t[1] is None else 1j * TR.to_f64(t[1]))      # noqa: E731
        re, im, B = TR.double_update(fam, cat(ftf(x[:, :n])), cat(ftf(x[:, n:])))
        fr, fi = ftf(x)
        assert float(abs(re - fr).max()) <= 1e-14 and (fi is None or float(abs(im - fi).max()) <= 1e-14)
        assert (TR.to_f64(B) > 0).all()


# ------------------------------------------------------------------------------------------------ caps, not too tight
def test_every_case_reaches_its_instance_and_table():
    ms = lambda e: {c.m for c in TC.cases("sparse") if c.entry == e}                          # noqa: E731
    for e in ("fftbr", "ifftbr", "fwht", "ifftbr_mul"):
        assert ms(e) == set(range(0, 25))                    # k_tiny<0..3>, k_single<4..12>, k_rows / k_cols, twm[13..24]
    for e in ("fftbr_real", "fftbr_real_half", "ifftbr_real", "ifftbr_real_rf"):
        assert ms(e) == set(range(17, 25))                   # PP = m - 13 = 4..11
    assert {m - TC.split_m2(m) for m in range(16, 25)} == set(range(4, 13))          # k_cols<4..12>
    assert {TC.split_m2(m) for m in range(13, 17)} == {9, 10, 11, 12}                # k_rows<9..12>
    for c in TC.by_name().values():
        s = TC.case_spec(c)
        assert s.dc[0] in ("none", "all") or s.dc_count <= TC.dc_cap(s), c.name


@pytest.mark.parametrize("name", [c.name for c in TC.cases("sparse") if c.m > MAX_M])
def test_caps_of_the_large_sparse_cases(name):
    c = TC.by_name()[name]
    TC.sparse_caps(c, TC.sparse_rows(c))
    assert TC.out_index(c.m, half=True, n_out=TC.n_out(c)).size <= 1 << 16


DENSE_TABLES = ("dense", "half", "mul", "single", "dc", "alias")


@pytest.mark.parametrize("name", [c.name for t in DENSE_TABLES for c in TC.cases(t)])
def test_floating_point_models_meet_the_dense_bounds(name):
    c = TC.by_name()[name]
    inp = TC._dense_inputs(name)
    exp = TC.dense_expected(name)
    for library in ((False, True) if not TC._single(c) else (False,)):
        r_all, r_off, C = TC.check_dense(c, model(c, inp["logical"], inp["f"], library=library), exp)
        assert r_all <= C and r_off <= C, (name, library, r_all, r_off, C)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("sparse") if c.m <= MAX_M])
def test_floating_point_models_meet_the_sparse_bounds(name):
    c = TC.by_name()[name]
    rows = TC.sparse_rows(c)
    exp = TC.sparse_expected(c, rows)
    x, f = _sparse_logical(c, rows)
    for library in ((False, True) if not TC._single(c) else (False,)):
        dev = model(c, x, f, unstable=not c.stable, library=library)[:, exp[2]]
        r, C = TC.check_sparse(c, dev, exp)
        assert r <= C, (name, library, r, C)


# ------------------------------------------------------------------------------------------------ not too loose
def test_a_twiddle_off_in_its_40th_bit_exceeds_the_sparse_bound():
    c = TC.by_name()["sparse-fftbr-m13-stable1"]
    rows = TC.sparse_rows(c)
    exp = TC.sparse_expected(c, rows)
    x, _ = _sparse_logical(c, rows)
    n = 1 << c.m
    assert any((p >= n // 2).any() for p, _ in rows)              # an input on the faulty butterfly's b branch
    good, C = TC.check_sparse(c, model(c, x), exp)
    bad, _ = TC.check_sparse(c, model(c, x, tw_fault=(n // 2, 1)), exp)
    assert good <= C < bad, (good, bad, C)


def test_a_flipped_butterfly_exceeds_the_dense_bound():
    name = "dense-fftbr-m13-stable1"
    c = TC.by_name()[name]
    inp = TC._dense_inputs(name)
    r_all, r_off, C = TC.check_dense(c, model(c, inp["logical"], flip=(16, 3, 5)))
    assert r_all > 1e6 * C and r_off > 1e6 * C


@pytest.mark.parametrize("name", [c.name for c in TC.cases("dc") if c.m >= 10])
def test_the_uncentred_transform_of_a_large_dc_exceeds_the_off_dc_bound(name):
    """What `stable` is for: without the centring the DC's roundings spread over every bin (about 2.7 roundings of
    2^16 sqrt n in the 2-norm against c (1 + m_eff) sqrt n: some 10^3 times the bound for lattices)."""
    c = TC.by_name()[name]
    inp = TC._dense_inputs(name)
    exp = TC.dense_expected(name)
    ok_all, ok_off, C = TC.check_dense(c, model(c, inp["logical"]), exp)
    bad_all, bad_off, _ = TC.check_dense(c, model(c, inp["logical"], unstable=True), exp)
    assert ok_all <= C and ok_off <= C
    assert bad_off >= 10 * C, (name, bad_off, C)
