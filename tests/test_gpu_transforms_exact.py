"""The transforms against the extended-precision reference (tests/transform_reference.py).

Every entry point of the transform family is called directly (_native.call) on the cases of tests/transform_cases.py,
so that each case reaches the kernel instance it names, and compared with the operation's definition evaluated in
80-bit arithmetic from the very arrays the kernel read:

  dense rows    || device - ref ||_2 <= u (c (1 + m_eff) ||data||_2 + dcc D) per row, and on the bins outside the path's
                DC set <= u c (1 + m_eff) ||data||_2 alone (what `stable` is for: a pass that skipped its centring
                fails there on the large-DC inputs);
  sparse rows   | device - ref |_k <= u (c (1 + m_eff) + dcc [k in DC set]) B per compared output, the reference by
                the closed form (every output up to m = 18, a fixed set of at most 2^16 from m = 19);
  element-wise  | device - ref | <= C u sum |terms| per element.

u = 2^-53 (2^-24 for the float / float2 instances); c, m_eff, dcc and the DC sets are derived in
tests/transform_cases.py from the kernels' roundings, none is taken from device output.  The printed figure (-s) is
ratio = error / (u bound / c), asserted <= c; the worst per variant is tabulated in DESIGN.md section 3.1.  Every call
is made twice and must repeat bit for bit; outputs must be finite; the caps that keep the bounds from being vacuous are
asserted on the arrays used.
"""
import numpy as np
import pytest
import torch

from fastgaussianprocesses_amd import _native as N
from tests import transform_cases as TC
from tests import transform_reference as TR
from tests.gpu_fixtures import DEV
from tests.transform_reference import LAT, NET

pytestmark = pytest.mark.gpu
WORST = {}          # variant -> (worst ratio, c)

_CDT = {False: torch.complex128, True: torch.complex64}
_RDT = {False: torch.float64, True: torch.float32}


def _stream():
    return N.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _path(c):
    if c.entry in TC.R2C + TC.C2R:
        return "half length"
    return "k_tiny" if c.m <= 3 else ("k_single" if c.m <= 12 else "two-pass")


def _variant(c):
    bits = [c.table, c.entry]
    if getattr(c, "single", 0):
        bits.append("single")
    if getattr(c, "fam", LAT) == NET:
        bits.append("net")
    return " ".join(bits) + " [" + _path(c) + "]"


def _note(c, what, ratio, C):
    w = WORST.get(_variant(c), (0.0, C))
    WORST[_variant(c)] = (max(w[0], ratio), C)
    print("%-62s %-8s ratio = %7.3f   c = %g" % (c.name, what, ratio, C))


def launch(c, x, f=None, out=None):
    """One call of case c's entry point on device rows x [batch, stride] (and factor rows f): the output tensor
    [batch, >= n_out].  out: write there instead of a fresh NaN-filled buffer (the aliasing cases)."""
    m, n, b = c.m, 1 << c.m, x.size(0)
    e = c.entry
    single = bool(TC._single(c)) and e != "fftbr_real_half_f32"
    cdt, rdt = _CDT[single], _RDT[single]
    st = _stream()
    stride = x.stride(0)
    fs = 0 if (f is None or f.size(0) == 1) else f.stride(0)
    if e in ("fftbr", "fftbr_c64"):
        out = _nan((b, n), cdt) if out is None else out
        N.call("fgp_" + e, N.ptr(x), stride, int(not x.is_complex()), N.ptr(out), b, m, c.stable, st)
    elif e in ("ifftbr", "ifftbr_c64"):
        out = _nan((b, n), rdt if c.out_real else cdt)
        work = _nan((b, n), cdt) if c.out_real else None
        N.call("fgp_" + e, N.ptr(x), stride, N.ptr(out), int(c.out_real), N.ptr(work), b, m, c.stable, st)
    elif e in ("fwht", "fwht_f32"):
        out = _nan((b, n), rdt) if out is None else out
        N.call("fgp_" + e, N.ptr(x), stride, N.ptr(out), b, m, c.stable, st)
    elif e == "ifftbr_mul":
        net = c.fam == NET
        real = net or c.out_real
        out = _nan((b, n), rdt if real else cdt)
        work = _nan((b, n), cdt) if (real and not net) else None
        N.call("fgp_ifftbr_mul", c.fam, int(single), N.ptr(x), stride, N.ptr(f), fs, N.ptr(out), int(bool(real and not net)),
               N.ptr(work), b, m, c.stable, st)
    elif e == "fftbr_real":
        out, work = _nan((b, n), torch.complex128), _nan((b, n), torch.complex128)
        N.call("fgp_fftbr_real", N.ptr(x), stride, N.ptr(out), N.ptr(work), b, m, st)
    elif e in ("fftbr_real_half", "fftbr_real_half_f32"):
        out, work = _nan((b, n // 2 + 1 + c.opad), torch.complex128), _nan((b, n), torch.complex128)
        N.call("fgp_" + e, N.ptr(x), stride, N.ptr(out), out.stride(0), N.ptr(work), b, m, st)
    elif e in ("ifftbr_real", "ifftbr_real_rf"):
        out, work = _nan((b, n), torch.float64), _nan((b, n), torch.complex128)
        N.call("fgp_" + e, N.ptr(x), stride, N.ptr(f), fs, N.ptr(out), n, N.ptr(work), b, m, st)
    else:
        raise AssertionError(e)
    return out


def _twice(c, x, f):
    """The output of two calls, which must agree bit for bit and be finite."""
    try:
        o1 = launch(c, x, f)
        o2 = launch(c, x, f)
        torch.cuda.synchronize()
    except RuntimeError as err:                    # a failed call or a device fault: nothing more runs on the device
        if not torch.cuda.is_available():
            raise
        pytest.exit("%s: %s" % (c.name, err), returncode=3)
    no = TC.n_out(c)
    assert bool(torch.isfinite(torch.view_as_real(o1[:, :no]) if o1.is_complex() else o1[:, :no]).all()), (c.name, "not finite")
    assert torch.equal(o1[:, :no], o2[:, :no]), (c.name, "two calls differ")
    return o1[:, :no]


def _dense(name):
    c = TC.by_name()[name]
    inp = TC._dense_inputs(name)
    out = _twice(c, _dev(inp["x"]), _dev(inp["f"]))
    r_all, r_off, C = TC.check_dense(c, out.cpu().numpy())
    _note(c, "all", r_all, C)
    if TC.case_spec(c).dc[0] not in ("none", "all"):
        _note(c, "off-DC", r_off, C)
    assert r_all <= C and r_off <= C, (name, r_all, r_off, C)
    return c, inp, out


@pytest.mark.parametrize("name", [c.name for c in TC.cases("dense")])
def test_dense_rows(name):
    _dense(name)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("half")])
def test_dense_rows_half_length(name):
    _dense(name)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("mul")])
def test_dense_rows_fused_product(name):
    _dense(name)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("single")])
def test_dense_rows_single_precision(name):
    _dense(name)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("dc")])
def test_large_dc_stays_in_the_dc_bins(name):
    _dense(name)


def _sparse_device(c, rows):
    """The sparse rows (and the shared factor row) built on the device."""
    n = 1 << c.m
    single = bool(TC._single(c))
    cx = not TC._real_in(c)
    dt = (_CDT if cx else _RDT)[single]
    rf = c.entry == "ifftbr_real_rf"
    width = n // 2 + 1 if rf else n
    x = torch.zeros((len(rows), width), dtype=dt, device=DEV)
    for r, (pos, val) in enumerate(rows):
        x[r, torch.from_numpy(pos).to(DEV)] = torch.from_numpy(val).to(DEV).to(dt)
    f = None
    if getattr(c, "f", None):
        k = torch.arange(n, device=DEV)
        if rf:
            k = torch.minimum(k, n - k)
        f = 0.75 + (k % 7).double() / 8.0
        if cx and not rf:
            f = torch.complex(f, ((k % 5) - 2).double() / 16.0)
        f = f.to(dt if not rf else torch.float64)[None, :].contiguous()
        ks = np.arange(min(n, 1000))
        assert np.array_equal(f[0, :ks.size].cpu().numpy().astype(np.complex128),
                              TC.factor_row(ks, n, cx=cx and not rf, even=rf).astype(np.complex128))
    return x, f


@pytest.mark.parametrize("name", [c.name for c in TC.cases("sparse")])
def test_sparse_rows(name):
    c = TC.by_name()[name]
    rows = TC.sparse_rows(c)
    exp = TC.sparse_expected(c, rows)
    x, f = _sparse_device(c, rows)
    out = _twice(c, x, f)
    dev = out[:, torch.from_numpy(exp[2]).to(DEV)].cpu().numpy()
    r, C = TC.check_sparse(c, dev, exp)
    _note(c, "sparse", r, C)
    assert r <= C, (name, r, C)


@pytest.mark.parametrize("name", [c.name for c in TC.cases("alias")])
def test_in_place_equals_out_of_place(name):
    """The aliasing include/fgp_hip.h allows: fgp_fftbr of complex contiguous rows and fgp_fwht with out == in."""
    c, inp, out = _dense(name)
    y = _dev(inp["x"]).clone()
    assert y.is_contiguous() and y.stride(0) == 1 << c.m
    res = launch(c, y, None, out=y)
    assert res.data_ptr() == y.data_ptr() and torch.equal(y, out), (name, "in place differs")


# ------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("fam,m", TC.DOUBLE_CASES)
def test_double_update(fam, m):
    n = 1 << m
    prev, nxt = TC.double_inputs(fam, m)
    dp, dn = _dev(prev), _dev(nxt)
    outs = []
    for _ in range(2):
        out = _nan((3, 2 * n + 1), torch.complex128 if fam == LAT else torch.float64)
        N.call("fgp_double_update", fam, N.ptr(dp), dp.stride(0), N.ptr(dn), dn.stride(0), 3, m, N.ptr(out), out.stride(0),
               _stream())
        outs.append(out[:, :2 * n])
    assert torch.equal(outs[0], outs[1])
    dev = outs[0].cpu().numpy()
    assert np.isfinite(dev).all()
    re, im, B = TR.double_update(fam, prev[:, :n], nxt[:, :n])
    e, _ = TC._err(dev, re, im if fam == LAT else None)
    ratio = TC._ratio(e, TR.U64 * B)
    print("double_update fam %d m %2d   ratio = %6.3f   C = %g" % (fam, m, ratio, TC.C_DOUBLE[fam]))
    WORST["elem fgp_double_update " + ("lattice" if fam == LAT else "net")] = (
        max(ratio, WORST.get("elem fgp_double_update " + ("lattice" if fam == LAT else "net"), (0, 0))[0]), TC.C_DOUBLE[fam])
    assert ratio <= TC.C_DOUBLE[fam]


@pytest.mark.parametrize("kind,G", TC.SUMSQ_CASES)
def test_sum_sq(kind, G):
    x = TC.sumsq_inputs(kind, G)
    n, R = TC.SUMSQ_N, TC.SUMSQ_R
    dx = _dev(x)
    outs = []
    for _ in range(2):
        out = _nan((G, n), torch.float64)
        N.call("fgp_sum_sq", N.ptr(dx), dx.stride(0), kind, R, G, n, N.ptr(out), _stream())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    dev = outs[0].cpu().numpy()
    Y = TR.sum_sq(x[:, :n], G)
    C = TC.c_sum_sq(R, kind in (1, 3))
    ratio = TC._ratio(abs(TR._x(dev) - Y), TR.U64 * Y)
    print("sum_sq kind %d G %d   ratio = %6.3f   C = %d" % (kind, G, ratio, C))
    WORST["elem fgp_sum_sq"] = (max(ratio, WORST.get("elem fgp_sum_sq", (0, 0))[0]), C)
    assert np.isfinite(dev).all() and ratio <= C


def test_sum_sq_half():
    m, R, G = 17, 2, 2
    n = 1 << m
    g = np.random.default_rng(17)
    xh = np.zeros((R * G, n // 2 + 2), np.complex128)
    xh[:, :n // 2 + 1] = g.standard_normal((R * G, n // 2 + 1)) + 1j * g.standard_normal((R * G, n // 2 + 1))
    dx = _dev(xh)
    outs = []
    for _ in range(2):
        out = _nan((G, n), torch.float64)
        N.call("fgp_sum_sq_half", N.ptr(dx), dx.stride(0), R, G, n, N.ptr(out), _stream())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    dev = outs[0].cpu().numpy()
    Y = TR.sum_sq_half(xh[:, :n // 2 + 1], n, G)
    C = TC.c_sum_sq(R, True)
    ratio = TC._ratio(abs(TR._x(dev) - Y), TR.U64 * Y)
    print("sum_sq_half m %d   ratio = %6.3f   C = %d" % (m, ratio, C))
    WORST["elem fgp_sum_sq_half"] = (ratio, C)
    assert np.isfinite(dev).all() and ratio <= C


def test_zz_worst_ratios_per_variant():
    """Prints (-s) the table of DESIGN.md section 3.1; every entry was asserted where it was measured."""
    for v in sorted(WORST):
        print("%-52s worst ratio %7.3f   c = %g" % (v, WORST[v][0], WORST[v][1]))
        assert WORST[v][0] <= WORST[v][1]
