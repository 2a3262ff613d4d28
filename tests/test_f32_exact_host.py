"""tests/f32_exact.py without a GPU: fma32 against libm's fmaf bit for bit, and the float32 restatements built from it
(three_nn_ref.interpolate32 / backward32, chamfer_ref.search32 / grad32) against the host models of the kernels' device functions,
bit for bit, on the fixtures and shape lists the GPU tests then hold the device to.

If a restatement and a host model disagree, one of them does not follow so3_device.h: there is no tolerance here to hide behind."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import chamfer_ref
import f32_exact as fx
from support import bits
import test_chamfer_host as chost
import test_three_nn_host as thost
import three_nn_ref
from test_chamfer_host import model as chamfer_model       # noqa: F401 -- the host-model fixtures, built once per module
from test_three_nn_host import model as three_nn_model     # noqa: F401


@pytest.fixture(scope="module")
def fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float

    def run(a, b, c):
        a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (a, b, c)))
        return np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())], np.float32).reshape(a.shape)

    return run


def naive(a, b, c):
    """The spelling that rounds twice: to float64, then to float32."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def mismatches(fmaf, a, b, c):
    return int((bits(fx.fma32(a, b, c)) != bits(fmaf(a, b, c))).sum())


# ---- fma32 against libm ---------------------------------------------------------------------------------------------------------
def test_fma32_equals_fmaf_on_random_triples_over_ten_decades(fmaf):
    """a * b against c at every relative scale from 1e-5 to 1e5 (10 decades), both signs, operands from 1e-3 to 1e3."""
    rng = np.random.default_rng(3201)
    n = 200_000
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    c = (a.astype(np.float64) * b * rng.choice([-1.0, 1.0], n) * rng.uniform(1, 10, n) * 10.0 ** rng.uniform(-5, 4, n)).astype(np.float32)
    ratio = np.abs(c.astype(np.float64) / (a.astype(np.float64) * b))
    assert ratio.min() < 2e-5 and ratio.max() > 5e4
    bad = mismatches(fmaf, a, b, c)
    print("fma32 against fmaf: %d mismatches on %d random triples" % (bad, n))
    assert bad == 0


def halfway_family(rng):
    """Triples whose exact a * b + c lies ON a float32 halfway point (i == 0) or 2^-46 i^2 relative next to it, too close for float64
    to tell: a = 1 + i 2^-23, b = 2^g (1 - i 2^-23), so a b = 2^g (1 - i^2 2^-46); c = k 2^(g+1) with 2^23 <= k < 2^24 has 2^(g+1) for
    its ulp, so a b + c = 2^(g+1) (k + 1/2 - i^2 2^-47).  Every sign of a and c; k even and odd.  A second part lands ON halfway
    points with short operands: a, b of 12 bits, r a float32 near a b, c = (r + ulp(r) / 2) - a b where that is a float32."""
    i = np.repeat(np.arange(0, 360), 32).astype(np.float64)
    n = len(i)
    g = rng.integers(-20, 21, n).astype(np.float64)
    k = rng.integers(2 ** 23, 2 ** 24, n).astype(np.float64)
    a = (1 + i * 2.0 ** -23) * rng.choice([-1.0, 1.0], n)
    b = 2.0 ** g * (1 - i * 2.0 ** -23)
    c = k * 2.0 ** (g + 1) * rng.choice([-1.0, 1.0], n)
    a2 = rng.integers(2 ** 11, 2 ** 12, 20_000).astype(np.float64) * 2.0 ** rng.integers(-16, 5, 20_000)
    b2 = rng.integers(2 ** 11, 2 ** 12, 20_000).astype(np.float64) * rng.choice([-1.0, 1.0], 20_000)
    r = (a2 * b2 * rng.uniform(0.6, 1.6, 20_000)).astype(np.float32)
    half = r.astype(np.float64) + np.spacing(r).astype(np.float64) / 2
    c2 = half - a2 * b2
    keep = c2.astype(np.float32).astype(np.float64) == c2
    a, b, c = np.concatenate([a, a2[keep]]), np.concatenate([b, b2[keep]]), np.concatenate([c, c2[keep]])
    for v in (a, b, c):
        assert (v.astype(np.float32).astype(np.float64) == v).all()
    return a.astype(np.float32), b.astype(np.float32), c.astype(np.float32), int(keep.sum())


def test_fma32_equals_fmaf_on_and_next_to_halfway_points(fmaf):
    a, b, c, on = halfway_family(np.random.default_rng(3202))
    assert on >= 5000 and len(a) >= 16_000
    got = fx.fma32(a, b, c)
    bad = int((bits(got) != bits(fmaf(a, b, c))).sum())
    told_apart = int((bits(naive(a, b, c)) != bits(got)).sum())
    print("fma32 against fmaf: %d mismatches on %d triples on and next to halfway points; the double-rounded spelling differs on %d" % (bad, len(a), told_apart))
    assert bad == 0
    assert told_apart >= 1000                                  # the family sees what rounding twice does


def test_fma32_on_the_constructed_double_rounding_case(fmaf):
    """fma(1 + 2^-23, 64 (1 - 2^-23), 2^30 + 2^7) = 2^30 + 2^7 + 64 - 2^-40: just below the halfway point 2^30 + 192, so 2^30 + 128.
    float64 cannot hold the 2^-40 beside 2^30: the naive spelling lands ON the halfway point and rounds to even, 2^30 + 256."""
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(64 * (1 - 2.0 ** -23)), np.float32(2.0 ** 30 + 2.0 ** 7)
    for sign in (1, -1):
        sa, sc = np.float32(sign) * a, np.float32(sign) * c
        want = np.float32(sign * (2.0 ** 30 + 2.0 ** 7))
        assert bits(fx.fma32(sa, b, sc)) == bits(want) == bits(fmaf(sa, b, sc))
        assert naive(sa, b, sc) == np.float32(sign * (2.0 ** 30 + 2.0 ** 8))     # the family can tell the two apart


def test_fma32_signed_zeros_subnormals_and_overflow(fmaf):
    f = np.float32
    tiny, big = f(2.0 ** -149), f(np.finfo(np.float32).max)
    cases = [(0.0, 1.0, -0.0), (-0.0, 1.0, -0.0), (-0.0, 5.0, 0.0), (1.0, -1.0, 1.0), (-1.0, 1.0, 1.0), (0.0, -3.0, 0.0), (-2.0, 0.0, -0.0),
             (2.0 ** -75, 2.0 ** -70, tiny), (2.0 ** -75, 2.0 ** -75, tiny), (2.0 ** -75, 2.0 ** -75 * (1 + 2.0 ** -23), tiny), (2.0 ** -75, -2.0 ** -75, tiny),
             (2.0 ** -80, 2.0 ** -80, 0.0), (2.0 ** -100, 2.0 ** -30, -2.0 ** -128), (1 + 2.0 ** -23, 2.0 ** -126, -2.0 ** -126), (3 * 2.0 ** -75, 2.0 ** -75, 2.0 ** -148),
             (2.0 ** 127, 2.0, 0.0), (-2.0 ** 127, 2.0, 0.0), (big, 1.0, big), (big, 1.0, 2.0 ** 102), (big, 1.0, 2.0 ** 103), (big, 2.0, -big), (2.0 ** 64, 2.0 ** 64, -2.0 ** 127)]
    a, b, c = (np.array(v, np.float32) for v in zip(*cases))
    got, want = fx.fma32(a, b, c), fmaf(a, b, c)
    assert np.array_equal(bits(got), bits(want)), [(k, got[k], want[k]) for k in np.flatnonzero(bits(got) != bits(want))]
    assert np.signbit(got[[1, 6]]).all() and not np.signbit(got[[0, 2, 3, 4, 5]]).any() and (got[:7] == 0).all()      # the zeros' signs
    assert 0 < abs(got[7]) < 2.0 ** -126 and 0 < abs(got[12]) < 2.0 ** -126                                          # subnormal results
    assert np.isposinf(got[15]) and np.isneginf(got[16]) and np.isposinf(got[17]) and np.isfinite(got[18])           # overflow, and just not


def test_the_other_functions_are_their_one_line_definitions(fmaf):
    rng = np.random.default_rng(3203)
    d = rng.uniform(-2, 2, (3, 500)).astype(np.float32)
    want = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]))
    assert np.array_equal(bits(fx.pair_dist2_32(*d)), bits(want))
    m, p = rng.uniform(-2, 2, (4, 12)).astype(np.float32), rng.uniform(-2, 2, (4, 30, 3)).astype(np.float32)
    got = fx.pose_point32(m, p)
    assert got.shape == p.shape and got.dtype == np.float32
    for c in range(3):
        row = m[:, None, 4 * c:4 * c + 4]
        want = fmaf(row[..., 0], p[..., 0], fmaf(row[..., 1], p[..., 1], fmaf(row[..., 2], p[..., 2], row[..., 3])))
        assert np.array_equal(bits(got[..., c]), bits(want))
    d2 = np.array([[3, 1, 1, 2], [0, 0, 0, 0], [5, 4, 3, 3]], np.float32)
    assert fx.first_argmin32(d2).tolist() == [1, 0, 2]                            # strict <: the first of equal candidates


# ---- three_interpolate: the restatement against the host model --------------------------------------------------------------------
def _interp_equal(model, name, c, want32):
    """The host model in both layouts against want32 = test_three_nn_host.expected32(c), the channel-last restatement (an element's
    arithmetic does not depend on the layout: test_the_restatements_take_both_layouts)."""
    for cf in (False, True):
        feat, grad = thost.layouts(c, cf)
        out32, grad32 = (a.transpose(0, 2, 1) if cf else a for a in want32)
        got = thost.model_fwd(model, feat, c["idx"], c["weight"], cf)
        assert got.shape == out32.shape and np.array_equal(bits(got), bits(out32)), (name, cf, int((bits(got) != bits(out32)).sum()))
        got = thost.model_bwd(model, grad, c["idx"], c["weight"], c["feat"].shape[1], cf)
        assert got.shape == grad32.shape and np.array_equal(bits(got), bits(grad32)), (name, cf, int((bits(got) != bits(grad32)).sum()))


def test_the_restatements_take_both_layouts():
    c = next(c for c in thost.interp_shape_cases() if c["name"] == "B=3 N=65 S=4 D=65")
    out32, grad32 = thost.expected32(c)
    feat, grad = thost.layouts(c, True)
    assert np.array_equal(bits(three_nn_ref.interpolate32(feat, c["idx"], c["weight"], True)), bits(out32.transpose(0, 2, 1)))
    assert np.array_equal(bits(three_nn_ref.backward32(grad, c["idx"], c["weight"], 4, True)), bits(grad32.transpose(0, 2, 1)))
    assert out32.shape == (3, 65, 65) and grad32.shape == (3, 4, 65) and out32.dtype == grad32.dtype == np.float32


def test_interpolate32_and_backward32_equal_the_host_model_on_g24(three_nn_model):      # noqa: F811
    rng = np.random.default_rng(2403)
    for c in three_nn_ref.cases(three_nn_ref.g24()):
        _, idx, w = three_nn_ref.three_nn(c["xyz1"], c["xyz2"])
        grad = rng.standard_normal(c["xyz1"].shape[:2] + (three_nn_ref.D_FIXTURE,)).astype(np.float32)
        case = {"feat": c["feat"], "idx": idx, "weight": w, "grad": grad}
        _interp_equal(three_nn_model, c["name"], case, thost.expected32(case))


def test_interpolate32_and_backward32_equal_the_host_model_on_the_shape_list(three_nn_model):      # noqa: F811
    for i, c in enumerate(thost.interp_shape_cases()):
        _interp_equal(three_nn_model, c["name"], c, thost.interp_expected32(i))


# ---- chamfer: the restatement against the host model ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g27_cases():
    return chamfer_ref.cases(chamfer_ref.g27())


def test_a_small_last_hit_is_inside_the_float64_bound_and_changes_the_bits(chamfer_model):      # noqa: F811
    """The case tests/test_gpu_chamfer.py runs for what the bound cannot see: the premise (the last hit of x_0's 2500-hit chain is
    below the gradient figure's bound and above the running sum's ulp), and the host model equal to the restatement on it."""
    c = chamfer_ref.small_last_hit_case()
    got = chost.host_run(chamfer_model, c)
    want = chamfer_ref.search32(c["X"], c["Y"])
    assert (got["nearest_y"] == 0).all() and all(np.array_equal(got[k], want[k]) for k in ("nearest_x", "nearest_y"))
    sx, sy = chamfer_ref.scales(1)
    dX, dY = chamfer_ref.grad32(c["X"], c["Y"], None, None, got["nearest_x"], got["nearest_y"], sx, sy)
    assert np.array_equal(bits(got["dX"]), bits(dX)) and np.array_equal(bits(got["dY"]), bits(dY))
    terms = np.abs(np.float64(sy[0]) * 2 * (c["X"][0, 0].astype(np.float64) - c["Y"][0].astype(np.float64)))       # (2500, 3): the hits on x_0
    assert (terms[-1] < 0.25 * chost.GRAD_TOL * terms.sum(0)).all()                     # dropped, the figure moves by a quarter of its bound at most
    assert (terms[-1] > 4 * np.spacing(np.abs(dX[0, 0]))).all()                         # and the bits move
    dropped = got["nearest_y"].copy()
    dropped[0, -1] = -1                                                                 # names no owner: the chain loses its last hit
    without = chamfer_ref.grad32(c["X"], c["Y"], None, None, got["nearest_x"], dropped, sx, sy)[0]
    assert (bits(without[0, 0]) != bits(dX[0, 0])).all()                                # the chain without its last hit: other bits in every coordinate
    f = chamfer_ref.gradient_figures(c["X"], c["Y"], None, None, True, got["nearest_x"], got["nearest_y"], sx, sy, without, None)
    assert f["grad"] <= chost.GRAD_TOL                                                  # ... which the float64 figure accepts


def test_search32_and_grad32_equal_the_host_model_on_g27(chamfer_model, g27_cases):      # noqa: F811
    """Every case of G27, ragged ones included (padded slots 0 / -1): the indices in both flavours, and in the squared one d^2 and both
    gradients; the many-to-one family's 2500-hit chain is among them.  Then the x direction alone on two geometries."""
    longest = 0
    for c in g27_cases:
        got = chost.host_run(chamfer_model, c)
        want = chost.expected_search32(c)                       # chamfer_ref.search32, once per geometry
        for k in ("nearest_x", "nearest_y"):
            assert np.array_equal(got[k], want[k]), (c["name"], k, np.argwhere(got[k] != want[k])[:4])
        if not c["squared"]:
            continue
        for k in ("dist_x", "dist_y"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (c["name"], k)
        sx, sy = chamfer_ref.scales(c["b"])
        dX, dY = chamfer_ref.grad32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], got["nearest_x"], got["nearest_y"], sx, sy)
        assert np.array_equal(bits(got["dX"]), bits(dX)) and np.array_equal(bits(got["dY"]), bits(dY)), c["name"]
        longest = max(longest, int(np.bincount(got["nearest_y"][got["nearest_y"] >= 0]).max()))
    assert longest == 2500
    for c in (c for c in g27_cases if c["geometry"] in ("random_257x1025", "subset_300x700") and c["squared"]):
        got = chost.host_run(chamfer_model, c, single=True)
        want = chamfer_ref.search32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], single=True)
        assert np.array_equal(got["nearest_x"], want["nearest_x"]) and np.array_equal(bits(got["dist_x"]), bits(want["dist_x"])), c["name"]
        dX, dY = chamfer_ref.grad32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], got["nearest_x"], None, chamfer_ref.scales(c["b"])[0], None)
        assert np.array_equal(bits(got["dX"]), bits(dX)) and np.array_equal(bits(got["dY"]), bits(dY)), c["name"]
