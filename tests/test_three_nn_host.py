"""three_nn, three_interpolate, interpolate_features and propagate_features (so3_three_nn_f32, so3_three_interpolate_f32,
so3_three_interpolate_bwd_f32) without a GPU: the boundary (header, binding table, exports, argument validation, the Python names),
the G24 fixture, and the kernels' device functions compiled for the host (tests/host_model/three_nn.cpp with SO3_HOST_MODEL).

The search's arithmetic is a definition (include/so3proj.h), so distances, indices and weights are compared EXACTLY:
  1  the host model equals the numpy restatement (tests/three_nn_ref.py) bit for bit on all of G24 and on the shape lists below,
     however the scan is split (1, 2 or 4 lists merged on (d, j));
  2  its indices equal the ones the reference's own code produced (G24) outside near_tie -- the reference takes its distances from
     |a|^2 + |b|^2 - 2 a.b, so two candidates within 2e-6 can swap there.  The mask may cover at most 1 % of a case's rows (re-asserted
     here: exclusions cannot hide a failure); inside it rows must still be in range, distinct and non-decreasing in dist2;
  3  interpolated values equal interpolate32 (the defined fma order through tests/f32_exact.py) bit for bit, lie within
     8 * 2^-24 * sum_k w_k |f_k| of the float64 restatement, and within ref_dev + that bound of the reference's recorded output
     outside near_tie | near_zero (not for the subset case: its reference weights are noise);
  4  the backward equals backward32 (fused multiply-adds from +0 in ascending (n, k)) bit for bit, lies within
     (h + 2) * 2^-24 * sum |w g| of the float64 restatement for a known point with h hits, and is exactly 0 for a known point nobody
     selected.
tests/test_gpu_three_nn.py imports the shape lists and the checks and runs them on the device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from support import bits, boundary, build_host_model, np_ptr, on_own_thread
import three_nn_ref as ref

NEW_SYMBOLS = {"so3_three_nn_f32": 9, "so3_three_interpolate_f32": 10, "so3_three_interpolate_bwd_f32": 10}
SRC = os.path.join(ROOT, "tests", "host_model", "three_nn.cpp")
GRID_CAP = 8192                      # so3proj.hip: kThreeMaxGrid
TILE = 1024                          # so3_device.h: kThreeNnTile, the known points per LDS tile
SPLIT_ITEMS, SPLIT_S = 1024, 64      # so3_device.h: kThreeNnSplitItems, kThreeNnSplitS -- four waves per point below / from
BWD_CHANNELS = 256                   # so3_device.h: kThreeBwdChannels, the channel-last backward's channels per pass
BWD_TILE = 1024                      # so3proj.hip: kThreeBwdTile, the unknown points per LDS tile of the channel-last backward
NN_KERNELS = {"k_three_nn<%d, %s>" % (w, t) for w in (1, 4) for t in ("true", "false")}


def waves_per_point(b, n, s):
    return 4 if s >= SPLIT_S and b * ((n + 255) // 256) < SPLIT_ITEMS else 1


# ---- the shape lists, shared with tests/test_gpu_three_nn.py ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nn_shape_cases():
    """Dicts (name, xyz1 (B,N,3), xyz2 (B,S,3)).  B in {1, 3}; N = 1, around the wave (64), the work item (256) and beyond; S = 1, 2, 3
    (padded slots), 4, around the S switch of the dispatch (64), around the LDS tile (1024); around the work-item switch of the dispatch
    (1024 items); a batch beyond the launch's grid; the edge cases."""
    rng = np.random.default_rng(2401)
    out = []

    def add(name, xyz1, xyz2):
        out.append({"name": name, "xyz1": np.ascontiguousarray(xyz1, np.float32), "xyz2": np.ascontiguousarray(xyz2, np.float32)})

    for b in (1, 3):
        for n in (1, 63, 64, 65, 255, 256, 257, 600):
            for s in (1, 2, 3, 4, 63, 64, 65):
                add("B=%d N=%d S=%d" % (b, n, s), rng.uniform(-1, 1, (b, n, 3)), rng.uniform(-1, 1, (b, s, 3)))
        for s in (TILE - 1, TILE, TILE + 1, 2 * TILE + 9):
            add("B=%d N=70 S=%d (tile)" % (b, s), rng.uniform(-1, 1, (b, 70, 3)), rng.uniform(-1, 1, (b, s, 3)))
    for b in (SPLIT_ITEMS - 1, SPLIT_ITEMS, SPLIT_ITEMS + 1):
        add("B=%d N=3 S=64 (work-item switch)" % b, rng.uniform(-1, 1, (b, 3, 3)), rng.uniform(-1, 1, (b, SPLIT_S, 3)))
    add("B=%d beyond the grid" % (GRID_CAP + 3), rng.uniform(-1, 1, (GRID_CAP + 3, 2, 3)), rng.uniform(-1, 1, (GRID_CAP + 3, 3, 3)))
    for b in (1, 3):
        known = rng.uniform(-1, 1, (b, 90, 3))
        add("unknown points that are known points B=%d" % b, np.concatenate([known[:, ::3], rng.uniform(-1, 1, (b, 40, 3))], 1), known)
        dup = rng.uniform(-1, 1, (b, 40, 3))
        add("duplicated known points B=%d" % b, rng.uniform(-1, 1, (b, 130, 3)), np.concatenate([dup, dup[:, ::-1], dup], 1))
        add("all-equal known cloud B=%d" % b, rng.uniform(-1, 1, (b, 70, 3)), np.full((b, 80, 3), 0.25))
        add("coordinates at 1e3 B=%d" % b, rng.uniform(-1e3, 1e3, (b, 300, 3)), rng.uniform(-1e3, 1e3, (b, 100, 3)))
    return out


@functools.lru_cache(maxsize=None)
def nn_nonfinite_cases():
    """Dicts (name, xyz1, xyz2) with NaN and infinite coordinates: the clouds of the device's test_non_finite_coordinates_keep_indices
    _in_range.  A NaN or +inf d fails every <, so a list may end without a candidate; what is written is unspecified but every index
    stays in [0, S) -- three_nn_finish's clamp.  Judged by check_nn_in_range, not by the restatement."""
    rng = np.random.default_rng(2404)
    xyz1, xyz2 = rng.uniform(0, 1, (2, 300, 3)).astype(np.float32), rng.uniform(0, 1, (2, 70, 3)).astype(np.float32)
    xyz1[0, 5, 0], xyz1[1, 0, 1], xyz2[0, 7, 2], xyz2[1, 0, 0], xyz2[1, 69, 1] = np.nan, np.inf, np.inf, np.nan, -np.inf
    return [{"name": "non-finite S=70", "xyz1": xyz1, "xyz2": xyz2}, {"name": "non-finite S=2", "xyz1": xyz1, "xyz2": xyz2[:, :2].copy()},
            {"name": "an all-NaN known cloud S=5", "xyz1": xyz1, "xyz2": np.full((2, 5, 3), np.nan, np.float32)}]


@functools.lru_cache(maxsize=None)
def nn_expected():
    return [ref.three_nn(c["xyz1"], c["xyz2"]) for c in nn_shape_cases()]


@functools.lru_cache(maxsize=None)
def interp_shape_cases():
    """Dicts (name, feat (B,S,D) channel-last, idx (B,N,3) int64, weight (B,N,3) float32, grad (B,N,D) channel-last); both layouts are run
    from them.  D in {1, 3, 63, 64, 65, 257} (257: one above the channel-last backward's 256 channels per pass, and five 64-channel
    groups of the channel-first one); N around the channel-first backward's tile (64) and the channel-last one's (1024); S around the 16
    and 64 known points of a backward work item; batches beyond the grid of every launch; a known point selected by every unknown point in
    all three slots (h = 3 N hits) beside known points selected by none; an unknown point that is a known point; a 600-hit chain whose
    last hit is far inside the backward's any-order bound (what only the bit comparison sees)."""
    rng = np.random.default_rng(2402)
    out = []

    def add(name, b, n, s, d, idx=None, weight=None, xyz=None):
        feat, grad = rng.standard_normal((b, s, d)).astype(np.float32), rng.standard_normal((b, n, d)).astype(np.float32)
        if idx is None:
            xyz = (rng.uniform(-1, 1, (b, n, 3)), rng.uniform(-1, 1, (b, s, 3))) if xyz is None else xyz
            _, idx, weight = ref.three_nn(*xyz)
        out.append({"name": name, "feat": feat, "idx": np.ascontiguousarray(idx, np.int64), "weight": np.ascontiguousarray(weight, np.float32), "grad": grad})

    for d in (1, 3, 63, 64, 65, BWD_CHANNELS + 1):
        for b, n, s in ((3, 65, 4), (1, 257, 65), (1, 63, 17), (3, 64, 2)):
            add("B=%d N=%d S=%d D=%d" % (b, n, s, d), b, n, s, d)
    for n, s in ((600, 63), (BWD_TILE - 1, 5), (BWD_TILE, 16), (BWD_TILE + 1, 130), (1, 1), (5, 1)):
        add("B=1 N=%d S=%d D=5" % (n, s), 1, n, s, 5)
    big = GRID_CAP + 5
    add("B=%d beyond the backwards' and the channel-first forward's grid" % big, big, 2, 3, 3)
    add("B=%d beyond the channel-last forward's grid" % big, big, 5, 3, 33)
    n, s = 200, 9
    everyone = np.zeros((2, n, 3), np.int64)
    everyone[1] = rng.integers(2, s, (n, 3))                                     # cloud 1: known points 0 and 1 are selected by nobody
    add("h = 3N hits and none", 2, n, s, 70, everyone, rng.uniform(0, 1, (2, n, 3)))
    known = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(1, 27, 3) * 0.5      # a grid: every other distance is >= 0.25
    add("an unknown point that is a known point", 1, 27, 27, 6, xyz=(known[:, ::-1], known))
    out[-1]["feat"] = np.ascontiguousarray(rng.uniform(1, 2, (1, 27, 6)), np.float32)
    # what only the bit comparison sees: a chain of 600 hits whose LAST hit weighs 1e-4 -- at most a fortieth of the backward's any-order
    # bound (602 * 2^-24 * sum |w g|) and typically forty ulps of the running sum.  Dropping it, or taking it twice, stays inside the
    # bound and changes the bits (test_the_shape_lists_hold_what_they_promise).  Added last: the cases above keep their random streams.
    small = rng.uniform(0.25, 1, (1, n, 3))
    small[0, -1, 2] = 1e-4
    add("h = 3N hits, the last a small one", 1, n, s, 70, np.zeros((1, n, 3), np.int64), small)
    return out


def layouts(c, channels_first):
    """(feat, grad) of an interpolation case in the asked layout, contiguous."""
    if channels_first:
        return np.ascontiguousarray(c["feat"].transpose(0, 2, 1)), np.ascontiguousarray(c["grad"].transpose(0, 2, 1))
    return c["feat"], c["grad"]


def test_the_shape_lists_hold_what_they_promise():
    seen = set()
    for c, (d3, idx, w) in zip(nn_shape_cases(), nn_expected()):
        b, n, s = c["xyz1"].shape[0], c["xyz1"].shape[1], c["xyz2"].shape[1]
        seen.add(waves_per_point(b, n, s))
        ref.row_properties(d3, idx, s)
        assert np.isfinite(w).all() and (w >= 0).all() and np.abs(w.sum(-1) - 1).max() < 1e-6, c["name"]
        if s == 1:
            assert (w[..., 0] == 1).all() and (w[..., 1:] == 0).all() and (idx == 0).all()
        if c["name"].startswith("unknown points that are"):
            assert (d3[:, :30, 0] == 0).all() and (idx[:, :30, 0] == 3 * np.arange(30)).all()
        if c["name"].startswith("duplicated"):
            assert (idx[..., 0] < 40).all() and (d3[..., 0] == d3[..., 1]).all() and (d3[..., 1] == d3[..., 2]).all()       # the lower index wins
            assert (idx[..., 1] == 79 - idx[..., 0]).all() and (idx[..., 2] == 80 + idx[..., 0]).all()
        if c["name"].startswith("all-equal"):
            assert (idx == np.arange(3)).all()
    assert seen == {1, 4}
    assert {waves_per_point(b, 3, 64) for b in (SPLIT_ITEMS - 1, SPLIT_ITEMS)} == {1, 4} and waves_per_point(1, 600, 63) == 1
    hits = {c["name"]: ref.backward(c["grad"], c["idx"], c["weight"], c["feat"].shape[1])[2] for c in interp_shape_cases()}
    h = hits["h = 3N hits and none"]
    assert h[0, 0] == 600 and (h[0, 1:] == 0).all() and (h[1, :2] == 0).all()
    c = interp_shape_cases()[-1]
    want, bound, h = ref.backward(c["grad"], c["idx"], c["weight"], c["feat"].shape[1])
    last = np.abs(np.float64(c["weight"][0, -1, 2]) * c["grad"][0, -1])                 # the last hit of known point 0's chain, per channel
    assert c["name"].startswith("h = 3N hits, the last") and h[0, 0] == 600 and (last < bound[0, 0] / 10).all()       # far inside the bound ...
    assert (last > 2 * np.spacing(np.abs(want[0, 0]).astype(np.float32))).mean() > 0.9                                # ... and above the sum's ulp


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_THREE_MAX_D (\d+)", raw).group(1)) == _lib.THREE_MAX_D == 65536


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    nn = lambda b, n, s, a=p, k=p, d=p, i=p, w=p: lib.so3_three_nn_f32(a, k, d, i, w, b, n, s, None)
    fwd = lambda b, n, s, d, cf=0, f=p, i=p, w=p, o=p: lib.so3_three_interpolate_f32(f, i, w, o, cf, b, n, s, d, None)
    bwd = lambda b, n, s, d, cf=0, f=p, i=p, w=p, o=p: lib.so3_three_interpolate_bwd_f32(f, i, w, o, cf, b, n, s, d, None)
    assert nn(0, 8, 8, None, None, None, None, None) == 0                                         # B == 0: a no-op, whatever the pointers
    assert fwd(0, 8, 8, 4, 0, None, None, None, None) == 0 and bwd(0, 8, 8, 4, 1, None, None, None, None) == 0
    big = _lib.ADD_S_MAX_N + 1
    for b, n, s in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, -3, 8), (4, big, 8), (4, 8, 0), (4, 8, -1), (4, 8, big)):
        assert nn(b, n, s) != 0 and b"so3_three_nn_f32: B/N/S" in err(), (b, n, s, err())
        for fn, name in ((fwd, b"so3_three_interpolate_f32: B/N/S/D"), (bwd, b"so3_three_interpolate_bwd_f32: B/N/S/D")):
            assert fn(b, n, s, 4) != 0 and name in err(), (b, n, s, err())
    for d in (0, -1, _lib.THREE_MAX_D + 1):
        for cf in (0, 1):
            assert fwd(4, 8, 8, d, cf) != 0 and b"so3_three_interpolate_f32: B/N/S/D" in err(), (d, err())
            assert bwd(4, 8, 8, d, cf) != 0 and b"so3_three_interpolate_bwd_f32: B/N/S/D" in err(), (d, err())
    for kw in ({"a": None}, {"k": None}, {"d": None}, {"i": None}):                              # weight alone may be null
        assert nn(4, 8, 8, **kw) != 0 and b"so3_three_nn_f32: null pointer" in err(), kw
    for kw in ({"f": None}, {"i": None}, {"w": None}, {"o": None}):
        assert fwd(4, 8, 8, 4, **kw) != 0 and b"so3_three_interpolate_f32: null pointer" in err(), kw
        assert bwd(4, 8, 8, 4, **kw) != 0 and b"so3_three_interpolate_bwd_f32: null pointer" in err(), kw


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("three_nn", "three_interpolate", "interpolate_features", "propagate_features"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    xyz1, xyz2, feat = torch.zeros(2, 9, 3), torch.zeros(2, 4, 3), torch.zeros(2, 4, 5)
    idx, w = torch.zeros(2, 9, 3, dtype=torch.long), torch.zeros(2, 9, 3)
    for fn in (lambda: pa.three_nn(xyz1, xyz2), lambda: pa.three_nn(xyz1, xyz2, return_weights=True), lambda: pa.three_interpolate(feat, idx, w),
               lambda: pa.three_interpolate(feat.transpose(1, 2), idx, w, channels_first=True), lambda: pa.interpolate_features(xyz1, xyz2, feat),
               lambda: pa.propagate_features(xyz1.transpose(1, 2), xyz2.transpose(1, 2), None, feat.transpose(1, 2))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g24_cases():
    return ref.cases(ref.g24())


def test_g24_holds_the_cases_and_the_caps(g24_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    assert [(c["kind"],) + c["xyz1"].shape[:2] + (c["xyz2"].shape[1],) for c in g24_cases] == list(ref.CASES)
    for c in g24_cases:
        assert c["xyz1"].dtype == c["xyz2"].dtype == c["feat"].dtype == np.float32 and c["feat"].shape[-1] == ref.D_FIXTURE == 16
        both = np.concatenate([c["xyz1"], c["xyz2"]], 1)
        assert np.isfinite(both).all() and np.linalg.norm(both, axis=-1).max() <= 1.0 + 1e-6, c["name"]            # unit radius
        tie, zero = ref.masks(c["xyz1"], c["xyz2"])
        assert np.array_equal(tie, c["near_tie"]) and np.array_equal(zero, c["near_zero"]), c["name"]
        assert tie.mean() <= ref.MASK_CAP, (c["name"], tie.mean())
        if c["kind"] == "disjoint":
            assert (tie | zero).mean() <= ref.MASK_CAP, (c["name"], (tie | zero).mean())
            assert 0 < c["ref_dev"] < 1e-3
        if c["kind"] == "subset":
            assert 0.45 <= zero.mean() <= 0.55 and c["ref_negative_weights"] > 0                                  # the point of the case
            d3, _, _ = ref.three_nn(c["xyz1"], c["xyz2"])
            assert (d3[..., 0] == 0).mean() == 0.5                                                              # exactly 0 from coordinate differences


# ---- the checks, shared with tests/test_gpu_three_nn.py -----------------------------------------------------------------------
def check_nn(name, run_nn, xyz1, xyz2, want=None):
    """run_nn(xyz1, xyz2, want_weight) -> (dist2, idx, weight or None).  Bit-equal to the restatement, with and without weights."""
    d3, idx, w = ref.three_nn(xyz1, xyz2) if want is None else want
    got_d, got_i, got_w = run_nn(xyz1, xyz2, True)
    assert np.array_equal(np.asarray(got_i, np.int64), idx), (name, np.argwhere(np.asarray(got_i, np.int64) != idx)[:4])
    assert np.asarray(got_d).dtype == np.float32 and np.array_equal(np.asarray(got_d).view(np.uint32), d3.view(np.uint32)), name
    assert np.asarray(got_w).dtype == np.float32 and np.array_equal(np.asarray(got_w).view(np.uint32), w.view(np.uint32)), name
    alone_d, alone_i, none = run_nn(xyz1, xyz2, False)
    assert none is None and np.array_equal(alone_i, got_i) and np.array_equal(np.asarray(alone_d).view(np.uint32), d3.view(np.uint32)), name
    return d3, idx, w


def check_nn_in_range(name, run_nn, xyz1, xyz2):
    """Non-finite coordinates: every index stays in [0, S), with and without weights; the rows they do not reach equal the restatement."""
    s = xyz2.shape[1]
    for want_weight in (True, False):
        got_d, got_i, _ = run_nn(xyz1, xyz2, want_weight)
        got_i = np.asarray(got_i, np.int64)
        assert got_i.shape == xyz1.shape[:2] + (3,) and got_i.min() >= 0 and got_i.max() < s, (name, got_i.min(), got_i.max())
        clean = np.isfinite(xyz1).all(-1) & np.isfinite(xyz2).all((-1, -2))[:, None]
        d3, idx, _ = ref.three_nn(np.where(np.isfinite(xyz1), xyz1, 0), np.where(np.isfinite(xyz2), xyz2, 0))
        assert np.array_equal(got_i[clean], idx[clean]) and np.array_equal(np.asarray(got_d)[clean].view(np.uint32), d3[clean].view(np.uint32)), name


def expected32(c):
    """(out, grad_feat) of an interpolation case in the DEFINED float32 order, channel-last; the other layout is their transpose (the
    arithmetic of an element does not depend on the layout)."""
    return ref.interpolate32(c["feat"], c["idx"], c["weight"]), ref.backward32(c["grad"], c["idx"], c["weight"], c["feat"].shape[1])


@functools.lru_cache(maxsize=None)
def interp_expected32(i):
    return expected32(interp_shape_cases()[i])


def check_interp(name, run_fwd, run_bwd, c, channels_first, want32=None):
    """run_fwd(feat, idx, weight, channels_first) -> out; run_bwd(grad, idx, weight, s, channels_first) -> grad_feat, in the layout asked
    for.  Both bit for bit with the float32 restatement of the defined order (want32: expected32's pair, when it is at hand), and
    beside that within the derived bounds of the float64 restatement."""
    feat, grad = layouts(c, channels_first)
    s = c["feat"].shape[1]
    out32, grad32 = (a.transpose(0, 2, 1) if channels_first else a for a in (expected32(c) if want32 is None else want32))
    want, bound = ref.interpolate(feat, c["idx"], c["weight"], channels_first)
    got = np.asarray(run_fwd(feat, c["idx"], c["weight"], channels_first))
    assert got.dtype == np.float32 and got.shape == want.shape, name
    assert (np.abs(got - want) <= bound).all(), (name, channels_first, np.abs(got - want).max(), (np.abs(got - want) - bound).max())
    assert np.array_equal(bits(got), bits(out32)), (name, channels_first, "out", int((bits(got) != bits(out32)).sum()), np.argwhere(bits(got) != bits(out32))[:4])
    want_g, bound_g, hits = ref.backward(grad, c["idx"], c["weight"], s, channels_first)
    got_g = np.asarray(run_bwd(grad, c["idx"], c["weight"], s, channels_first))
    assert got_g.dtype == np.float32 and got_g.shape == want_g.shape, name
    assert (np.abs(got_g - want_g) <= bound_g).all(), (name, channels_first, np.abs(got_g - want_g).max(), (np.abs(got_g - want_g) - bound_g).max())
    assert np.array_equal(bits(got_g), bits(grad32)), (name, channels_first, "grad_feat", int((bits(got_g) != bits(grad32)).sum()),
                                                       np.argwhere(bits(got_g) != bits(grad32))[:4])
    untouched = np.broadcast_to((hits == 0)[:, None, :] if channels_first else (hits == 0)[:, :, None], got_g.shape)
    assert (got_g[untouched] == 0).all(), name                                      # exactly 0 (and written: the buffers start as NaN)
    return got, got_g


G24_EXPECTED32 = {}


def check_against_g24(g24_cases, run_nn, run_fwd, run_bwd):
    for c in g24_cases:
        s = c["xyz2"].shape[1]
        d3, idx, w = check_nn(c["name"], run_nn, c["xyz1"], c["xyz2"])                                           # 1
        assert c["near_tie"].mean() <= ref.MASK_CAP, c["name"]
        keep = ~c["near_tie"]
        assert np.array_equal(idx[keep], c["ref_idx"][keep]), (c["name"], np.argwhere((idx != c["ref_idx"]).any(-1) & keep)[:4])      # 2
        ref.row_properties(d3, idx, s)                                                                           # in the mask as well
        rng = np.random.default_rng(2403)
        case = {"feat": c["feat"], "idx": idx, "weight": w, "grad": rng.standard_normal(c["xyz1"].shape[:2] + (ref.D_FIXTURE,)).astype(np.float32)}
        if c["name"] not in G24_EXPECTED32:                  # computed once: the host model and the device's two routes share it
            G24_EXPECTED32[c["name"]] = expected32(case)
        want32 = G24_EXPECTED32[c["name"]]
        for channels_first in (False, True):
            got, _ = check_interp(c["name"], run_fwd, run_bwd, case, channels_first, want32)                     # 3, 4
            if c["kind"] == "subset":
                continue                                                                                         # indices only
            got = got.transpose(0, 2, 1) if channels_first else got
            keep = ~(c["near_tie"] | c["near_zero"])
            if c["kind"] == "disjoint":
                assert (~keep).mean() <= ref.MASK_CAP, c["name"]
            bound = ref.interpolate(c["feat"], idx, w)[1]
            assert (np.abs(got - c["ref_out"])[keep] <= (c["ref_dev"] + bound)[keep]).all(), (c["name"], np.abs(got - c["ref_out"])[keep].max())
        if c["kind"] == "subset":                                                   # a coincident point takes (all but 1e-6 of) the weight
            same = d3[..., 0] == 0
            assert same.mean() == 0.5 and (w >= 0).all() and (w[same][:, 0] > 1 - 1e-4).all()


# ---- the host model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "three_nn", SRC)
    lib.model_three_nn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    lib.model_three_interpolate.argtypes = lib.model_three_interpolate_bwd.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int64] + [ctypes.c_int32] * 3
    lib.model_three_nn_waves_per_point.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.model_three_nn.restype = lib.model_three_interpolate.restype = lib.model_three_interpolate_bwd.restype = None
    lib.model_three_nn_waves_per_point.restype = ctypes.c_int32
    return lib


def model_nn(lib, xyz1, xyz2, want_weight, slices=1):
    xyz1, xyz2 = np.ascontiguousarray(xyz1, np.float32), np.ascontiguousarray(xyz2, np.float32)
    b, n, s = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    d3, idx = np.full((b, n, 3), np.nan, np.float32), np.full((b, n, 3), -1, np.int32)
    w = np.full((b, n, 3), np.nan, np.float32) if want_weight else None
    lib.model_three_nn(np_ptr(xyz1), np_ptr(xyz2), np_ptr(d3), np_ptr(idx), None if w is None else np_ptr(w), b, n, s, slices)
    return d3, idx, w


def model_fwd(lib, feat, idx, weight, channels_first):
    feat, idx, weight = np.ascontiguousarray(feat, np.float32), np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(weight, np.float32)
    b, n = idx.shape[:2]
    d, s = (feat.shape[1], feat.shape[2]) if channels_first else (feat.shape[2], feat.shape[1])
    out = np.full((b, d, n) if channels_first else (b, n, d), np.nan, np.float32)
    lib.model_three_interpolate(np_ptr(feat), np_ptr(idx), np_ptr(weight), np_ptr(out), int(channels_first), b, n, s, d)
    return out


def model_bwd(lib, grad, idx, weight, s, channels_first):
    grad, idx, weight = np.ascontiguousarray(grad, np.float32), np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(weight, np.float32)
    b, n = idx.shape[:2]
    d = grad.shape[1] if channels_first else grad.shape[2]
    out = np.full((b, d, s) if channels_first else (b, s, d), np.nan, np.float32)
    lib.model_three_interpolate_bwd(np_ptr(grad), np_ptr(idx), np_ptr(weight), np_ptr(out), int(channels_first), b, n, s, d)
    return out


def test_host_model_on_g24(model, g24_cases):
    check_against_g24(g24_cases, lambda a, k, wt: model_nn(model, a, k, wt), lambda *a: model_fwd(model, *a), lambda *a: model_bwd(model, *a))


def test_host_model_equals_the_restatement_however_the_scan_is_split(model):
    for c, want in zip(nn_shape_cases(), nn_expected()):
        for slices in (1, 2, 4):
            check_nn(c["name"], lambda a, k, wt: model_nn(model, a, k, wt, slices), c["xyz1"], c["xyz2"], want)
        b, n, s = c["xyz1"].shape[0], c["xyz1"].shape[1], c["xyz2"].shape[1]
        assert model.model_three_nn_waves_per_point(b, n, s) == waves_per_point(b, n, s), c["name"]


def test_host_model_non_finite_coordinates_keep_indices_in_range(model):
    seen = 0
    for c in nn_nonfinite_cases():
        for slices in (1, 2, 4):
            check_nn_in_range(c["name"], lambda a, k, wt: model_nn(model, a, k, wt, slices), c["xyz1"], c["xyz2"])
        seen += int((~np.isfinite(c["xyz1"]).all(-1) | np.isnan(c["xyz2"]).all((-1, -2))[:, None]).sum())
    assert seen >= 600                                                                   # rows whose list ends without a candidate


def test_host_model_interpolation_and_backward_on_the_shape_lists(model):
    for i, c in enumerate(interp_shape_cases()):
        for channels_first in (False, True):
            got, _ = check_interp(c["name"], lambda *a: model_fwd(model, *a), lambda *a: model_bwd(model, *a), c, channels_first, interp_expected32(i))
            if c["name"] == "an unknown point that is a known point":
                got = got.transpose(0, 2, 1) if channels_first else got
                own = c["feat"][0][c["idx"][0, :, 0]]
                assert (np.abs(got[0] - own) <= 1e-6 * np.abs(own)).all()
