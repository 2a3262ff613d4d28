"""group_points, sample_and_group_all, set_abstraction_group and set_abstraction_msg_group (so3_group_points_f32,
so3_group_points_bwd_f32) without a GPU: the boundary (header, binding table, exports, argument validation, the Python names), the G25
fixture, and the kernels' device functions compiled for the host (tests/host_model/grouping.cpp with SO3_HOST_MODEL).

  1  The forward is a definition, so it is compared EXACTLY: the host model equals the numpy restatement (tests/grouping_ref.py) bit for
     bit on G25 and on the shape list, in both layouts and both channel orders, and on G25 it equals the tensors the reference's own
     classes produced, the group_all case included.
  2  The backward's order is part of the definition: the host model equals the restatement's float32 order bit for bit; any device
     result must lie within gamma_{h-1} * sum |g| of the float64 restatement for an element with h terms (grouping_ref.py), must be
     exactly 0 where nobody selected the point, and every subset of the three outputs must give the bits of the whole.
  3  On G25 the sum of our gradient paths is compared with the reference's recorded autograd gradients (check_g25_gradients).
tests/test_gpu_grouping.py imports the shape list and the checks and runs them on the device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import grouping_ref as ref
from support import bits, boundary, build_host_model, np_ptr, on_own_thread

NEW_SYMBOLS = {"so3_group_points_f32": 13, "so3_group_points_bwd_f32": 13}
NEW_NAMES = ("group_points", "sample_and_group_all", "set_abstraction_group", "set_abstraction_msg_group")
SRC = os.path.join(ROOT, "tests", "host_model", "grouping.cpp")
GRID_CAP = 8192                      # so3proj.hip: kThreeMaxGrid
NARROW_C = 8                         # so3_device.h: kGroupNarrowC -- 3 + D up to this: k_group_bwd<., 8, 2>, above k_group_bwd<., 64, 16>
NARROW_TILE, WIDE_TILE = 1024, 128   # so3_device.h: kGroupNarrowTile, kGroupWideTile, the slots of grad_out per LDS tile
OWNERS = 64                          # so3_device.h: kGroupNarrowOwners, kGroupWideOwners, the points of a backward work item
WIDE_CHANNELS = 64                   # so3_device.h: kGroupWideChannels
FWD_CF_CHANNELS, FWD_CF_CENTRES = 16, 256      # k_group_fwd<true>: channels and centres per work item
KERNELS = ({"k_group_fwd<%s>" % t for t in ("true", "false")} | {"k_group_centres_bwd<%s>" % t for t in ("true", "false")}
           | {"k_group_bwd<%s, %s>" % (t, w) for t in ("true", "false") for w in ("8, 2", "64, 16")})
LAYOUTS = [(cf, ff) for cf in (False, True) for ff in (False, True)]


def bwd_kernel(d, channels_first):
    return "k_group_bwd<%s, %s>" % ("true" if channels_first else "false", "8, 2" if 3 + d <= NARROW_C else "64, 16")


# ---- the shape list, shared with tests/test_gpu_grouping.py --------------------------------------------------------------------------
def ball_rows(rng, b, n, s, k):
    """idx (B, S, K) exactly as query_ball_point pads its rows: ascending distinct hits, then the first hit repeated."""
    idx = np.zeros((b, s, k), np.int64)
    for bb in range(b):
        for ss in range(s):
            m = rng.integers(1, min(n, k) + 1)
            hits = np.sort(rng.choice(n, m, replace=False))
            idx[bb, ss, :m], idx[bb, ss, m:] = hits, hits[0]
    return idx


@functools.lru_cache(maxsize=None)
def shape_cases():
    """Dicts (name, xyz (B,N,3), centres (B,S,3), feat (B,N,D) channel-last or None, idx (B,S,K) int64, grad (B,S,K,3+D) channel-last);
    every layout and channel order is run from them.  B in {1, 3} and one batch beyond the grid cap of every launch; N in
    {1, 63, 64, 65, 257} (the 64 points of a backward work item, the 16 of a wave); S in {1, 3, 63, 64, 65} and around the 256 centres
    of a channel-first forward work item; K in {1, 5, 64, 65, 130}; D in {0, 1, 3, 63, 64, 65} plus 5 | 6 (the narrow / wide switch of
    the backward), 13 | 14 (the 16 channels of a channel-first forward work item), 61 | 62 (the wide kernel's 64-channel chunk) and 130
    (above every chunk: three of them); S * K below, at and above the LDS tile of both backward kernels (1024 and 128 slots)."""
    rng = np.random.default_rng(2501)
    out = []

    def add(name, b, n, s, k, d, idx=None, scale=1.0):
        xyz, centres = rng.uniform(-scale, scale, (b, n, 3)), rng.uniform(-scale, scale, (b, s, 3))
        idx = ball_rows(rng, b, n, s, k) if idx is None else idx
        out.append({"name": name, "xyz": xyz.astype(np.float32), "centres": centres.astype(np.float32),
                    "feat": rng.standard_normal((b, n, d)).astype(np.float32) if d else None, "idx": np.ascontiguousarray(idx, np.int64),
                    "grad": rng.standard_normal((b, s, k, 3 + d)).astype(np.float32)})

    ns, ss, ks, ds = (1, 63, 64, 65, 257), (1, 3, 63, 64, 65), (1, 5, 64, 65, 130), (0, 1, 3, 63, 64, 65)
    for i in range(6):                                                   # every value of every axis, each with changing neighbours
        b, n, s, k, d = (1, 3)[i % 2], ns[i % 5], ss[(i + 1) % 5], ks[(i + 2) % 5], ds[i]
        add("B=%d N=%d S=%d K=%d D=%d" % (b, n, s, k, d), b, n, s, k, d)
    for n, s, k in ((257, 65, 130), (64, 63, 64), (65, 64, 1)):
        add("B=3 N=%d S=%d K=%d D=3" % (n, s, k), 3, n, s, k, 3)
    for d in (5, 6, 13, 14, 61, 62, 130):
        add("B=1 N=65 S=3 K=5 D=%d (channel switches)" % d, 1, 65, 3, 5, d)
    for s in (FWD_CF_CENTRES - 1, FWD_CF_CENTRES, FWD_CF_CENTRES + 1):
        add("B=1 N=9 S=%d K=3 D=1 (forward work item)" % s, 1, 9, s, 3, 1)
    for s, k in ((3, 341), (64, 16), (25, 41), (1, 2 * NARROW_TILE + 7)):
        add("B=1 N=70 S=%d K=%d D=2 (narrow tile, %d slots)" % (s, k, s * k), 1, 70, s, k, 2)
    for s, k in ((1, 127), (64, 2), (3, 43), (5, 77)):
        add("B=1 N=70 S=%d K=%d D=9 (wide tile, %d slots)" % (s, k, s * k), 1, 70, s, k, 9)
    big = GRID_CAP + 3
    add("B=%d beyond every grid, narrow" % big, big, 2, 2, 1, 1)
    add("B=%d beyond every grid, wide (four rows per forward block)" % big, big, 3, 1, 5, 65)
    n, s, k = 90, 7, 11
    one = np.full((2, s, k), 17, np.int64)
    one[1] = rng.integers(2, n, (s, k))                                  # cloud 1: points 0 and 1 are selected by nobody
    for d in (3, 20):
        add("h = S*K hits and none D=%d" % d, 2, n, s, k, d, one)
    bad = ball_rows(rng, 3, 40, 9, 6)
    bad[0, 2], bad[1, 5], bad[2] = 40, 40, 40                            # empty balls, as query_ball_point writes them; a whole cloud of them
    bad[0, 4, 1::2], bad[1, 0, :3], bad[1, 8, 5] = -1, -7, 2 ** 31 - 1   # negative and far indices mixed with valid ones
    for d in (0, 4, 12):
        add("idx == N, negative and valid mixed D=%d" % d, 3, 40, 9, 6, d, bad)
    for d in (3, 10):
        add("coordinates at 1e3 D=%d" % d, 2, 100, 20, 8, d, scale=1e3)
    return out


def in_layout(c, channels_first):
    """(feat, grad) of a case in the asked layout, contiguous."""
    if not channels_first:
        return c["feat"], c["grad"]
    return (None if c["feat"] is None else np.ascontiguousarray(c["feat"].transpose(0, 2, 1))), np.ascontiguousarray(c["grad"].transpose(0, 3, 2, 1))


@functools.lru_cache(maxsize=None)
def expected(i, channels_first, features_first):
    """(forward, float32-order backward, float64 backward) of shape case i: computed once, shared, read-only."""
    c = shape_cases()[i]
    feat, grad = in_layout(c, channels_first)
    n = c["xyz"].shape[1]
    fwd = ref.forward(c["xyz"], c["centres"], feat, c["idx"], channels_first, features_first)
    fwd.setflags(write=False)
    return fwd, ref.backward(grad, c["idx"], n, channels_first, features_first, np.float32), ref.backward(grad, c["idx"], n, channels_first, features_first, np.float64)


def test_the_shape_list_holds_what_it_promises():
    cs = shape_cases()
    for axis, vals in (("B", {1, 3}), ("N", {1, 63, 64, 65, 257}), ("S", {1, 3, 63, 64, 65, 255, 256, 257}), ("K", {1, 5, 64, 65, 130})):
        seen = {{"B": c["idx"].shape[0], "N": c["xyz"].shape[1], "S": c["idx"].shape[1], "K": c["idx"].shape[2]}[axis] for c in cs}
        assert vals <= seen, (axis, vals - seen)
    ds = {0 if c["feat"] is None else c["feat"].shape[2] for c in cs}
    assert {0, 1, 3, 5, 6, 13, 14, 61, 62, 63, 64, 65, 130} <= ds and max(ds) + 3 > 2 * WIDE_CHANNELS
    assert max(c["idx"].shape[0] for c in cs) > GRID_CAP
    for tile, narrow in ((NARROW_TILE, True), (WIDE_TILE, False)):
        slots = {c["idx"].shape[1] * c["idx"].shape[2] for c in cs if ((0 if c["feat"] is None else c["feat"].shape[2]) + 3 <= NARROW_C) == narrow}
        assert {tile - 1, tile, tile + 1} <= slots and max(slots) > 2 * tile, (tile, sorted(slots))
    for c in cs:
        if c["name"].startswith("h = S*K"):
            h = ref.backward(c["grad"], c["idx"], 90)["hits"]
            assert h[0, 17] == 77 and h[0].sum() == 77 and (h[1, :2] == 0).all()
        if c["name"].startswith("idx == N"):
            ok = ref.valid(c["idx"], 40)
            assert not ok[2].any() and not ok[0, 2].any() and 0 < ok[0, 4].sum() < 6 and (c["idx"] < 0).any()
        if "B=1 N=65 S=3 K=5" in c["name"]:                               # rows as query_ball_point pads them
            assert all((row[np.argmax(np.diff(row) <= 0) + 1:] == row[0]).all() for row in c["idx"][0] if (np.diff(row) <= 0).any())


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_GROUP_MAX_K (\d+)", raw).group(1)) == _lib.GROUP_MAX_K == 65536


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    fwd = lambda b, n, s, k, d, ff=0, cf=0, x=p, c=p, f=p, i=p, o=p: lib.so3_group_points_f32(x, c, f, i, o, ff, cf, b, n, s, k, d, None)
    bwd = lambda b, n, s, k, d, ff=0, cf=0, g=p, i=p, x=p, c=p, f=p: lib.so3_group_points_bwd_f32(g, i, x, c, f, ff, cf, b, n, s, k, d, None)
    for cf in (0, 1):                                                                             # B == 0: a no-op, whatever the pointers
        assert fwd(0, 8, 8, 4, 2, 0, cf, None, None, None, None, None) == 0 and bwd(0, 8, 8, 4, 2, 1, cf, None, None, None, None, None) == 0
    big = _lib.ADD_S_MAX_N + 1
    dims = ((-1, 8, 8, 4, 2), (2 ** 62, 8, 8, 4, 2), (4, 0, 8, 4, 2), (4, -3, 8, 4, 2), (4, big, 8, 4, 2), (4, 8, 0, 4, 2), (4, 8, -1, 4, 2), (4, 8, big, 4, 2),
            (4, 8, 8, 0, 2), (4, 8, 8, -1, 2), (4, 8, 8, _lib.GROUP_MAX_K + 1, 2), (4, 8, 8, 4, -1), (4, 8, 8, 4, _lib.THREE_MAX_D + 1))
    for args in dims:
        for fn, name in ((fwd, b"so3_group_points_f32: B/N/S/K/D"), (bwd, b"so3_group_points_bwd_f32: B/N/S/K/D")):
            for cf in (0, 1):
                assert fn(*args, 0, cf) != 0 and name in err(), (args, err())
    for kw in ({"x": None}, {"c": None}, {"f": None}, {"i": None}, {"o": None}):
        assert fwd(4, 8, 8, 4, 2, **kw) != 0 and b"so3_group_points_f32: null pointer" in err(), kw
    for kw in ({"x": None}, {"c": None}, {"i": None}, {"o": None}):                               # D == 0: feat is not looked at
        assert fwd(4, 8, 8, 4, 0, f=None, **kw) != 0 and b"so3_group_points_f32: null pointer" in err(), kw
    for kw in ({"g": None}, {"i": None}):                                                         # the three outputs may be null
        assert bwd(4, 8, 8, 4, 2, **kw) != 0 and b"so3_group_points_bwd_f32: null pointer" in err(), kw


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in NEW_NAMES:
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    xyz, new_xyz, pts = torch.zeros(2, 9, 3), torch.zeros(2, 4, 3), torch.zeros(2, 9, 5)
    idx = torch.zeros(2, 4, 6, dtype=torch.long)
    for fn in (lambda: pa.group_points(xyz, new_xyz, pts, idx), lambda: pa.group_points(xyz, new_xyz, None, idx),
               lambda: pa.group_points(xyz, new_xyz, pts.transpose(1, 2), idx, channels_first=True, features_first=True),
               lambda: pa.set_abstraction_group(4, 0.5, 6, xyz.transpose(1, 2), pts.transpose(1, 2)),
               lambda: pa.set_abstraction_group(None, None, None, xyz.transpose(1, 2), None, group_all=True),
               lambda: pa.set_abstraction_msg_group(4, [0.5, 1.0], [6, 8], xyz.transpose(1, 2), pts.transpose(1, 2))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


def test_sample_and_group_all_is_the_references(g25):
    """Plain torch, so it runs here: the reference's recorded group_all tensor, bit for bit, and its zeros."""
    import poseestimation_amd as pa
    xyz, pts = torch.from_numpy(g25["xyz_all"]), torch.from_numpy(g25["points_all"])
    new_xyz, new_points = pa.sample_and_group_all(xyz, pts)
    assert new_xyz.shape == (2, 1, 3) and not new_xyz.any() and new_points.shape == (2, 1, ref.N_ALL, 3 + ref.D_FIXTURE)
    assert np.array_equal(new_points.permute(0, 3, 2, 1).numpy().view(np.uint32), g25["all"]["t"].view(np.uint32))
    assert np.array_equal(g25["all"]["new_xyz"], np.zeros((2, 3, 1), np.float32))
    assert torch.equal(pa.sample_and_group_all(xyz, None)[1], xyz.view(2, 1, ref.N_ALL, 3))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g25():
    return ref.cases(ref.g25())


def test_g25_holds_the_cases_and_the_cap(g25):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    n, s, d = ref.N_FIXTURE, ref.S_FIXTURE, ref.D_FIXTURE
    assert g25["xyz"].shape == (2, n, 3) and g25["points"].shape == (2, n, d) and g25["xyz"].dtype == g25["points"].dtype == np.float32
    assert np.linalg.norm(g25["xyz"], axis=-1).max() <= 1.0 + 1e-6                                                   # unit radius
    for tag, ks in (("sa", [ref.RADII[1][1]]), ("msg", [k for _, k in ref.RADII])):
        c = g25[tag]
        assert c["fps"].shape == (2, s) and c["new_xyz"].shape == (2, 3, s) and c["grad_xyz"].shape == (2, 3, n) and c["grad_points"].shape == (2, d, n)
        assert np.array_equal(c["new_xyz"].transpose(0, 2, 1), np.stack([x[i] for x, i in zip(g25["xyz"], c["fps"])]))
        assert all(len(set(row)) == s for row in c["fps"])
        for k, idx, t in zip(ks, c["idx"], c["t"]):
            assert idx.shape == (2, s, k) and t.shape == (2, 3 + d, k, s) and t.dtype == np.float32
            assert idx.min() >= 0 and idx.max() < n                                                                 # no empty ball: nothing is masked
            assert (idx[:, :, 0] <= c["fps"]).all()                                                                 # every centre hits itself
    assert g25["all"]["t"].shape == (2, 3 + d, ref.N_ALL, 1)


# ---- the checks, shared with tests/test_gpu_grouping.py ------------------------------------------------------------------------------
def f32_bits(a):
    """support.bits of what must be float32 already: bits() alone would round a float64 result and then find it equal."""
    assert np.asarray(a).dtype == np.float32, np.asarray(a).dtype
    return bits(a)


def check_forward(name, run_fwd, xyz, centres, feat, idx, channels_first, features_first, want=None):
    """run_fwd(xyz, centres, feat, idx, channels_first, features_first) -> out.  Bit-equal to the restatement."""
    want = ref.forward(xyz, centres, feat, idx, channels_first, features_first) if want is None else want
    got = np.asarray(run_fwd(xyz, centres, feat, idx, channels_first, features_first))
    assert got.shape == want.shape and np.array_equal(f32_bits(got), f32_bits(want)), (name, channels_first, features_first, np.argwhere(f32_bits(got) != f32_bits(want))[:4])
    bad = ~ref.valid(idx, xyz.shape[1])
    if bad.any():
        slots = got.transpose(0, 3, 2, 1) if channels_first else got
        assert not f32_bits(slots[bad]).any(), name                                   # +0 in every channel of an invalid slot
    return got


def check_backward(name, run_bwd, grad, idx, n, d, channels_first, features_first, exact, want32=None, want64=None, subsets=True):
    """run_bwd(grad, idx, n, d, channels_first, features_first, (want_xyz, want_centres, want_feat)) -> (grad_xyz, grad_centres, grad_feat),
    None where not requested; buffers start as NaN.  exact: the float32 order bit for bit beside the bound (the host model and the device both run with it)."""
    want32 = ref.backward(grad, idx, n, channels_first, features_first, np.float32) if want32 is None else want32
    want64 = ref.backward(grad, idx, n, channels_first, features_first, np.float64) if want64 is None else want64
    bound = ref.bounds(want64, channels_first)
    keys = ("grad_xyz", "grad_centres", "grad_feat")
    got = dict(zip(keys, run_bwd(grad, idx, n, d, channels_first, features_first, (True, True, d > 0))))
    hits = want64["hits"]
    for key in keys:
        if key == "grad_feat" and d == 0:
            assert got[key] is None
            continue
        g = np.asarray(got[key])
        assert g.dtype == np.float32 and g.shape == want64[key].shape, (name, key, g.shape)
        assert np.isfinite(g).all(), (name, key)                                   # written everywhere
        err = np.abs(g.astype(np.float64) - want64[key])
        assert (err <= bound[key]).all(), (name, key, channels_first, features_first, err.max(), (err - bound[key]).max())
        if exact:
            assert np.array_equal(f32_bits(g), f32_bits(want32[key])), (name, key, channels_first, features_first)
        if key == "grad_centres":
            assert not f32_bits(g[want64["slots"] == 0]).any(), name                   # a row without a valid slot: +0
        else:
            none = hits == 0
            untouched = np.broadcast_to(none[:, None, :] if key == "grad_feat" and channels_first else none[:, :, None], g.shape)
            assert not f32_bits(g[untouched]).any(), (name, key)                       # exactly +0 (and written: the buffers start as NaN)
    if subsets:
        for sel in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
            if sel[2] and d == 0:
                continue
            alone = run_bwd(grad, idx, n, d, channels_first, features_first, sel)
            for key, asked, a in zip(keys, sel, alone):
                assert (a is not None) == asked, (name, sel)
                if asked:
                    assert np.array_equal(f32_bits(a), f32_bits(got[key])), (name, key, sel)
    return got


def check_shape_case(i, run_fwd, run_bwd, exact, layouts=LAYOUTS):
    c = shape_cases()[i]
    n, d = c["xyz"].shape[1], 0 if c["feat"] is None else c["feat"].shape[2]
    for cf, ff in layouts:
        feat, grad = in_layout(c, cf)
        fwd, w32, w64 = expected(i, cf, ff)
        check_forward(c["name"], run_fwd, c["xyz"], c["centres"], feat, c["idx"], cf, ff, fwd)
        check_backward(c["name"], run_bwd, grad, c["idx"], n, d, cf, ff, exact, w32, w64, subsets=c["idx"].shape[0] <= 3)


def check_g25_forward(g25, run_fwd):
    """Given the reference's recorded idx, the output equals the restatement AND the reference's recorded tensor bit for bit, in both
    layouts (the channel-last one is the recorded tensor permuted back) and in both channel orders (the single-scale layer puts the
    coordinates first, the Msg layer the features), and so does the group_all case (zero centres, idx = 0 .. N-1, S = 1, K = N)."""
    xyz, pts = g25["xyz"], g25["points"]
    for tag, ff in (("sa", False), ("msg", True)):
        c = g25[tag]
        centres = np.ascontiguousarray(c["new_xyz"].transpose(0, 2, 1))
        for idx, t in zip(c["idx"], c["t"]):
            for cf in (False, True):
                feat = np.ascontiguousarray(pts.transpose(0, 2, 1)) if cf else pts
                got = check_forward("G25 " + tag, run_fwd, xyz, centres, feat, idx, cf, ff)
                assert np.array_equal(f32_bits(got if cf else got.transpose(0, 3, 2, 1)), f32_bits(t)), (tag, cf)
    a = g25["all"]
    idx = np.broadcast_to(np.arange(ref.N_ALL), (2, 1, ref.N_ALL))
    got = check_forward("G25 group_all", run_fwd, g25["xyz_all"], np.zeros((2, 1, 3), np.float32), np.ascontiguousarray(g25["points_all"].transpose(0, 2, 1)),
                        idx, True, False)
    assert np.array_equal(f32_bits(got), f32_bits(a["t"]))


def check_g25_gradients(g25, run_bwd, exact):
    """The reference's recorded autograd gradients of sum_i (T_i * G_i).sum() against the sum of our gradient paths, added in float64.

    Into points one path per radius arrives (the gathered features), into xyz two per radius: the gathered coordinates (grad_xyz) and,
    because new_xyz = xyz[fps], the centre's -sum over k (grad_centres, placed at the centre's own point).  Every path is a sum of
    float32 terms g; with h terms and their magnitudes mag = sum |g|, ANY float32 summation order lies within gamma_{h-1} * mag of the
    exact sum -- ours (checked against the float64 restatement in check_backward) and the reference's (index_put_ with accumulate, and
    sum(2) for the centre) alike.  So |ours - reference| <= 2 * sum_paths gamma_{h_p - 1} * mag_p  for the paths themselves.  The
    reference then adds its P paths in float32, P - 1 roundings of a partial result no larger than M = sum_paths (mag_p + bound_p):
    one rounding u * M where two paths meet.  We add ours in float64, which adds nothing.  group_all has one path with one term per
    element: the gradient is G itself, exactly."""
    n, d = ref.N_FIXTURE, ref.D_FIXTURE
    for tag, ff in (("sa", False), ("msg", True)):
        c = g25[tag]
        for cf in (False, True):
            total_x, tol_x, mag_x, paths_x = np.zeros((2, n, 3)), np.zeros((2, n, 3)), np.zeros((2, n, 3)), 0
            total_f, tol_f, mag_f = np.zeros((2, n, d)), np.zeros((2, n, d)), np.zeros((2, n, d))
            for i, (idx, t) in enumerate(zip(c["idx"], c["t"])):
                g = ref.seeded_g(i, t.shape)                                        # (B, C, K, S), the reference's layout
                grad = g if cf else np.ascontiguousarray(g.transpose(0, 3, 2, 1))
                got = check_backward("G25 " + tag, run_bwd, grad, idx, n, d, cf, ff, exact)
                want = ref.backward(grad, idx, n, cf, ff, np.float64)
                bound = ref.bounds(want, cf)
                tr = (lambda a: a.transpose(0, 2, 1)) if cf else (lambda a: a)
                total_f += tr(got["grad_feat"]).astype(np.float64)
                tol_f += 2 * tr(bound["grad_feat"])
                mag_f += tr(want["mag_feat"]) + tr(bound["grad_feat"])
                total_x += got["grad_xyz"].astype(np.float64)
                tol_x += 2 * bound["grad_xyz"]
                mag_x += want["mag_xyz"] + bound["grad_xyz"]
                for b in range(2):                                                  # new_xyz = xyz[fps]: distinct points (asserted above)
                    total_x[b, c["fps"][b]] += got["grad_centres"][b].astype(np.float64)
                    tol_x[b, c["fps"][b]] += 2 * bound["grad_centres"][b]
                    mag_x[b, c["fps"][b]] += want["mag_centres"][b] + bound["grad_centres"][b]
                paths_x += 2
            paths_f = len(c["idx"])
            err_x = np.abs(total_x - c["grad_xyz"].transpose(0, 2, 1))
            err_f = np.abs(total_f - c["grad_points"].transpose(0, 2, 1))
            lim_x, lim_f = tol_x + (paths_x - 1) * ref.U * mag_x, tol_f + (paths_f - 1) * ref.U * mag_f
            assert (err_x <= lim_x).all(), (tag, cf, err_x.max(), (err_x - lim_x).max())
            assert (err_f <= lim_f).all(), (tag, cf, err_f.max(), (err_f - lim_f).max())
            assert err_x.max() < 1e-4 and err_f.max() < 1e-4 and np.abs(c["grad_xyz"]).max() > 1      # the bounds are not vacuous
    a = g25["all"]
    g = ref.seeded_g(0, a["t"].shape)
    idx = np.broadcast_to(np.arange(ref.N_ALL), (2, 1, ref.N_ALL))
    got = check_backward("G25 group_all", run_bwd, g, idx, ref.N_ALL, d, True, False, exact)
    assert np.array_equal(f32_bits(got["grad_xyz"].transpose(0, 2, 1)), f32_bits(a["grad_xyz"])) and np.array_equal(f32_bits(got["grad_feat"]), f32_bits(a["grad_points"]))
    assert np.array_equal(f32_bits(got["grad_xyz"].transpose(0, 2, 1)), f32_bits(g[:, :3, :, 0]))


# ---- the host model -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "grouping", SRC)
    lib.model_group_points.argtypes = lib.model_group_points_bwd.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 + [ctypes.c_int64] + [ctypes.c_int32] * 4
    lib.model_group_points.restype = lib.model_group_points_bwd.restype = None
    lib.model_group_bwd_narrow.argtypes, lib.model_group_bwd_narrow.restype = [ctypes.c_int32], ctypes.c_int32
    return lib


def model_fwd(lib, xyz, centres, feat, idx, channels_first, features_first):
    xyz, centres, idx = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(centres, np.float32), np.ascontiguousarray(idx, np.int32)
    feat = None if feat is None else np.ascontiguousarray(feat, np.float32)
    b, n, s, k = xyz.shape[0], xyz.shape[1], idx.shape[1], idx.shape[2]
    d = 0 if feat is None else feat.shape[1 if channels_first else 2]
    out = np.full((b, 3 + d, k, s) if channels_first else (b, s, k, 3 + d), np.nan, np.float32)
    lib.model_group_points(np_ptr(xyz), np_ptr(centres), np_ptr(feat), np_ptr(idx), np_ptr(out), int(features_first), int(channels_first), b, n, s, k, d)
    return out


def model_bwd(lib, grad, idx, n, d, channels_first, features_first, sel):
    grad, idx = np.ascontiguousarray(grad, np.float32), np.ascontiguousarray(idx.astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1), np.int32)
    b, s, k = idx.shape
    gx = np.full((b, n, 3), np.nan, np.float32) if sel[0] else None
    gc = np.full((b, s, 3), np.nan, np.float32) if sel[1] else None
    gf = np.full((b, d, n) if channels_first else (b, n, d), np.nan, np.float32) if sel[2] and d else None
    lib.model_group_points_bwd(np_ptr(grad), np_ptr(idx), np_ptr(gx), np_ptr(gc), np_ptr(gf), int(features_first), int(channels_first), b, n, s, k, d)
    return gx, gc, gf


def test_host_model_on_g25(model, g25):
    check_g25_forward(g25, lambda *a: model_fwd(model, *a))
    check_g25_gradients(g25, lambda *a: model_bwd(model, *a), exact=True)


@pytest.mark.parametrize("i", range(len(shape_cases())), ids=lambda i: shape_cases()[i]["name"].replace(" ", "_"))
def test_host_model_equals_the_restatement_on_the_shape_list(model, i):
    check_shape_case(i, lambda *a: model_fwd(model, *a), lambda *a: model_bwd(model, *a), exact=True)
    c = shape_cases()[i]
    d = 0 if c["feat"] is None else c["feat"].shape[2]
    assert model.model_group_bwd_narrow(d) == (1 if 3 + d <= NARROW_C else 0)
