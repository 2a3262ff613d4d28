"""farthest_point_sample, query_ball_point, index_points and sample_and_group (so3_fps_f32, so3_ball_query_f32) without a GPU: the
boundary (header, binding table, exports, argument validation, the Python names), the G22 fixture, and the kernels' device functions
compiled for the host (tests/host_model/pointnet.cpp with SO3_HOST_MODEL).

Farthest-point sampling is a chain, so its arithmetic is a definition (include/so3proj.h) and every comparison here is EXACT:
  1  the host model equals the numpy restatement of the definition (tests/pointnet_ref.py) on all of G22 and on the shape lists below;
  2  the host model equals the indices the reference's farthest_point_sample produced (G22), index for index;
  3  the host model equals the rows the reference's query_ball_point produced (G22) wherever near_boundary is false -- the reference
     takes its distances from |a|^2 + |b|^2 - 2 a.b, so a point within 1e-5 r^2 of the sphere may fall on the other side.  The mask may
     cover at most 1 % of a case's rows (re-asserted here: exclusions cannot hide a failure); inside it rows must still be ascending,
     in range and padded by their first entry.
tests/test_gpu_pointnet.py imports the shape lists and runs the same comparisons on the device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import pointnet_ref as ref
from support import boundary, build_host_model, np_ptr, on_own_thread

NEW_SYMBOLS = {"so3_fps_f32": 7, "so3_ball_query_f32": 10}
SRC = os.path.join(ROOT, "tests", "host_model", "pointnet.cpp")
FPS_KERNELS = {(1, 256), (2, 256), (4, 256), (8, 256), (4, 1024), (8, 1024), (16, 1024)}      # k_fps<PPL, BLOCK>: every instantiation
FPS_GRID_CAP = 4096                  # so3proj.hip: kFpsMaxGrid
BALL_WAVES_PER_BLOCK = 4


# ---- the shape lists, shared with tests/test_gpu_pointnet.py ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fps_shape_cases():
    """Dicts (name, xyz (B,N,3) float32, start (B,) int64, npoint).  N = 1; around the wave (64) and the block (256); just below, at
    and above every switch of the dispatch (256, 512, 1024, 2048 | 4096, 8192, 16384 points); npoint > N; start at N - 1; duplicated
    points and an all-equal cloud; coordinates at 1e3; a batch larger than the launch's grid."""
    rng = np.random.default_rng(2201)
    out = []

    def add(name, xyz, start, npoint):
        xyz = np.ascontiguousarray(xyz, np.float32)
        out.append({"name": name, "xyz": xyz, "start": np.broadcast_to(np.asarray(start, np.int64), (len(xyz),)).copy(), "npoint": npoint})

    for b in (1, 3):
        for npoint in (1, 3):
            add("N=1 npoint=%d B=%d" % (npoint, b), rng.standard_normal((b, 1, 3)), 0, npoint)
        for n in (63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, ref.FPS_MAX_N):
            npoint = 33 if n < 4095 else 8
            add("N=%d npoint=%d B=%d" % (n, npoint, b), rng.uniform(-1, 1, (b, n, 3)), rng.integers(0, n, b), npoint)
        add("npoint > N B=%d" % b, rng.uniform(-1, 1, (b, 5, 3)), rng.integers(0, 5, b), 9)
        add("npoint > N, N=65 B=%d" % b, rng.uniform(-1, 1, (b, 65, 3)), rng.integers(0, 65, b), 70)
        add("start = N - 1 B=%d" % b, rng.uniform(-1, 1, (b, 300, 3)), 299, 20)
        dup = rng.uniform(-1, 1, (b, 40, 3))
        add("duplicated points B=%d" % b, np.concatenate([dup, dup[:, ::-1], dup], 1), rng.integers(0, 120, b), 60)
        add("all equal B=%d" % b, np.full((b, 70, 3), 0.25), 37, 6)
        add("coordinates at 1e3 B=%d" % b, rng.uniform(-1e3, 1e3, (b, 500, 3)), rng.integers(0, 500, b), 40)
    big = FPS_GRID_CAP + 3
    add("B=%d beyond the grid" % big, rng.uniform(-1, 1, (big, 7, 3)), rng.integers(0, 7, big), 4)
    return out


@functools.lru_cache(maxsize=None)
def ball_shape_cases():
    """Dicts (name, xyz (B,N,3), centres (B,S,3), radius, nsample).  Centre 0 of every cloud is the cloud's point 0, the last centre is
    far away (no hit); radius 0 (the centre itself), balls with fewer, exactly as many and more points than nsample, a ball that holds
    the whole cloud; S is never a multiple of the waves per block; N around the wave, the scan's unroll (256) and beyond it."""
    rng = np.random.default_rng(2202)
    out = []

    def add(name, xyz, centres, radius, nsample):
        out.append({"name": name, "xyz": np.ascontiguousarray(xyz, np.float32), "centres": np.ascontiguousarray(centres, np.float32),
                    "radius": float(radius), "nsample": int(nsample)})

    for b in (1, 3):
        for n in (1, 63, 64, 65, 200, 256, 257, 600):
            xyz = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
            for s in (1, 5, 7):
                assert s % BALL_WAVES_PER_BLOCK
                centres = rng.uniform(0, 1, (b, s, 3)).astype(np.float32)
                centres[:, 0] = xyz[:, 0]
                if s > 1:
                    centres[:, -1] = 100.0
                for nsample in sorted({1, 5, n, n + 3}):
                    for radius in (0.0, 0.25, 0.6, 5.0):
                        add("N=%d S=%d K=%d r=%g B=%d" % (n, s, nsample, radius, b), xyz, centres, radius, nsample)
    xyz = rng.uniform(0, 1, (1, 200, 3)).astype(np.float32)                      # exactly nsample points in the ball
    c = rng.uniform(0.3, 0.7, (1, 1, 3)).astype(np.float32)
    d = np.sort(ref.dist2(xyz[0][None], c[0], np.float64)[0])
    add("exactly nsample", xyz, c, np.sqrt((d[4] + d[5]) / 2), 5)
    s = 32 * 256 * BALL_WAVES_PER_BLOCK // 3 + 11                                # more centres than the launch has waves on 256 compute units
    add("B*S beyond the grid", rng.uniform(0, 1, (3, 63, 3)), rng.uniform(0, 1, (3, s, 3)), 0.3, 5)
    return out


@functools.lru_cache(maxsize=None)
def fps_expected():
    return [ref.fps(c["xyz"], c["npoint"], c["start"]) for c in fps_shape_cases()]


@functools.lru_cache(maxsize=None)
def ball_expected():
    return [ref.ball_query(c["radius"], c["nsample"], c["xyz"], c["centres"]) for c in ball_shape_cases()]


def test_the_shape_lists_hold_what_they_promise():
    want = fps_expected()
    for c, idx in zip(fps_shape_cases(), want):
        if c["name"].startswith("all equal"):
            assert (idx[:, 0] == 37).all() and (idx[:, 1:] == 0).all()                   # the lowest index among equal values
        if c["name"].startswith("npoint > N"):
            n = c["xyz"].shape[1]
            assert all(sorted(r[:n]) == list(range(n)) for r in idx) and (idx[:, n:] == 0).all()
    counts = {c["name"]: cnt for c, (_, cnt) in zip(ball_shape_cases(), ball_expected())}
    assert counts["exactly nsample"].tolist() == [[5]]
    seen = set()
    for c, (idx, cnt) in zip(ball_shape_cases(), ball_expected()):
        n, k = c["xyz"].shape[1], c["nsample"]
        ref.row_properties(idx, n)
        seen |= {"fewer"} if ((cnt > 0) & (cnt < min(k, n))).any() else set()
        seen |= {"equal"} if (cnt == k).any() else set()
        seen |= {"more"} if (cnt > k).any() else set()
        seen |= {"empty"} if (cnt == 0).any() else set()
        if c["radius"] == 0.0:
            assert (cnt[:, 0] >= 1).all() and (idx[:, 0, 0] == 0).all()                  # a centre that is a cloud point holds itself
        if (c["centres"][:, -1] == 100.0).all():
            assert (cnt[:, -1] == 0).all() and (idx[:, -1] == n).all()                   # the far-away centre
    assert seen == {"fewer", "equal", "more", "empty"}


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_FPS_MAX_N (\d+)", raw).group(1)) == _lib.FPS_MAX_N == ref.FPS_MAX_N >= 16384


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    fps = lambda b, n, npoint, xyz=p, start=p, out=p: lib.so3_fps_f32(xyz, start, out, b, n, npoint, None)
    ball = lambda b, n, s, k=4, xyz=p, c=p, idx=p: lib.so3_ball_query_f32(xyz, c, 0.5, k, idx, None, b, n, s, None)
    assert fps(0, 8, 8, None, None, None) == 0 and ball(0, 8, 8, 4, None, None, None) == 0                  # B == 0: a no-op, whatever the pointers
    for b, n, npoint in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, -3, 8), (4, _lib.FPS_MAX_N + 1, 8), (4, 8, 0), (4, 8, _lib.FPS_MAX_N + 1)):
        assert fps(b, n, npoint) != 0 and b"so3_fps_f32: B/N/npoint" in err(), (b, n, npoint, err())
    big = _lib.ADD_S_MAX_N + 1
    for b, n, s, k in ((-1, 8, 8, 4), (2**62, 8, 8, 4), (4, 0, 8, 4), (4, 8, 0, 4), (4, big, 8, 4), (4, 8, big, 4), (4, 8, 8, 0), (4, 8, 8, -2)):
        assert ball(b, n, s, k) != 0 and b"so3_ball_query_f32: B/N/S/nsample" in err(), (b, n, s, k, err())
    for kw in ({"xyz": None}, {"start": None}, {"out": None}):
        assert fps(4, 8, 8, **kw) != 0 and b"so3_fps_f32: null pointer" in err(), kw
    for kw in ({"xyz": None}, {"c": None}, {"idx": None}):
        assert ball(4, 8, 8, **kw) != 0 and b"so3_ball_query_f32: null pointer" in err(), kw


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("farthest_point_sample", "query_ball_point", "index_points", "sample_and_group"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    xyz, feat = torch.zeros(2, 9, 3), torch.zeros(2, 9, 4)
    for fn in (lambda: pa.farthest_point_sample(xyz, 4), lambda: pa.farthest_point_sample(xyz, 4, start=0), lambda: pa.query_ball_point(0.5, 3, xyz, xyz[:, :2]),
               lambda: pa.query_ball_point(0.5, 3, xyz, xyz[:, :2], return_counts=True), lambda: pa.sample_and_group(4, 0.5, 3, xyz, feat, start=1)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


def test_index_points_is_the_gather_and_differentiable():
    """Plumbing in plain torch: (B,S) -> (B,S,C), (B,S,K) -> (B,S,K,C), the gradient scatters back (repeats add up)."""
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(3, 11, 5, generator=g, dtype=torch.float64, requires_grad=True)
    for shape in ((3, 4), (3, 4, 6)):
        idx = torch.randint(0, 11, shape, generator=g)
        got = pa.index_points(pts, idx)
        want = torch.stack([pts[b][idx[b]] for b in range(3)])
        assert got.shape == shape + (5,) and torch.equal(got, want)
        (grad,) = torch.autograd.grad(got.sum(), [pts])
        hits = torch.stack([torch.bincount(idx[b].reshape(-1), minlength=11) for b in range(3)]).double()
        assert torch.equal(grad, hits[..., None].expand(-1, -1, 5))
    with pytest.raises(RuntimeError, match="index_points"):
        pa.index_points(pts, torch.zeros(2, 4, dtype=torch.long))


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g22_cases():
    return ref.cases(ref.g22())


def test_g22_holds_the_cases_and_the_boundary_cap(g22_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    fps = [c for c in g22_cases if c["kind"] == "fps"]
    ball = [c for c in g22_cases if c["kind"] == "ball"]
    assert [(c["xyz"].shape[0], c["xyz"].shape[1], c["npoint"]) for c in fps] == list(ref.FPS_CASES)
    assert [(c["xyz"].shape[1], c["centres"].shape[1], c["radius"], c["nsample"]) for c in ball] == list(ref.BALL_CASES)
    for c in g22_cases:
        assert c["xyz"].dtype == np.float32 and np.isfinite(c["xyz"]).all() and np.linalg.norm(c["xyz"], axis=-1).max() <= 1.0, c["name"]     # pc_normalize
    for c in ball:
        assert np.array_equal(c["near"], ref.near_boundary(c["radius"], c["xyz"], c["centres"])), c["name"]
        assert c["near"].mean() <= ref.BOUNDARY_CAP, (c["name"], c["near"].mean())
        assert c["idx"].shape == c["near"].shape + (c["nsample"],)
        ref.row_properties(c["idx"], c["xyz"].shape[1])
        want, _ = ref.ball_query(c["radius"], c["nsample"], c["xyz"], c["centres"], np.float64)      # the generator's own assertion
        assert np.array_equal(want[~c["near"]], c["idx"][~c["near"]]), c["name"]


# ---- the checks, shared with tests/test_gpu_pointnet.py -----------------------------------------------------------------------
def check_against_g22(g22_cases, run_fps, run_ball):
    """run_fps(xyz, npoint, start) -> (B, npoint) indices; run_ball(radius, nsample, xyz, centres) -> (idx, count or None)."""
    for c in g22_cases:
        n = c["xyz"].shape[1]
        if c["kind"] == "fps":
            got = np.asarray(run_fps(c["xyz"], c["npoint"], c["start"]), np.int64)
            assert np.array_equal(got, c["idx"]), (c["name"], np.argwhere(got != c["idx"])[:4])                       # 2: the reference's sequence
            assert np.array_equal(got, ref.fps(c["xyz"], c["npoint"], c["start"])), c["name"]                        # 1: the restatement's
        else:
            got, count = run_ball(c["radius"], c["nsample"], c["xyz"], c["centres"])
            got = np.asarray(got, np.int64)
            want, want_count = ref.ball_query(c["radius"], c["nsample"], c["xyz"], c["centres"])
            assert np.array_equal(got, want), (c["name"], np.argwhere(got != want)[:4])                               # 1
            assert count is None or np.array_equal(np.asarray(count, np.int64), want_count), c["name"]
            assert c["near"].mean() <= ref.BOUNDARY_CAP, c["name"]
            keep = ~c["near"]
            assert np.array_equal(got[keep], c["idx"][keep]), (c["name"], np.argwhere((got != c["idx"]).any(-1) & keep)[:4])      # 3
            ref.row_properties(got, n)                                                                             # in the mask as well


# ---- the host model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "pointnet", SRC)
    lib.model_fps.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.model_ball_query.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_int32, ctypes.c_int32]
    lib.model_fps_shape.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.model_fps.restype = lib.model_ball_query.restype = lib.model_fps_shape.restype = None
    return lib


def model_fps(lib, xyz, npoint, start):
    xyz = np.ascontiguousarray(xyz, np.float32)
    b, n, _ = xyz.shape
    first = np.ascontiguousarray(np.broadcast_to(np.asarray(start), (b,)), np.int32)
    out = np.full((b, npoint), -1, np.int32)
    lib.model_fps(np_ptr(xyz), np_ptr(first), np_ptr(out), b, n, npoint)
    return out


def model_ball(lib, radius, nsample, xyz, centres, want_count=True):
    xyz, centres = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(centres, np.float32)
    b, n, _ = xyz.shape
    s = centres.shape[1]
    idx = np.full((b, s, min(nsample, n)), -1, np.int32)
    count = np.full((b, s), -1, np.int32) if want_count else None
    lib.model_ball_query(np_ptr(xyz), np_ptr(centres), radius, nsample, np_ptr(idx), None if count is None else np_ptr(count), b, n, s)
    return idx, count


def fps_kernel_of(lib, n):
    ppl, block = ctypes.c_int32(), ctypes.c_int32()
    lib.model_fps_shape(n, ctypes.byref(ppl), ctypes.byref(block))
    return ppl.value, block.value


def test_host_model_on_g22(model, g22_cases):
    check_against_g22(g22_cases, lambda xyz, npoint, start: model_fps(model, xyz, npoint, start),
                      lambda r, k, xyz, c: model_ball(model, r, k, xyz, c))


def test_host_model_equals_the_restatement_on_the_shape_lists(model):
    for c, want in zip(fps_shape_cases(), fps_expected()):
        assert np.array_equal(model_fps(model, c["xyz"], c["npoint"], c["start"]), want), c["name"]
    for c, (want, want_count) in zip(ball_shape_cases(), ball_expected()):
        idx, count = model_ball(model, c["radius"], c["nsample"], c["xyz"], c["centres"])
        assert np.array_equal(idx, want) and np.array_equal(count, want_count), c["name"]
        idx, _ = model_ball(model, c["radius"], c["nsample"], c["xyz"], c["centres"], want_count=False)
        assert np.array_equal(idx, want), c["name"]


def test_the_fps_shapes_reach_every_instantiation(model):
    assert {fps_kernel_of(model, c["xyz"].shape[1]) for c in fps_shape_cases()} == FPS_KERNELS
    for n, want in ((1, (1, 256)), (256, (1, 256)), (257, (2, 256)), (1024, (4, 256)), (2048, (8, 256)), (2049, (4, 1024)), (4097, (8, 1024)),
                    (8193, (16, 1024)), (ref.FPS_MAX_N, (16, 1024))):
        assert fps_kernel_of(model, n) == want, n
