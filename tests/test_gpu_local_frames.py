"""local_frames and estimate_normals on the GPU: the covariance bit for bit against tests/local_frames_ref.py's cov32 and the eigen
stage under its judges, through the Python surface and through the raw C ABI into NaN-pre-filled, guarded buffers -- G29, every
launch geometry (K, N around a wave's and a workgroup's queries, B, a batch above the grid cap), each optional output left out, a
shared cloud, int32 and int64 indices and lengths, indices straight from knn_points, knn_group's search and query_ball_point, the
power-of-two property, repeatability, the reversed batch, a NaN cloud, sign ties and a viewpoint exactly in the plane,
replay from a graph, estimate_normals, the warning, the surface's errors, and the speed condition against the torch spelling."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import local_frames_ref as ref
from support import bits, dev, guarded, guards_intact, ptr, to_device  # noqa: F401
import test_local_frames_host as host

pytestmark = pytest.mark.gpu
WIDTHS = (6, 3, 3, 9)                # cov, eigenvalues, normals, frames
ALL = (True, True, True, True)


@pytest.fixture(scope="module")
def g29_cases():
    return ref.cases(ref.g29())


def make_case(name, Y, idx, xl=None, yl=None, view=None):
    """A fresh case in the fixture's layout: cov32 and frames64 computed here, once."""
    Y, idx = np.ascontiguousarray(Y, np.float32), np.ascontiguousarray(idx, np.int32)
    c = {"name": name, "family": "fresh", "Y": Y, "idx": idx, "x_lengths": xl, "y_lengths": yl, "viewpoint": view,
         "cov32": ref.cov32(Y, idx, xl, yl), "ref64": ref.frames64(Y, idx, xl, yl), "m": Y.shape[-2]}
    c["b"], c["n"], c["K"] = idx.shape
    return c


def abi_run(c, dev, want=ALL, shared=False):
    """The raw C ABI into NaN-pre-filled buffers with GUARD elements in front of and behind each output.  -> the outputs as numpy
    arrays, None where not wanted."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, m, K = c["b"], c["n"], c["m"], c["K"]
    Yd, id_, vd = to_device(c["Y"], dev), to_device(c["idx"], dev, np.int32), to_device(c["viewpoint"], dev)
    xld, yld = to_device(c["x_lengths"], dev, np.int32), to_device(c["y_lengths"], dev, np.int32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    whole, outs = zip(*(guarded((b * n * w,), float("nan"), torch.float32, dev) if flag else (None, None) for flag, w in zip(want, WIDTHS)))
    _lib.check(lib.so3_local_frames_f32(ptr(Yd), 0 if shared else 3 * m, ptr(id_), ptr(xld), ptr(yld), ptr(vd), *(ptr(o) for o in outs), K, b, n, m, st),
               "so3_local_frames_f32")
    assert lib.so3_last_kernel().decode() == "k_local_frames"
    torch.cuda.synchronize()
    for t in whole:
        assert t is None or guards_intact(t, float("nan")), "a guard was written"
    return tuple(None if o is None else o.view(b, n, w).cpu().numpy() for o, w in zip(outs, WIDTHS))


def surface_run(c, dev, long=False, shared=False):
    import poseestimation_amd as pa
    itype = np.int64 if long else np.int32
    Y = to_device(c["Y"][0] if shared else c["Y"], dev)
    lam, frames, cov = pa.local_frames(Y, to_device(c["idx"], dev, itype), to_device(c["x_lengths"], dev, itype), to_device(c["y_lengths"], dev, itype),
                                       to_device(c["viewpoint"], dev), return_covariance=True)
    b, n = c["b"], c["n"]
    assert lam.shape == (b, n, 3) and frames.shape == cov.shape == (b, n, 3, 3) and lam.dtype == frames.dtype == cov.dtype == torch.float32
    assert not (lam.requires_grad or frames.requires_grad or cov.requires_grad) and torch.equal(cov, cov.transpose(-1, -2))
    frames = frames.cpu().numpy()
    cov6 = cov.reshape(b, n, 9)[..., [0, 1, 2, 4, 5, 8]].cpu().numpy()
    return cov6, lam.cpu().numpy(), np.ascontiguousarray(frames[..., :, 0]), frames.reshape(b, n, 9)


def same_bits(a, b_):
    return all((u is None and v is None) or np.array_equal(bits(u), bits(v)) for u, v in zip(a, b_))


# ---- G29 --------------------------------------------------------------------------------------------------------------------
def test_g29_through_the_c_abi(dev, g29_cases):
    worst = host.check_against_g29(g29_cases, lambda c: abi_run(c, dev), "abi")
    print("device over G29, in units of u t (orth: u):", {k: round(v, 2) for k, v in sorted(worst.items())})


def test_g29_through_the_python_surface(dev, g29_cases):
    host.check_against_g29(g29_cases, lambda c: surface_run(c, dev), "surface")
    some = [c for c in g29_cases if c["family"] in ("mixed", "ragged", "view", "flat")]              # int64 indices and lengths
    host.check_against_g29(some, lambda c: surface_run(c, dev, long=True), "surface int64")


def test_each_optional_output_left_out(dev, g29_cases):
    for name in ("blob_257x300x16", "ragged", "view_outside"):
        c = next(c for c in g29_cases if c["name"] == name)
        full = abi_run(c, dev)
        for drop in range(4):
            want = tuple(k != drop for k in range(4))
            assert same_bits(abi_run(c, dev, want), tuple(o if w else None for o, w in zip(full, want))), (name, drop)
        for only in range(4):                                                                        # each alone; normals alone is estimate_normals' call
            want = tuple(k == only for k in range(4))
            assert same_bits(abi_run(c, dev, want), tuple(o if w else None for o, w in zip(full, want))), (name, only)


# ---- every launch geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_every_k_and_n(dev, b):
    """K: odd values put a row's indices at 4-byte alignment only.  N: around a wave's (64) and a workgroup's (256) queries."""
    rng = np.random.default_rng(2910 + b)
    m = 70
    Y = ref.blob(rng, b, m)
    for K in (1, 2, 3, 4, 5, 16, 63, 64):
        for n in ((1, 65) if K not in (5, 16) else (1, 63, 64, 65, 255, 256, 257)):
            idx = rng.integers(0, m, (b, n, K)).astype(np.int32)
            idx[:, :, 0] = np.arange(n)[None] % m
            if K > 2:
                idx[:, ::3, 1] = -1                                                                  # some invalid slots on the way
            c = make_case("B=%d K=%d N=%d" % (b, K, n), Y, idx, view=ref.blob(rng, b) if (K + n) % 2 else None)
            host.check_case("abi", c, abi_run(c, dev))
            if (K + n) % 3 == 0:
                host.check_case("surface", c, surface_run(c, dev, long=bool(n % 2)))


def test_a_batch_above_the_grid_cap(dev):
    rng = np.random.default_rng(2920)
    b, n, m, K = host.GRID_CAP + 3, 5, 12, 4
    assert -(-n // host.BLOCK) * b > host.GRID_CAP
    Y = ref.blob(rng, b, m)
    xl, yl = rng.integers(0, n + 1, b).astype(np.int32), rng.integers(0, m + 1, b).astype(np.int32)
    c = make_case("beyond the grid", Y, rng.integers(-1, m + 1, (b, n, K)).astype(np.int32), xl, yl)
    host.check_case("abi", c, abi_run(c, dev))                                                       # abi_run asserts so3_last_kernel


def test_a_shared_cloud_is_the_expanded_one(dev):
    rng = np.random.default_rng(2930)
    b, n, m, K = 3, 100, 80, 9
    Y = ref.sphere(rng, 1, m)
    c = make_case("shared", np.broadcast_to(Y, (b, m, 3)), rng.integers(0, m, (b, n, K)).astype(np.int32), None, np.array([80, 40, 5], np.int32))
    expanded = abi_run(c, dev)
    host.check_case("expanded", c, expanded)
    assert same_bits(abi_run(c, dev, shared=True), expanded) and same_bits(surface_run(c, dev, shared=True), expanded)


# ---- where the sign rules branch exactly (tests/local_frames_ref.py: the branch cases) -------------------------------------------------
def test_sign_ties_the_lowest_index_decides(dev):
    """Lattice patches on the planes x_p = +-x_q and along e_p - e_q: the tied components are bit-equal in magnitude and the lower index
    is positive -- N = 257, B = 3, K = 9 of 16 slots, each optional output left out once, the shared cloud, the surface, 2^+-20."""
    c = ref.sign_tie_case()
    base = host.check_left_out_and_shared("abi", c, lambda d, want, shared: abi_run(d, dev, want, shared))
    host.check_sign_ties("abi", c, base)
    host.check_sign_ties("surface", c, surface_run(c, dev))
    assert same_bits(surface_run(c, dev, long=True, shared=True), base)
    host.check_power_of_two("abi", c, base, lambda d: abi_run(d, dev))


@pytest.mark.parametrize("mirror", [False, True])
def test_a_viewpoint_exactly_in_the_plane_keeps_the_sign(dev, mirror):
    cases = ref.viewpoint_cases(mirror)
    host.check_viewpoint_in_the_plane("abi", cases, lambda c: abi_run(c, dev))
    host.check_viewpoint_in_the_plane("surface", cases, lambda c: surface_run(c, dev, long=mirror))
    for k in ("in", "below"):
        host.check_power_of_two("abi", cases[k], abi_run(cases[k], dev), lambda d: abi_run(d, dev))


# ---- indices from the library's own searches -------------------------------------------------------------------------------------
def test_indices_straight_from_the_searches(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2940)
    b, n, s = 2, 200, 40
    xyz = to_device(ref.sphere(rng, b, n), dev)
    lengths = to_device(np.array([200, 150]), dev, np.int64)
    _, idx = pa.knn_points(xyz, xyz, 12, lengths, lengths)                                           # int64, -1 rows past the length
    lam, frames = pa.local_frames(xyz, idx, lengths, lengths)
    c = make_case("knn_points", xyz.cpu().numpy(), idx.cpu().numpy(), np.array([200, 150], np.int32), np.array([200, 150], np.int32))
    fr = frames.cpu().numpy()
    host.check_case("knn_points", c, (None, lam.cpu().numpy(), np.ascontiguousarray(fr[..., :, 0]), fr.reshape(b, n, 9)))
    assert (frames[1, 150:] == 0).all() and (frames[1, :150].abs().sum((-1, -2)) > 0).all()
    new_xyz = xyz[:, :s].contiguous()                                                                # knn_group's search: centres against the cloud
    _, gidx = pa.knn_points(new_xyz, xyz, 8)
    lam, frames = pa.local_frames(xyz, gidx)
    c = make_case("knn_group's search", xyz.cpu().numpy(), gidx.cpu().numpy())
    fr = frames.cpu().numpy()
    host.check_case("knn_group's search", c, (None, lam.cpu().numpy(), np.ascontiguousarray(fr[..., :, 0]), fr.reshape(b, s, 9)))
    centres = new_xyz.clone()
    centres[:, 0] = 5.0                                                                              # an empty ball: its slots hold N
    ball = pa.query_ball_point(0.4, 16, xyz, centres)
    assert (ball[:, 0] == n).all() and (ball[:, 1:, 0] < n).all()
    lam, frames = pa.local_frames(xyz, ball)
    c = make_case("query_ball_point", xyz.cpu().numpy(), ball.cpu().numpy())
    fr = frames.cpu().numpy()
    host.check_case("query_ball_point", c, (None, lam.cpu().numpy(), np.ascontiguousarray(fr[..., :, 0]), fr.reshape(b, s, 9)))
    assert (frames[:, 0] == 0).all() and (lam[:, 0] == 0).all()


# ---- properties ---------------------------------------------------------------------------------------------------------------
def test_power_of_two_on_the_device(dev, g29_cases):
    for c in g29_cases:
        if c["name"] in ("sphere_257x300x16", "plane_64x64x3", "lattice_plane", "cube", "all_equal", "mixed", "ragged", "view_outside"):
            host.check_power_of_two("abi", c, abi_run(c, dev), lambda d: abi_run(d, dev))


def test_repeatable_reversed_and_isolated(dev):
    rng = np.random.default_rng(2950)
    b, n, m, K = 5, 130, 200, 20
    Y = ref.blob(rng, b, m)
    idx = rng.integers(-1, m + 1, (b, n, K)).astype(np.int32)
    xl, yl, view = rng.integers(1, n + 1, b).astype(np.int32), rng.integers(1, m + 1, b).astype(np.int32), ref.blob(rng, b) * 3
    c = make_case("five clouds", Y, idx, xl, yl, view)
    one = abi_run(c, dev)
    host.check_case("abi", c, one)
    assert same_bits(one, abi_run(c, dev))                                                           # two calls, the same bits
    rev = dict(c, Y=Y[::-1], idx=idx[::-1], x_lengths=xl[::-1], y_lengths=yl[::-1], viewpoint=view[::-1])
    assert same_bits(one, tuple(o[::-1] for o in abi_run(rev, dev)))                                 # the reversed batch, per cloud
    bad = Y.copy()
    bad[2] = np.nan
    keep = [0, 1, 3, 4]
    assert same_bits(tuple(o[keep] for o in one), tuple(o[keep] for o in abi_run(dict(c, Y=bad), dev)))      # a NaN cloud changes no other cloud


def test_replay_from_a_captured_graph(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2960)
    b, n, K = 2, 150, 10
    Y, view = to_device(ref.sphere(rng, b, n), dev), to_device(np.zeros((b, 3)), dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pa.estimate_normals(Y, K, viewpoint=view, return_curvature=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        normals, variation = pa.estimate_normals(Y, K, viewpoint=view, return_curvature=True)
        _, idx = pa.knn_points(Y, Y, K)
        lam, frames = pa.local_frames(Y, idx, viewpoint=view)
    Yn = ref.sphere(rng, b, n)
    Y.copy_(to_device(Yn, dev))
    graph.replay()
    torch.cuda.synchronize()
    c = make_case("replay", Yn, idx.cpu().numpy(), view=np.zeros((b, 3), np.float32))
    fr = frames.cpu().numpy()
    host.check_case("replay", c, (None, lam.cpu().numpy(), normals.cpu().numpy(), fr.reshape(b, n, 9)))
    assert torch.equal(variation, lam[..., 0] / lam.sum(-1))


# ---- estimate_normals -----------------------------------------------------------------------------------------------------------
def test_estimate_normals_is_knn_points_then_local_frames(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2970)
    b, n, K = 3, 300, 16
    Y = to_device(ref.sphere(rng, b, n), dev)
    lengths = to_device(np.array([300, 1, 120]), dev, np.int32)
    for ln, view in ((None, None), (lengths, None), (lengths, torch.zeros(3, device=dev)), (None, torch.zeros(b, 3, device=dev, dtype=torch.float64))):
        normals, variation = pa.estimate_normals(Y, K, ln, view, return_curvature=True)
        _, idx = pa.knn_points(Y, Y, K, ln, ln)
        lam, frames = pa.local_frames(Y, idx, ln, ln, view)
        assert normals.shape == (b, n, 3) and variation.shape == (b, n) and torch.equal(normals, frames[..., :, 0])
        assert torch.equal(normals, pa.estimate_normals(Y, K, ln, view))
        total = lam.sum(-1)
        assert torch.equal(variation, torch.where(total > 0, lam[..., 0] / total.clamp_min(1e-30), torch.zeros_like(total)))
        assert (idx[..., 0] == torch.arange(n, device=dev))[idx[..., 0] >= 0].all()                  # the point itself is slot 0: the pivot
        if ln is not None:                                                                           # a one-point cloud: the identity frame, then zeros
            assert (normals[1, 0] == torch.tensor([1.0, 0.0, 0.0], device=dev)).all() and (normals[1, 1:] == 0).all() and (normals[2, 120:] == 0).all()
    n64 = pa.estimate_normals(Y.double(), K)                                                        # the cloud's dtype
    assert n64.dtype == torch.float64 and torch.equal(n64, pa.estimate_normals(Y, K).double())


def test_the_lattice_plane_is_flat_and_the_sphere_faces_its_centre(dev, g29_cases):
    import poseestimation_amd as pa
    c = next(c for c in g29_cases if c["name"] == "lattice_plane")
    normals, variation = pa.estimate_normals(to_device(c["Y"], dev), c["K"], return_curvature=True)
    assert (variation == 0).all() and (normals == torch.tensor([0.0, 0.0, 1.0], device=dev)).all()
    flat, zero = pa.estimate_normals(to_device(np.zeros((1, 20, 3)), dev), 4, return_curvature=True)       # all lambda 0: the variation is 0, not NaN
    assert (zero == 0).all() and (flat == torch.tensor([1.0, 0.0, 0.0], device=dev)).all()
    rng = np.random.default_rng(2980)
    Yn = ref.sphere(rng, 2, 400)
    normals = pa.estimate_normals(to_device(Yn, dev), 12, viewpoint=torch.zeros(3, device=dev)).cpu().numpy()
    idx = ref.self_knn(Yn, 400, 12)
    c = make_case("sphere, the centre as viewpoint", Yn, idx, view=np.zeros((2, 3), np.float32))
    frames = pa.local_frames(to_device(Yn, dev), to_device(idx, dev, np.int32), viewpoint=torch.zeros(2, 3, device=dev))[1].cpu().numpy()
    host.check_case("surface", c, (None, None, normals, frames.reshape(2, 400, 9)))                  # within the normal bound of float64's normal ...
    inward = -(normals.astype(np.float64) * Yn).sum(-1)                                             # ... which is -x / |x| up to the patch's lean
    assert (inward > np.cos(np.radians(20.0))).all(), inward.min()


def test_the_requires_grad_warning_appears_once(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    rr._WARNED.discard("local_frames")
    Y = torch.rand(1, 30, 3, device=dev, requires_grad=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        normals = pa.estimate_normals(Y, 4)
        lam, frames = pa.local_frames(Y, torch.zeros(1, 5, 3, dtype=torch.int32, device=dev))
        pa.local_frames(Y.detach(), torch.zeros(1, 5, 3, dtype=torch.int32, device=dev), viewpoint=torch.zeros(3, device=dev, requires_grad=True))
    mine = [w for w in seen if "forward-only" in str(w.message)]
    assert len(mine) == 1 and issubclass(mine[0].category, RuntimeWarning)
    assert not (normals.requires_grad or lam.requires_grad or frames.requires_grad)


def test_the_surface_refuses_bad_arguments_on_the_device(dev):
    import poseestimation_amd as pa
    Y, idx = torch.zeros(2, 7, 3, device=dev), torch.zeros(2, 5, 4, dtype=torch.long, device=dev)
    shapes = r"local_frames: expected points \(B, M, 3\) or \(M, 3\) and idx \(B, N, K\) \(int32 or int64\) with 1 <= N, M <= 1048576 and 1 <= K <= 64, got"
    for bad_y, bad_i in ((Y[..., :2], idx), (Y[None], idx), (Y[:1], idx), (Y, idx[0]), (Y, idx.float()), (Y, idx.short()), (Y[:, :0], idx), (Y, idx[:, :0]),
                         (Y, idx[:, :, :0]), (Y, torch.zeros(2, 5, 65, dtype=torch.long, device=dev)), (torch.zeros(3, 7, 3, device=dev), idx)):
        with pytest.raises(ValueError, match=shapes) as info:
            pa.local_frames(bad_y, bad_i)
        assert str(tuple(bad_y.shape)) in str(info.value) and str(tuple(bad_i.shape)) in str(info.value)
    for name, xl, yl in (("x_lengths", torch.tensor([1.0, 2.0], device=dev), None), ("x_lengths", torch.tensor([1, 2, 3], device=dev), None),
                         ("y_lengths", None, torch.tensor([[1, 2]], device=dev)), ("y_lengths", None, torch.tensor([1, 2], dtype=torch.int16, device=dev))):
        with pytest.raises(ValueError, match=r"local_frames: expected %s as a \(B,\) int32 or int64 tensor on .* for B = 2, got" % name):
            pa.local_frames(Y, idx, xl, yl)
    for view in (torch.zeros(2, 2, device=dev), torch.zeros(3, 3, device=dev), torch.zeros(2, 3, dtype=torch.long, device=dev)):
        with pytest.raises(ValueError, match=r"local_frames: expected viewpoint as a \(B, 3\) or \(3,\) floating-point tensor on .* for B = 2, got"):
            pa.local_frames(Y, idx, viewpoint=view)
    with pytest.raises(RuntimeError, match="HIP device only"):                                       # lengths, a viewpoint on the host
        pa.local_frames(Y, idx, torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="HIP device only"):
        pa.estimate_normals(Y, 3, viewpoint=torch.zeros(3))
    for k in (0, -1, 65, 3.0, None):
        with pytest.raises(ValueError, match="estimate_normals: expected an int 1 <= K <= 64, got"):
            pa.estimate_normals(Y, k)
    with pytest.raises(ValueError, match=r"estimate_normals: expected points \(B, N, 3\), got \(7, 3\)"):
        pa.estimate_normals(Y[0])
    lam, frames = pa.local_frames(Y, torch.zeros(2, 5, 64, dtype=torch.int32, device=dev))          # the limit itself is legal
    assert (lam == 0).all() and (frames == torch.eye(3, device=dev)).all()


# ---- the speed condition ----------------------------------------------------------------------------------------------------------
def test_not_slower_than_the_torch_spelling(dev):
    """32 x 1024, K = 16, idx given, HIP events, 5 warm-ups, the median of 20, in this process: local_frames must not be slower than the
    torch spelling on the same device -- knn_gather, the centred einsum, torch.linalg.eigh.  Measured on an MI355X: see
    profiles/local_frames_bench.txt."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    rng = np.random.default_rng(2999)
    b, n, K = 32, 1024, 16
    Y = to_device(ref.sphere(rng, b, n), dev)
    _, idx = pa.knn_points(Y, Y, K)

    def ours():
        return pa.local_frames(Y, idx)

    def spelling():
        g = pa.knn_gather(Y, idx)
        e = g - g.mean(2, keepdim=True)
        return torch.linalg.eigh(torch.einsum("bnka,bnkc->bnac", e, e) / K)

    def median_ms(fn):
        times = []
        for rep in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    t_ours, t_torch = median_ms(ours), median_ms(spelling)
    ratio = t_torch / t_ours
    REPORT_LINES.append("local_frames 32 x 1024, K = 16, idx given: %.3f ms, torch spelling (knn_gather, einsum, linalg.eigh) %.3f ms, ratio %.2f"
                        % (t_ours, t_torch, ratio))
    print(REPORT_LINES[-1])
    assert ratio >= 1.0, (t_ours, t_torch)
