"""farthest_point_sample, query_ball_point, index_points and sample_and_group on the GPU.  Every comparison of indices is EXACT (no
tolerance anywhere): against the reference's recorded output (G22, outside the boundary mask for the ball query), against the numpy
restatement of the definition (tests/pointnet_ref.py) on the shape lists of tests/test_pointnet_host.py, through the Python surface and
through the raw C ABI; then the composition, determinism and replay from a graph, the documented errors, and the speed conditions
against the torch spellings the feature replaces."""
import ctypes

import numpy as np
import pytest
import torch

import pointnet_ref as ref
from support import dev, last_kernel, median_ms, ptr, to_device  # noqa: F401
import test_pointnet_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g22_cases():
    return ref.cases(ref.g22())


def surface_fps(xyz, npoint, start, dev):
    import poseestimation_amd as pa
    out = pa.farthest_point_sample(to_device(xyz, dev), npoint, to_device(start, dev, np.int64))
    assert out.shape == (len(xyz), npoint) and out.dtype == torch.int64 and out.is_cuda
    return out.cpu().numpy()


def surface_ball(radius, nsample, xyz, centres, dev):
    import poseestimation_amd as pa
    x, c = to_device(xyz, dev), to_device(centres, dev)
    idx, count = pa.query_ball_point(radius, nsample, x, c, return_counts=True)
    assert last_kernel() == "k_ball_query<true>"
    alone = pa.query_ball_point(radius, nsample, x, c)                       # the scan with the early exit writes the same rows
    assert last_kernel() == "k_ball_query<false>"
    assert idx.dtype == count.dtype == alone.dtype == torch.int64 and torch.equal(alone, idx)
    assert idx.shape == (len(xyz), centres.shape[1], min(nsample, xyz.shape[1])) and count.shape == idx.shape[:2]
    return idx.cpu().numpy(), count.cpu().numpy()


def abi_fps(xyz, npoint, start, dev):
    """The raw C ABI into a buffer pre-filled with -1."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    x, first = to_device(xyz, dev), to_device(start, dev, np.int32)
    out = torch.full((len(xyz), npoint), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_fps_f32(ptr(x), ptr(first), ptr(out), len(xyz), xyz.shape[1], npoint, st), "so3_fps_f32")
    return out.cpu().numpy()


def abi_ball(radius, nsample, xyz, centres, dev):
    """The raw C ABI into buffers pre-filled with -1, with count given and omitted."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    x, c = to_device(xyz, dev), to_device(centres, dev)
    b, n, s = len(xyz), xyz.shape[1], centres.shape[1]
    idx, idx2 = (torch.full((b, s, min(nsample, n)), -1, dtype=torch.int32, device=dev) for _ in range(2))
    count = torch.full((b, s), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_ball_query_f32(ptr(x), ptr(c), radius, nsample, ptr(idx), ptr(count), b, n, s, st), "so3_ball_query_f32")
    _lib.check(lib.so3_ball_query_f32(ptr(x), ptr(c), radius, nsample, ptr(idx2), None, b, n, s, st), "so3_ball_query_f32")
    assert torch.equal(idx, idx2)
    return idx.cpu().numpy(), count.cpu().numpy()


# ---- G22 ------------------------------------------------------------------------------------------------------------------------
def test_g22_through_the_python_surface(dev, g22_cases):
    host.check_against_g22(g22_cases, lambda x, k, s: surface_fps(x, k, s, dev), lambda r, k, x, c: surface_ball(r, k, x, c, dev))


def test_g22_through_the_c_abi(dev, g22_cases):
    host.check_against_g22(g22_cases, lambda x, k, s: abi_fps(x, k, s, dev), lambda r, k, x, c: abi_ball(r, k, x, c, dev))


# ---- the shape lists --------------------------------------------------------------------------------------------------------------
def test_fps_shapes_equal_the_restatement_and_reach_every_instantiation(dev):
    import poseestimation_amd as pa
    seen = set()
    for c, want in zip(host.fps_shape_cases(), host.fps_expected()):
        got = surface_fps(c["xyz"], c["npoint"], c["start"], dev)
        seen.add(last_kernel())
        assert np.array_equal(got, want), (c["name"], np.argwhere(got != want)[:4])
        if (c["start"] == c["start"][0]).all():                                            # the same start as an int
            again = pa.farthest_point_sample(to_device(c["xyz"], dev), c["npoint"], start=int(c["start"][0]))
            assert np.array_equal(again.cpu().numpy(), want), c["name"]
        if c["xyz"].shape[1] <= 257:
            assert np.array_equal(abi_fps(c["xyz"], c["npoint"], c["start"], dev), want), c["name"]
    assert seen == {"k_fps<%d, %d>" % k for k in host.FPS_KERNELS}, seen


def test_ball_query_shapes_equal_the_restatement(dev):
    for c, (want, want_count) in zip(host.ball_shape_cases(), host.ball_expected()):
        idx, count = surface_ball(c["radius"], c["nsample"], c["xyz"], c["centres"], dev)     # with and without the early exit
        assert np.array_equal(idx, want), (c["name"], np.argwhere(idx != want)[:4])
        assert np.array_equal(count, want_count), c["name"]


def test_other_dtypes_and_strides_are_converted(dev):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(8)
    xyz = torch.rand(3, 3, 150, generator=g).to(dev).transpose(1, 2)                       # (3, 150, 3), not contiguous
    assert not xyz.is_contiguous()
    want = pa.farthest_point_sample(xyz.contiguous(), 40, start=3)
    centres = pa.index_points(xyz, want)
    rows = pa.query_ball_point(0.3, 9, xyz.contiguous(), centres.contiguous())
    for x in (xyz, xyz.double(), xyz.half().float().half()):
        base = x.float().contiguous()
        assert torch.equal(pa.farthest_point_sample(x, 40, start=3), pa.farthest_point_sample(base, 40, start=3))
        c = pa.index_points(x, want)
        assert torch.equal(pa.query_ball_point(0.3, 9, x, c), pa.query_ball_point(0.3, 9, base, c.float().contiguous()))
    assert torch.equal(pa.farthest_point_sample(xyz, 40, start=3), want) and torch.equal(pa.query_ball_point(0.3, 9, xyz, centres), rows)
    drawn = pa.farthest_point_sample(xyz, 150)                                             # start=None: a drawn first index, then a permutation
    assert all(sorted(r) == list(range(150)) for r in drawn.cpu().tolist())


def test_non_finite_coordinates_keep_indices_in_range(dev):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(9)
    xyz = torch.rand(2, 300, 3, generator=g)
    xyz[0, 5, 0], xyz[0, 77, 2], xyz[1, 0, 1], xyz[1, 299, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
    xyz = xyz.to(dev)
    idx = pa.farthest_point_sample(xyz, 64, start=1)
    assert idx.min().item() >= 0 and idx.max().item() < 300
    rows, count = pa.query_ball_point(0.4, 16, xyz, xyz[:, :7], return_counts=True)
    assert rows.min().item() >= 0 and rows.max().item() <= 300 and count.min().item() >= 0 and count.max().item() <= 300


# ---- the composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_points", [True, False], ids=["points", "xyz only"])
def test_sample_and_group_is_the_composition(dev, with_points):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(10)
    b, n, d, npoint, radius, k = 3, 333, 6, 50, 0.35, 12
    xyz = torch.rand(b, n, 3, generator=g).to(dev).requires_grad_(True)
    pts = torch.randn(b, n, d, generator=g).to(dev).requires_grad_(True) if with_points else None
    start = torch.tensor([7, 0, 332], device=dev)
    new_xyz, new_points, grouped_xyz, fps_idx = pa.sample_and_group(npoint, radius, k, xyz, pts, returnfps=True, start=start)
    two = pa.sample_and_group(npoint, radius, k, xyz, pts, start=start)
    assert len(two) == 2 and torch.equal(two[0], new_xyz) and torch.equal(two[1], new_points)
    assert new_xyz.shape == (b, npoint, 3) and new_points.shape == (b, npoint, k, 3 + (d if with_points else 0))
    assert grouped_xyz.shape == (b, npoint, k, 3) and fps_idx.shape == (b, npoint) and fps_idx.dtype == torch.int64 and not fps_idx.requires_grad
    x2 = xyz.detach().clone().requires_grad_(True)
    p2 = pts.detach().clone().requires_grad_(True) if with_points else None
    fi = pa.farthest_point_sample(x2, npoint, start)
    centres = pa.index_points(x2, fi)
    gi = pa.query_ball_point(radius, k, x2, centres)
    gx = pa.index_points(x2, gi)
    want = gx - centres.view(b, npoint, 1, 3)
    if with_points:
        want = torch.cat([want, pa.index_points(p2, gi)], dim=-1)
    assert torch.equal(fps_idx, fi) and torch.equal(new_xyz, centres) and torch.equal(grouped_xyz, gx) and torch.equal(new_points, want)
    assert np.array_equal(fi.cpu().numpy(), ref.fps(xyz.detach().cpu().numpy(), npoint, start.cpu().numpy()))
    new_points.sum().backward()
    want.sum().backward()
    assert torch.equal(xyz.grad, x2.grad) and xyz.grad.abs().max().item() > 0
    if with_points:
        assert torch.equal(pts.grad, p2.grad) and pts.grad.abs().max().item() > 0


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_replay_from_a_graph(dev, g22_cases):
    """Two eager calls give the same bits; one call of each function captured and replayed twice into zeroed outputs equals them."""
    import poseestimation_amd as pa
    c = next(c for c in g22_cases if c["kind"] == "ball" and c["nsample"] == 64 and c["xyz"].shape[1] == 1024)
    xyz, centres = to_device(c["xyz"], dev), to_device(c["centres"], dev)

    def call():
        rows, count = pa.query_ball_point(c["radius"], c["nsample"], xyz, centres, return_counts=True)
        return [pa.farthest_point_sample(xyz, 512, start=11), rows, count, pa.query_ball_point(c["radius"], c["nsample"], xyz, centres)]

    eager = [x.clone() for x in call()]
    for a, b in zip(eager, call()):
        assert torch.equal(a, b)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                                                     # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call()
    for _ in range(2):
        for x in captured:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


# ---- the documented errors --------------------------------------------------------------------------------------------------------
def test_errors(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import _lib
    xyz = torch.rand(2, 20, 3, device=dev)
    bad = [lambda: pa.farthest_point_sample(xyz.cpu(), 4), lambda: pa.query_ball_point(0.5, 4, xyz.cpu(), xyz[:, :3]),
           lambda: pa.query_ball_point(0.5, 4, xyz, xyz[:, :3].cpu()), lambda: pa.sample_and_group(4, 0.5, 4, xyz.cpu(), None),
           lambda: pa.farthest_point_sample(xyz[0], 4), lambda: pa.farthest_point_sample(xyz[..., :2], 4), lambda: pa.farthest_point_sample(xyz, 0),
           lambda: pa.farthest_point_sample(xyz, _lib.FPS_MAX_N + 1), lambda: pa.farthest_point_sample(torch.zeros(1, _lib.FPS_MAX_N + 1, 3, device=dev), 4),
           lambda: pa.farthest_point_sample(xyz, 4, start=20), lambda: pa.farthest_point_sample(xyz, 4, start=-1),
           lambda: pa.farthest_point_sample(xyz, 4, start=torch.tensor([0, 20], device=dev)), lambda: pa.farthest_point_sample(xyz, 4, start=torch.tensor([-1, 3])),
           lambda: pa.farthest_point_sample(xyz, 4, start=torch.tensor([0, 1, 2], device=dev)), lambda: pa.farthest_point_sample(xyz, 4, start=torch.tensor([0.0, 1.0], device=dev)),
           lambda: pa.query_ball_point(0.5, 4, xyz, xyz[0]), lambda: pa.query_ball_point(0.5, 4, xyz, xyz[:1]), lambda: pa.query_ball_point(0.5, 0, xyz, xyz),
           lambda: pa.query_ball_point(0.5, 4, xyz[..., :2], xyz), lambda: pa.index_points(xyz, torch.zeros(3, 4, dtype=torch.long, device=dev))]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("call %d did not raise" % k)
    with pytest.raises(RuntimeError, match="HIP device only"):
        pa.farthest_point_sample(xyz.cpu(), 4)
    with pytest.raises(RuntimeError, match=r"outside \[0, 20\)"):
        pa.farthest_point_sample(xyz, 4, start=20)
    with pytest.raises(RuntimeError, match="N <= %d" % _lib.FPS_MAX_N):
        pa.farthest_point_sample(torch.zeros(1, _lib.FPS_MAX_N + 1, 3, device=dev), 4)
    assert pa.farthest_point_sample(xyz, 4, start=19)[:, 0].tolist() == [19, 19]                # and the library is still usable


# ---- the speed conditions -------------------------------------------------------------------------------------------------------
def torch_fps_loop(xyz, npoint, start):
    """The loop farthest_point_sample replaces, in torch on the device: npoint iterations, each a gather of the centre, the squared
    distances, the running minimum (torch.minimum: no masked assignment, which would synchronise with the host) and an argmax."""
    b, n, _ = xyz.shape
    out = torch.empty(b, npoint, dtype=torch.long, device=xyz.device)
    dist = torch.full((b, n), 1e10, device=xyz.device)
    rows = torch.arange(b, device=xyz.device)
    cur = start
    for i in range(npoint):
        out[:, i] = cur
        dist = torch.minimum(dist, ((xyz - xyz[rows, cur][:, None, :]) ** 2).sum(-1))
        cur = dist.argmax(-1)
    return out


def torch_ball_by_sorting(radius, nsample, xyz, centres):
    """The composition query_ball_point replaces: the (B, S, N) squared distances in expanded form (one batched matmul), every index
    outside the ball replaced by N, a sort along N, the first nsample columns, and N replaced by the row's first entry."""
    n = xyz.shape[1]
    d = (centres ** 2).sum(-1)[:, :, None] + (xyz ** 2).sum(-1)[:, None, :] - 2 * centres @ xyz.transpose(1, 2)
    idx = torch.where(d > radius * radius, n, torch.arange(n, device=xyz.device).expand(d.shape))
    idx = idx.sort(-1).values[:, :, :nsample]
    return torch.where(idx == n, idx[:, :, :1], idx)


def test_sampling_and_grouping_are_not_slower_than_the_torch_spellings(dev):
    """HIP events, 5 warm-ups, median of 20, same process.  (a) farthest_point_sample at 32 x 1024 -> 512 against the torch loop;
    (b) query_ball_point at 32 x 1024, 512 centres, r = 0.2, 64 samples against mask, sort and slice."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n, npoint, radius, k = 32, 1024, 512, 0.2, 64
    g = torch.Generator().manual_seed(221)
    raw = torch.rand(b, n, 3, generator=g) - 0.5
    xyz = (raw / (raw.amax(1) - raw.amin(1)).norm(dim=-1)[:, None, None]).to(dev)          # the scale of pc_normalize
    start = torch.randint(0, n, (b,), generator=g).to(dev)
    with torch.no_grad():
        fps_idx = pa.farthest_point_sample(xyz, npoint, start)
        loop_idx = torch_fps_loop(xyz, npoint, start)
        centres = pa.index_points(xyz, fps_idx)
        rows, count = pa.query_ball_point(radius, k, xyz, centres, return_counts=True)
        sorted_rows = torch_ball_by_sorting(radius, k, xyz, centres)
        assert torch.equal(fps_idx[:, :8], loop_idx[:, :8])                                # the same quantity (not an accuracy check:
        assert (rows != sorted_rows).any(-1).float().mean().item() < 0.01                 #  torch rounds its own way)
        ours_a = median_ms(lambda: pa.farthest_point_sample(xyz, npoint, start))
        theirs_a = median_ms(lambda: torch_fps_loop(xyz, npoint, start))
        ours_b = median_ms(lambda: pa.query_ball_point(radius, k, xyz, centres))
        ours_c = median_ms(lambda: pa.query_ball_point(radius, k, xyz, centres, return_counts=True))
        theirs_b = median_ms(lambda: torch_ball_by_sorting(radius, k, xyz, centres))
    for line in ("farthest_point_sample 32x1024->512: %.4f ms (%.3f us per iteration), torch loop %.4f ms (x%.1f)" % (ours_a, 1e3 * ours_a / npoint, theirs_a, theirs_a / ours_a),
                 "query_ball_point 32x1024, 512 centres, r=0.2, K=64 (mean count %.1f): %.4f ms, with counts %.4f ms, mask + sort + slice %.4f ms (x%.1f)"
                 % (count.float().mean().item(), ours_b, ours_c, theirs_b, theirs_b / ours_b)):
        print(line)
        REPORT_LINES.append(line)
    assert theirs_a / ours_a >= 1, (ours_a, theirs_a)
    assert theirs_b / ours_b >= 1, (ours_b, theirs_b)
