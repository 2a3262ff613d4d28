"""three_nn, three_interpolate, interpolate_features and propagate_features on the GPU.  Distances, indices and weights are compared
EXACTLY with the numpy restatement of the definition (tests/three_nn_ref.py), indices with the reference's recorded ones outside
near_tie (G24); interpolation and backward BIT FOR BIT with interpolate32 / backward32, the defined order of fused multiply-adds
restated through tests/f32_exact.py, in both layouts and on every shape of the lists (D = 257: the channel-last backward's second
channel pass; N = 1023, 1024, 1025: its LDS tile; S either side of 16 and 64; batches beyond the grid; h = 3N hits and none), and
beside that within the bounds derived there -- all through the checks of tests/test_three_nn_host.py, on
its shape lists, through the Python surface and through the raw C ABI into buffers pre-filled with -1 / NaN, with `weight` asked for
and omitted.  Then autograd, determinism and replay from a graph, the composition, the documented errors and the warn-once, and the
speed condition against the torch spelling the feature replaces."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from support import bits, dev, last_kernel, median_ms, ptr, to_device  # noqa: F401
import three_nn_ref as ref
import test_three_nn_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g24_cases():
    return ref.cases(ref.g24())


def _dims(feat, idx, channels_first):
    b, n = idx.shape[:2]
    d, s = (feat.shape[1], feat.shape[2]) if channels_first else (feat.shape[2], feat.shape[1])
    return b, n, s, d


SEEN = set()


def surface_nn(xyz1, xyz2, want_weight, dev):
    import poseestimation_amd as pa
    out = pa.three_nn(to_device(xyz1, dev), to_device(xyz2, dev), return_weights=want_weight)
    SEEN.add(last_kernel())
    b, n, s = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    assert last_kernel() == "k_three_nn<%d, %s>" % (host.waves_per_point(b, n, s), "true" if want_weight else "false")
    assert len(out) == (3 if want_weight else 2) and out[0].dtype == torch.float32 and out[1].dtype == torch.int64
    assert all(t.shape == (b, n, 3) and t.is_cuda and not t.requires_grad for t in out)
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy() if want_weight else None


def abi_nn(xyz1, xyz2, want_weight, dev):
    """The raw C ABI into buffers pre-filled with NaN / -1."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    a, k = to_device(xyz1, dev), to_device(xyz2, dev)
    b, n, s = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    d3 = torch.full((b, n, 3), float("nan"), device=dev)
    idx = torch.full((b, n, 3), -1, dtype=torch.int32, device=dev)
    w = torch.full((b, n, 3), float("nan"), device=dev) if want_weight else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_three_nn_f32(ptr(a), ptr(k), ptr(d3), ptr(idx), ptr(w), b, n, s, st), "so3_three_nn_f32")
    return d3.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy() if want_weight else None


def surface_fwd(feat, idx, weight, channels_first, dev):
    import poseestimation_amd as pa
    out = pa.three_interpolate(to_device(feat, dev), to_device(idx, dev, np.int64), to_device(weight, dev), channels_first)
    assert last_kernel() == "k_three_interp<%s>" % ("true" if channels_first else "false")
    return out.cpu().numpy()


def surface_bwd(grad, idx, weight, s, channels_first, dev):
    """Through autograd: one backward launch into the gradient of a points2 of zeros."""
    import poseestimation_amd as pa
    b, n = idx.shape[:2]
    d = grad.shape[1] if channels_first else grad.shape[2]
    feat = torch.zeros((b, d, s) if channels_first else (b, s, d), device=dev, requires_grad=True)
    out = pa.three_interpolate(feat, to_device(idx, dev, np.int32), to_device(weight, dev), channels_first)
    out.backward(to_device(grad, dev))                                                  # (on autograd's thread: so3_last_kernel is per thread, see abi_bwd)
    return feat.grad.cpu().numpy()


def abi_fwd(feat, idx, weight, channels_first, dev):
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, s, d = _dims(feat, idx, channels_first)
    f, i, w = to_device(feat, dev), to_device(idx, dev, np.int32), to_device(weight, dev)
    out = torch.full((b, d, n) if channels_first else (b, n, d), float("nan"), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_three_interpolate_f32(ptr(f), ptr(i), ptr(w), ptr(out), int(channels_first), b, n, s, d, st), "so3_three_interpolate_f32")
    assert last_kernel() == "k_three_interp<%s>" % ("true" if channels_first else "false")
    return out.cpu().numpy()


def abi_bwd(grad, idx, weight, s, channels_first, dev):
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n = idx.shape[:2]
    d = grad.shape[1] if channels_first else grad.shape[2]
    g, i, w = to_device(grad, dev), to_device(idx, dev, np.int32), to_device(weight, dev)
    out = torch.full((b, d, s) if channels_first else (b, s, d), float("nan"), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_three_interpolate_bwd_f32(ptr(g), ptr(i), ptr(w), ptr(out), int(channels_first), b, n, s, d, st), "so3_three_interpolate_bwd_f32")
    assert last_kernel() == ("k_three_interp_bwd_cf" if channels_first else "k_three_interp_bwd_cl")
    return out.cpu().numpy()


def _runners(kind, dev):
    if kind == "surface":
        return (lambda a, k, wt: surface_nn(a, k, wt, dev), lambda *a: surface_fwd(*a, dev), lambda *a: surface_bwd(*a, dev))
    return (lambda a, k, wt: abi_nn(a, k, wt, dev), lambda *a: abi_fwd(*a, dev), lambda *a: abi_bwd(*a, dev))


# ---- G24 and the shape lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["surface", "abi"])
def test_g24(dev, g24_cases, kind):
    host.check_against_g24(g24_cases, *_runners(kind, dev))


def test_search_shapes_equal_the_restatement_and_reach_every_instantiation(dev):
    SEEN.clear()
    surface, abi = _runners("surface", dev)[0], _runners("abi", dev)[0]
    for c, want in zip(host.nn_shape_cases(), host.nn_expected()):
        host.check_nn(c["name"], surface, c["xyz1"], c["xyz2"], want)
        host.check_nn(c["name"], abi, c["xyz1"], c["xyz2"], want)
    assert SEEN == host.NN_KERNELS, SEEN


@pytest.mark.parametrize("kind", ["surface", "abi"])
def test_interpolation_shapes_in_both_layouts(dev, kind):
    _, fwd, bwd = _runners(kind, dev)
    for i, c in enumerate(host.interp_shape_cases()):
        for channels_first in (False, True):
            got, _ = host.check_interp(c["name"], fwd, bwd, c, channels_first, host.interp_expected32(i))
            if c["name"] == "an unknown point that is a known point":
                got = got.transpose(0, 2, 1) if channels_first else got
                own = c["feat"][0][c["idx"][0, :, 0]]
                assert (np.abs(got[0] - own) <= 1e-6 * np.abs(own)).all()


def test_non_finite_coordinates_keep_indices_in_range(dev):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(9)
    xyz1, xyz2 = torch.rand(2, 300, 3, generator=g), torch.rand(2, 70, 3, generator=g)
    xyz1[0, 5, 0], xyz1[1, 0, 1], xyz2[0, 7, 2], xyz2[1, 0, 0], xyz2[1, 69, 1] = float("nan"), float("inf"), float("inf"), float("nan"), float("-inf")
    for s in (70, 2):
        _, idx, _ = pa.three_nn(xyz1.to(dev), xyz2[:, :s].to(dev), return_weights=True)
        assert idx.min().item() >= 0 and idx.max().item() < s
    _, idx = pa.three_nn(xyz1.to(dev), torch.full((2, 5, 3), float("nan"), device=dev))
    assert idx.min().item() >= 0 and idx.max().item() < 5


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_first", [False, True], ids=["channel-last", "channel-first"])
def test_gradient_against_autograd_through_the_float64_restatement(dev, channels_first):
    """grad_out arrives non-contiguous (a transposed view); the float64 restatement is index_points * weight summed, in torch."""
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(11)
    b, n, s, d = 3, 301, 47, 70
    xyz1, xyz2 = torch.rand(b, n, 3, generator=g).to(dev), torch.rand(b, s, 3, generator=g).to(dev)
    feat = torch.randn((b, d, s) if channels_first else (b, s, d), generator=g).to(dev).requires_grad_(True)
    _, idx, w = pa.three_nn(xyz1, xyz2, return_weights=True)
    out = pa.three_interpolate(feat, idx, w, channels_first)
    grad = torch.randn((b, n, d) if channels_first else (b, d, n), generator=g).to(dev).transpose(1, 2)
    assert grad.shape == out.shape and not grad.is_contiguous()
    (got,) = torch.autograd.grad(out, [feat], grad)
    f64 = feat.detach().double().requires_grad_(True)
    rows = f64.transpose(1, 2) if channels_first else f64                                                # (B, S, D)
    want_out = (pa.index_points(rows, idx) * w.double()[..., None]).sum(2)
    want_out = want_out.transpose(1, 2) if channels_first else want_out
    (want,) = torch.autograd.grad(want_out, [f64], grad.double())
    hits = torch.stack([torch.bincount(idx[k].reshape(-1), minlength=s) for k in range(b)]).double()
    mag = torch.zeros(b, s, d, dtype=torch.float64, device=dev)
    g_rows = (grad.transpose(1, 2) if channels_first else grad).double().abs()
    for k in range(3):
        mag.scatter_add_(1, idx[..., k, None].expand(-1, -1, d), w[..., k, None].double() * g_rows)
    bound = (hits[..., None] + 2) * ref.U * mag
    bound = bound.transpose(1, 2) if channels_first else bound
    assert (out.double() - want_out.detach()).abs().max().item() < 1e-5
    assert ((got.double() - want).abs() <= bound).all(), ((got.double() - want).abs().max().item())
    # autograd's gradient is the C ABI's, bit for bit, and both are the defined order's
    direct = abi_bwd(grad.contiguous().cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy(), s, channels_first, dev)
    assert np.array_equal(bits(got.cpu().numpy()), bits(direct))
    assert np.array_equal(bits(direct), bits(ref.backward32(grad.contiguous().cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy(), s, channels_first)))
    with pytest.raises(RuntimeError, match="differentiate twice|double backward"):
        f2 = feat.detach().clone().requires_grad_(True)
        o2 = pa.three_interpolate(f2, idx, w, channels_first)
        (g1,) = torch.autograd.grad(o2, [f2], torch.ones_like(o2, requires_grad=True), create_graph=True)
        g1.sum().backward()


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_graph_replays_them(dev, g24_cases):
    import poseestimation_amd as pa
    c = g24_cases[0]
    xyz1, xyz2 = to_device(c["xyz1"], dev), to_device(c["xyz2"], dev)
    g = torch.Generator().manual_seed(12)
    grad = torch.randn(2, 1024, 16, generator=g).to(dev)
    feats = [to_device(c["feat"], dev), to_device(c["feat"].transpose(0, 2, 1), dev)]
    grads = [grad, grad.transpose(1, 2).contiguous()]
    from poseestimation_amd import _lib
    lib = _lib.load()

    def call():
        d3, idx, w = pa.three_nn(xyz1, xyz2, return_weights=True)
        out = [d3, idx, w]
        i32 = idx.int()
        for cf in (0, 1):
            out.append(pa.three_interpolate(feats[cf], idx, w, bool(cf)))
            gf = torch.empty_like(feats[cf])
            _lib.check(lib.so3_three_interpolate_bwd_f32(ptr(grads[cf]), ptr(i32), ptr(w), ptr(gf), cf, 2, 1024, 512, 16,
                                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "so3_three_interpolate_bwd_f32")
            out.append(gf)
        return out

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


# ---- the composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [40, 1], ids=["S=40", "S=1"])
@pytest.mark.parametrize("with_points1", [True, False], ids=["points1", "None"])
def test_propagate_features_is_the_composition(dev, s, with_points1):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(13)
    b, n, d1, d2 = 3, 130, 5, 9
    xyz1, xyz2 = torch.rand(b, 3, n, generator=g).to(dev), torch.rand(b, 3, s, generator=g).to(dev)
    p1 = torch.randn(b, d1, n, generator=g).to(dev).requires_grad_(True) if with_points1 else None
    p2 = torch.randn(b, d2, s, generator=g).to(dev).requires_grad_(True)
    got = pa.propagate_features(xyz1, xyz2, p1, p2)
    assert got.shape == (b, (d1 if with_points1 else 0) + d2, n)
    q2 = p2.detach().clone().requires_grad_(True)
    _, idx, w = pa.three_nn(xyz1.transpose(1, 2), xyz2.transpose(1, 2), return_weights=True)
    inter = pa.three_interpolate(q2, idx, w, channels_first=True)
    assert torch.equal(inter, pa.interpolate_features(xyz1.transpose(1, 2), xyz2.transpose(1, 2), q2, channels_first=True))
    last = pa.interpolate_features(xyz1.transpose(1, 2), xyz2.transpose(1, 2), q2.transpose(1, 2).contiguous())
    assert torch.equal(last.transpose(1, 2), inter)                                 # the two layouts compute the same numbers
    want = torch.cat([p1.detach(), inter], 1) if with_points1 else inter
    assert torch.equal(got, want)
    if s == 1:
        assert torch.equal(inter, q2.detach().expand(-1, -1, n))                   # the reference's `repeat` branch, exactly
    cot = torch.randn(got.shape, generator=g).to(dev)
    got.backward(cot)
    want.backward(cot)
    assert torch.equal(p2.grad, q2.grad) and p2.grad.abs().max().item() > 0
    if with_points1:
        assert torch.equal(p1.grad, cot[:, :d1])


def test_other_dtypes_and_strides_are_converted(dev):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(14)
    xyz1 = torch.rand(2, 3, 90, generator=g).to(dev).transpose(1, 2)
    xyz2, feat = torch.rand(2, 30, 3, generator=g).to(dev), torch.randn(2, 30, 7, generator=g).to(dev)
    d3, idx, w = pa.three_nn(xyz1.contiguous(), xyz2, return_weights=True)
    for a in (xyz1, xyz1.double()):
        got = pa.three_nn(a, xyz2.double(), return_weights=True)
        assert torch.equal(got[0], d3) and torch.equal(got[1], idx) and torch.equal(got[2], w)
    want = pa.three_interpolate(feat, idx, w)
    assert torch.equal(pa.three_interpolate(feat, idx.int(), w.double()), want)
    out = pa.three_interpolate(feat.double(), idx, w)
    assert out.dtype == torch.float64 and torch.equal(out, want.double())
    assert torch.equal(pa.three_interpolate(feat.transpose(1, 2), idx, w, channels_first=True), want.transpose(1, 2))      # a strided points2


# ---- the documented errors and the warn-once ---------------------------------------------------------------------------------------
def test_errors_and_warnings(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    xyz1, xyz2, feat = torch.rand(2, 20, 3, device=dev), torch.rand(2, 6, 3, device=dev), torch.rand(2, 6, 4, device=dev)
    _, idx, w = pa.three_nn(xyz1, xyz2, return_weights=True)
    bad = [lambda: pa.three_nn(xyz1.cpu(), xyz2), lambda: pa.three_nn(xyz1, xyz2.cpu()), lambda: pa.three_nn(xyz1[0], xyz2), lambda: pa.three_nn(xyz1, xyz2[:1]),
           lambda: pa.three_nn(xyz1[..., :2], xyz2), lambda: pa.three_nn(xyz1, xyz2[:, :0]),
           lambda: pa.three_interpolate(feat.cpu(), idx, w), lambda: pa.three_interpolate(feat, idx.cpu(), w), lambda: pa.three_interpolate(feat[0], idx, w),
           lambda: pa.three_interpolate(feat, idx[..., :2], w[..., :2]), lambda: pa.three_interpolate(feat, idx, w[:, :5]),
           lambda: pa.three_interpolate(feat, idx.float(), w), lambda: pa.three_interpolate(feat.long(), idx, w), lambda: pa.three_interpolate(feat[:1], idx, w),
           lambda: pa.interpolate_features(xyz1, xyz2, feat.cpu()), lambda: pa.propagate_features(xyz1, xyz2, None, feat),
           lambda: pa.propagate_features(xyz1.transpose(1, 2), xyz2.transpose(1, 2), torch.rand(2, 4, 19, device=dev), feat.transpose(1, 2))]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("call %d did not raise" % k)
    with pytest.raises(RuntimeError, match="HIP device only"):
        pa.three_nn(xyz1.cpu(), xyz2)
    with pytest.raises(RuntimeError, match="three_nn: expected"):
        pa.three_nn(xyz1, xyz2[:1])
    with pytest.raises(RuntimeError, match="three_interpolate: expected"):
        pa.three_interpolate(feat, idx[..., :2], w[..., :2])
    with pytest.raises(RuntimeError, match="propagate_features: expected"):
        pa.propagate_features(xyz1, xyz2, None, feat)
    for key in ("three_nn", "three_interpolate"):
        rr._WARNED.discard(key)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            pa.three_nn(xyz1.clone().requires_grad_(True), xyz2)
            pa.three_interpolate(feat, idx, w.clone().requires_grad_(True))
    assert sum("three_nn is not differentiable" in str(x.message) for x in seen) == 1
    assert sum("three_interpolate is differentiable with respect to points2 only" in str(x.message) for x in seen) == 1
    assert pa.three_interpolate(feat, idx, w).shape == (2, 20, 4)                     # and the library is still usable


# ---- the speed condition --------------------------------------------------------------------------------------------------------
def torch_interpolate(xyz1, xyz2, points2):
    """The torch spelling of point_cloud/pointnet_utils.py:286-293 on the device: the expanded squared distances, a full sort along S,
    the weight lines, the (B, N, 3, D) gather, product and sum."""
    b, n, _ = xyz1.shape
    dists = -2 * torch.matmul(xyz1, xyz2.permute(0, 2, 1))
    dists += torch.sum(xyz1 ** 2, -1).view(b, n, 1)
    dists += torch.sum(xyz2 ** 2, -1).view(b, 1, -1)
    dists, idx = dists.sort(dim=-1)
    dists, idx = dists[:, :, :3], idx[:, :, :3]
    dist_recip = 1.0 / (dists + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
    batch = torch.arange(b, device=xyz1.device).view(b, 1, 1)
    return torch.sum(points2[batch, idx, :] * weight.view(b, n, 3, 1), dim=2)


def test_feature_interpolation_is_not_slower_than_the_torch_spelling(dev):
    """HIP events, 5 warm-ups, median of 20, same process: interpolate_features forward, and forward + backward, at the reference model's
    first propagation level (32 x 1024 <- 512, D = 128) against the torch spelling."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n, s, d = 32, 1024, 512, 128
    g = torch.Generator().manual_seed(241)
    xyz1, xyz2 = (torch.rand(b, n, 3, generator=g) - 0.5).to(dev), (torch.rand(b, s, 3, generator=g) - 0.5).to(dev)
    feat = torch.randn(b, s, d, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(b, n, d, generator=g).to(dev)
    with torch.no_grad():
        ours, theirs = pa.interpolate_features(xyz1, xyz2, feat), torch_interpolate(xyz1, xyz2, feat)
        assert ((ours - theirs).abs().amax(-1) > 1e-3).float().mean().item() < 0.01   # the same quantity (not an accuracy check)
        ours_f = median_ms(lambda: pa.interpolate_features(xyz1, xyz2, feat))
        theirs_f = median_ms(lambda: torch_interpolate(xyz1, xyz2, feat))

    def both(fn):
        feat.grad = None
        fn(xyz1, xyz2, feat).backward(cot)

    ours_fb = median_ms(lambda: both(pa.interpolate_features))
    theirs_fb = median_ms(lambda: both(torch_interpolate))
    line = ("interpolate_features 32x1024<-512, D=128: forward %.4f ms, torch spelling %.4f ms (x%.1f); forward + backward %.4f ms, torch %.4f ms (x%.1f)"
            % (ours_f, theirs_f, theirs_f / ours_f, ours_fb, theirs_fb, theirs_fb / ours_fb))
    print(line)
    REPORT_LINES.append(line)
    assert theirs_f / ours_f >= 1, (ours_f, theirs_f)
    assert theirs_fb / ours_fb >= 1, (ours_fb, theirs_fb)
