"""group_points, set_abstraction_group and set_abstraction_msg_group on the GPU.  The forward is compared EXACTLY with the numpy
restatement of the definition (tests/grouping_ref.py) and, on G25, with the tensors the reference's own classes recorded; the backward
bit for bit with the float32 restatement of its defined order (plain additions from 0 in the ascending memory order of the slots) and,
beside it, within gamma_{h-1} * sum |g| of the float64 restatement -- all through the checks of tests/test_grouping_host.py, on its shape list,
through the Python surface and through the raw C ABI into buffers pre-filled with NaN, every subset of the outputs asked for alone.
Then autograd with a non-contiguous grad_out, determinism and replay from a graph, the composition, the documented errors, and the speed
condition against the torch spelling the feature replaces."""
import ctypes

import numpy as np
import pytest
import torch

import grouping_ref as ref
from support import dev, last_kernel, median_ms, ptr, to_device  # noqa: F401
import test_grouping_host as host

pytestmark = pytest.mark.gpu
SEEN = set()


@pytest.fixture(scope="module")
def g25():
    return ref.cases(ref.g25())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def surface_fwd(xyz, centres, feat, idx, channels_first, features_first, dev):
    import poseestimation_amd as pa
    out = pa.group_points(to_device(xyz, dev), to_device(centres, dev), to_device(feat, dev), to_device(idx, dev, np.int64), channels_first, features_first)
    assert last_kernel() == "k_group_fwd<%s>" % ("true" if channels_first else "false")
    assert out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
    return out.cpu().numpy()


def surface_bwd(grad, idx, n, d, channels_first, features_first, sel, dev):
    """Through autograd: one backward call into the gradients of zero inputs; only the inputs in `sel` require grad."""
    import poseestimation_amd as pa
    b, s, _ = idx.shape
    xyz = torch.zeros(b, n, 3, device=dev, requires_grad=sel[0])
    centres = torch.zeros(b, s, 3, device=dev, requires_grad=sel[1])
    feat = torch.zeros((b, d, n) if channels_first else (b, n, d), device=dev, requires_grad=sel[2]) if d else None
    out = pa.group_points(xyz, centres, feat, to_device(idx.clip(-2 ** 31, 2 ** 31 - 1), dev, np.int32), channels_first, features_first)
    out.backward(to_device(grad, dev))
    return tuple(None if t is None or t.grad is None else t.grad.cpu().numpy() for t in (xyz, centres, feat))


def abi_fwd(xyz, centres, feat, idx, channels_first, features_first, dev):
    """The raw C ABI into a buffer pre-filled with NaN."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, s, k = xyz.shape[0], xyz.shape[1], idx.shape[1], idx.shape[2]
    d = 0 if feat is None else feat.shape[1 if channels_first else 2]
    x, c, f, i = to_device(xyz, dev), to_device(centres, dev), to_device(feat, dev), to_device(idx, dev, np.int32)
    out = torch.full((b, 3 + d, k, s) if channels_first else (b, s, k, 3 + d), float("nan"), device=dev)
    _lib.check(lib.so3_group_points_f32(ptr(x), ptr(c), ptr(f), ptr(i), ptr(out), int(features_first), int(channels_first), b, n, s, k, d, _stream()),
               "so3_group_points_f32")
    SEEN.add(last_kernel())
    return out.cpu().numpy()


def abi_bwd(grad, idx, n, d, channels_first, features_first, sel, dev):
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, s, k = idx.shape
    g, i = to_device(grad, dev), to_device(idx.clip(-2 ** 31, 2 ** 31 - 1), dev, np.int32)
    gx = torch.full((b, n, 3), float("nan"), device=dev) if sel[0] else None
    gc = torch.full((b, s, 3), float("nan"), device=dev) if sel[1] else None
    gf = torch.full((b, d, n) if channels_first else (b, n, d), float("nan"), device=dev) if sel[2] and d else None
    _lib.check(lib.so3_group_points_bwd_f32(ptr(g), ptr(i), ptr(gx), ptr(gc), ptr(gf), int(features_first), int(channels_first), b, n, s, k, d,
                                            _stream()), "so3_group_points_bwd_f32")
    SEEN.add(last_kernel())
    if gx is not None or gf is not None:
        assert last_kernel() == host.bwd_kernel(d, channels_first)
    elif gc is not None:
        assert last_kernel() == "k_group_centres_bwd<%s>" % ("true" if channels_first else "false")
    return tuple(None if t is None else t.cpu().numpy() for t in (gx, gc, gf))


def _runners(kind, dev):
    if kind == "surface":
        return (lambda *a: surface_fwd(*a, dev)), (lambda *a: surface_bwd(*a, dev))
    return (lambda *a: abi_fwd(*a, dev)), (lambda *a: abi_bwd(*a, dev))


# ---- G25 and the shape list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["surface", "abi"])
def test_g25(dev, g25, kind):
    fwd, bwd = _runners(kind, dev)
    host.check_g25_forward(g25, fwd)
    host.check_g25_gradients(g25, bwd, exact=True)


def test_shape_list_through_the_c_abi_reaches_every_instantiation(dev):
    SEEN.clear()
    fwd, bwd = _runners("abi", dev)
    for i in range(len(host.shape_cases())):
        host.check_shape_case(i, fwd, bwd, exact=True)
    assert SEEN == host.KERNELS, SEEN ^ host.KERNELS


def test_shape_list_through_the_python_surface(dev):
    """One layout pair per case (they alternate), all four on the edge cases: the C-ABI test above runs every pair everywhere."""
    fwd, bwd = _runners("surface", dev)
    for i, c in enumerate(host.shape_cases()):
        edge = c["name"].startswith(("h = S*K", "idx == N", "coordinates"))
        host.check_shape_case(i, fwd, bwd, exact=True, layouts=host.LAYOUTS if edge else [host.LAYOUTS[i % 4], host.LAYOUTS[(i + 3) % 4]])


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cf,ff", host.LAYOUTS)
def test_autograd_with_a_non_contiguous_grad_out(dev, cf, ff):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2502)
    b, n, s, k, d = 2, 70, 9, 12, 7
    xyz, centres, feat = rng.uniform(-1, 1, (b, n, 3)), rng.uniform(-1, 1, (b, s, 3)), rng.standard_normal((b, d, n) if cf else (b, n, d))
    idx = host.ball_rows(rng, b, n, s, k)
    idx[1, 3] = n                                                                    # an empty ball
    shape = (b, 3 + d, k, s) if cf else (b, s, k, 3 + d)
    wide = rng.standard_normal(shape[:-1] + (2 * shape[-1],)).astype(np.float32)
    ts = [to_device(a, dev).requires_grad_(True) for a in (xyz, centres, feat)]
    out = pa.group_points(ts[0], ts[1], ts[2], to_device(idx, dev, np.int64), cf, ff)
    assert out.requires_grad and out.shape == shape
    cot = to_device(wide, dev)[..., ::2]
    assert not cot.is_contiguous()
    grads = torch.autograd.grad(out, ts, cot)
    want = ref.backward(wide[..., ::2], idx, n, cf, ff, np.float64)
    bound = ref.bounds(want, cf)
    for got, key in zip(grads, ("grad_xyz", "grad_centres", "grad_feat")):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want[key])
        assert (err <= bound[key]).all(), (key, err.max())
    assert not grads[1][1, 3].any()                                                  # the empty ball gives its centre nothing
    # only what is needed is requested: a features-only graph, and one without any input that requires grad
    f = ts[2].detach().clone().requires_grad_(True)
    only = torch.autograd.grad(pa.group_points(ts[0].detach(), ts[1].detach(), f, to_device(idx, dev, np.int64), cf, ff), [f], cot)[0]
    assert torch.equal(only, grads[2])
    assert not pa.group_points(ts[0].detach(), ts[1].detach(), f.detach(), to_device(idx, dev, np.int64), cf, ff).requires_grad
    x = ts[0].detach().clone().requires_grad_(True)
    out = pa.group_points(x, ts[1].detach(), None, to_device(idx, dev, np.int32), cf, ff)
    (gx,) = torch.autograd.grad(out, [x], torch.ones_like(out), create_graph=True)    # create_graph alone runs as always
    with pytest.raises(RuntimeError, match="differentiate twice"):
        torch.autograd.grad(pa.group_points(x, ts[1].detach(), None, to_device(idx, dev, np.int32), cf, ff), [x], (x * 1.0).sum() * torch.ones_like(out), create_graph=True)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_a_graph_replays_them(dev, g25):
    import poseestimation_amd as pa
    from poseestimation_amd import _lib
    lib = _lib.load()
    n, s, d = ref.N_FIXTURE, ref.S_FIXTURE, ref.D_FIXTURE
    xyz, centres = to_device(g25["xyz"], dev), to_device(g25["msg"]["new_xyz"].transpose(0, 2, 1), dev)
    feats = [to_device(g25["points"], dev), to_device(g25["points"].transpose(0, 2, 1), dev)]
    wide = torch.randn(2, n, 40, generator=torch.Generator().manual_seed(25)).to(dev)             # a wide-kernel case beside the narrow one
    jobs = []
    for i, idx in enumerate(g25["msg"]["idx"]):
        k = idx.shape[2]
        for cf in (0, 1):
            for f in (feats[cf], wide.transpose(1, 2).contiguous() if cf else wide):
                c = 3 + (f.shape[1] if cf else f.shape[2])
                g = torch.randn((2, c, k, s) if cf else (2, s, k, c), generator=torch.Generator().manual_seed(26 + i)).to(dev)
                jobs.append((f, to_device(idx, dev, np.int32), g, cf, k, c - 3))

    def call():
        out = []
        for f, idx, g, cf, k, dd in jobs:
            out.append(pa.group_points(xyz, centres, f, idx, bool(cf), True))
            gx, gc, gf = torch.empty(2, n, 3, device=dev), torch.empty(2, s, 3, device=dev), torch.empty_like(f)
            _lib.check(lib.so3_group_points_bwd_f32(ptr(g), ptr(idx), ptr(gx), ptr(gc), ptr(gf), 1, cf, 2, n, s, k, dd, _stream()), "so3_group_points_bwd_f32")
            out += [gx, gc, gf]
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
            x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


# ---- the composition ------------------------------------------------------------------------------------------------------------
def test_set_abstraction_groups_are_the_composition(dev, g25):
    import poseestimation_amd as pa
    xyz, pts = to_device(g25["xyz"], dev), to_device(g25["points"], dev)
    x_cf, p_cf = xyz.transpose(1, 2).contiguous(), pts.transpose(1, 2).contiguous()
    s = ref.S_FIXTURE
    (r0, k0), (r1, k1) = ref.RADII
    for tag in ("sa", "msg"):
        start = to_device(g25[tag]["fps"][:, 0], dev, np.int64)
        fps = pa.farthest_point_sample(xyz, s, start)
        assert np.array_equal(fps.cpu().numpy(), g25[tag]["fps"])
        centres = pa.index_points(xyz, fps)
        if tag == "sa":
            new_xyz, got = pa.set_abstraction_group(s, r1, k1, x_cf, p_cf, start=start)
            idx = pa.query_ball_point(r1, k1, xyz, centres)
            assert got.shape == (2, 3 + ref.D_FIXTURE, k1, s) and got.is_contiguous()
            assert torch.equal(got, pa.group_points(xyz, centres, p_cf, idx, channels_first=True))
            assert torch.equal(pa.set_abstraction_group(s, r1, k1, x_cf, None, start=start)[1], pa.group_points(xyz, centres, None, idx, channels_first=True))
            _, grouped = pa.sample_and_group(s, r1, k1, xyz, pts, start=start)     # the existing torch spelling: the same forward bits
            assert torch.equal(grouped, pa.group_points(xyz, centres, pts, idx)) and torch.equal(grouped.permute(0, 3, 2, 1), got)
        else:
            new_xyz, groups = pa.set_abstraction_msg_group(s, [r0, r1], [k0, k1], x_cf, p_cf, start=start)
            assert len(groups) == 2
            for (r, k), got in zip(ref.RADII, groups):
                idx = pa.query_ball_point(r, k, xyz, centres)
                assert got.shape == (2, ref.D_FIXTURE + 3, k, s)
                assert torch.equal(got, pa.group_points(xyz, centres, p_cf, idx, channels_first=True, features_first=True))
        assert new_xyz.shape == (2, 3, s) and np.array_equal(host.f32_bits(new_xyz.cpu().numpy()), host.f32_bits(g25[tag]["new_xyz"]))
    xa, pa_ = to_device(g25["xyz_all"], dev), to_device(g25["points_all"], dev)
    new_xyz, got = pa.set_abstraction_group(None, None, None, xa.transpose(1, 2), pa_.transpose(1, 2), group_all=True)
    assert new_xyz.shape == (2, 3, 1) and not new_xyz.any() and np.array_equal(host.f32_bits(got.cpu().numpy()), host.f32_bits(g25["all"]["t"]))
    zeros, grouped = pa.sample_and_group_all(xa, pa_)
    assert torch.equal(grouped.permute(0, 3, 2, 1), got) and zeros.shape == (2, 1, 3) and zeros.is_cuda
    assert pa.set_abstraction_group(None, None, None, xa.transpose(1, 2), None, group_all=True)[1].shape == (2, 3, ref.N_ALL, 1)


def test_gradients_flow_through_the_layer_functions(dev, g25):
    """xyz receives both paths (the gathered coordinates and, through new_xyz = xyz[fps], the centres): the reference's recorded
    gradients within the tolerance of check_g25_gradients plus our own float32 additions of the paths (one rounding per meeting)."""
    import poseestimation_amd as pa
    n, d, s = ref.N_FIXTURE, ref.D_FIXTURE, ref.S_FIXTURE
    c = g25["msg"]
    x = to_device(g25["xyz"].transpose(0, 2, 1), dev).requires_grad_(True)
    p = to_device(g25["points"].transpose(0, 2, 1), dev).requires_grad_(True)
    new_xyz, groups = pa.set_abstraction_msg_group(s, [r for r, _ in ref.RADII], [k for _, k in ref.RADII], x, p, start=to_device(c["fps"][:, 0], dev, np.int64))
    sum((t * to_device(ref.seeded_g(i, tuple(t.shape)), dev)).sum() for i, t in enumerate(groups)).backward()
    wants = [ref.backward(ref.seeded_g(i, t.shape), idx, n, True, True, np.float64) for i, (idx, t) in enumerate(zip(c["idx"], c["t"]))]
    mag, terms = sum(w["mag_xyz"] for w in wants), sum(w["hits"] for w in wants)[:, :, None].astype(np.float64)
    for b in range(2):
        mag[b, c["fps"][b]] += sum(w["mag_centres"][b] for w in wants)
        terms[b, c["fps"][b]] += sum(w["slots"][b] for w in wants)[:, None]
    # each side adds an element's `terms` float32 terms in some order, partial sums included: within gamma_{terms - 1} * sum |g| of the exact sum
    err = np.abs(x.grad.cpu().numpy().astype(np.float64) - c["grad_xyz"]).transpose(0, 2, 1)
    assert (err <= 2 * ref.gamma(terms - 1) * mag).all(), err.max()
    assert np.abs(p.grad.cpu().numpy().astype(np.float64) - c["grad_points"]).max() < 1e-4


# ---- the documented errors ----------------------------------------------------------------------------------------------------------
def test_errors(dev):
    import poseestimation_amd as pa
    xyz, cen, pts = torch.rand(2, 20, 3, device=dev), torch.rand(2, 6, 3, device=dev), torch.rand(2, 20, 4, device=dev)
    idx = torch.zeros(2, 6, 5, dtype=torch.long, device=dev)
    bad = [lambda: pa.group_points(xyz.cpu(), cen, pts, idx), lambda: pa.group_points(xyz, cen, pts, idx.cpu()), lambda: pa.group_points(xyz[0], cen, pts, idx),
           lambda: pa.group_points(xyz, cen[:1], pts, idx), lambda: pa.group_points(xyz, cen, pts[:, :19], idx), lambda: pa.group_points(xyz, cen, pts, idx[:, :5]),
           lambda: pa.group_points(xyz, cen, pts, idx.float()), lambda: pa.group_points(xyz.double(), cen, pts, idx), lambda: pa.group_points(xyz, cen, pts.half(), idx),
           lambda: pa.group_points(xyz, cen, pts, idx, channels_first=True), lambda: pa.group_points(xyz[..., :2], cen, pts, idx),
           lambda: pa.set_abstraction_group(4, 0.5, 6, xyz, pts), lambda: pa.set_abstraction_msg_group(4, [0.5], [6, 8], xyz.transpose(1, 2), None),
           lambda: pa.set_abstraction_msg_group(4, [0.5], [6], xyz.transpose(1, 2), pts)]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("call %d did not raise" % k)
    with pytest.raises(RuntimeError, match="group_points: float32 only"):
        pa.group_points(xyz.double(), cen, pts, idx)
    with pytest.raises(RuntimeError, match="group_points: expected"):
        pa.group_points(xyz, cen[:1], pts, idx)
    assert pa.group_points(xyz[:0], cen[:0], pts[:0], idx[:0]).shape == (0, 6, 5, 7)
    assert pa.group_points(xyz, cen, pts, idx).shape == (2, 6, 5, 7)                  # and the library is still usable


# ---- the speed condition --------------------------------------------------------------------------------------------------------
def torch_group(xyz, new_xyz, points, idx):
    """The torch spelling of point_cloud/pointnet_utils.py:117-122 and :185 on the device: index_points twice, the subtraction, cat, and
    the permute made contiguous as the first Conv2d makes it."""
    import poseestimation_amd as pa
    grouped = pa.index_points(xyz, idx) - new_xyz[:, :, None, :]
    return torch.cat([grouped, pa.index_points(points, idx)], dim=-1).permute(0, 3, 2, 1).contiguous()


def test_grouping_is_not_slower_than_the_torch_spelling(dev):
    """HIP events, 5 warm-ups, median of 20, same process, whole Python calls: group_points(channels_first=True) forward, and forward +
    backward into xyz, new_xyz and points, at the reference model's first set-abstraction level (32 x 1024, 512 centres, K = 64,
    D = 3) against the torch spelling and its autograd backward."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n, s, k, d = 32, 1024, 512, 64, 3
    g = torch.Generator().manual_seed(251)
    xyz = (torch.rand(b, n, 3, generator=g) - 0.5).to(dev).requires_grad_(True)
    pts = torch.randn(b, n, d, generator=g).to(dev).requires_grad_(True)
    pts_cf = pts.detach().transpose(1, 2).contiguous().requires_grad_(True)
    with torch.no_grad():
        centres = pa.index_points(xyz, pa.farthest_point_sample(xyz, s, 0))
        idx = pa.query_ball_point(0.2, k, xyz, centres)
    centres.requires_grad_(True)
    cot = torch.randn(b, 3 + d, k, s, generator=g).to(dev)
    ours = lambda: pa.group_points(xyz, centres, pts_cf, idx, channels_first=True)
    theirs = lambda: torch_group(xyz, centres, pts, idx)
    with torch.no_grad():
        assert torch.equal(ours(), theirs())
        ours_f, theirs_f = median_ms(ours), median_ms(theirs)

    def both(fn):
        for t in (xyz, centres, pts, pts_cf):
            t.grad = None
        fn().backward(cot)

    ours_fb, theirs_fb = median_ms(lambda: both(ours)), median_ms(lambda: both(theirs))
    line = ("group_points 32x1024, 512 centres, K=64, D=3, channel-first: forward %.4f ms, torch spelling %.4f ms (x%.1f); forward + backward %.4f ms, "
            "torch %.4f ms (x%.1f)" % (ours_f, theirs_f, theirs_f / ours_f, ours_fb, theirs_fb, theirs_fb / ours_fb))
    print(line)
    REPORT_LINES.append(line)
    assert theirs_f / ours_f >= 1, (ours_f, theirs_f)
    assert theirs_fb / ours_fb >= 1, (ours_fb, theirs_fb)
