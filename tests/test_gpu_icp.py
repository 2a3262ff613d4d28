"""nearest_neighbors and icp_align on the GPU: G21 through the Python surface and through the raw C ABI with the checks and bounds of
tests/test_icp_host.py (4 x the float32 host model's error; see its docstring), batch shapes that force each work-item size of
k_icp_step against the float64 restatement on the same random input, the boundary cases, replay from a graph, and the speed
conditions against the compositions the feature replaces."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import icp_ref as ref
from support import dev, median_ms, ptr, to_device  # noqa: F401
import test_icp_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21_cases():
    return ref.cases(ref.g21())


def surface_run(c, dev):
    import poseestimation_amd as pa
    P, Q, w, R0, t0 = (to_device(c[k], dev) for k in ("P", "Q", "w", "R0", "t0"))
    if c["kind"] == "search":
        dist, idx = pa.nearest_neighbors(P, Q)
        assert dist.shape == idx.shape == (c["b"], c["n"]) and dist.dtype == torch.float32 and idx.dtype == torch.int64
        return {"dist": dist.cpu().numpy(), "nearest": idx.cpu().numpy()}
    R, t, info = pa.icp_align(P, Q, R0, t0, iterations=c["iterations"], max_distance=c["max_distance"], weights=w, return_info=True)
    assert R.shape == (c["b"], 3, 3) and t.shape == (c["b"], 3) and info["rmse"].shape == info["inliers"].shape == (c["iterations"], c["b"])
    assert info["nearest"].dtype == torch.int64 and info["inliers"].dtype == torch.int64 and info["dist"].shape == (c["b"], c["n"])
    R2, t2 = pa.icp_align(P, Q, R0, t0, iterations=c["iterations"], max_distance=c["max_distance"], weights=w)      # the same bits from call to call
    assert torch.equal(R2, R) and torch.equal(t2, t)
    return {"R": R.cpu().numpy(), "t": t.cpu().numpy(), **{k: v.cpu().numpy() for k, v in info.items()}}


def abi_run(c, dev):
    """One case through the raw C ABI, on device buffers filled with NaN / -1 and a workspace filled with NaN (it needs no zero-fill)."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, m, it = c["b"], c["n"], c["m"], c["iterations"]
    P, Q, w, T0 = to_device(c["P"], dev), to_device(c["Q"], dev), to_device(c["w"], dev), to_device(host.initial_rows(c), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"dist": torch.full((b, n), np.nan, device=dev), "nearest": torch.full((b, n), -1, dtype=torch.int32, device=dev)}
    stride = 0 if c["shared"] else 3 * m
    if c["kind"] == "search":
        _lib.check(lib.so3_nearest_f32(ptr(P), ptr(Q), stride, ptr(out["dist"]), ptr(out["nearest"]), b, n, m, st), "so3_nearest_f32")
        d2 = torch.full((b, n), np.nan, device=dev)                                        # nearest is optional
        _lib.check(lib.so3_nearest_f32(ptr(P), ptr(Q), stride, ptr(d2), None, b, n, m, st), "so3_nearest_f32")
        assert torch.equal(d2, out["dist"])
    else:
        out.update(R=torch.full((b, 3, 3), np.nan, device=dev), t=torch.full((b, 3), np.nan, device=dev), rmse=torch.full((it, b), np.nan, device=dev),
                   inliers=torch.full((it, b), -1, dtype=torch.int32, device=dev))
        work = torch.full((lib.so3_icp_workspace_bytes(b, n) // 4,), np.nan, device=dev)
        md = -1.0 if c["max_distance"] is None else c["max_distance"]
        _lib.check(lib.so3_icp_f32(ptr(P), ptr(Q), stride, ptr(w), ptr(T0), md, it, ptr(out["R"]), ptr(out["t"]), ptr(out["rmse"]), ptr(out["inliers"]),
                                   ptr(out["nearest"]), ptr(out["dist"]), ptr(work), b, n, m, st), "so3_icp_f32")
        R2, t2 = torch.full((b, 3, 3), np.nan, device=dev), torch.full((b, 3), np.nan, device=dev)      # every optional output left out
        _lib.check(lib.so3_icp_f32(ptr(P), ptr(Q), stride, ptr(w), ptr(T0), md, it, ptr(R2), ptr(t2), None, None, None, None, ptr(work), b, n, m, st),
                   "so3_icp_f32")
        assert torch.equal(R2, out["R"]) and torch.equal(t2, out["t"])
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- G21 ------------------------------------------------------------------------------------------------------------------------
def test_g21_through_the_python_surface(dev, g21_cases):
    host.check_against_g21(g21_cases, lambda c: surface_run(c, dev), "surface")


def test_g21_through_the_c_abi(dev, g21_cases):
    host.check_against_g21(g21_cases, lambda c: abi_run(c, dev), "abi")


# ---- every work-item size -------------------------------------------------------------------------------------------------------
def _rule(b, n, cus):
    u = 4
    while u > 1 and b * ((n + 256 * u - 1) // (256 * u)) < 2 * cus:
        u >>= 1
    return u


SHAPES = [(1, 1000), (64, 1024), (300, 1024), (600, 1024)]       # on 256 compute units: U = 1, 1, 2, 4


@pytest.mark.parametrize("b,n", SHAPES, ids=lambda v: str(v))
def test_batch_shapes_against_float64(dev, b, n):
    """One weighted step from a small initial motion at M = 1024: checks 1 and 2 against icp_ref on the same random input (its search in
    float64 on the GPU), and the instantiation the launcher's rule names."""
    import poseestimation_amd as pa
    from poseestimation_amd import _lib
    m = 1024
    rng = np.random.default_rng(1000 + b)
    ball = lambda *shape: (lambda d: d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0, 1, shape + (1,)) ** (1 / 3))(rng.standard_normal(shape + (3,)))
    Q = ball(b, m).astype(np.float32)
    P = (Q[:, rng.permutation(m)[:n] if n <= m else rng.integers(0, m, n)] + 0.03 * rng.standard_normal((b, n, 3))).astype(np.float32)
    w = rng.uniform(0.05, 1.0, (b, n)).astype(np.float32)
    ang = np.deg2rad(2.0)
    R0 = np.broadcast_to(np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]], np.float32), (b, 3, 3)).copy()
    t0 = np.full((b, 3), 0.02, np.float32)
    R, t, info = pa.icp_align(to_device(P, dev), to_device(Q, dev), to_device(R0, dev), to_device(t0, dev), iterations=1, weights=to_device(w, dev), return_info=True)
    name = _lib.load().so3_last_kernel().decode()
    u = _rule(b, n, torch.cuda.get_device_properties(dev).multi_processor_count)
    assert name == "k_icp_step<true, false, true, %d>" % u, (name, u)
    got = {"R": R.cpu().numpy(), "t": t.cpu().numpy(), **{k: v.cpu().numpy() for k, v in info.items()}}
    R64, t64 = R0.astype(np.float64), t0.astype(np.float64)
    f = host.search_figures(ref.pose_points(P, R64, t64), Q, got["dist"], got["nearest"], device=dev)
    f.update(host.step_figures(P, Q, w, R64, t64, None, got))
    print("B=%d N=%d U=%d  " % (b, n, u) + "  ".join("%s %.2e" % kv for kv in f.items()))
    for k, v in f.items():
        assert v <= host.bounds()[k], (k, v, host.bounds()[k])
    dist, idx = pa.nearest_neighbors(to_device(ref.pose_points(P, R64, t64), dev), to_device(Q, dev))          # the search alone, same U
    assert _lib.load().so3_last_kernel().decode() == "k_icp_step<false, false, false, %d>" % u
    f = host.search_figures(ref.pose_points(P, R64, t64).astype(np.float32), Q, dist.cpu().numpy(), idx.cpu().numpy(), device=dev)
    assert max(f.values()) <= host.SEARCH_TOL, f


def test_the_shapes_cover_every_work_item_size(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert {_rule(b, n, cus) for b, n in SHAPES} == {1, 2, 4}, cus


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_zero_iterations_empty_inliers_shapes_and_warnings(dev):
    import poseestimation_amd as pa
    g = torch.Generator().manual_seed(5)
    P, Q = torch.rand(3, 70, 3, generator=g).to(dev), torch.rand(3, 90, 3, generator=g).to(dev) + 5.0
    R0 = torch.linalg.qr(torch.randn(3, 3, 3, generator=g))[0]
    R0 = (R0 * torch.linalg.det(R0)[:, None, None]).to(dev)
    t0 = torch.randn(3, 3, generator=g).to(dev)
    R, t, info = pa.icp_align(P, Q, R0, t0, iterations=0, return_info=True)                  # the initial pose, and the search at it
    assert torch.equal(R, R0) and torch.equal(t, t0) and info["rmse"].shape == (0, 3) and info["inliers"].shape == (0, 3)
    d, idx = pa.nearest_neighbors(torch.einsum("bij,bnj->bni", R0, P) + t0[:, None], Q)
    assert (info["dist"] - d).abs().max().item() <= 1e-5 and info["nearest"].shape == (3, 70)      # torch posed these points: not an accuracy check
    R, t = pa.icp_align(P, Q, iterations=0)
    assert torch.equal(R, torch.eye(3, device=dev).expand(3, 3, 3)) and (t == 0).all()
    R, t, info = pa.icp_align(P, Q, R0, t0, iterations=4, max_distance=1e-3, return_info=True)      # nothing within reach: the pose stays
    assert torch.equal(R, R0) and torch.equal(t, t0) and (info["rmse"] == 0).all() and (info["inliers"] == 0).all()
    R, t, info = pa.icp_align(P, Q, iterations=2, weights=torch.zeros(3, 70, device=dev), return_info=True)
    assert torch.equal(R, torch.eye(3, device=dev).expand(3, 3, 3)) and (t == 0).all() and (info["inliers"] == 0).all()
    for bad in (lambda: pa.icp_align(P, Q[:2]), lambda: pa.icp_align(P, Q, weights=torch.zeros(3, 71, device=dev)), lambda: pa.icp_align(P, Q, R0[:2]),
                lambda: pa.icp_align(P, Q, iterations=-1), lambda: pa.nearest_neighbors(P[0], Q), lambda: pa.nearest_neighbors(P, Q[..., :2])):
        with pytest.raises(RuntimeError):
            bad()
    from poseestimation_amd import rotation_representation as rr
    rr._WARNED.discard("icp_align")
    rr._WARNED.discard("nearest_neighbors")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            R, t = pa.icp_align(P.clone().requires_grad_(True), Q, iterations=1)
            d, _ = pa.nearest_neighbors(P, Q.clone().requires_grad_(True))
    assert not R.requires_grad and not d.requires_grad
    assert sum("icp_align is not differentiable" in str(w.message) for w in seen) == 1
    assert sum("nearest_neighbors is an evaluation call" in str(w.message) for w in seen) == 1


def test_the_documented_gradient_path(dev, g21_cases):
    """rigid_align on the returned correspondences reproduces the last step and is differentiable."""
    import poseestimation_amd as pa
    c = next(c for c in g21_cases if c["kind"] == "noise" and c["max_distance"] is not None)
    P, Q, R0, t0 = (to_device(c[k], dev) for k in ("P", "Q", "R0", "t0"))
    R, t, info = pa.icp_align(P, Q, R0, t0, iterations=20, max_distance=c["max_distance"], return_info=True)
    Pg = P.clone().requires_grad_(True)
    w = (info["dist"] <= c["max_distance"]).float()
    R2, t2 = pa.rigid_align(Pg, Q.gather(1, info["nearest"][..., None].expand(-1, -1, 3)), w)
    assert (R2 - R).abs().max().item() <= 2 * host.R_TOL and (t2 - t).abs().max().item() <= 2 * host.T_TOL
    (g,) = torch.autograd.grad(R2.sum() + t2.sum(), [Pg])
    assert torch.isfinite(g).all() and g.abs().max().item() > 0


def test_replay_from_a_graph(dev, g21_cases):
    """One call captured and replayed twice: a single chain of launches, no host synchronisation, the same bits every time."""
    import poseestimation_amd as pa
    c = next(c for c in g21_cases if c["kind"] == "noise" and c["max_distance"] is not None)
    P, Q, R0, t0 = (to_device(c[k], dev) for k in ("P", "Q", "R0", "t0"))
    call = lambda: pa.icp_align(P, Q, R0, t0, iterations=5, max_distance=c["max_distance"], return_info=True)
    R, t, info = call()
    eager = [R.clone(), t.clone()] + [info[k].clone() for k in ("rmse", "inliers", "nearest", "dist")]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                                                     # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        R, t, info = call()
    captured = [R, t] + [info[k] for k in ("rmse", "inliers", "nearest", "dist")]
    for _ in range(2):
        for x in captured:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


# ---- the speed conditions -------------------------------------------------------------------------------------------------------
def test_icp_is_not_slower_than_the_composition(dev):
    """B = 256, N = M = 1024, HIP events, 5 warm-ups, median of 20, same process.  (a) nearest_neighbors against torch.cdist(X, Y).min(-1);
    (b) icp_align(iterations=10) against what the parent commit offers: cdist -> argmin -> gather -> rigid_align -> apply, ten times."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n = 256, 1024
    g = torch.Generator().manual_seed(211)
    Q = (torch.rand(b, n, 3, generator=g) - 0.5).to(dev)
    rot = torch.tensor([[np.cos(0.03), -np.sin(0.03), 0.0], [np.sin(0.03), np.cos(0.03), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    P = (Q[:, torch.randperm(n, generator=g).to(dev)] - 0.01) @ rot + 0.005 * torch.randn(b, n, 3, generator=g).to(dev)

    def composed(iterations=10):
        R = torch.eye(3, device=dev).expand(b, 3, 3)
        t = torch.zeros(b, 3, device=dev)
        for _ in range(iterations):
            x = torch.einsum("bij,bnj->bni", R, P) + t[:, None]
            idx = torch.cdist(x, Q).argmin(-1)
            R, t = pa.rigid_align(P, Q.gather(1, idx[..., None].expand(-1, -1, 3)))
        return R, t

    with torch.no_grad():
        ours_a = median_ms(lambda: pa.nearest_neighbors(P, Q))
        theirs_a = median_ms(lambda: torch.cdist(P, Q).min(-1))
        ours_b = median_ms(lambda: pa.icp_align(P, Q, iterations=10))
        theirs_b = median_ms(composed)
        (R, t), (Rc, tc) = pa.icp_align(P, Q, iterations=10), composed()
    assert (R - Rc).abs().max().item() < 1e-3 and (t - tc).abs().max().item() < 1e-3      # the same quantity (not an accuracy check)
    for line in ("nearest_neighbors B=256 N=M=1024: %.4f ms, torch.cdist(X, Y).min(-1) %.4f ms (x%.1f)" % (ours_a, theirs_a, theirs_a / ours_a),
                 "icp_align(iterations=10) B=256 N=M=1024: %.4f ms, cdist + argmin + gather + rigid_align x 10 %.4f ms (x%.1f)" % (ours_b, theirs_b, theirs_b / ours_b)):
        print(line)
        REPORT_LINES.append(line)
    assert theirs_a / ours_a >= 1, (ours_a, theirs_a)
    assert theirs_b / ours_b >= 1, (ours_b, theirs_b)
