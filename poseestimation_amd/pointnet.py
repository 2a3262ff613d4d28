"""The PointNet++ operators: farthest-point sampling, ball query and grouping (set abstraction), and three_nn / three_interpolate
(feature propagation).  One family of the Python mirror; rotation_representation re-exports its public names."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._runtime import _capturing, _cloud_f32, _launch, _no_double_backward, _ptr, _require_device, _wants_grad, _warn_once


# --------------------------------------------------------------------------------------------
# PointNet++ sampling and grouping (reference: point_cloud/pointnet_utils.py)
# --------------------------------------------------------------------------------------------
def farthest_point_sample(xyz: torch.Tensor, npoint: int, start=None) -> torch.Tensor:
    """point_cloud/pointnet_utils.py:53-74 in one launch: (B, npoint) int64 indices of the farthest-point sample of xyz (B, N, 3).
    out[:, 0] is the first index; every further index is the point farthest from all chosen so far, the lowest index among equals.

    start=None draws the first index with torch.randint(0, N, (B,)) as the reference does (on the device).  An int, or a (B,)
    integer tensor, fixes it; an index outside [0, N) raises a RuntimeError.  An int or a CPU tensor is checked on the host; a
    DEVICE tensor is checked by reading one flag back, which synchronises -- except while the stream is being captured into a graph,
    where the kernel clamps the index into range instead.  With start=None or an int nothing synchronises with the host.

    The arithmetic is a definition (include/so3proj.h): d = ((dx * dx) + (dy * dy)) + (dz * dz) in float32 without fused
    multiply-add, a running minimum from 1e10, the argmax with the lowest index among equal values.  It equals the reference's loop
    on the CPU index for index from the same start.  1 <= N <= FPS_MAX_N (16384), 1 <= npoint <= FPS_MAX_N; npoint > N gives index 0
    once every point is taken.  One workgroup per cloud (so3_fps_f32).  Other float dtypes are converted to float32.  The
    indices carry no gradient, as the reference's."""
    dev, x = _cloud_f32("farthest_point_sample", "xyz", xyz)
    b, n = x.shape[0], x.shape[1]
    npoint = int(npoint)
    if n > _lib.FPS_MAX_N or not 1 <= npoint <= _lib.FPS_MAX_N:
        raise RuntimeError("farthest_point_sample: expected 1 <= N <= %d and 1 <= npoint <= %d, got N = %d, npoint = %d"
                           % (_lib.FPS_MAX_N, _lib.FPS_MAX_N, n, npoint))
    if start is None:
        first = torch.randint(0, n, (b,), device=dev, dtype=torch.int32)
    elif isinstance(start, torch.Tensor):
        if start.dim() != 1 or start.shape[0] != b or start.dtype.is_floating_point or start.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise RuntimeError("farthest_point_sample: start must be an int or an integer tensor of shape (%d,), got %s %s"
                               % (b, start.dtype, tuple(start.shape)))
        if b and not (start.is_cuda and _capturing(dev)) and bool(((start < 0) | (start >= n)).any()):
            raise RuntimeError("farthest_point_sample: start index outside [0, %d)" % n)
        first = start.detach().to(device=dev, dtype=torch.int32).contiguous()
    else:
        if not 0 <= int(start) < n:
            raise RuntimeError("farthest_point_sample: start index %d outside [0, %d)" % (int(start), n))
        first = torch.full((b,), int(start), device=dev, dtype=torch.int32)
    out = torch.empty((b, npoint), dtype=torch.int32, device=dev)
    _launch(dev, "so3_fps_f32", _ptr(x), _ptr(first), _ptr(out), b, n, npoint)
    return out.long()


def query_ball_point(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, return_counts: bool = False):
    """point_cloud/pointnet_utils.py:77-97 in one launch, without the (B, S, N) tensors and the sort: for every centre new_xyz[b, s]
    the first nsample indices j, in ascending j, of the points of xyz[b] with |new_xyz_s - xyz_j|^2 <= radius^2; the remaining slots
    repeat the first hit.  xyz: (B, N, 3), new_xyz: (B, S, 3); the result is (B, S, min(nsample, N)) int64.

    A centre WITHOUT a hit gets N in every slot, as the reference does -- an index one past the cloud, which index_points would
    refuse.  return_counts=True also returns a (B, S) int64 count of the points in each ball, NOT clipped to nsample: look there
    (count == 0) before gathering when centres may be empty.  Centres that are cloud points (sample_and_group's) always hit themselves.

    The distance comes from coordinate differences, d = ((dx * dx) + (dy * dy)) + (dz * dz) in float32, and the test is
    not (d > radius * radius) (include/so3proj.h).  The reference expands |a|^2 + |b|^2 - 2 a.b, so a point within rounding of the
    sphere can fall on the other side there; that is the only difference.  One wave per centre (so3_ball_query_f32); without
    return_counts a centre's scan stops once its row is full.  Nothing synchronises with the host.  No gradient, as the reference's."""
    dev, x = _cloud_f32("query_ball_point", "xyz", xyz)
    _, c = _cloud_f32("query_ball_point", "new_xyz", new_xyz)
    _require_device(x, c)
    b, n, s = x.shape[0], x.shape[1], c.shape[1]
    nsample = int(nsample)
    if c.shape[0] != b or n > _lib.ADD_S_MAX_N or s > _lib.ADD_S_MAX_N or nsample < 1:
        raise RuntimeError("query_ball_point: expected xyz (B, N, 3) and new_xyz (B, S, 3) with 1 <= N, S <= %d and nsample >= 1, got %s, %s "
                           "and nsample = %d" % (_lib.ADD_S_MAX_N, tuple(xyz.shape), tuple(new_xyz.shape), nsample))
    idx = torch.empty((b, s, min(nsample, n)), dtype=torch.int32, device=dev)
    count = torch.empty((b, s), dtype=torch.int32, device=dev) if return_counts else None
    _launch(dev, "so3_ball_query_f32", _ptr(x), _ptr(c), float(radius), min(nsample, 2**31 - 1), _ptr(idx), _ptr(count), b, n, s)
    return (idx.long(), count.long()) if return_counts else idx.long()


def index_points(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """point_cloud/pointnet_utils.py:34-50: points (B, N, C) gathered by idx (B, S) -> (B, S, C) or (B, S, K) -> (B, S, K, C).
    Plain torch indexing on the tensors' device, differentiable in points."""
    if points.dim() != 3 or idx.dim() not in (2, 3) or idx.shape[0] != points.shape[0]:
        raise RuntimeError("index_points: expected points (B, N, C) and idx (B, S) or (B, S, K), got %s and %s" % (tuple(points.shape), tuple(idx.shape)))
    batch = torch.arange(points.shape[0], dtype=torch.long, device=points.device).view(-1, *([1] * (idx.dim() - 1)))
    return points[batch, idx.long(), :]


def sample_and_group(npoint: int, radius: float, nsample: int, xyz: torch.Tensor, points: torch.Tensor, returnfps: bool = False, start=None):
    """point_cloud/pointnet_utils.py:100-128, a set-abstraction layer's sampling and grouping: farthest_point_sample (from `start`),
    the sampled centres new_xyz (B, npoint, 3), query_ball_point around them, and new_points (B, npoint, K, 3 + D) = the grouped
    coordinates relative to their centre, concatenated with the grouped features of points (B, N, D) (points=None: the coordinates
    alone); K = min(nsample, N).  Returns (new_xyz, new_points), with returnfps=True (new_xyz, new_points, grouped_xyz, fps_idx).
    new_points is differentiable in xyz and points through the gathers; the indices carry no gradient."""
    fps_idx = farthest_point_sample(xyz, npoint, start)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    grouped_xyz = index_points(xyz, idx)
    new_points = grouped_xyz - new_xyz[:, :, None, :]
    if points is not None:
        new_points = torch.cat([new_points, index_points(points, idx)], dim=-1)
    if returnfps:
        return new_xyz, new_points, grouped_xyz, fps_idx
    return new_xyz, new_points


def sample_and_group_all(xyz: torch.Tensor, points: torch.Tensor):
    """point_cloud/pointnet_utils.py:131-148, the group_all branch of a set-abstraction layer, plain torch: xyz (B, N, 3) and points
    (B, N, D) or None -> (new_xyz (B, 1, 3) zeros, new_points (B, 1, N, 3 + D)), the coordinates as they are (no centre is subtracted)
    followed by the features.  Differentiable in xyz and points."""
    if xyz.dim() != 3 or (points is not None and (points.dim() != 3 or points.shape[:2] != xyz.shape[:2])):
        raise RuntimeError("sample_and_group_all: expected xyz (B, N, C) and points (B, N, D) or None, got %s and %s"
                           % (tuple(xyz.shape), None if points is None else tuple(points.shape)))
    b, n, c = xyz.shape
    new_xyz = torch.zeros(b, 1, c, device=xyz.device)
    grouped_xyz = xyz.view(b, 1, n, c) if xyz.is_contiguous() else xyz.reshape(b, 1, n, c)
    if points is None:
        return new_xyz, grouped_xyz
    return new_xyz, torch.cat([grouped_xyz, points.reshape(b, 1, n, -1)], dim=-1)


class _GroupPoints(torch.autograd.Function):
    """group_points as a graph node: backward is one call of so3_group_points_bwd_f32, a gather over the stored indices in a fixed
    order (no atomics: the same bits from call to call), reading grad_out in the forward's output layout; only the gradients that are
    needed are requested."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, points, idx32, channels_first, features_first, dims):
        b, n, s, k, d = dims
        dev = xyz.device
        x, c = xyz.detach().contiguous(), new_xyz.detach().contiguous()
        f = points.detach().contiguous() if d else None
        cf, ff = 1 if channels_first else 0, 1 if features_first else 0
        out = torch.empty((b, 3 + d, k, s) if channels_first else (b, s, k, 3 + d), dtype=torch.float32, device=dev)
        _launch(dev, "so3_group_points_f32", _ptr(x), _ptr(c), _ptr(f), _ptr(idx32), _ptr(out), ff, cf, b, n, s, k, d)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(idx32)
        ctx.meta = (cf, ff, dims, dev)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx32,) = ctx.saved_tensors
        cf, ff, (b, n, s, k, d), dev = ctx.meta
        need = ctx.needs_input_grad
        if grad_out is None or not (need[0] or need[1] or (need[2] and d)):
            return None, None, None, None, None, None, None
        _no_double_backward(grad_out)
        g = grad_out.detach().contiguous()
        gx = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if need[0] else None
        gc = torch.empty((b, s, 3), dtype=torch.float32, device=dev) if need[1] else None
        gf = torch.empty((b, d, n) if cf else (b, n, d), dtype=torch.float32, device=dev) if need[2] and d else None
        _launch(dev, "so3_group_points_bwd_f32", _ptr(g), _ptr(idx32), _ptr(gx), _ptr(gc), _ptr(gf), ff, cf, b, n, s, k, d)
        return gx, gc, gf, None, None, None, None


def group_points(xyz: torch.Tensor, new_xyz: torch.Tensor, points, idx: torch.Tensor, channels_first: bool = False,
                 features_first: bool = False) -> torch.Tensor:
    """point_cloud/pointnet_utils.py:117-124 (sample_and_group) and :234-242 (PointNetSetAbstractionMsg.forward) in one launch: the
    coordinates xyz (B, N, 3) gathered by idx (B, S, K) relative to their centre new_xyz (B, S, 3), concatenated with the gathered
    features.  points is None, (B, N, D), or (B, D, N) with channels_first=True; the result is (B, S, K, 3 + D), or with
    channels_first=True (B, 3 + D, K, S), what the layer's permute(0, 3, 2, 1) hands to its Conv2d -- already contiguous.
    features_first=False is sample_and_group's channel order, cat([xyz_norm, points]); features_first=True the Msg layer's,
    cat([grouped_points, grouped_xyz]).  idx is int64 or int32, as query_ball_point returns it.

    The forward is a definition (include/so3proj.h): one float32 subtraction per coordinate, a copy per feature.  AN INDEX OUTSIDE
    [0, N) -- query_ball_point writes N into every slot of an empty ball -- gives 0 in every channel of that slot and takes no
    gradient, where the reference's index_points raises an IndexError; nothing is read or written outside the tensors.

    Differentiable in xyz, new_xyz and points through ONE backward call (so3_group_points_bwd_f32) that computes only the gradients
    that are needed: every point sums its hits in the ascending memory order of grad_out's slots -- no atomics, no zero-fill, the same
    bits from call to call; a point nobody selected gets exactly 0.  A non-contiguous grad_out is copied first.  Double backward is
    refused.  float32 only.  1 <= N, S <= ADD_S_MAX_N, 1 <= K <= GROUP_MAX_K, D <= THREE_MAX_D."""
    tensors = (xyz, new_xyz, idx) if points is None else (xyz, new_xyz, points, idx)
    dev = _require_device(*tensors)
    ok = xyz.dim() == 3 and new_xyz.dim() == 3 and idx.dim() == 3 and xyz.shape[-1] == 3 and new_xyz.shape[-1] == 3 \
        and new_xyz.shape[0] == xyz.shape[0] and idx.shape[:2] == new_xyz.shape[:2]
    if ok and points is not None:
        ok = points.dim() == 3 and points.shape[0] == xyz.shape[0] and points.shape[2 if channels_first else 1] == xyz.shape[1]
    if not ok or idx.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("group_points: expected xyz (B, N, 3), new_xyz (B, S, 3), points %s or None and idx (B, S, K) (int32 or int64), got "
                           "%s, %s, %s and %s %s" % ("(B, D, N)" if channels_first else "(B, N, D)", tuple(xyz.shape), tuple(new_xyz.shape),
                                                     None if points is None else tuple(points.shape), idx.dtype, tuple(idx.shape)))
    if any(t.dtype is not torch.float32 for t in tensors[:-1]):
        raise RuntimeError("group_points: float32 only, got %s" % ", ".join(str(t.dtype) for t in tensors[:-1]))
    b, n, s, k = xyz.shape[0], xyz.shape[1], idx.shape[1], idx.shape[2]
    d = 0 if points is None else points.shape[1 if channels_first else 2]
    if not (1 <= n <= _lib.ADD_S_MAX_N and 1 <= s <= _lib.ADD_S_MAX_N and 1 <= k <= _lib.GROUP_MAX_K and d <= _lib.THREE_MAX_D):
        raise RuntimeError("group_points: expected 1 <= N, S <= %d, 1 <= K <= %d and D <= %d, got N = %d, S = %d, K = %d, D = %d"
                           % (_lib.ADD_S_MAX_N, _lib.GROUP_MAX_K, _lib.THREE_MAX_D, n, s, k, d))
    if b == 0:
        return xyz.new_zeros((0, 3 + d, k, s) if channels_first else (0, s, k, 3 + d))
    idx32 = idx.detach().contiguous().int()
    return _GroupPoints.apply(xyz, new_xyz, points if d else None, idx32, bool(channels_first), bool(features_first), (b, n, s, k, d))


def _abstraction_args(name, xyz, points):
    _require_device(*((xyz,) if points is None else (xyz, points)))
    if xyz.dim() != 3 or xyz.shape[1] != 3 or (points is not None and (points.dim() != 3 or points.shape[0] != xyz.shape[0] or points.shape[2] != xyz.shape[2])):
        raise RuntimeError("%s: expected xyz (B, 3, N) and points (B, D, N) or None, got %s and %s"
                           % (name, tuple(xyz.shape), None if points is None else tuple(points.shape)))
    return xyz.transpose(1, 2).contiguous()


def set_abstraction_group(npoint: int, radius: float, nsample: int, xyz: torch.Tensor, points, group_all: bool = False, start=None):
    """PointNetSetAbstraction.forward up to its MLP (point_cloud/pointnet_utils.py:175-185), in the layer's own channel-first layouts:
    xyz (B, 3, N), points (B, D, N) or None -> (new_xyz (B, 3, S), new_points (B, 3 + D, K, S)), S = npoint, K = min(nsample, N), the
    relative coordinates first.  Three launches: farthest_point_sample (from `start`), query_ball_point and
    group_points(..., channels_first=True), whose output is what the first Conv2d takes -- no permute, no copy.  With group_all=True
    (sample_and_group_all, :131-148) it returns ((B, 3, 1) zeros, (B, 3 + D, N, 1)): the coordinates as they are, then the features.
    Differentiable in xyz and points."""
    pts = _abstraction_args("set_abstraction_group", xyz, points)
    if group_all:
        new_points = (xyz if points is None else torch.cat([xyz, points], dim=1)).unsqueeze(-1)
        return torch.zeros(xyz.shape[0], 3, 1, device=xyz.device), new_points
    fps_idx = farthest_point_sample(pts, npoint, start)
    new_xyz = index_points(pts, fps_idx)
    idx = query_ball_point(radius, nsample, pts, new_xyz)
    return new_xyz.transpose(1, 2), group_points(pts, new_xyz, points, idx, channels_first=True)


def set_abstraction_msg_group(npoint: int, radius_list, nsample_list, xyz: torch.Tensor, points, start=None):
    """PointNetSetAbstractionMsg.forward up to its convolutions (point_cloud/pointnet_utils.py:223-242), in the layer's own layouts:
    xyz (B, 3, N), points (B, D, N) or None -> (new_xyz (B, 3, S), [(B, D + 3, K_i, S) for every radius]), the features first.  One
    farthest_point_sample (from `start`), then per radius one query_ball_point and one group_points(..., channels_first=True,
    features_first=True).  Differentiable in xyz and points."""
    pts = _abstraction_args("set_abstraction_msg_group", xyz, points)
    if len(radius_list) != len(nsample_list):
        raise RuntimeError("set_abstraction_msg_group: %d radii and %d sample counts" % (len(radius_list), len(nsample_list)))
    new_xyz = index_points(pts, farthest_point_sample(pts, npoint, start))
    groups = [group_points(pts, new_xyz, points, query_ball_point(radius, nsample, pts, new_xyz), channels_first=True, features_first=True)
              for radius, nsample in zip(radius_list, nsample_list)]
    return new_xyz.transpose(1, 2), groups


# --------------------------------------------------------------------------------------------
# PointNet++ feature propagation (reference: point_cloud/pointnet_utils.py:266-300, PointNetFeaturePropagation.forward)
# --------------------------------------------------------------------------------------------
def three_nn(xyz1: torch.Tensor, xyz2: torch.Tensor, return_weights: bool = False):
    """For every point of xyz1 (B, N, 3) the three nearest points of xyz2 (B, S, 3): (dist2, idx) with dist2 (B, N, 3) float32 the
    squared distances in ascending order and idx (B, N, 3) int64; with return_weights=True also weight (B, N, 3) float32, the
    normalised inverse-distance weights of point_cloud/pointnet_utils.py:290-292.  One launch (so3_three_nn_f32) instead of the
    (B, N, S) distance tensor and its full sort.

    The arithmetic is a definition (include/so3proj.h): d = ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences in
    float32 without fused multiply-add, the three smallest with the lower index first among equal d; r_k = 1 / (d_k + 1e-8),
    w_k = r_k / ((r_0 + r_1) + r_2).  A point of xyz1 that is also in xyz2 gets d = 0 exactly and (almost) all the weight, where the
    reference's expanded form returns rounding noise.  S < 3 is legal: the missing slots repeat slot 0's index with dist2 = +inf and
    weight 0 (S == 1: weight exactly 1, the reference's `repeat` branch).  1 <= N, S <= ADD_S_MAX_N.  Other float dtypes are converted
    to float32.  Nothing synchronises with the host.  The outputs carry no gradient (nor do the CUDA PointNet++ ops'); a cloud that
    requires grad is warned about once."""
    dev, x = _cloud_f32("three_nn", "xyz1", xyz1)
    _, y = _cloud_f32("three_nn", "xyz2", xyz2)
    _require_device(x, y)
    b, n, s = x.shape[0], x.shape[1], y.shape[1]
    if y.shape[0] != b or n > _lib.ADD_S_MAX_N or s > _lib.ADD_S_MAX_N:
        raise RuntimeError("three_nn: expected xyz1 (B, N, 3) and xyz2 (B, S, 3) with 1 <= N, S <= %d, got %s and %s"
                           % (_lib.ADD_S_MAX_N, tuple(xyz1.shape), tuple(xyz2.shape)))
    if _wants_grad(xyz1, xyz2):
        _warn_once("three_nn", "three_nn is not differentiable: distances, indices and weights carry no gradient although a cloud requires "
                               "grad (the reference's autograd reaches xyz through square_distance; nothing in its models sits upstream of xyz).")
    dist2 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=dev)
    weight = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if return_weights else None
    _launch(dev, "so3_three_nn_f32", _ptr(x), _ptr(y), _ptr(dist2), _ptr(idx), _ptr(weight), b, n, s)
    return (dist2, idx.long(), weight) if return_weights else (dist2, idx.long())


def _three_args(name, points2, idx, weight, channels_first):
    """Checked, contiguous float32 / int32 operands of the interpolation and (B, N, S, D)."""
    dev = _require_device(points2, idx, weight)
    ok = points2.dim() == 3 and idx.dim() == 3 and idx.shape[-1] == 3 and idx.shape == weight.shape and idx.shape[0] == points2.shape[0]
    if not ok or not points2.dtype.is_floating_point or not weight.dtype.is_floating_point or idx.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("%s: expected points2 %s (float), idx (B, N, 3) (int32 or int64) and weight (B, N, 3) (float), got %s %s, %s %s and %s %s"
                           % (name, "(B, D, S)" if channels_first else "(B, S, D)", points2.dtype, tuple(points2.shape), idx.dtype, tuple(idx.shape),
                              weight.dtype, tuple(weight.shape)))
    b, n = idx.shape[0], idx.shape[1]
    d, s = (points2.shape[1], points2.shape[2]) if channels_first else (points2.shape[2], points2.shape[1])
    if not (1 <= n <= _lib.ADD_S_MAX_N and 1 <= s <= _lib.ADD_S_MAX_N and 1 <= d <= _lib.THREE_MAX_D):
        raise RuntimeError("%s: expected 1 <= N, S <= %d and 1 <= D <= %d, got N = %d, S = %d, D = %d" % (name, _lib.ADD_S_MAX_N, _lib.THREE_MAX_D, n, s, d))
    return dev, idx.detach().contiguous().int(), weight.detach().contiguous().float(), b, n, s, d


class _ThreeInterpolate(torch.autograd.Function):
    """three_interpolate as a graph node: backward is one launch of so3_three_interpolate_bwd_f32, a gather over the stored indices in
    a fixed order (no atomics: the same bits from call to call), reading grad_out in the forward's output layout."""

    @staticmethod
    def forward(ctx, points2, idx32, w32, channels_first, dims):
        b, n, s, d = dims
        dev = points2.device
        f = points2.detach().contiguous().float()
        out = torch.empty((b, d, n) if channels_first else (b, n, d), dtype=torch.float32, device=dev)
        _launch(dev, "so3_three_interpolate_f32", _ptr(f), _ptr(idx32), _ptr(w32), _ptr(out), 1 if channels_first else 0, b, n, s, d)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(idx32, w32)
        ctx.meta = (bool(channels_first), dims, points2.dtype, dev)
        return out if points2.dtype is torch.float32 else out.to(points2.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        idx32, w32 = ctx.saved_tensors
        channels_first, (b, n, s, d), dtype, dev = ctx.meta
        if grad_out is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = grad_out.float().contiguous()
        grad = torch.empty((b, d, s) if channels_first else (b, s, d), dtype=torch.float32, device=dev)
        _launch(dev, "so3_three_interpolate_bwd_f32", _ptr(g), _ptr(idx32), _ptr(w32), _ptr(grad), 1 if channels_first else 0, b, n, s, d)
        return (grad if dtype is torch.float32 else grad.to(dtype)), None, None, None, None


def three_interpolate(points2: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor, channels_first: bool = False) -> torch.Tensor:
    """point_cloud/pointnet_utils.py:293 without the (B, N, 3, D) gather: out[b, n, c] = sum_k weight[b, n, k] * points2[b, idx[b, n, k], c].
    points2 is (B, S, D) and the result (B, N, D); with channels_first=True points2 is (B, D, S) and the result (B, D, N), the layout a
    PointNetFeaturePropagation layer receives and its Conv1d takes, so no permute().contiguous() is needed on either side.  idx and
    weight are (B, N, 3), as three_nn returns them (int64 or int32 indices; any weights).

    The order is fixed (include/so3proj.h): fma(w_2, f_2, fma(w_1, f_1, w_0 * f_0)) in float32.  Differentiable in points2: the
    backward is one launch that sums, for every known point, its hits in ascending (n, k) -- no atomics, the same bits from call to
    call; a known point nobody selected gets exactly 0.  Double backward is refused.  There is no gradient to weight or idx: a weight
    that requires grad is warned about once.

    EVERY INDEX MUST LIE IN [0, S).  The indices are not validated (three_nn's always are in range); the kernels clamp an index outside
    into the range, forward and backward alike, so a bad index gives a wrong value, never an access outside the tensors."""
    dev, idx32, w32, b, n, s, d = _three_args("three_interpolate", points2, idx, weight, channels_first)
    if _wants_grad(weight):
        _warn_once("three_interpolate", "three_interpolate is differentiable with respect to points2 only: weight carries no gradient although it "
                                        "requires grad.")
    if b == 0:
        return points2.new_zeros((0, d, n) if channels_first else (0, n, d))
    return _ThreeInterpolate.apply(points2, idx32, w32, bool(channels_first), (b, n, s, d))


def interpolate_features(xyz1: torch.Tensor, xyz2: torch.Tensor, points2: torch.Tensor, channels_first: bool = False) -> torch.Tensor:
    """point_cloud/pointnet_utils.py:283-293 in two launches: the features points2 of the known points xyz2 (B, S, 3) carried to the
    points xyz1 (B, N, 3) by inverse-distance weighting over the three nearest known points; three_nn(..., return_weights=True)
    followed by three_interpolate.  The clouds are (B, ., 3) in both layouts; channels_first only says how points2 and the result are laid out:
    (B, S, D) -> (B, N, D), or (B, D, S) -> (B, D, N).  Differentiable in points2."""
    _, idx, weight = three_nn(xyz1, xyz2, return_weights=True)
    return three_interpolate(points2, idx, weight, channels_first)


def propagate_features(xyz1: torch.Tensor, xyz2: torch.Tensor, points1, points2: torch.Tensor) -> torch.Tensor:
    """PointNetFeaturePropagation.forward up to its MLP (point_cloud/pointnet_utils.py:276-301), in the layer's own channel-first
    layout: xyz1 (B, 3, N), xyz2 (B, 3, S), points1 (B, D1, N) or None, points2 (B, D2, S) -> (B, D1 + D2, N), points1 first.  The
    interpolated half is interpolate_features(..., channels_first=True), S == 1 included (every point then takes the one known feature
    with weight 1); the concatenation is plain torch.  Differentiable in points1 and points2."""
    _require_device(xyz1, xyz2, points2)
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[1] != 3 or xyz2.shape[1] != 3:
        raise RuntimeError("propagate_features: expected xyz1 (B, 3, N) and xyz2 (B, 3, S), got %s and %s" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    out = interpolate_features(xyz1.transpose(1, 2), xyz2.transpose(1, 2), points2, channels_first=True)
    if points1 is None:
        return out
    _require_device(points1)
    if points1.dim() != 3 or points1.shape[0] != out.shape[0] or points1.shape[2] != out.shape[2]:
        raise RuntimeError("propagate_features: expected points1 (B, D1, N) with N = %d, got %s" % (out.shape[2], tuple(points1.shape)))
    return torch.cat([points1, out], dim=1)
