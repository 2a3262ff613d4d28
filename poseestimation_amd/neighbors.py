"""Clouds without known correspondences: the nearest-neighbour search and what stands on it -- both ICPs, the Chamfer distance,
K nearest neighbours with their gather and grouping, the per-point local frames and normals, FPFH descriptors with their matching, and
RANSAC over the matches up to a whole global registration.  One family of the Python mirror;
rotation_representation re-exports its public names."""
from __future__ import annotations

import torch

from . import _lib
from ._runtime import _cloud_lengths, _grad_to, _launch, _libh, _no_double_backward, _ptr, _require_device, _wants_grad, _warn_once
from .pointnet import group_points


# --------------------------------------------------------------------------------------------
# nearest neighbours between two clouds, and ICP on top of them
# --------------------------------------------------------------------------------------------
def _cloud_pair(name, X, Y, error=RuntimeError, shared_target=True):
    """float32 copies of a source (B,N,3) and a target (B,M,3) -- or, where `shared_target` allows it, one (M,3) for the batch --, and
    the target's stride in floats (0: shared).  The one shape check of the pair operations: `name` raises `error`."""
    dev = _require_device(X, Y)
    ok = X.dim() == 3 and X.shape[-1] == 3 and Y.dim() in ((2, 3) if shared_target else (3,)) and Y.shape[-1] == 3 \
        and (Y.dim() == 2 or Y.shape[0] == X.shape[0])
    if not ok or not 1 <= X.shape[1] <= _lib.ADD_S_MAX_N or not 1 <= Y.shape[-2] <= _lib.ADD_S_MAX_N:
        raise error("%s: expected a source (B, N, 3) and a target (B, M, 3)%s with 1 <= N, M <= %d, got %s and %s"
                    % (name, " or (M, 3)" if shared_target else "", _lib.ADD_S_MAX_N, tuple(X.shape), tuple(Y.shape)))
    x = X.detach().contiguous().float()
    y = Y.detach().contiguous().float()
    m = y.shape[-2]
    return dev, x, y, (0 if y.dim() == 2 else 3 * m), x.shape[0], x.shape[1], m


def nearest_neighbors(X: torch.Tensor, Y: torch.Tensor):
    """For every point of X its closest point of Y: (dist, idx) with dist (B,N) float32 = min_j |x_i - y_j|_2 and idx (B,N) int64 the
    argmin (the first of equal candidates).  X: (B,N,3); Y: (B,M,3), or (M,3) for one target shared by the batch.  N and M are
    independent.  One launch (so3_nearest_f32), N * M arithmetic per cloud and nothing of that size in memory; distances come from
    coordinate differences, so a point that is in both clouds gets exactly 0.  An evaluation call: not differentiable."""
    dev, x, y, stride, b, n, m = _cloud_pair("nearest_neighbors", X, Y)
    if _wants_grad(X, Y):
        _warn_once("nearest_neighbors", "nearest_neighbors is an evaluation call: dist carries no gradient although an argument requires grad.  "
                                        "(X - Y.gather(...)).norm() on the returned indices is the differentiable spelling.")
    dist = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n), dtype=torch.int32, device=dev)
    _launch(dev, "so3_nearest_f32", _ptr(x), _ptr(y), stride, _ptr(dist), _ptr(idx), b, n, m)
    return dist, idx.long()


def _icp_args(name, dev, b, n, R_init, t_init, weights, iterations, return_info):
    """What both ICPs do with their common arguments once the clouds are checked: the shape check of the extras (`name` raises), then
    (t0, w, r, t, rmse, inl, nearest, dist) -- the initial pose as (B, 3, 4) rows (R | t) or None, the float32 weights or None, the
    outputs R and t, and the info buffers, None unless return_info."""
    if (R_init is not None and tuple(R_init.shape) != (b, 3, 3)) or (t_init is not None and tuple(t_init.shape) != (b, 3)) or \
            (weights is not None and tuple(weights.shape) != (b, n)):
        raise RuntimeError("%s: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = %d, N = %d, got %s"
                           % (name, b, n, [None if x is None else tuple(x.shape) for x in (R_init, t_init, weights)]))
    t0 = None
    if R_init is not None or t_init is not None:
        r0 = R_init.detach().float() if R_init is not None else torch.eye(3, dtype=torch.float32, device=dev).expand(b, 3, 3)
        tt = t_init.detach().float() if t_init is not None else torch.zeros((b, 3), dtype=torch.float32, device=dev)
        t0 = torch.cat([r0, tt[:, :, None]], 2).contiguous()                       # (B, 3, 4): the rows (R | t)
    w = None if weights is None else weights.detach().contiguous().float()
    r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    rmse = inl = nearest = dist = None
    if return_info:
        rmse = torch.empty((iterations, b), dtype=torch.float32, device=dev)
        inl = torch.empty((iterations, b), dtype=torch.int32, device=dev)
        nearest = torch.empty((b, n), dtype=torch.int32, device=dev)
        dist = torch.empty((b, n), dtype=torch.float32, device=dev)
    return t0, w, r, t, rmse, inl, nearest, dist


def icp_align(P: torch.Tensor, Q: torch.Tensor, R_init: torch.Tensor = None, t_init: torch.Tensor = None, iterations: int = 10,
              max_distance: float = None, weights: torch.Tensor = None, return_info: bool = False):
    """Point-to-point ICP (iterative closest point): the pose (R, t) that registers the source clouds P onto the target clouds Q when
    the correspondences are NOT known.  P: (B,N,3); Q: (B,M,3), or (M,3) for one target shared by the batch; N and M are independent.
    Returns R (B,3,3) and t (B,3) in float32.

    One iteration, from the pose (R_k, t_k): x_i = R_k p_i + t_k; j(i) = the point of Q closest to x_i and d_i its distance;
    w'_i = w_i * [d_i <= max_distance] (all of w_i when max_distance is None; w_i = 1 when weights is None); (R_k+1, t_k+1) =
    rigid_align's answer for the pairs (p_i, q_j(i)) with weights w'.  The pose is solved from the unposed p_i every time, so it is
    an absolute pose and no composition error builds up.  A cloud without inlier weight keeps its pose.

    R_init (B,3,3) and t_init (B,3) give the initial pose (default: the identity).  Exactly `iterations` iterations run, without an
    early exit -- a converged cloud repeats its fixed point --, so nothing synchronises with the host and the call can be captured
    in a graph; the same inputs give the same bits.  iterations=0 returns the initial pose.  weights: None or (B,N), w_i >= 0.

    return_info=True also returns a dict: "rmse" (iterations,B) float32 = sqrt(sum w' d^2 / sum w') and "inliers" (iterations,B)
    int64 = #{w'_i > 0}, both measured at the pose the iteration STARTED from (0 and 0 where there was no inlier), and "nearest"
    (B,N) int64, "dist" (B,N) float32 of the last iteration's search.

    Not differentiable (the search is piecewise constant).  For gradients, differentiate the last step on the correspondences:
        R, t, info = icp_align(P, Q, ..., return_info=True)
        R, t = rigid_align(P, Q.gather(1, info["nearest"][..., None].expand(-1, -1, 3)), w)     # w: weights * (info["dist"] <= max_distance)"""
    dev, p, q, stride, b, n, m = _cloud_pair("icp_align", P, Q)
    extra = [x for x in (R_init, t_init, weights) if x is not None]
    if extra:
        _require_device(p, *extra)
    iterations = int(iterations)
    if iterations < 0:
        raise RuntimeError("icp_align: iterations must be >= 0, got %d" % iterations)
    t0, w, r, t, rmse, inl, nearest, dist = _icp_args("icp_align", dev, b, n, R_init, t_init, weights, iterations, return_info)
    if _wants_grad(P, Q, R_init, t_init, weights):
        _warn_once("icp_align", "icp_align is not differentiable: R and t carry no gradient although an argument requires grad.  Call "
                                "rigid_align on the returned correspondences (see the docstring) for a differentiable last step.")
    work = torch.empty((max(int(_libh().so3_icp_workspace_bytes(b, n)) // 4, 1),), dtype=torch.float32, device=dev)
    _launch(dev, "so3_icp_f32", _ptr(p), _ptr(q), stride, _ptr(w), _ptr(t0), -1.0 if max_distance is None else float(max_distance), iterations,
            _ptr(r), _ptr(t), _ptr(rmse), _ptr(inl), _ptr(nearest), _ptr(dist), _ptr(work), b, n, m)
    if return_info:
        return r, t, {"rmse": rmse, "inliers": inl.long(), "nearest": nearest.long(), "dist": dist}
    return r, t


def icp_align_plane(P: torch.Tensor, Q: torch.Tensor, normals: torch.Tensor = None, R_init: torch.Tensor = None, t_init: torch.Tensor = None,
                    iterations: int = 10, max_distance: float = None, weights: torch.Tensor = None, damping: float = 0.0,
                    normal_neighbors: int = 16, return_info: bool = False):
    """Point-to-plane ICP: as icp_align, but an iteration minimises sum w'_i (n_j(i) . (R p_i + t - q_j(i)))^2 over the target's surface
    normals instead of the point distances, so the source may slide along the surface and the pose converges in a fraction of the
    iterations on smooth scans.  P: (B,N,3); Q: (B,M,3), or (M,3) for one target shared by the batch.  Returns R (B,3,3), t (B,3).

    normals: (B,M,3), or (M,3) with a shared Q; None computes estimate_normals(Q, normal_neighbors) first.  Their sign does not
    matter (negating any of them changes no bit of the result), and a zero normal (a row past a length, a flat patch) takes its
    point out of the sums.  One iteration from (R_k, t_k): icp_align's search; w'_i = w_i [d_i <= max_distance] [n_i != 0]; the 6x6
    Gauss-Newton system of the linearised residuals about the posed first source point, its diagonal scaled by (1 + damping)
    (Levenberg-Marquardt; damping >= 0), solved by a Cholesky factorisation in registers; the pose is updated by the Cayley
    retraction of the rotation step and projected back onto SO(3), so long runs do not drift.  A cloud whose system has no unique
    solution (a plane, a sphere about its centre, fewer than six inliers: a pivot below 2^-7 of its diagonal entry) keeps its pose
    and reports solved = 0; damping > 0 makes such a system solvable.  Exactly `iterations` iterations, two launches each, no host
    synchronisation, no atomics: graph-capturable, the same bits every time.

    return_info=True also returns a dict: "rmse" (iterations,B) the point-to-plane rmse sqrt(sum w' r^2 / sum w'), "rmse_point"
    (iterations,B) = icp_align's rmse, "inliers" (iterations,B) int64 and "solved" (iterations,B) bool, all at the pose the iteration
    STARTED from, and "nearest" (B,N) int64, "dist" (B,N) float32 of the last iteration's search.

    Not differentiable.  For gradients, differentiate the last step on the correspondences with rigid_align, as icp_align's
    docstring shows (the point-to-point step on the converged pairs)."""
    dev, p, q, stride, b, n, m = _cloud_pair("icp_align_plane", P, Q)
    extra = [x for x in (normals, R_init, t_init, weights) if x is not None]
    if extra:
        _require_device(p, *extra)
    iterations = int(iterations)
    if iterations < 0:
        raise RuntimeError("icp_align_plane: iterations must be >= 0, got %d" % iterations)
    damping = float(damping)
    if not damping >= 0.0:
        raise RuntimeError("icp_align_plane: damping must be >= 0, got %r" % damping)
    if normals is not None and tuple(normals.shape) != tuple(Q.shape):
        raise RuntimeError("icp_align_plane: expected normals of the target's shape %s, got %s" % (tuple(Q.shape), tuple(normals.shape)))
    t0, w, r, t, rmse, inl, nearest, dist = _icp_args("icp_align_plane", dev, b, n, R_init, t_init, weights, iterations, return_info)
    if _wants_grad(P, Q, normals, R_init, t_init, weights):
        _warn_once("icp_align_plane", "icp_align_plane is not differentiable: R and t carry no gradient although an argument requires grad.  "
                                      "Call rigid_align on the returned correspondences (see icp_align's docstring) for a differentiable last step.")
    if normals is None:
        nrm = estimate_normals(q if q.dim() == 3 else q[None], int(normal_neighbors))
        nrm = (nrm if q.dim() == 3 else nrm[0]).contiguous()
    else:
        nrm = normals.detach().contiguous().float()
    rmse_point = solved = None
    if return_info:
        rmse_point = torch.empty((iterations, b), dtype=torch.float32, device=dev)
        solved = torch.empty((iterations, b), dtype=torch.int32, device=dev)
    work = torch.empty((max(int(_libh().so3_icp_plane_workspace_bytes(b, n)) // 4, 1),), dtype=torch.float32, device=dev)
    _launch(dev, "so3_icp_plane_f32", _ptr(p), _ptr(q), _ptr(nrm), stride, _ptr(w), _ptr(t0), -1.0 if max_distance is None else float(max_distance),
            damping, iterations, _ptr(r), _ptr(t), _ptr(rmse), _ptr(rmse_point), _ptr(inl), _ptr(solved), _ptr(nearest), _ptr(dist), _ptr(work),
            b, n, m)
    if return_info:
        return r, t, {"rmse": rmse, "rmse_point": rmse_point, "inliers": inl.long(), "solved": solved.bool(), "nearest": nearest.long(), "dist": dist}
    return r, t


# --------------------------------------------------------------------------------------------
# the Chamfer distance: a loss between two clouds, differentiable in both
# --------------------------------------------------------------------------------------------

def _chamfer_reduce(rows, nx, ny, n, m, point_reduction, batch_reduction, single):
    """The loss from the (B,2) means a forward left (the distance's or the normal term's): a few (B,)-sized torch statements.
    nx, ny: the point counts as float32, None for the full lengths n, m."""
    cham_x, cham_y = rows[:, 0], rows[:, 1]
    if point_reduction == "sum":                       # rows holds the means
        cham_x = cham_x * (float(n) if nx is None else nx)
        cham_y = cham_y * (float(m) if ny is None else ny)
    per_cloud = cham_x if single else cham_x + cham_y
    return per_cloud.mean() if batch_reduction == "mean" else (per_cloud.sum() if batch_reduction == "sum" else per_cloud.contiguous())


def _chamfer_scales(grad_out, nx, ny, b, n, m, point_reduction, batch_reduction, single):
    """_chamfer_reduce's backward folded with the upstream gradient into the per-cloud scales (scale_x, scale_y) the backward kernels
    take, on the device; scale_y is None for a single direction."""
    g = grad_out.detach().float()
    if batch_reduction is None:
        g = g.reshape(b)
    else:                                              # one upstream scalar for every cloud, kept on the device
        g = (g.reshape(1) * (1.0 / max(b, 1)) if batch_reduction == "mean" else g.reshape(1)).expand(b)
    if point_reduction == "mean":                      # an empty cloud takes no gradient: the kernel writes its rows as 0
        scale_x = g * (1.0 / n) if nx is None else g / nx.clamp(min=1.0)
        scale_y = g * (1.0 / m) if ny is None else g / ny.clamp(min=1.0)
    else:
        scale_x = scale_y = g
    return scale_x.contiguous(), None if single else scale_y.contiguous()



class _Chamfer(torch.autograd.Function):
    """chamfer_distance: so3_chamfer_fwd_f32 searches both directions and leaves the (B,2) means; the reductions over them are a few
    (B,)-sized torch statements.  The backward folds the upstream gradient and those reductions into per-cloud scales on the device
    and makes one so3_chamfer_bwd_f32 call through the stored indices."""

    @staticmethod
    def forward(ctx, X, Y, x_lengths, y_lengths, squared, point_reduction, batch_reduction, single, return_nearest):
        dev, x, y, _, b, n, m = _cloud_pair("chamfer_distance", X, Y, shared_target=False)
        xl = _cloud_lengths("chamfer_distance", RuntimeError, "x_lengths", x_lengths, b, n, dev)
        yl = _cloud_lengths("chamfer_distance", RuntimeError, "y_lengths", y_lengths, b, m, dev)
        nx, ny = (None if l is None else l.to(torch.float32) for l in (xl, yl))       # the point counts; None: the full length
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_grad = want_x or want_y
        flags = (0 if squared else _lib.CHAMFER_UNSQUARED) | (_lib.CHAMFER_SINGLE if single else 0)

        def buf(rows, dtype, wanted):
            return torch.empty((b, rows), dtype=dtype, device=dev) if wanted else None

        near_x = buf(n, torch.int32, want_grad or return_nearest)
        near_y = buf(m, torch.int32, (want_grad or return_nearest) and not single)
        dist_x = buf(n, torch.float32, return_nearest)
        dist_y = buf(m, torch.float32, return_nearest and not single)
        rows = torch.empty((b, 2), dtype=torch.float32, device=dev)
        work = torch.empty((max(int(_libh().so3_chamfer_workspace_bytes(b, n, m)) // 4, 1),), dtype=torch.float32, device=dev)
        _launch(dev, "so3_chamfer_fwd_f32", _ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(dist_x), _ptr(near_x), _ptr(dist_y), _ptr(near_y), _ptr(rows),
                _ptr(work), flags, b, n, m)
        out = _chamfer_reduce(rows, nx, ny, n, m, point_reduction, batch_reduction, single)
        if want_grad:
            ctx.save_for_backward(x, y, xl, yl, near_x, near_y, nx, ny)
        ctx.meta = (want_x, want_y, flags, point_reduction, batch_reduction, X.dtype, Y.dtype, b, n, m)
        if not return_nearest:
            return out
        extras = (near_x.long(), dist_x) if single else (near_x.long(), dist_x, near_y.long(), dist_y)
        ctx.mark_non_differentiable(*extras)
        return (out,) + extras

    @staticmethod
    def backward(ctx, grad_out, *unused):
        _no_double_backward(grad_out)
        want_x, want_y, flags, point_reduction, batch_reduction, x_dtype, y_dtype, b, n, m = ctx.meta
        if not (want_x or want_y):
            return (None,) * 9
        x, y, xl, yl, near_x, near_y, nx, ny = ctx.saved_tensors
        dev = x.device
        scale_x, scale_y = _chamfer_scales(grad_out, nx, ny, b, n, m, point_reduction, batch_reduction, bool(flags & _lib.CHAMFER_SINGLE))
        dx = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if want_x else None
        dy = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if want_y else None
        _launch(dev, "so3_chamfer_bwd_f32", _ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(near_x), _ptr(near_y), _ptr(scale_x), _ptr(scale_y),
                _ptr(dx), _ptr(dy), flags, b, n, m)
        return (_grad_to(dx, x_dtype), _grad_to(dy, y_dtype)) + (None,) * 7


class _ChamferNormals(torch.autograd.Function):
    """chamfer_distance with normals: ONE so3_chamfer_normals_fwd_f32 call leaves the distance's and the normal term's (B,2) means,
    _Chamfer's reductions make (loss, loss_normals) of them.  The backward folds each upstream gradient into per-cloud scales on the
    device and launches so3_chamfer_bwd_f32 only for a loss that received a gradient and a cloud that wants one,
    so3_chamfer_normals_bwd_f32 only for a loss_normals that received one and a normal tensor that wants one."""

    @staticmethod
    def forward(ctx, X, Y, NX, NY, x_lengths, y_lengths, squared, point_reduction, batch_reduction, single, return_nearest, abs_cosine):
        ctx.set_materialize_grads(False)                   # an unused output costs no launch
        dev, x, y, _, b, n, m = _cloud_pair("chamfer_distance", X, Y, shared_target=False)
        _require_device(x, NX, NY)
        if tuple(NX.shape) != tuple(X.shape) or tuple(NY.shape) != tuple(Y.shape) or not (NX.is_floating_point() and NY.is_floating_point()):
            raise RuntimeError("chamfer_distance: expected floating-point x_normals of X's shape %s and y_normals of Y's shape %s, got %s %s and %s %s"
                               % (tuple(X.shape), tuple(Y.shape), NX.dtype, tuple(NX.shape), NY.dtype, tuple(NY.shape)))
        nrm_x, nrm_y = NX.detach().contiguous().float(), NY.detach().contiguous().float()
        xl = _cloud_lengths("chamfer_distance", RuntimeError, "x_lengths", x_lengths, b, n, dev)
        yl = _cloud_lengths("chamfer_distance", RuntimeError, "y_lengths", y_lengths, b, m, dev)
        nx, ny = (None if l is None else l.to(torch.float32) for l in (xl, yl))       # the point counts; None: the full length
        want = tuple(ctx.needs_input_grad[:4])
        want_cloud, want_normal = want[0] or want[1], want[2] or want[3]
        want_grad = want_cloud or want_normal
        flags = (0 if squared else _lib.CHAMFER_UNSQUARED) | (_lib.CHAMFER_SINGLE if single else 0) | (0 if abs_cosine else _lib.CHAMFER_SIGNED_COSINE)

        def buf(rows, dtype, wanted):
            return torch.empty((b, rows), dtype=dtype, device=dev) if wanted else None

        near_x = buf(n, torch.int32, want_grad or return_nearest)
        near_y = buf(m, torch.int32, (want_grad or return_nearest) and not single)
        dist_x = buf(n, torch.float32, return_nearest)
        dist_y = buf(m, torch.float32, return_nearest and not single)
        term_x = buf(n, torch.float32, return_nearest)
        term_y = buf(m, torch.float32, return_nearest and not single)
        rows = torch.empty((b, 2), dtype=torch.float32, device=dev)
        rows_n = torch.empty((b, 2), dtype=torch.float32, device=dev)
        work = torch.empty((max(int(_libh().so3_chamfer_normals_workspace_bytes(b, n, m)) // 4, 1),), dtype=torch.float32, device=dev)
        _launch(dev, "so3_chamfer_normals_fwd_f32", _ptr(x), _ptr(y), _ptr(nrm_x), _ptr(nrm_y), _ptr(xl), _ptr(yl), _ptr(dist_x), _ptr(near_x),
                _ptr(dist_y), _ptr(near_y), _ptr(term_x), _ptr(term_y), _ptr(rows), _ptr(rows_n), _ptr(work), flags, b, n, m)
        out = _chamfer_reduce(rows, nx, ny, n, m, point_reduction, batch_reduction, single)
        out_n = _chamfer_reduce(rows_n, nx, ny, n, m, point_reduction, batch_reduction, single)
        if want_grad:
            ctx.save_for_backward(x if want_cloud else None, y if want_cloud else None, nrm_x if want_normal else None,
                                  nrm_y if want_normal else None, xl, yl, near_x, near_y, nx, ny)
        ctx.meta = (want, flags, point_reduction, batch_reduction, (X.dtype, Y.dtype, NX.dtype, NY.dtype), b, n, m)
        if not return_nearest:
            return out, out_n
        extras = (near_x.long(), dist_x, term_x) if single else (near_x.long(), dist_x, term_x, near_y.long(), dist_y, term_y)
        ctx.mark_non_differentiable(*extras)
        return (out, out_n) + extras

    @staticmethod
    def backward(ctx, grad_out, grad_normals, *unused):
        _no_double_backward(grad_out, grad_normals)
        want, flags, point_reduction, batch_reduction, dtypes, b, n, m = ctx.meta
        grads = [None, None, None, None]
        if any(want) and (grad_out is not None or grad_normals is not None):
            x, y, nrm_x, nrm_y, xl, yl, near_x, near_y, nx, ny = ctx.saved_tensors
            dev = near_x.device
            single = bool(flags & _lib.CHAMFER_SINGLE)

            def outs(wx, wy):
                return (torch.empty((b, n, 3), dtype=torch.float32, device=dev) if wx else None,
                        torch.empty((b, m, 3), dtype=torch.float32, device=dev) if wy else None)

            if grad_out is not None and (want[0] or want[1]):
                scale_x, scale_y = _chamfer_scales(grad_out, nx, ny, b, n, m, point_reduction, batch_reduction, single)
                grads[0], grads[1] = outs(want[0], want[1])
                _launch(dev, "so3_chamfer_bwd_f32", _ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(near_x), _ptr(near_y), _ptr(scale_x), _ptr(scale_y),
                        _ptr(grads[0]), _ptr(grads[1]), flags & ~_lib.CHAMFER_SIGNED_COSINE, b, n, m)
            if grad_normals is not None and (want[2] or want[3]):
                scale_x, scale_y = _chamfer_scales(grad_normals, nx, ny, b, n, m, point_reduction, batch_reduction, single)
                grads[2], grads[3] = outs(want[2], want[3])
                _launch(dev, "so3_chamfer_normals_bwd_f32", _ptr(nrm_x), _ptr(nrm_y), _ptr(xl), _ptr(yl), _ptr(near_x), _ptr(near_y), _ptr(scale_x),
                        _ptr(scale_y), _ptr(grads[2]), _ptr(grads[3]), flags, b, n, m)
        return tuple(_grad_to(g, d) for g, d in zip(grads, dtypes)) + (None,) * 8


def chamfer_distance(X: torch.Tensor, Y: torch.Tensor, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None, squared: bool = True,
                     point_reduction: str = "mean", batch_reduction: str = "mean", single_directional: bool = False,
                     return_nearest: bool = False, x_normals: torch.Tensor = None, y_normals: torch.Tensor = None, abs_cosine: bool = True):
    """The Chamfer distance between the clouds X (B,N,3) and Y (B,M,3), differentiable in BOTH clouds:

        loss_b = mean_{i < n_b} min_{j < m_b} |x_i - y_j|^2  +  mean_{j < m_b} min_{i < n_b} |y_j - x_i|^2.

    x_lengths, y_lengths: optional (B,) int32 / int64 tensors; cloud b uses its first n_b = clip(x_lengths[b], 0, N) and m_b points, a
    point past the length is neither a source nor a candidate.  A cloud with n_b == 0 or m_b == 0 scores 0 and takes no gradient.
    squared=False sums the distances instead of their squares (one square root after the minimum; its gradient is the unit direction,
    0 where the two points coincide).  point_reduction: "mean" or "sum" over a cloud's points; batch_reduction: "mean", "sum" or None
    for the (B,) rows; single_directional=True keeps the first term alone.

    The searches are nearest_neighbors' (coordinate differences, the first of equal candidates: a point that is in both clouds gets
    exactly 0) and run in ONE launch; the backward is one launch that gathers both gradients through the stored indices in a fixed
    order.  No atomics and nothing synchronises with the host: the same inputs give the same bits, and the call captures into a graph.

    return_nearest=True returns (loss, info) with info["nearest_x"] (B,N), info["nearest_y"] (B,M) int64 (-1 in slots past the length)
    and info["dist_x"], info["dist_y"] float32, the per-point terms (0 in those slots); single_directional leaves the y entries out.

    x_normals (B,N,3) and y_normals (B,M,3), both or neither, add the normal term of the same pairs and the call returns
    (loss, loss_normals), or (loss, loss_normals, info) with info["normal_x"], info["normal_y"] float32, the per-point terms:

        loss_normals_b = mean_{i < n_b} (1 - |cos(nx_i, ny_j(i))|)  +  mean_{j < m_b} (1 - |cos(ny_j, nx_i(j))|),

    reduced as loss is; abs_cosine=False takes 1 - cos.  The normals need not be of unit length and may have any float dtype (the
    arithmetic is float32); a pair with a zero, NaN or infinite normal scores 1 and gives no gradient.  loss_normals is differentiable
    in both normal tensors and gives no gradient to the clouds (the pairing is piecewise constant); loss is the same bits, with the
    same gradients, as without normals.  Still one forward launch; the backward makes one launch for each of the two losses that
    received a gradient, the normals' a gather in a fixed order as the clouds' is."""
    if point_reduction not in ("mean", "sum") or batch_reduction not in ("mean", "sum", None):
        raise ValueError("chamfer_distance: point_reduction is 'mean' or 'sum' and batch_reduction 'mean', 'sum' or None, got %r and %r"
                         % (point_reduction, batch_reduction))
    if (x_normals is None) != (y_normals is None):
        raise ValueError("chamfer_distance: x_normals and y_normals go together (single_directional pairs nx_i with ny_j(i) too), got %s alone"
                         % ("x_normals" if y_normals is None else "y_normals"))
    if x_normals is not None:
        res = _ChamferNormals.apply(X, Y, x_normals, y_normals, x_lengths, y_lengths, bool(squared), point_reduction, batch_reduction,
                                    bool(single_directional), bool(return_nearest), bool(abs_cosine))
        if not return_nearest:
            return res
        names = ("nearest_x", "dist_x", "normal_x") if single_directional else ("nearest_x", "dist_x", "normal_x", "nearest_y", "dist_y", "normal_y")
        return res[0], res[1], dict(zip(names, res[2:]))
    res = _Chamfer.apply(X, Y, x_lengths, y_lengths, bool(squared), point_reduction, batch_reduction, bool(single_directional), bool(return_nearest))
    if not return_nearest:
        return res
    names = ("nearest_x", "dist_x") if single_directional else ("nearest_x", "dist_x", "nearest_y", "dist_y")
    return res[0], dict(zip(names, res[1:]))


# --------------------------------------------------------------------------------------------
# K nearest neighbours between two clouds, differentiable in both
# --------------------------------------------------------------------------------------------
class _KnnPoints(torch.autograd.Function):
    """knn_points: one so3_knn_f32 launch; the backward is one so3_knn_bwd_f32 launch that gathers both gradients through the stored
    int32 indices in a fixed order."""

    @staticmethod
    def forward(ctx, X, Y, k, x_lengths, y_lengths):
        dev, x, y, stride, b, n, m = _cloud_pair("knn_points", X, Y, error=ValueError)
        if stride == 0 and ctx.needs_input_grad[1]:
            raise ValueError("knn_points: a shared (M, 3) target takes no gradient; pass Y.expand(B, M, 3) to differentiate in it")
        xl = _cloud_lengths("knn_points", ValueError, "x_lengths", x_lengths, b, n, dev)
        yl = _cloud_lengths("knn_points", ValueError, "y_lengths", y_lengths, b, m, dev)
        dist2 = torch.empty((b, n, k), dtype=torch.float32, device=dev)
        idx = torch.empty((b, n, k), dtype=torch.int32, device=dev)
        _launch(dev, "so3_knn_f32", _ptr(x), _ptr(y), stride, _ptr(xl), _ptr(yl), _ptr(dist2), _ptr(idx), k, b, n, m)
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if want_x or want_y:
            ctx.save_for_backward(x, y, xl, yl, idx)
        ctx.meta = (want_x, want_y, X.dtype, Y.dtype, k, b, n, m)
        idx64 = idx.long()
        ctx.mark_non_differentiable(idx64)
        return dist2.to(X.dtype), idx64

    @staticmethod
    def backward(ctx, grad_dist2, unused):
        _no_double_backward(grad_dist2)
        want_x, want_y, x_dtype, y_dtype, k, b, n, m = ctx.meta
        if not (want_x or want_y):
            return None, None, None, None, None
        x, y, xl, yl, idx = ctx.saved_tensors
        dev = x.device
        if y.dim() == 2:                                   # a shared target: the backward takes per-cloud targets
            y = y.expand(b, m, 3).contiguous()
        g = grad_dist2.detach().float().contiguous()
        dx = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if want_x else None
        dy = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if want_y else None
        _launch(dev, "so3_knn_bwd_f32", _ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(idx), _ptr(g), _ptr(dx), _ptr(dy), k, b, n, m)
        return _grad_to(dx, x_dtype), _grad_to(dy, y_dtype), None, None, None


def knn_points(X: torch.Tensor, Y: torch.Tensor, K: int, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None):
    """For every point of X (B,N,3) its K nearest points of Y (B,M,3): (dist2, idx) with dist2 (B,N,K) the squared distances in
    ascending order and idx (B,N,K) int64, among equal distances the lower index first.  1 <= K <= KNN_MAX_K (64); K > M is legal.

    x_lengths, y_lengths: optional (B,) int32 / int64 tensors; cloud b uses its first n_b = clip(x_lengths[b], 0, N) and m_b points.
    dist2 = 0 and idx = -1 fill the slots k >= min(K, m_b), the rows i >= n_b and every slot of a cloud with m_b == 0 -- what
    knn_gather and group_points read as an empty slot.

    The arithmetic is a definition (include/so3proj.h): d = ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences in
    float32 without fused multiply-add, three_nn's distance: K = 3 gives three_nn's bits, and a point that is in both clouds gets
    exactly 0.  One launch (so3_knn_f32): a wave keeps a query's sorted list across its lanes, nothing of size N * M is in memory.

    dist2 is differentiable in BOTH clouds (dist2 and the gradients come back in the clouds' dtypes; the arithmetic is float32):
    one backward launch gathers both gradients through the stored indices in a fixed order, without atomics -- the same inputs give
    the same bits.  Nothing synchronises with the host, so the call captures into a graph.  idx carries no gradient; double
    backward is refused.  Y may be ONE (M,3) target shared by the batch, forward only: a shared target that requires grad raises
    (expand it to (B,M,3) instead)."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= _lib.KNN_MAX_K:
        raise ValueError("knn_points: expected an int 1 <= K <= %d, got %r" % (_lib.KNN_MAX_K, K))
    return _KnnPoints.apply(X, Y, K, x_lengths, y_lengths)


def knn_gather(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """points (B,M,C) gathered by knn_points' idx (B,N,K) -> (B,N,K,C); a slot of -1 gives a row of zeros.  Plain torch on the tensors'
    device, differentiable in points."""
    if points.dim() != 3 or idx.dim() != 3 or idx.shape[0] != points.shape[0] or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("knn_gather: expected points (B, M, C) and idx (B, N, K) (int32 or int64), got %s and %s %s"
                         % (tuple(points.shape), idx.dtype, tuple(idx.shape)))
    b, n, k = idx.shape
    c = points.shape[2]
    at = idx.long().clamp(min=0).reshape(b, n * k, 1).expand(b, n * k, c)
    out = points.gather(1, at).reshape(b, n, k, c)
    return torch.where((idx >= 0)[..., None], out, torch.zeros((), dtype=out.dtype, device=out.device))


def knn_group(K: int, xyz: torch.Tensor, new_xyz: torch.Tensor, points, channels_first: bool = False) -> torch.Tensor:
    """The kNN alternative to query_ball_point + group_points: the K nearest points of xyz (B,N,3) around every centre new_xyz (B,S,3)
    (knn_points(new_xyz, xyz, K)), grouped by group_points with its layouts: (B,S,K,3 + D), or with channels_first=True (points then
    (B,D,N)) (B,3 + D,K,S).  Differentiable in xyz, new_xyz and points through the grouping; the indices carry no gradient."""
    _, idx = knn_points(new_xyz.detach(), xyz.detach(), K)
    return group_points(xyz, new_xyz, points, idx, channels_first=channels_first)


# --------------------------------------------------------------------------------------------
# Local frames: per-point PCA over a neighbourhood (forward only)
# --------------------------------------------------------------------------------------------
def _frames_forward_only(*ts):
    if _wants_grad(*ts):
        _warn_once("local_frames", "local_frames and estimate_normals are forward-only: eigenvalues, frames and normals carry no gradient "
                                   "although an argument requires grad (the gradient through an eigenvector is unbounded at ties).  A loss "
                                   "that needs one can differentiate the covariance in torch.")


def _local_frames_call(points, idx, x_lengths, y_lengths, viewpoint, want):
    """One so3_local_frames_f32 launch; want = (cov, eigenvalues, normals, frames) flags -> the float32 outputs, None where not wanted."""
    dev = _require_device(points, idx)
    _frames_forward_only(points, viewpoint)
    ok = points.dim() in (2, 3) and points.shape[-1] == 3 and idx.dim() == 3 and (points.dim() == 2 or points.shape[0] == idx.shape[0])
    if (not ok or idx.dtype not in (torch.int32, torch.int64) or not 1 <= points.shape[-2] <= _lib.ADD_S_MAX_N
            or not 1 <= idx.shape[1] <= _lib.ADD_S_MAX_N or not 1 <= idx.shape[2] <= _lib.KNN_MAX_K):
        raise ValueError("local_frames: expected points (B, M, 3) or (M, 3) and idx (B, N, K) (int32 or int64) with 1 <= N, M <= %d and "
                         "1 <= K <= %d, got %s and %s %s" % (_lib.ADD_S_MAX_N, _lib.KNN_MAX_K, tuple(points.shape), idx.dtype, tuple(idx.shape)))
    b, n, k = idx.shape
    m = points.shape[-2]
    if viewpoint is not None:
        _require_device(viewpoint)
        if viewpoint.device != dev or tuple(viewpoint.shape) not in ((b, 3), (3,)) or not viewpoint.is_floating_point():
            raise ValueError("local_frames: expected viewpoint as a (B, 3) or (3,) floating-point tensor on %s for B = %d, got %s %s on %s"
                             % (dev, b, tuple(viewpoint.shape), viewpoint.dtype, viewpoint.device))
        viewpoint = viewpoint.detach().float().expand(b, 3).contiguous()
    y = points.detach().contiguous().float()
    xl = _cloud_lengths("local_frames", ValueError, "x_lengths", x_lengths, b, n, dev)
    yl = _cloud_lengths("local_frames", ValueError, "y_lengths", y_lengths, b, m, dev)
    # an index beyond int32 is invalid either way: clamp it to one that stays invalid (M <= 2^20) instead of letting it wrap
    ix = (idx if idx.dtype == torch.int32 else idx.clamp(-1, _lib.ADD_S_MAX_N).to(torch.int32)).contiguous()
    outs = [torch.empty((b, n, w), dtype=torch.float32, device=dev) if flag else None for flag, w in zip(want, (6, 3, 3, 9))]
    _launch(dev, "so3_local_frames_f32", _ptr(y), 0 if points.dim() == 2 else 3 * m, _ptr(ix), _ptr(xl), _ptr(yl), _ptr(viewpoint),
            *(_ptr(o) for o in outs), k, b, n, m)
    return outs


def local_frames(points: torch.Tensor, idx: torch.Tensor, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None,
                 viewpoint: torch.Tensor = None, return_covariance: bool = False):
    """Per-point PCA: for every row of idx (B,N,K) -- as knn_points, knn_group's search or query_ball_point return it, int32 or int64 --
    the covariance of the points of `points` (B,M,3), or one shared (M,3), that it names, decomposed: (eigenvalues (B,N,3) ascending and
    >= 0, frames (B,N,3,3) with the unit eigenvectors as columns, right-handed; frames[..., 0] is the surface normal).  With
    return_covariance=True also cov (B,N,3,3), symmetric.

    A slot is valid when 0 <= idx < m_b; -1 padding, an empty ball's N and anything else are skipped, wherever in the row they stand.
    x_lengths, y_lengths: optional (B,) int32 / int64: cloud b's rows i < n_b are live, its points j < m_b exist.  The covariance is a
    fixed-order float32 definition centred on the row's first valid point (include/so3proj.h), so it keeps its digits far from the
    origin and repeats bit for bit; the eigen stage is a fixed number of Jacobi sweeps in registers, one launch for everything
    (so3_local_frames_f32), nothing goes to a batched solver.  Signs: the largest-magnitude component of the normal and of the third
    axis is positive; with viewpoint (B,3) or (3,) the normal faces the viewpoint instead.  A row whose neighbours are all equal gets
    eigenvalues 0 and the identity frame, with or without a viewpoint; a row without a valid slot, a row past n_b and a cloud with m_b == 0 get zeros.

    Forward only: the outputs carry no gradient (an argument that requires grad is warned about once).  Outputs are computed in
    float32 and returned in the cloud's dtype."""
    cov, lam, _, frames = _local_frames_call(points, idx, x_lengths, y_lengths, viewpoint, (bool(return_covariance), True, False, True))
    b, n = lam.shape[:2]
    res = (lam.to(points.dtype), frames.view(b, n, 3, 3).to(points.dtype))
    if return_covariance:
        res += (cov[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].view(b, n, 3, 3).to(points.dtype),)
    return res


def estimate_normals(points: torch.Tensor, K: int = 16, lengths: torch.Tensor = None, viewpoint: torch.Tensor = None, return_curvature: bool = False):
    """Surface normals of a cloud (B,N,3) from its K nearest neighbours: knn_points(points, points, K, lengths, lengths) followed by
    local_frames' kernel with only the normals requested -> (B,N,3) unit vectors (zeros in the rows past lengths[b]).  The point
    itself is its own nearest neighbour and so the pivot of its covariance.  viewpoint (B,3) or (3,): the normals face it; without one
    their largest-magnitude component is positive.  return_curvature=True also returns the surface variation
    l0 / (l0 + l1 + l2) (B,N), 0 where the sum is 0.  Forward only, as local_frames."""
    _frames_forward_only(points, viewpoint)
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= _lib.KNN_MAX_K:
        raise ValueError("estimate_normals: expected an int 1 <= K <= %d, got %r" % (_lib.KNN_MAX_K, K))
    _require_device(points)
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("estimate_normals: expected points (B, N, 3), got %s" % (tuple(points.shape),))
    pts = points.detach()
    _, idx = knn_points(pts, pts, K, lengths, lengths)
    _, lam, normals, _ = _local_frames_call(pts, idx, lengths, lengths, viewpoint, (False, bool(return_curvature), True, False))
    normals = normals.to(points.dtype)
    if not return_curvature:
        return normals
    total = lam.sum(-1)
    variation = torch.where(total > 0, lam[..., 0] / total.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(total))
    return normals, variation.to(points.dtype)


# --------------------------------------------------------------------------------------------
# FPFH: a rigid-motion invariant descriptor per point, and matching by it (forward only)
# --------------------------------------------------------------------------------------------
def fpfh_features(points: torch.Tensor, normals: torch.Tensor, idx: torch.Tensor = None, K: int = 16, lengths: torch.Tensor = None,
                  return_spfh: bool = False):
    """Fast Point Feature Histograms (Rusu et al. 2009; PCL's and Open3D's descriptor): for every point of points (B,N,3) with unit
    normals (B,N,3) -- estimate_normals' -- 33 floats (B,N,33) that do not change when the cloud is moved rigidly: three 11-bin
    histograms of the angles between the point's normal, its neighbours' normals and the lines to them, each summing to 100, plus
    the 1 / d^2-weighted mean of the neighbours' own histograms (each sub-histogram of the result sums to 200).

    idx (B,N,K) int32 / int64: row i is point i's neighbourhood in the SAME cloud, as knn_points(points, points, K) or
    query_ball_point(r, K, points, points) return it; idx=None runs knn_points(points, points, K, lengths, lengths).  A slot counts
    when 0 <= idx < n_b, it is not the point itself, the two points differ, neither normal is zero and the line is not parallel to
    the source normal; everything else (-1 padding, an empty ball's N) is skipped.  A row is a multiset: an index that stands twice
    counts twice.  query_ball_point pads a short row by repeating its first hit -- overwrite that padding with -1 where a set is
    meant.  lengths: optional (B,) int32 / int64, cloud b has n_b = clip(lengths[b], 0, N) points; rows past it are zeros.

    Two launches (so3_spfh_f32, so3_fpfh_f32), no atomics and nothing of size (B,N,K,.) in memory; the same inputs give the same
    bits, and scaling the cloud by a power of two changes none.  The normals are used as given.  return_spfh=True also returns
    spfh (B,N,33) and pairs (B,N) int64, the number of slots that counted.  Any float dtype is accepted; the arithmetic is float32
    and the histograms come back in float32.  Forward only: a histogram is piecewise constant (an argument that requires grad is
    warned about once).  match_features pairs two clouds by these descriptors."""
    dev = _require_device(points, normals)
    if _wants_grad(points, normals):
        _warn_once("fpfh_features", "fpfh_features is forward-only: a histogram is piecewise constant, so the descriptor carries no gradient "
                                    "although an argument requires grad.")
    if (points.dim() != 3 or points.shape[-1] != 3 or tuple(normals.shape) != tuple(points.shape) or not points.is_floating_point()
            or not normals.is_floating_point() or not 1 <= points.shape[1] <= _lib.ADD_S_MAX_N):
        raise ValueError("fpfh_features: expected points and normals as (B, N, 3) floating-point tensors with 1 <= N <= %d, got %s %s and %s %s"
                         % (_lib.ADD_S_MAX_N, points.dtype, tuple(points.shape), normals.dtype, tuple(normals.shape)))
    b, n = points.shape[:2]
    x = points.detach().contiguous().float()
    nr = normals.detach().contiguous().float()
    if idx is None:
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= _lib.KNN_MAX_K:
            raise ValueError("fpfh_features: expected an int 1 <= K <= %d, got %r" % (_lib.KNN_MAX_K, K))
        _, idx = knn_points(x, x, K, lengths, lengths)
    else:
        _require_device(idx)
        if (idx.device != dev or idx.dim() != 3 or tuple(idx.shape[:2]) != (b, n) or idx.dtype not in (torch.int32, torch.int64)
                or not 1 <= idx.shape[2] <= _lib.KNN_MAX_K):
            raise ValueError("fpfh_features: expected idx (B, N, K) (int32 or int64) on %s with B = %d, N = %d and 1 <= K <= %d, got %s %s on %s"
                             % (dev, b, n, _lib.KNN_MAX_K, idx.dtype, tuple(idx.shape), idx.device))
    k = idx.shape[2]
    ln = _cloud_lengths("fpfh_features", ValueError, "lengths", lengths, b, n, dev)
    # an index beyond int32 is invalid either way: clamp it to one that stays invalid (N <= 2^20) instead of letting it wrap
    ix = (idx if idx.dtype == torch.int32 else idx.clamp(-1, _lib.ADD_S_MAX_N).to(torch.int32)).contiguous()
    spfh = torch.empty((b, n, 33), dtype=torch.float32, device=dev)
    pairs = torch.empty((b, n), dtype=torch.int32, device=dev)
    fpfh = torch.empty((b, n, 33), dtype=torch.float32, device=dev)
    _launch(dev, "so3_spfh_f32", _ptr(x), _ptr(nr), _ptr(ix), _ptr(ln), _ptr(spfh), _ptr(pairs), k, b, n)
    _launch(dev, "so3_fpfh_f32", _ptr(x), _ptr(ix), _ptr(ln), _ptr(spfh), _ptr(pairs), _ptr(fpfh), k, b, n)
    return (fpfh, spfh, pairs.long()) if return_spfh else fpfh


def match_features(fx: torch.Tensor, fy: torch.Tensor, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None, mutual: bool = True):
    """Correspondences by descriptor: for every row of fx (B,N,D) the nearest row of fy (B,M,D) in the Euclidean distance -> (B,N) int64,
    the first of equal candidates.  -1 for the rows past x_lengths[b], for every row when cloud b of fy has no row to match
    (y_lengths[b] == 0, or every row dead), and, with mutual=True, where the match does not point back (the nearest row of fx to
    fy[b, j] is not i).  Rows of fy past y_lengths[b] are never matched.  A row that holds a NaN or an infinity is a dead row on
    either side, as a row past the lengths is: as a query it gets -1, as a candidate it is never matched, and it changes no other
    row's answer.

    Plain torch on the tensors' device (CPU tensors work too), as index_points.  The (B,N,M) distance matrix is evaluated as
    sqrt(sum (a - b)^2) on the differences themselves (torch.cdist with compute_mode="donot_use_mm_for_euclid_dist"), never as
    |a|^2 + |b|^2 - 2 a.b: at FPFH's magnitudes (|f|^2 of 1e4 to 1e5) the GEMM form's cancellation turns squared distances below
    about 1e-2 into noise and names wrong rows, and a common offset makes it worse.  The arithmetic is the promoted dtype of fx and
    fy, and float32 where that is float16 or bfloat16; each cloud's answer is independent of the others in the batch.  One (B,N,M)
    matrix plus masks, no host synchronisation: the call captures into a graph.  The exact route is slower than the GEMM: on an
    MI355X, float32, D = 33, mutual, 5.23 ms against 0.45 ms at 2 x 2048 x 2048 (11.7 x) and 0.36 ms against 0.33 ms at
    2 x 257 x 300 (1.09 x) (profiles/match_features_bench.txt): end-to-end times, no kernel trace was taken.

    With keep = match[b] >= 0, the pairs P[b, keep] and Q[b, match[b, keep]] -- or, batched, Q gathered by match.clamp(min=0)
    with keep.float() as the weights -- are what rigid_align takes: fpfh_features on two clouds in arbitrary relative pose,
    match_features, rigid_align, then icp_align from that start.  No gradient."""
    if (fx.dim() != 3 or fy.dim() != 3 or fx.shape[0] != fy.shape[0] or fx.shape[2] != fy.shape[2] or fx.device != fy.device
            or not fx.is_floating_point() or not fy.is_floating_point()):
        raise ValueError("match_features: expected fx (B, N, D) and fy (B, M, D) as floating-point tensors on one device, got %s %s on %s and %s %s on %s"
                         % (fx.dtype, tuple(fx.shape), fx.device, fy.dtype, tuple(fy.shape), fy.device))
    b, n, m = fx.shape[0], fx.shape[1], fy.shape[1]
    dev = fx.device
    lens = []
    for name, lengths, full in (("x_lengths", x_lengths, n), ("y_lengths", y_lengths, m)):
        if lengths is None:
            lens.append(torch.full((b,), full, dtype=torch.long, device=dev))
            continue
        if (not isinstance(lengths, torch.Tensor) or lengths.device != dev or tuple(lengths.shape) != (b,)
                or lengths.dtype not in (torch.int32, torch.int64)):
            raise ValueError("match_features: expected %s as a (B,) int32 or int64 tensor on %s for B = %d" % (name, dev, b))
        lens.append(lengths.detach().long().clamp(0, full))
    nl, ml = lens
    if n == 0 or m == 0 or b == 0:
        return torch.full((b, n), -1, dtype=torch.long, device=dev)
    with torch.no_grad():
        dtype = torch.promote_types(fx.dtype, fy.dtype)
        if dtype in (torch.float16, torch.bfloat16):
            dtype = torch.float32
        x, y = fx.detach().to(dtype), fy.detach().to(dtype)
        live_x = (torch.arange(n, device=dev)[None, :] < nl[:, None]) & torch.isfinite(x).all(-1)    # (B, N)
        live_y = (torch.arange(m, device=dev)[None, :] < ml[:, None]) & torch.isfinite(y).all(-1)    # (B, M)
        live = live_x[:, :, None] & live_y[:, None, :]
        # the differences themselves: the GEMM route (|a|^2 + |b|^2 - 2 a.b, cdist's default above 25 rows) cancels
        dist = torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")                        # (B, N, M)
        inf = torch.full((), float("inf"), dtype=dist.dtype, device=dev)
        dist = torch.where(live, dist, inf)
        forward = _first_argmin(dist, live, 2)                                                       # (B, N)
        keep = live_x & live_y.any(1)[:, None]
        if mutual:
            back = _first_argmin(dist, live, 1)                                                      # (B, M)
            keep = keep & (back.gather(1, forward) == torch.arange(n, device=dev)[None, :])
        return torch.where(keep, forward, torch.full((), -1, dtype=torch.long, device=dev))


def _first_argmin(dist, live, dim):
    """argmin along dim over the entries of `live`, the FIRST of equal candidates (torch.argmin leaves the choice among ties open).
    dist is +inf outside live; a live entry that overflowed to +inf still comes before a dead one."""
    best = dist.min(dim, keepdim=True).values
    size = dist.shape[dim]
    shape = [1, 1, 1]
    shape[dim] = size
    at = torch.arange(size, device=dist.device).view(shape)
    return torch.where((dist == best) & live, at, torch.full((), size, dtype=torch.long, device=dist.device)).min(dim).values.clamp(max=size - 1)


# --------------------------------------------------------------------------------------------
# RANSAC over the matches: a pose from correspondences that are mostly wrong, and the whole global registration (forward only)
# --------------------------------------------------------------------------------------------
def _ransac_samples(valid, hypotheses, generator):
    """(B,H,3) int32 triples of indices drawn uniformly among each cloud's valid pairs, on the device and without a host sync: ranks in
    [0, c_b) from torch.rand, mapped to indices through a stable sort of the validity mask (the valid rows first, in ascending order).
    A cloud with c_b < 3 gets -1 everywhere: every hypothesis of it is inadmissible."""
    b, n = valid.shape
    c = valid.sum(1)
    order = torch.sort((~valid).to(torch.uint8), dim=1, stable=True).indices
    u = torch.rand((b, hypotheses * 3), dtype=torch.float32, device=valid.device, generator=generator)
    rank = torch.minimum((u * c[:, None]).long(), (c - 1).clamp(min=0)[:, None])
    idx = torch.where((c >= 3)[:, None], order.gather(1, rank), torch.full((), -1, dtype=torch.long, device=valid.device))
    return idx.view(b, hypotheses, 3).to(torch.int32)


def ransac_align(P: torch.Tensor, Q: torch.Tensor, corr: torch.Tensor, max_distance: float, hypotheses: int = 4096, edge_similarity: float = 0.9,
                 samples: torch.Tensor = None, generator: torch.Generator = None, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None,
                 refine: bool = True, return_info: bool = False):
    """Global registration from correspondences of which a large share is wrong: the pose (R (B,3,3), t (B,3)) that maps the most pairs
    (p_i, Q[b, corr[b,i]]) to within max_distance of each other.  P: (B,N,3) source clouds, Q: (B,M,3) target clouds, corr: (B,N)
    int64 as match_features returns it, or int32; a pair is valid when i < n_b and 0 <= corr < m_b (-1 and anything else out of range
    is "no match").  The step between match_features and icp_align (PCL's SampleConsensusPrerejective, Open3D's
    registration_ransac_based_on_correspondence).

    `hypotheses` triples of valid pairs are drawn per cloud; a triple whose three edge lengths in P and in Q do not agree within the
    ratio edge_similarity (0 <= . <= 1; 0 switches the test off), or that repeats a source or a target point, is rejected before it
    is scored; each remaining one gives rigid_align's pose of its three pairs, scored by the number of valid pairs it brings within
    max_distance (ties: the smaller sum of squared distances, then the earlier hypothesis).  Two launches (so3_ransac_score_f32: one
    hypothesis per lane, the pairs streamed through on-chip memory, nothing of size B * H * N in memory; so3_ransac_select_f32), no
    atomics and no host synchronisation: the call captures into a graph.  include/so3proj.h holds the bit-exact definition of the
    score and the selection.

    samples: (B,H,3) int32 / int64 indices into the source cloud; given, the call is a pure function of its inputs (the same bits every
    time).  None draws them on the device from torch.rand(generator=generator), uniformly among the valid pairs; a cloud with fewer
    than three valid pairs has no admissible hypothesis and gets the identity with zero inliers.  x_lengths, y_lengths: optional (B,)
    int32 / int64, cloud b has n_b and m_b points.  refine=True ends with rigid_align on the winner's inliers (one more launch);
    refine=False returns the winning triple's own pose.

    return_info=True also returns a dict: "best" (B,) int64 the winning hypothesis (-1: none), "inliers" (B,) int64, "rmse" (B,) float32
    over the inliers at the winning pose, "weights" (B,N) float32 the 0 / 1 inlier mask, "targets" (B,N,3) float32 the matched target
    points (a finite stand-in where there is no match), "samples" (B,H,3) int64 and "T_best" (B,3,4) the rows (R | t) before refinement.

    Forward only (the vote is piecewise constant; an argument that requires grad is warned about once).  The differentiable tail is
    rigid_align(P, info["targets"], info["weights"]), which is what refine=True computes."""
    dev, p, q, _, b, n, m = _cloud_pair("ransac_align", P, Q, shared_target=False)
    _require_device(p, corr)
    if corr.device != dev or tuple(corr.shape) != (b, n) or corr.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("ransac_align: expected corr (B, N) (int32 or int64) on %s with B = %d, N = %d, got %s %s on %s"
                           % (dev, b, n, corr.dtype, tuple(corr.shape), corr.device))
    max_distance, edge_similarity = float(max_distance), float(edge_similarity)
    if not 0.0 <= max_distance < float("inf") or not 0.0 <= edge_similarity <= 1.0:
        raise RuntimeError("ransac_align: expected a finite max_distance >= 0 and 0 <= edge_similarity <= 1, got %r and %r"
                           % (max_distance, edge_similarity))
    if samples is None:
        if isinstance(hypotheses, bool) or not isinstance(hypotheses, int) or not 1 <= hypotheses <= _lib.RANSAC_MAX_HYPOTHESES:
            raise RuntimeError("ransac_align: expected an int 1 <= hypotheses <= %d, got %r" % (_lib.RANSAC_MAX_HYPOTHESES, hypotheses))
    else:
        _require_device(p, samples)
        if (samples.dim() != 3 or samples.shape[0] != b or samples.shape[2] != 3 or samples.dtype not in (torch.int32, torch.int64)
                or not 1 <= samples.shape[1] <= _lib.RANSAC_MAX_HYPOTHESES):
            raise RuntimeError("ransac_align: expected samples (B, H, 3) (int32 or int64) with B = %d and 1 <= H <= %d, got %s %s"
                               % (b, _lib.RANSAC_MAX_HYPOTHESES, samples.dtype, tuple(samples.shape)))
    if _wants_grad(P, Q):
        _warn_once("ransac_align", "ransac_align is forward-only: R and t carry no gradient although an argument requires grad.  "
                                   "rigid_align(P, info['targets'], info['weights']) on return_info=True's dict is the differentiable tail.")
    xl = _cloud_lengths("ransac_align", RuntimeError, "x_lengths", x_lengths, b, n, dev)
    yl = _cloud_lengths("ransac_align", RuntimeError, "y_lengths", y_lengths, b, m, dev)
    # an index beyond int32 is invalid either way: clamp it to one that stays invalid (M <= 2^20) instead of letting it wrap
    cr = (corr if corr.dtype == torch.int32 else corr.detach().clamp(-1, _lib.ADD_S_MAX_N).to(torch.int32)).contiguous()
    if samples is None:
        # xl, yl are _cloud_lengths' (already clipped to [0, N] and [0, M]): the mask is the kernels' "valid pair"
        rows = torch.arange(n, device=dev)[None, :]
        valid = (cr >= 0) & (cr < (m if yl is None else yl[:, None]))
        if xl is not None:
            valid = valid & (rows < xl[:, None])
        sm = _ransac_samples(valid, hypotheses, generator)
    else:
        sm = (samples if samples.dtype == torch.int32 else samples.detach().clamp(-1, _lib.ADD_S_MAX_N).to(torch.int32)).contiguous()
    h = sm.shape[1]
    t_hyp = torch.empty((b, h, 12), dtype=torch.float32, device=dev)
    count = torch.empty((b, h), dtype=torch.int32, device=dev)
    err = torch.empty((b, h), dtype=torch.float32, device=dev)
    best = torch.empty((b,), dtype=torch.int32, device=dev)
    t_best = torch.empty((b, 3, 4), dtype=torch.float32, device=dev)
    inliers = torch.empty((b,), dtype=torch.int32, device=dev)
    rmse = torch.empty((b,), dtype=torch.float32, device=dev)
    weights = torch.empty((b, n), dtype=torch.float32, device=dev)
    targets = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    _launch(dev, "so3_ransac_score_f32", _ptr(p), _ptr(q), _ptr(cr), _ptr(xl), _ptr(yl), _ptr(sm), max_distance, edge_similarity, _ptr(t_hyp),
            _ptr(count), _ptr(err), b, n, m, h)
    _launch(dev, "so3_ransac_select_f32", _ptr(p), _ptr(q), _ptr(cr), _ptr(xl), _ptr(yl), _ptr(t_hyp), _ptr(count), _ptr(err), max_distance,
            _ptr(best), _ptr(t_best), _ptr(inliers), _ptr(rmse), _ptr(weights), _ptr(targets), b, n, m, h)
    if refine:
        r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        t = torch.empty((b, 3), dtype=torch.float32, device=dev)
        _launch(dev, "so3_rigid_align_f32", _ptr(p), _ptr(targets), _ptr(weights), _ptr(r), _ptr(t), None, None, b, n)
    else:
        r, t = t_best[:, :, :3].contiguous(), t_best[:, :, 3].contiguous()
    if return_info:
        return r, t, {"best": best.long(), "inliers": inliers.long(), "rmse": rmse, "weights": weights, "targets": targets,
                      "samples": sm.long() if samples is None else samples.detach().long(), "T_best": t_best}
    return r, t


def global_registration(P: torch.Tensor, Q: torch.Tensor, max_distance: float, K: int = 16, hypotheses: int = 4096, icp_iterations: int = 10,
                        generator: torch.Generator = None, return_info: bool = False):
    """The pose (R (B,3,3), t (B,3)) that registers the clouds P (B,N,3) onto Q (B,M,3) from ARBITRARY relative pose, without an
    initial guess: estimate_normals and fpfh_features on both clouds (K neighbours), match_features (mutual), ransac_align on the
    matches and icp_align from its answer (icp_iterations iterations, the same max_distance).  A plain composition of those calls,
    full clouds only; generator seeds ransac_align's draws.  The normals face each cloud's own centroid: a rule a rigid motion
    carries along, which the default sign rule of estimate_normals (largest component positive) is not, and the descriptor depends
    on the normals' sides.  return_info=True also returns a dict: "corr" (B,N) int64 the matches,
    "R_ransac", "t_ransac" the pose before ICP, and ransac_align's entries.  Forward only."""
    fp = fpfh_features(P, estimate_normals(P, K, viewpoint=P.detach().mean(1)), K=K)
    fq = fpfh_features(Q, estimate_normals(Q, K, viewpoint=Q.detach().mean(1)), K=K)
    corr = match_features(fp, fq)
    r0, t0, info = ransac_align(P, Q, corr, max_distance, hypotheses=hypotheses, generator=generator, return_info=True)
    r, t = icp_align(P, Q, R_init=r0, t_init=t0, iterations=icp_iterations, max_distance=max_distance)
    if return_info:
        return r, t, dict(info, corr=corr, R_ransac=r0, t_ransac=t0)
    return r, t
