"""Clouds with known correspondences: Kabsch, rigid_align, rotating and normalising clouds, and the samplers of the point-cloud
path.  One family of the Python mirror; rotation_representation re-exports its public names."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from ._runtime import _grad_to, _launch, _ptr, _require_device, _wants_grad, _warn_once


# --------------------------------------------------------------------------------------------
# K5: Kabsch
# --------------------------------------------------------------------------------------------
def _kabsch_call(P, Q, want_h):
    """K5 on float32 copies of the clouds: (p, q, R, H or None).  Both the plain call and the graph node run exactly this."""
    dev = _require_device(P, Q)
    if P.dim() != 3 or P.shape[-1] != 3 or P.shape != Q.shape:
        raise RuntimeError(f"kabsch_rotation: expected two (B, N, 3) tensors, got {tuple(P.shape)} and {tuple(Q.shape)}")
    p = P.detach().contiguous().float()
    q = Q.detach().contiguous().float()
    b, n, _ = p.shape
    r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    h = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if want_h else None
    _launch(dev, "so3_kabsch_f32", _ptr(p), _ptr(q), _ptr(r), _ptr(h), b, n)
    return p, q, r, h


class _Kabsch(torch.autograd.Function):
    """kabsch_rotation as a graph node: the reference's expression symmetric_orthogonalization(bmm(Q^T, P)) is differentiable.
    Forward asks K5 for H as well and keeps it; backward is K5b (so3_kabsch_bwd_f32): dH = K2(H, gR) + gH, dQ = dH p, dP = dH^T q."""

    @staticmethod
    def forward(ctx, P, Q, return_h):
        p, q, r, h = _kabsch_call(P, Q, True)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p, q, h)
        ctx.meta = ((P.shape, P.dtype), (Q.shape, Q.dtype))
        return (r, h) if return_h else r

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_r, grad_h=None):
        p, q, h = ctx.saved_tensors
        (shape_p, dtype_p), (shape_q, dtype_q) = ctx.meta
        need_p, need_q = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (grad_r is None and grad_h is None) or not (need_p or need_q):
            return None, None, None
        dev = p.device
        gr = None if grad_r is None else grad_r.reshape(-1, 9).float().contiguous()
        gh = None if grad_h is None else grad_h.reshape(-1, 9).float().contiguous()
        dp = torch.empty_like(p) if need_p else None
        dq = torch.empty_like(q) if need_q else None
        b, n, _ = p.shape
        _launch(dev, "so3_kabsch_bwd_f32", _ptr(p), _ptr(q), _ptr(h), _ptr(gr), _ptr(gh), _ptr(dp), _ptr(dq), b, n)
        return _grad_to(dp, dtype_p, shape_p), _grad_to(dq, dtype_q, shape_q), None


def kabsch_rotation(P: torch.Tensor, Q: torch.Tensor, return_h: bool = False):
    """R_b = argmin_R sum_i |R p_bi - q_bi|^2 over SO(3) = proj(sum_i q_bi p_bi^T).

    P, Q: (B, N, 3) float32 clouds as in point_cloud/main.py:171-181 (q = R p, no translation).
    Equivalent to symmetric_orthogonalization(torch.bmm(Q.transpose(1, 2), P)) in one launch, and differentiable like
    that expression with respect to both clouds (K5b, so3_kabsch_bwd_f32); with return_h=True, H = bmm(Q^T, P) is a
    differentiable output too.  Gradients come back in each argument's dtype; where H has a vanishing singular-value
    gap (collinear or empty clouds) K2's clamp keeps them finite where the reference's autograd gives Inf / NaN."""
    if _wants_grad(P, Q):
        _require_device(P, Q)
        return _Kabsch.apply(P, Q, return_h)
    _, _, r, h = _kabsch_call(P, Q, return_h)
    return (r, h) if return_h else r


# --------------------------------------------------------------------------------------------
# K5c / K5d: rigid_align, the weighted and centred Kabsch giving a pose
# --------------------------------------------------------------------------------------------
def _rigid_align_call(P, Q, weights, want_h, want_stats):
    """K5c on float32 copies: (p, q, w or None, R, t, H or None, stats or None).  The plain call and the graph node run exactly this."""
    dev = _require_device(P, Q) if weights is None else _require_device(P, Q, weights)
    if P.dim() != 3 or P.shape[-1] != 3 or P.shape != Q.shape or (weights is not None and weights.shape != P.shape[:2]):
        raise RuntimeError("rigid_align: expected two (B, N, 3) tensors and weights of None or (B, N), got %s, %s and %s"
                           % (tuple(P.shape), tuple(Q.shape), None if weights is None else tuple(weights.shape)))
    p = P.detach().contiguous().float()
    q = Q.detach().contiguous().float()
    w = None if weights is None else weights.detach().contiguous().float()
    b, n, _ = p.shape
    r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    h = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if want_h else None
    stats = torch.empty((b, 7), dtype=torch.float32, device=dev) if want_stats else None
    _launch(dev, "so3_rigid_align_f32", _ptr(p), _ptr(q), _ptr(w), _ptr(r), _ptr(t), _ptr(h), _ptr(stats), b, n)
    return p, q, w, r, t, h, stats


class _RigidAlign(torch.autograd.Function):
    """rigid_align as a graph node.  Forward keeps H, R and the per-cloud (pbar, qbar, W); backward is one launch of K5d
    (so3_rigid_align_bwd_f32) that writes only the gradients autograd asks for."""

    @staticmethod
    def forward(ctx, P, Q, weights, return_h):
        p, q, w, r, t, h, stats = _rigid_align_call(P, Q, weights, True, True)
        ctx.set_materialize_grads(False)
        ctx.has_w = w is not None
        ctx.save_for_backward(p, q, h, r, stats, *((w,) if w is not None else ()))
        ctx.meta = tuple((x.shape, x.dtype) if x is not None else None for x in (P, Q, weights))
        return (r, t, h) if return_h else (r, t)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_r, grad_t, grad_h=None):
        p, q, h, r, stats = ctx.saved_tensors[:5]
        w = ctx.saved_tensors[5] if ctx.has_w else None
        need = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_w and ctx.needs_input_grad[2]]
        if (grad_r is None and grad_t is None and grad_h is None) or not any(need):
            return None, None, None, None
        dev = p.device
        b, n, _ = p.shape
        gr = None if grad_r is None else grad_r.reshape(-1, 9).float().contiguous()
        gt = None if grad_t is None else grad_t.reshape(-1, 3).float().contiguous()
        gh = None if grad_h is None else grad_h.reshape(-1, 9).float().contiguous()
        outs = [torch.empty_like(p) if need[0] else None, torch.empty_like(q) if need[1] else None, torch.empty_like(w) if need[2] else None]
        _launch(dev, "so3_rigid_align_bwd_f32", _ptr(p), _ptr(q), _ptr(w), _ptr(h), _ptr(r), _ptr(stats), _ptr(gr), _ptr(gt), _ptr(gh),
                _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), b, n)
        for i, d in enumerate(outs):
            if d is not None:
                shape, dtype = ctx.meta[i]
                outs[i] = _grad_to(d, dtype, shape)
        return outs[0], outs[1], outs[2], None


def rigid_align(P: torch.Tensor, Q: torch.Tensor, weights: torch.Tensor = None, return_h: bool = False):
    """The pose (R, t) that best maps cloud P onto cloud Q: argmin over SO(3) x R^3 of sum_i w_i |R p_i + t - q_i|^2.

    P, Q: (B, N, 3) corresponding points; weights: None (all ones) or (B, N), w_i >= 0 -- confidences, or a 0/1 mask over
    clouds padded to a common N.  Returns R (B, 3, 3) and t (B, 3) in float32; with return_h=True also the weighted,
    centred covariance H = sum_i w_i (q_i - qbar)(p_i - pbar)^T (not divided by sum w), R = proj_SO(3)(H), t = qbar - R pbar.
    One launch (so3_rigid_align_f32) and one pass over the clouds; differentiable in P, Q and weights through R, t and H
    with one more launch (so3_rigid_align_bwd_f32); gradients come back in each argument's dtype.  No host synchronisation:
    the call and its backward can be captured in a graph.

    A cloud whose weights are all zero (or N == 0) gets R = I, t = 0, H = 0 and zero gradients.  Negative weights are
    undefined and NOT checked (a check would cost a synchronisation).  NaN in gives NaN out; points of weight 0 must be
    finite.  The sums are taken relative to each cloud's first point pair, so the clouds may lie anywhere in space -- as long
    as that first point lies within the cloud's extent, whatever its weight: pad at the END.  Where H has a vanishing
    singular-value gap (collinear or coincident points) R is still a rotation and K2's clamp keeps the gradients finite,
    as kabsch_rotation documents."""
    if _wants_grad(P, Q) or (weights is not None and _wants_grad(weights)):
        return _RigidAlign.apply(P, Q, weights, return_h)
    _, _, _, r, t, h, _ = _rigid_align_call(P, Q, weights, return_h, False)
    return (r, t, h) if return_h else (r, t)


# --------------------------------------------------------------------------------------------
# row a7: the cloud side of the point-cloud path
# --------------------------------------------------------------------------------------------
def _rotate_call(pc, R, transposed):
    dev = _require_device(pc, R)
    if pc.dim() != 3 or pc.shape[-1] != 3 or R.numel() != pc.shape[0] * 9:
        raise RuntimeError(f"rotate_point_clouds: expected (B, N, 3) and (B, 3, 3), got {tuple(pc.shape)} and {tuple(R.shape)}")
    p = pc.detach().contiguous().float()
    r = R.detach().reshape(-1, 9).contiguous().float()
    b, n, _ = p.shape
    out = torch.empty((b, 3, n) if transposed else (b, n, 3), dtype=torch.float32, device=dev)
    _launch(dev, "so3_rotate_clouds_f32", _ptr(p), _ptr(r), _ptr(out), 1 if transposed else 0, b, n)
    return p, r, out


class _RotateClouds(torch.autograd.Function):
    """rotate_point_clouds as a graph node (the reference's bmm is differentiable): backward is a7b, so3_rotate_clouds_bwd_f32,
    dpc = R^T g and dR = sum_i g p^T, reading g in the forward's output layout."""

    @staticmethod
    def forward(ctx, pc, R, transposed):
        p, r, out = _rotate_call(pc, R, transposed)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p if ctx.needs_input_grad[1] else None, r if ctx.needs_input_grad[0] else None)
        ctx.meta = ((pc.shape, pc.dtype), (R.shape, R.dtype), bool(transposed), p.shape[0], p.shape[1], p.device)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        p, r = ctx.saved_tensors
        (shape_p, dtype_p), (shape_r, dtype_r), transposed, b, n, dev = ctx.meta
        need_p, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_out is None or not (need_p or need_r):
            return None, None, None
        g = grad_out.float().contiguous()
        dp = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if need_p else None
        dr = torch.empty((b, 9), dtype=torch.float32, device=dev) if need_r else None
        _launch(dev, "so3_rotate_clouds_bwd_f32", _ptr(p), _ptr(r), _ptr(g), _ptr(dp), _ptr(dr), 1 if transposed else 0, b, n)
        return _grad_to(dp, dtype_p, shape_p), _grad_to(dr, dtype_r, shape_r), None


def rotate_point_clouds(pc: torch.Tensor, R: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """q_bi = R_b p_bi for every point of every cloud: the pairing rule of point_cloud/main.py:173-181 (expand the
    rotation to all points, bmm, view) in one launch.  pc: (B,N,3), R: (B,3,3).  Returns (B,N,3), or with
    `transposed` the contiguous (B,3,N) tensor the reference obtains from `.transpose(1, 2)` at :183.
    Differentiable with respect to pc and R, like the reference's bmm (a7b, so3_rotate_clouds_bwd_f32)."""
    if _wants_grad(pc, R):
        _require_device(pc, R)
        return _RotateClouds.apply(pc, R, transposed)
    return _rotate_call(pc, R, transposed)[2]


def pc_normalize(pc: torch.Tensor):
    """Centre a cloud on its bounding box and scale by the box diagonal; point_cloud/prepare.py:51-56.
    pc: (N,3) as the reference takes it, or a (B,N,3) batch.  Returns (pc, centroid, scale) like the reference
    (centroid (3,) / (B,3); scale 0-dim / (B,)), float32 on the device."""
    dev = _require_device(pc)
    if _wants_grad(pc):
        _warn_once("pc_normalize", "pc_normalize is data preparation (numpy in the reference, point_cloud/prepare.py:51-56): its outputs "
                                   "carry no gradient although the cloud requires grad.")
    single = pc.dim() == 2
    p = (pc.unsqueeze(0) if single else pc).detach().contiguous().float()
    if p.dim() != 3 or p.shape[-1] != 3 or p.shape[1] < 1:
        raise RuntimeError(f"pc_normalize: expected (N, 3) or (B, N, 3) with N >= 1, got {tuple(pc.shape)}")
    b, n, _ = p.shape
    out, cen, sc = torch.empty_like(p), torch.empty((b, 3), dtype=torch.float32, device=dev), torch.empty((b,), dtype=torch.float32, device=dev)
    _launch(dev, "so3_pc_normalize_f32", _ptr(p), _ptr(out), _ptr(cen), _ptr(sc), b, n)
    return (out[0], cen[0], sc[0]) if single else (out, cen, sc)


# --------------------------------------------------------------------------------------------
# next row f4: on-device pair synthesis for Kabsch
# --------------------------------------------------------------------------------------------
def get_sampled_rotation_matrices_by_axisAngle(batch: int, device="cuda", generator: torch.Generator = None) -> torch.Tensor:
    """Random rotations by the reference's recipe (point_cloud/prepare.py:21-49): theta ~ U(-pi, pi), axis =
    normalised N(0, I), quaternion (cos theta, axis sin theta).  torch draws the random numbers; the quaternion ->
    matrix arithmetic runs in the HIP library."""
    dev = torch.device(device)
    theta = (torch.rand(batch, device=dev, generator=generator) * 2 - 1) * torch.pi
    axis = torch.randn(batch, 3, device=dev, generator=generator)
    return rotations_from_axis_angle_draws(theta, axis)


def rotations_from_axis_angle_draws(theta: torch.Tensor, axis: torch.Tensor) -> torch.Tensor:
    dev = _require_device(theta, axis)
    if _wants_grad(theta, axis):
        _warn_once("rotations_from_axis_angle_draws",
                   "rotations_from_axis_angle_draws (the sampler of get_sampled_rotation_matrices_by_axisAngle) draws targets: its rotations "
                   "carry no gradient although a draw requires grad.")
    t = theta.detach().reshape(-1).contiguous().float()
    a = axis.detach().reshape(-1, 3).contiguous().float()
    if a.shape[0] != t.shape[0]:
        raise RuntimeError("rotations_from_axis_angle_draws: theta (B,) and axis (B,3) disagree")
    r = torch.empty((t.shape[0], 3, 3), dtype=torch.float32, device=dev)
    _launch(dev, "so3_rotations_axis_angle_f32", _ptr(t), _ptr(a), _ptr(r), t.shape[0])
    return r


def kabsch_rotation_synthetic(P: torch.Tensor, R_gt: torch.Tensor, sigma: float = 0.0, seed: int = 0, return_h: bool = False):
    """Kabsch with the second cloud synthesised in the kernel: q = R_gt p + sigma * n(seed, cloud, point).
    Only P is read from HBM (config #3 with half the traffic)."""
    dev = _require_device(P, R_gt)
    if P.dim() != 3 or P.shape[-1] != 3 or R_gt.shape[0] != P.shape[0]:
        raise RuntimeError("kabsch_rotation_synthetic: expected P (B,N,3) and R_gt (B,3,3)")
    if _wants_grad(P, R_gt):
        _warn_once("kabsch_rotation_synthetic",
                   "kabsch_rotation_synthetic is not differentiable (its second cloud exists only inside the kernel): R and H carry no "
                   "gradient although an argument requires grad.  kabsch_rotation(P, rotate_point_clouds(P, R_gt) + noise) is the "
                   "differentiable spelling.")
    p = P.detach().contiguous().float()
    g = R_gt.detach().reshape(-1, 9).contiguous().float()
    b, n, _ = p.shape
    r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    h = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if return_h else None
    _launch(dev, "so3_kabsch_synth_f32", _ptr(p), _ptr(g), float(sigma), int(seed) & 0xFFFFFFFF, _ptr(r), _ptr(h), b, n)
    return (r, h) if return_h else r
