"""Losses and metrics on 4x4 poses: the iterative refiner's SE(3) update, ADD-L1 and its disentangled form, ADD, ADD-S, the model
diameter, and ADD / ADD-L1 / MSSD up to a symmetry group.  One family of the Python mirror; rotation_representation re-exports its
public names."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._runtime import _launch, _no_double_backward, _ptr, _require_device, _wants_grad, _warn_once
from .symmetry import SymmetryTable, _table_class_ids


# --------------------------------------------------------------------------------------------
# next row f1: the SE(3) pose update of the iterative refiner
# --------------------------------------------------------------------------------------------
def get_scene_parameters():
    """Focal lengths in pixels, as Iterative/utility.py:73-88: 50 mm lens, 36 mm sensor, 320 px."""
    sw, img_res, flen = 36, 320, 50
    fx = fy = flen / (sw / img_res)
    return fx, fy


class _Se3Update(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model_output, t_init, fx, fy):
        dev = _require_device(model_output, t_init)
        if model_output.dim() != 2 or model_output.shape[1] < 12 or tuple(t_init.shape[1:]) != (4, 4):
            raise RuntimeError("calculate_T_pred expects model_output (B, >=12) and T_init (B, 4, 4)")
        o = model_output.detach()[:, :12].contiguous().float()
        t = t_init.detach().reshape(-1, 16).contiguous().float()
        b = o.shape[0]
        tp = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
        _launch(dev, "so3_se3_update_f32", _ptr(o), _ptr(t), _ptr(tp), fx, fy, b)
        ctx.save_for_backward(o, t)
        ctx.meta = (model_output.shape, model_output.dtype, fx, fy)
        return tp

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_t):
        o, t = ctx.saved_tensors
        shape, dtype, fx, fy = ctx.meta
        dev = o.device
        g = grad_t.reshape(-1, 16).contiguous().float()
        d = torch.empty_like(o)
        _launch(dev, "so3_se3_update_bwd_f32", _ptr(o), _ptr(t), _ptr(g), _ptr(d), fx, fy, o.shape[0])
        full = torch.zeros(shape, dtype=torch.float32, device=dev)
        full[:, :12] = d
        return full.to(dtype), None, None, None


def calculate_T_pred(model_output: torch.Tensor, T_init: torch.Tensor, device=None, rot_repr: str = "SVD") -> torch.Tensor:
    """SE(3) update of the iterative refiner (Iterative/utility.py:90-128), one fused launch.

    model_output: (B,12) = 9 numbers for the SVD head + (vx, vy, vz); T_init: (B,4,4).  Returns T_pred (B,4,4)
    float32, differentiable w.r.t. model_output (T_init is a constant, as the reference's loop detaches it).
    `device` is accepted for signature compatibility and ignored (the result lives where the inputs do), and so is
    `rot_repr`: the reference never reads it -- its body always runs the SVD head on the first nine outputs
    (Iterative/utility.py:105), whatever the string says."""
    fx, fy = get_scene_parameters()
    return _Se3Update.apply(model_output, T_init, float(fx), float(fy))


# --------------------------------------------------------------------------------------------
# next row f6: the ADD-L1 losses on calculate_T_pred's output (Iterative/loss.py)
# --------------------------------------------------------------------------------------------
def _add_l1_args(t_gt, t_pred, points):
    bsz = len(t_gt)
    assert t_pred.shape == (bsz, 4, 4) and t_gt.shape == (bsz, 4, 4)            # reference: Iterative/loss.py:18
    assert points.dim() == 3 and points.shape[-1] == 3                          # :19
    assert points.shape[0] == bsz                                               # transform_pts, :58
    dev = _require_device(t_pred)
    _require_device(t_gt)
    _require_device(points)
    if points.shape[1] < 1:
        raise RuntimeError("ADD-L1: at least one model point per sample is needed")
    prep = lambda t: t.detach().contiguous().float()
    return dev, bsz, int(points.shape[1]), prep(t_gt), prep(t_pred), prep(points)


class _AddMean(torch.autograd.Function):
    """compute_ADD_L1_loss (entry so3_add_l1_f32) and compute_ADD_loss (so3_add_l2_f32): the loss and its gradient w.r.t. the
    predicted pose, one launch.  The two entry points share one prototype."""

    @staticmethod
    def forward(ctx, t_gt, t_pred, points, use_batch_mean, entry):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        want_grad = t_pred.requires_grad
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if want_grad else None
        dists = None if use_batch_mean else torch.empty((b,), dtype=torch.float32, device=dev)
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if use_batch_mean else None
        scale = 1.0 / max(b, 1) if use_batch_mean else 1.0
        _launch(dev, entry, _ptr(tg), _ptr(tp), _ptr(pts), _ptr(dists), _ptr(loss_sum), _ptr(dt), scale, b, n)
        ctx.dt, ctx.per_sample, ctx.in_dtype = dt, not use_batch_mean, t_pred.dtype
        if use_batch_mean:
            return loss_sum.to(torch.float32).mul_(1.0 / max(b, 1)).squeeze(0)
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.dt is None:
            return None, None, None, None, None
        g = grad_out.reshape(-1, 1, 1) if ctx.per_sample else grad_out
        return None, (ctx.dt * g).to(ctx.in_dtype), None, None, None


class _AddL1Disentangled(torch.autograd.Function):
    """compute_disentangled_ADD_L1_loss and its gradient, one launch (so3_add_l1_disentangled_f32)."""

    @staticmethod
    def forward(ctx, t_pred, t_gt, points):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if t_pred.requires_grad else None
        loss_sum = torch.empty((3,), dtype=torch.float64, device=dev)
        _launch(dev, "so3_add_l1_disentangled_f32", _ptr(tp), _ptr(tg), _ptr(pts), _ptr(loss_sum), _ptr(dt), 1.0 / max(b, 1), b, n)
        ctx.dt, ctx.in_dtype = dt, t_pred.dtype
        return loss_sum.sum().to(torch.float32).mul_(1.0 / max(b, 1))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.dt is None:
            return None, None, None
        return (ctx.dt * grad_out).to(ctx.in_dtype), None, None


def compute_ADD_L1_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, use_batch_mean: bool = True) -> torch.Tensor:
    """mean |T_gt p - T_pred p| over points and coordinates (and the batch); Iterative/loss.py:10-26.
    Differentiable w.r.t. TCO_pred (the ground-truth pose and the model points are constants in the reference's loops)."""
    return _AddMean.apply(TCO_gt, TCO_pred, points, bool(use_batch_mean), "so3_add_l1_f32")


def compute_disentangled_ADD_L1_loss(T_CO_pred: torch.Tensor, T_CO_gt: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """rotation + xy-translation + depth ADD-L1 terms; Iterative/loss.py:29-48, called right after calculate_T_pred
    (Iterative/main.py:94-95).  Differentiable w.r.t. T_CO_pred."""
    return _AddL1Disentangled.apply(T_CO_pred, T_CO_gt, points)


# --------------------------------------------------------------------------------------------
# the ADD / ADD-S pose metrics, the ADD-S loss and the model diameter
# --------------------------------------------------------------------------------------------
def _add_metric_points(name, t_gt, points):
    """(N,3) model points are broadcast to the batch (the copy is negligible beside the N^2 work); a ground-truth pose or points
    that require grad are constants here."""
    if _wants_grad(t_gt, points):
        _warn_once(name + "_constants", name + " is differentiable with respect to TCO_pred only: the ground-truth pose and the model "
                                               "points carry no gradient although one of them requires grad.")
    if isinstance(points, torch.Tensor) and points.dim() == 2:
        points = points.unsqueeze(0).expand(len(t_gt), -1, -1)
    return points


class _AddS(torch.autograd.Function):
    """compute_ADD_S_loss: the N^2 forward (so3_add_s_fwd_f32) keeps the argmin indices; the backward is one pass through them
    (so3_add_s_bwd_f32)."""

    @staticmethod
    def forward(ctx, t_gt, t_pred, points, use_batch_mean, return_nearest):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        if n > _lib.ADD_S_MAX_N:
            raise RuntimeError(f"compute_ADD_S_loss: at most {_lib.ADD_S_MAX_N} points per cloud, got {n}")
        want_grad = t_pred.requires_grad
        point_dist = torch.empty((b, n), dtype=torch.float32, device=dev)
        nearest = torch.empty((b, n), dtype=torch.int32, device=dev) if (want_grad or return_nearest) else None
        dists = torch.empty((b,), dtype=torch.float32, device=dev)
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if use_batch_mean else None
        _launch(dev, "so3_add_s_fwd_f32", _ptr(tg), _ptr(tp), _ptr(pts), _ptr(point_dist), _ptr(nearest), _ptr(dists), _ptr(loss_sum), b, n)
        if want_grad:
            ctx.save_for_backward(tg, tp, pts, nearest)
        ctx.meta = (want_grad, not use_batch_mean, t_pred.dtype, b, n)
        out = loss_sum.to(torch.float32).mul_(1.0 / max(b, 1)).squeeze(0) if use_batch_mean else dists
        if return_nearest:
            ctx.mark_non_differentiable(nearest)
            return out, nearest
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *unused):
        want_grad, per_sample, in_dtype, b, n = ctx.meta
        if not want_grad:
            return None, None, None, None, None
        tg, tp, pts, nearest = ctx.saved_tensors
        dev = tp.device
        g = grad_out.detach().contiguous().float()
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
        if per_sample:
            rows = g.reshape(-1)
        else:                                              # the batch mean: one upstream scalar for every row, kept on the device
            rows = (g.reshape(1) * (1.0 / max(b, 1))).expand(b).contiguous()
        _launch(dev, "so3_add_s_bwd_f32", _ptr(tg), _ptr(tp), _ptr(pts), _ptr(nearest), _ptr(rows), 1.0, _ptr(dt), b, n)
        return None, dt.to(in_dtype), None, None, None


def compute_ADD_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, use_batch_mean: bool = True) -> torch.Tensor:
    """The ADD metric: mean over the model points of |T_gt p - T_pred p|_2 (and over the batch; use_batch_mean=False gives (B,)).
    points: (B,N,3), or (N,3) for one model shared by the batch.  Differentiable w.r.t. TCO_pred."""
    points = _add_metric_points("compute_ADD_loss", TCO_gt, points)
    return _AddMean.apply(TCO_gt, TCO_pred, points, bool(use_batch_mean), "so3_add_l2_f32")


def compute_ADD_S_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, use_batch_mean: bool = True,
                       return_nearest: bool = False):
    """The ADD-S metric (PoseCNN / Hinterstoisser convention): mean over the points under the TRUE pose of the distance to the
    closest point under the ESTIMATED pose -- for symmetric objects, or objects whose symmetry is unknown.  use_batch_mean=False
    gives the (B,) metric; return_nearest=True also returns the (B,N) int32 argmin indices.  points: (B,N,3) or (N,3).
    Differentiable w.r.t. TCO_pred through the stored indices (the selected branch's gradient).  N^2 work per cloud, nothing of
    that size is materialised."""
    points = _add_metric_points("compute_ADD_S_loss", TCO_gt, points)
    return _AddS.apply(TCO_gt, TCO_pred, points, bool(use_batch_mean), bool(return_nearest))


def cloud_diameter(points: torch.Tensor) -> torch.Tensor:
    """max_ij |p_i - p_j|_2 per cloud, the scale of the acceptance threshold "ADD(-S) < 0.1 diameter": (B,) float32 for (B,N,3), a
    0-dim tensor for (N,3).  Not differentiable."""
    dev = _require_device(points)
    if _wants_grad(points):
        _warn_once("cloud_diameter", "cloud_diameter is an evaluation call: its result carries no gradient although the cloud requires grad.")
    single = points.dim() == 2
    p = (points.unsqueeze(0) if single else points).detach().contiguous().float()
    if p.dim() != 3 or p.shape[-1] != 3 or p.shape[1] < 1 or p.shape[1] > _lib.ADD_S_MAX_N:
        raise RuntimeError(f"cloud_diameter: expected (N, 3) or (B, N, 3) with 1 <= N <= {_lib.ADD_S_MAX_N}, got {tuple(points.shape)}")
    b, n, _ = p.shape
    work = torch.empty((b, n), dtype=torch.float32, device=dev)
    diam = torch.empty((b,), dtype=torch.float32, device=dev)
    _launch(dev, "so3_cloud_diameter_f32", _ptr(p), _ptr(work), _ptr(diam), b, n)
    return diam[0] if single else diam


# --------------------------------------------------------------------------------------------
# ADD, ADD-L1 and MSSD up to a symmetry group (so3_sym_add_f32)
# --------------------------------------------------------------------------------------------
def _sym_add_call(what, mode, t_gt, t_pred, points, table, class_ids, want_rows, want_sum, want_index, want_grad, scale):
    """One so3_sym_add_f32 launch: (rows, loss_sum, index, dT), each None unless asked for (rows are always taken: they are the
    work buffer of the batch sum)."""
    if not isinstance(table, SymmetryTable):
        raise TypeError(f"{what}: table must be a SymmetryTable, got {type(table).__name__}")
    dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
    cls = _table_class_ids(what, table, class_ids, t_pred, b)
    s = table._on(dev)
    rows = torch.empty((b,), dtype=torch.float32, device=dev) if (want_rows or want_sum) else None
    loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if want_sum else None
    idx = torch.empty((b,), dtype=torch.int32, device=dev) if want_index else None
    dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if want_grad else None
    _launch(dev, "so3_sym_add_f32", _ptr(tg), _ptr(tp), _ptr(pts), _ptr(s), _ptr(cls), table.num_classes, table.K, _ptr(rows), _ptr(idx),
            _ptr(loss_sum), _ptr(dt), scale, mode, b, n)
    if b == 0 and loss_sum is not None:               # the mean of no rows, as torch's .mean() gives it
        loss_sum.fill_(float("nan"))
    return rows, loss_sum, idx, dt


class _SymAdd(torch.autograd.Function):
    """compute_symmetric_ADD_loss / compute_symmetric_ADD_L1_loss: one launch writes the loss and, at unit upstream scale, the selected
    branch's gradient w.r.t. the predicted pose; backward scales it."""

    @staticmethod
    def forward(ctx, t_gt, t_pred, points, table, class_ids, use_batch_mean, return_index, mode, what):
        b = len(t_gt)
        want_grad = t_pred.requires_grad
        rows, loss_sum, idx, dt = _sym_add_call(what, mode, t_gt, t_pred, points, table, class_ids, not use_batch_mean, use_batch_mean,
                                                return_index, want_grad, 1.0 / max(b, 1) if use_batch_mean else 1.0)
        ctx.dt, ctx.per_sample, ctx.in_dtype = dt, not use_batch_mean, t_pred.dtype
        out = loss_sum.to(torch.float32).mul_(1.0 / max(b, 1)).squeeze(0) if use_batch_mean else rows
        if return_index:
            ctx.mark_non_differentiable(idx)
            return out, idx
        return out

    @staticmethod
    def backward(ctx, grad_out, *_):
        _no_double_backward(grad_out)
        if ctx.dt is None:
            return (None,) * 9
        g = grad_out.reshape(-1, 1, 1) if ctx.per_sample else grad_out
        return (None, (ctx.dt * g).to(ctx.in_dtype)) + (None,) * 7


def compute_symmetric_ADD_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, table: SymmetryTable,
                               class_ids: torch.Tensor = None, use_batch_mean: bool = True, return_index: bool = False):
    """ADD up to a discrete symmetry group: min_k ADD(T_gt, T_pred S_k), S_k the table's rotations of the row's class acting on the
    prediction from the right (about the model origin; symmetries with a translation part are not supported) -- the training loss for
    an object with discrete symmetries, O(N K) per sample.  use_batch_mean=False gives (B,); points: (B,N,3) or a shared (N,3).
    table / class_ids as in symmetric_angle_error; an id out of range makes the row (and the batch mean) NaN.
    return_index=True also returns k* (int32 (B,)), the smallest minimising k, -1 for a bad class id.
    Differentiable w.r.t. TCO_pred only: the selected branch's gradient, written by the forward launch.  No host sync: capturable in a
    graph once the table is on the device (`table.to(device)`).  A table {I} gives compute_ADD_loss (to rounding)."""
    points = _add_metric_points("compute_symmetric_ADD_loss", TCO_gt, points)
    return _SymAdd.apply(TCO_gt, TCO_pred, points, table, class_ids, bool(use_batch_mean), bool(return_index), _lib.SYM_ADD_L2,
                         "compute_symmetric_ADD_loss")


def compute_symmetric_ADD_L1_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, table: SymmetryTable,
                                  class_ids: torch.Tensor = None, use_batch_mean: bool = True, return_index: bool = False):
    """compute_ADD_L1_loss (Iterative/loss.py:10-26) up to a discrete symmetry group: min_k of the mean over points and coordinates of
    |T_gt p - T_pred S_k p|.  Arguments, gradient and capture as compute_symmetric_ADD_loss."""
    points = _add_metric_points("compute_symmetric_ADD_L1_loss", TCO_gt, points)
    return _SymAdd.apply(TCO_gt, TCO_pred, points, table, class_ids, bool(use_batch_mean), bool(return_index), _lib.SYM_ADD_L1,
                         "compute_symmetric_ADD_L1_loss")


def compute_MSSD(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, table: SymmetryTable, class_ids: torch.Tensor = None,
                 return_index: bool = False):
    """BOP's maximum symmetry-aware surface distance: min_k max_i |T_gt p_i - T_pred S_k p_i|_2, (B,) float32.  Arguments as
    compute_symmetric_ADD_loss.  An evaluation metric: no gradient."""
    if _wants_grad(TCO_gt, TCO_pred, points):
        _warn_once("compute_MSSD", "compute_MSSD is an evaluation call: its result carries no gradient although an argument requires grad.  "
                                   "compute_symmetric_ADD_loss is the differentiable symmetric spelling.")
    if isinstance(points, torch.Tensor) and points.dim() == 2:
        points = points.unsqueeze(0).expand(len(TCO_gt), -1, -1)
    rows, _, idx, _ = _sym_add_call("compute_MSSD", _lib.SYM_ADD_MAX, TCO_gt, TCO_pred, points, table, class_ids, True, False,
                                    bool(return_index), False, 1.0)
    return (rows, idx) if return_index else rows
