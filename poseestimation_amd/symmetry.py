"""Symmetric objects: the symmetry table, and the angle error and the Frobenius loss up to a symmetry group (K4s / K3s).
One family of the Python mirror; rotation_representation re-exports its public names."""
from __future__ import annotations

import numpy as np
import torch

from ._runtime import (_RANGE_MSG, _SMALL_BATCH, _capturing, _check, _f32_blocks, _is_f64, _launch, _libh, _no_double_backward, _on_device,
                       _ptr, _require_device, _stream, _wants_grad, _warn_once, _workspace)

# --------------------------------------------------------------------------------------------
# K4s / K3s: the metric and the loss up to a symmetry group
# --------------------------------------------------------------------------------------------
_SYM_MAX_K, _SYM_MAX_ENTRIES = 64, 256          # include/so3proj.h: 1 <= K <= 64, num_classes * K <= 256
_SYM_ORTHO_TOL = 1e-5


def _axis_vector(axis) -> np.ndarray:
    if isinstance(axis, str):
        if axis not in ("x", "y", "z"):
            raise ValueError(f"axis must be 'x', 'y', 'z' or a 3-vector, got {axis!r}")
        v = np.zeros(3)
        v["xyz".index(axis)] = 1.0
        return v
    v = np.asarray(axis.detach().cpu() if isinstance(axis, torch.Tensor) else axis, dtype=np.float64).reshape(-1)
    length = float(np.sqrt(v @ v)) if v.shape == (3,) else 0.0
    if not np.isfinite(length) or length == 0.0:
        raise ValueError(f"axis must be 'x', 'y', 'z' or a non-zero finite 3-vector, got {axis!r}")
    return v / length


def cyclic_symmetry(n: int, axis="z") -> torch.Tensor:
    """The cyclic group C_n about `axis` ("x", "y", "z" or a 3-vector): (n, 3, 3) float64 rotations by 2 pi j / n, j = 0 .. n-1,
    the identity first.  Sines and cosines within 1e-15 of 0 are 0, so a half or quarter turn about a coordinate axis is exact."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"n must be a positive integer, got {n!r}")
    a = _axis_vector(axis)
    th = 2.0 * np.pi * np.arange(int(n)) / int(n)
    c, s = np.cos(th), np.sin(th)
    c[np.abs(c) < 1e-15] = 0.0
    s[np.abs(s) < 1e-15] = 0.0
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    r = c[:, None, None] * np.eye(3) + (1.0 - c)[:, None, None] * np.outer(a, a) + s[:, None, None] * k      # Rodrigues
    return torch.from_numpy(r)


class SymmetryTable:
    """Per-class symmetry groups for symmetric_angle_error / symmetric_loss_frobenius.

    `groups` is one (K, 3, 3) array or tensor (one class: every row shares it) or a list of them, one per class id.  Each matrix
    must be a rotation (orthogonal to 1e-5, det > 0), checked once here in float64.  The identity goes to slot 0 (it is added if a
    group lacks it) and every class is padded with the identity to the largest K; K <= 64 and classes * K <= 256.
    `.matrices` is the (C, K, 3, 3) float64 table as used, so that an index k* returned by the functions reads as
    `table.matrices[class_id, k*]`.  The kernels hold its float32 rounding, uploaded to a device on first use and kept; in a graph
    capture that first use is an error -- call `table.to(device)` before capturing."""

    def __init__(self, groups):
        single = not isinstance(groups, (list, tuple))
        classes = [groups] if single else list(groups)
        if not classes:
            raise ValueError("SymmetryTable: no groups given")
        eye = np.eye(3)
        mats = []
        for c, g in enumerate(classes):
            a = np.asarray(g.detach().cpu() if isinstance(g, torch.Tensor) else g, dtype=np.float64)
            if a.shape == (3, 3):
                a = a[None]
            if a.ndim != 3 or a.shape[1:] != (3, 3) or a.shape[0] < 1:
                raise ValueError(f"SymmetryTable: class {c}: expected a (K, 3, 3) array of rotations, got shape {a.shape}")
            if not np.all(np.isfinite(a)):
                raise ValueError(f"SymmetryTable: class {c}: non-finite entries")
            err = np.abs(np.einsum("kji,kjl->kil", a, a) - eye).max(axis=(1, 2))
            if np.any(err > _SYM_ORTHO_TOL):
                raise ValueError(f"SymmetryTable: class {c}: element {int(np.argmax(err))} is not orthogonal "
                                 f"(|S^T S - I| = {err.max():.3g} > {_SYM_ORTHO_TOL})")
            det = np.linalg.det(a)
            if np.any(det <= 0):
                raise ValueError(f"SymmetryTable: class {c}: element {int(np.argmax(det <= 0))} is a reflection (det {det.min():.3g})")
            is_eye = np.abs(a - eye).max(axis=(1, 2)) <= _SYM_ORTHO_TOL
            mats.append(np.concatenate([eye[None], a[~is_eye]]))
        k = max(m.shape[0] for m in mats)
        if k > _SYM_MAX_K:
            raise ValueError(f"SymmetryTable: a class has {k} elements (identity included), at most {_SYM_MAX_K}")
        if len(mats) * k > _SYM_MAX_ENTRIES:
            raise ValueError(f"SymmetryTable: {len(mats)} classes x {k} elements > {_SYM_MAX_ENTRIES}")
        table = np.broadcast_to(eye, (len(mats), k, 3, 3)).copy()
        for c, m in enumerate(mats):
            table[c, :m.shape[0]] = m
        self.matrices = torch.from_numpy(table)
        self.num_classes, self.K = len(mats), k
        self._host = self.matrices.reshape(len(mats), k, 9).float().contiguous()      # the entries the kernels hold
        self._dev = {}

    def __repr__(self):
        return f"SymmetryTable(num_classes={self.num_classes}, K={self.K})"

    def to(self, device) -> "SymmetryTable":
        """Upload to `device` now (required before capturing a graph that uses the table there).  Returns self."""
        self._on(torch.device(device))
        return self

    def _on(self, dev: torch.device) -> torch.Tensor:
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        t = self._dev.get(idx)
        if t is None:
            if _capturing(dev):
                raise RuntimeError("SymmetryTable: first use on cuda:%d while a graph is being captured; call table.to(device) "
                                   "before the capture" % idx)
            t = self._host.to(torch.device("cuda", idx))
            self._dev[idx] = t
        return t


def _table_class_ids(what, table, class_ids, pred, n):
    """The (n,) int32 class ids the symmetric kernels take, on pred's device -- None for a single-class table."""
    if table.num_classes > 1:
        if class_ids is None:
            raise ValueError(f"{what}: a table of {table.num_classes} classes needs class_ids")
        _require_device(pred, class_ids)
        if class_ids.dtype not in (torch.int32, torch.int64) or class_ids.dim() != 1 or class_ids.shape[0] != n:
            raise ValueError(f"{what}: class_ids must be int32 or int64 of shape ({n},), got {class_ids.dtype} {tuple(class_ids.shape)}")
        if class_ids.dtype is torch.int64:            # out-of-range ids stay out of range in int32
            class_ids = class_ids.clamp(-1, table.num_classes).int()
        return class_ids.contiguous()
    if class_ids is not None:
        raise ValueError(f"{what}: class_ids given for a single-class table")
    return None


def _sym_args(R_pred, R_true, table, class_ids, what):
    """Kernel-ready (P, T, S, class ids) for the symmetric spellings."""
    if not isinstance(table, SymmetryTable):
        raise TypeError(f"{what}: table must be a SymmetryTable, got {type(table).__name__}")
    dev = _require_device(R_pred, R_true)
    if _is_f64(R_pred, R_true):
        raise TypeError(f"{what}: float64 arguments are not supported (the symmetric kernels read float32)")
    p, t = _f32_blocks(R_pred.detach()), _f32_blocks(R_true.detach())
    if p.shape != t.shape:
        raise RuntimeError(f"{what}: shape mismatch {tuple(R_pred.shape)} vs {tuple(R_true.shape)}")
    n = p.shape[0]
    cls = _table_class_ids(what, table, class_ids, R_pred, n)
    return dev, p, t, table._on(dev), cls, n


def symmetric_angle_error(R_pred: torch.Tensor, R_true: torch.Tensor, table: SymmetryTable, class_ids: torch.Tensor = None,
                          check: bool = True, return_index: bool = False):
    """Angle error up to a symmetry group: theta_b = min_k angle_error(R_pred_b @ S_k, R_true_b), float64 degrees, shape (B,).

    The group acts on the prediction from the right, as 3D-Pose/loss.py:14-24 (rotate_by_180).  S_k are the table's entries of
    row b's class (`class_ids`, int32 / int64 (B,), required for a multi-class table and refused for a single-class one).
    return_index=True also returns k*_b (int32 (B,)), the smallest k attaining the minimum, -1 for a class id out of range.
    The identity candidate is angle_error's arithmetic bit for bit, so a table {I} gives exactly angle_error.
    check=True reads one flag from the device: ValueError (angle_error's) where angle_error would raise, IndexError for a class
    id outside [0, C); check=False skips the read and leaves such rows NaN.  An evaluation metric: no gradient."""
    if _wants_grad(R_pred, R_true):
        _warn_once("symmetric_angle_error", "symmetric_angle_error is an evaluation call: its result carries no gradient although an "
                                            "argument requires grad.  symmetric_loss_frobenius is the differentiable symmetric spelling.")
    dev, p, t, s, cls, n = _sym_args(R_pred, R_true, table, class_ids, "symmetric_angle_error")
    deg = torch.empty((n,), dtype=torch.float64, device=dev)
    idx = torch.empty((n,), dtype=torch.int32, device=dev) if return_index else None
    if n > 0:
        flag = torch.empty((1,), dtype=torch.int32, device=dev) if check else None
        _launch(dev, "so3_sym_angle_error_f32", p.data_ptr(), t.data_ptr(), s.data_ptr(), _ptr(cls), table.num_classes, table.K,
                deg.data_ptr(), _ptr(idx), _ptr(flag), 0, n)
        if check:
            f = int(flag.item())
            if f & 1:
                raise ValueError(_RANGE_MSG)
            if f & 2:
                raise IndexError(f"symmetric_angle_error: a class id is outside [0, {table.num_classes})")
    return (deg, idx) if return_index else deg


class _SymLossFrobenius(torch.autograd.Function):
    """One launch writes the loss and, at unit upstream scale, the gradients the graph needs; backward scales them."""

    @staticmethod
    def forward(ctx, r_pred, r_true, table, class_ids, return_index):
        dev, p, t, s, cls, n = _sym_args(r_pred, r_true, table, class_ids, "symmetric_loss_frobenius")
        gp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        idx = torch.empty((n,), dtype=torch.int32, device=dev) if return_index else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        if n == 0:                                    # the mean of no rows, as torch's .mean() gives it
            loss.fill_(float("nan"))
            gp = None if gp is None else gp.zero_()
            gt = None if gt is None else gt.zero_()
        else:
            loss_sum = torch.empty((1,), dtype=torch.float64, device=dev)
            with _on_device(dev):
                st = _stream(dev)
                ws = _workspace(dev, st) if n > _SMALL_BATCH else None
                _check(_libh().so3_sym_frob_loss_f32(p.data_ptr(), t.data_ptr(), s.data_ptr(), _ptr(cls), table.num_classes, table.K,
                                                     _ptr(gp), _ptr(gt), _ptr(idx), loss_sum.data_ptr(), loss.data_ptr(), _ptr(ws), 0, n, st),
                       "so3_sym_frob_loss_f32")
        ctx.gp, ctx.gt = gp, gt
        ctx.shapes = (r_pred.shape, r_true.shape, r_pred.dtype, r_true.dtype)
        if return_index:
            ctx.mark_non_differentiable(idx)
            return loss, idx
        return loss

    @staticmethod
    def backward(ctx, grad_loss, *_):
        _no_double_backward(grad_loss)
        sp, st, dp, dt = ctx.shapes
        gp = (ctx.gp * grad_loss).to(dp).view(sp) if ctx.gp is not None else None
        gt = (ctx.gt * grad_loss).to(dt).view(st) if ctx.gt is not None else None
        return gp, gt, None, None, None


def symmetric_loss_frobenius(R_pred: torch.Tensor, R_true: torch.Tensor, table: SymmetryTable, class_ids: torch.Tensor = None,
                             return_index: bool = False):
    """Frobenius loss up to a symmetry group: mean_b min_k ||R_true_b - R_pred_b @ S_k||_F (not squared), a 0-dim float32 tensor
    -- the commented-out training block of 3D-Pose/main.py:63-84 (the best of rotate_by_180's flips), for any table.

    Differentiable in both arguments: the gradient is the selected branch's (k*, the smallest minimising k), gradients come back
    in each argument's dtype and shape.  One launch computes the loss and the gradients the graph needs; no host sync, so the call
    can be captured in a graph once the table is on the device (`table.to(device)`).  A table {I} gives loss_frobenius.
    class_ids as in symmetric_angle_error; an id out of range makes the loss NaN.  return_index=True also returns k* (int32 (B,))."""
    return _SymLossFrobenius.apply(R_pred, R_true, table, class_ids, return_index)
