"""Host-side mirror of the reference's hot-path interface, backed by libso3proj.so.

Same names, argument meaning and error behaviour as the reference functions they replace
(paths relative to the reference repository root):

    symmetric_orthogonalization(x)                     rotation_representation.py:192-206
    compute_geodesic_distance_from_two_matrices(m1,m2) rotation_representation.py:209-227
    angle_error(t_R1, t_R2)                            rotation_representation.py:230-242
    loss_frobenius(R_pred, R_true)                     3D-Pose/loss.py:7-11
    transform_output                                   rotation_representation.py:323-324

plus two fused entry points the reference spells as several calls:

    frobenius_head(x, R_true)      head + loss (+ backward in the same launch)   3D-Pose/main.py:60,85,90
    kabsch_rotation(P, Q)          bmm(Q^T, P) + head                            SURVEY.md section 8 a7

PyTorch is plumbing here: it owns device memory, the stream and autograd bookkeeping.  All
arithmetic happens in hand-written gfx950 kernels behind the C ABI (include/so3proj.h).  There is
no CPU path: a CPU tensor, or a missing libso3proj.so, raises.

This module defines what the reference's file of this name holds -- the heads, the metrics, the Frobenius loss, the inverse maps --
with their fused spellings, and it is the facade of the mirror: below its own definitions it re-exports every public name of the
other families (symmetry, angle_statistics, clouds, neighbors, pointnet, pose_losses) and the runtime's names that callers read through
it.  The plumbing all of them stand on is _runtime.py; DESIGN.md ("layout of the Python mirror") has the rules.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._runtime import (_RANGE_MSG, _SMALL_BATCH, _ZERO_POOL, _as_blocks, _check, _f32_blocks, _f64_blocks, _fn, _grad_to, _head_input, _is_f64,
                       _launch, _libh, _no_double_backward, _node, _on_device, _ptr, _require_device, _row_head, _stream, _wants_grad,
                       _warn_once, _workspace)

_HEAD_FNS = {}


def _head_fns(dtype):
    """(forward, backward) entry points and the dtype the rotation / upstream gradient travel in."""
    fns = _HEAD_FNS.get(dtype)
    if fns is None:
        if dtype == torch.bfloat16:
            fns = (_fn("so3_project_fwd_bf16"), _fn("so3_project_bwd_bf16"), torch.float32)
        elif dtype == torch.float64:
            fns = (_fn("so3_project_fwd_f64"), _fn("so3_project_bwd_f64"), torch.float64)
        else:
            fns = (_fn("so3_project_fwd_f32"), _fn("so3_project_bwd_f32"), torch.float32)
        _HEAD_FNS[dtype] = fns
    return fns


# --------------------------------------------------------------------------------------------
# K1 / K2: the head
# --------------------------------------------------------------------------------------------
class _SymmetricOrthogonalization(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        dev = x.device if x.is_cuda else _require_device(x)
        m = _head_input(x)
        b = m.shape[0]
        fn, _, out_dtype = _head_fns(m.dtype)
        r = torch.empty((b, 3, 3), dtype=out_dtype, device=dev)
        with _on_device(dev):
            _check(fn(m.data_ptr(), r.data_ptr(), None, b, _stream(dev)), "so3_project_fwd")
        ctx.save_for_backward(m)
        ctx.in_shape = x.shape
        ctx.in_dtype = x.dtype
        return r

    @staticmethod
    def backward(ctx, grad_r):
        _no_double_backward(grad_r)
        (m,) = ctx.saved_tensors
        dev = m.device
        _, fn, g_dtype = _head_fns(m.dtype)
        g = grad_r.reshape(-1, 9)
        if not g.is_contiguous():
            g = g.contiguous()
        if g.dtype is not g_dtype:
            g = g.to(g_dtype)
        b = m.shape[0]
        dm = torch.empty_like(m)
        with _on_device(dev):
            _check(fn(m.data_ptr(), g.data_ptr(), dm.data_ptr(), b, _stream(dev)), "so3_project_bwd")
        if dm.dtype is not ctx.in_dtype:
            dm = dm.to(ctx.in_dtype)
        return dm.view(ctx.in_shape)


def symmetric_orthogonalization(x: torch.Tensor) -> torch.Tensor:
    """Maps 9D input vectors onto SO(3) via symmetric orthogonalization (SVD).

    x: [batch_size, 9] (any shape whose numel is a multiple of 9, as `x.view(-1, 3, 3)` accepts).
    Returns [batch_size, 3, 3] rotations R = U diag(1,1,det(UV^T)) V^T, differentiable: float32 for float32,
    bfloat16 and float16 input, float64 for float64 input.
    """
    if isinstance(x, torch.Tensor) and not (x.requires_grad and torch.is_grad_enabled()):
        # inference / evaluation loops: no autograd node to build
        dev = x.device if x.is_cuda else _require_device(x)
        m = _head_input(x)
        fn, _, out_dtype = _head_fns(m.dtype)
        b = m.shape[0]
        r = torch.empty((b, 3, 3), dtype=out_dtype, device=dev)
        with _on_device(dev):
            _check(fn(m.data_ptr(), r.data_ptr(), None, b, _stream(dev)), "so3_project_fwd")
        return r
    node = _node()
    if node is not None and type(x) is torch.Tensor and x.is_cuda:
        r = node.symmetric_orthogonalization(x, _stream(x.device))          # the C++ node; None for what it does not cover
        if r is not None:
            return r
    return _SymmetricOrthogonalization.apply(x)


def symmetric_orthogonalization_with_flip(x: torch.Tensor):
    """(R, flip): flip[b] is True where det(U V^T) < 0, the sign the reference multiplies into the
    last row of V^T (rotation_representation.py:202-204).  Not differentiable."""
    dev = _require_device(x)
    m = _head_input(x.detach())
    b = m.shape[0]
    fn, _, out_dtype = _head_fns(m.dtype)
    r = torch.empty((b, 3, 3), dtype=out_dtype, device=dev)
    flip = torch.empty((b,), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        _check(fn(_ptr(m), _ptr(r), _ptr(flip), b, _stream(dev)), "so3_project_fwd")
    return r, flip.bool()


def symmetric_orthogonalization_segments(xs):
    """[(B_i, 9) float32, ...] -> [(B_i, 3, 3), ...]: up to eight independent batches in ONE launch of the streaming engine
    (so3_project_fwd_segments_f32: every B_i a positive multiple of 64).  The same bits as symmetric_orthogonalization on each;
    what it saves is the launch boundary between them.  Not differentiable."""
    import ctypes
    xs = list(xs)
    dev = _require_device(*xs)
    ms = []
    for x in xs:
        m = _as_blocks(x.detach())
        if m.dtype is not torch.float32:
            raise TypeError(f"symmetric_orthogonalization_segments: float32 input only, got {m.dtype}")
        ms.append(m)
    rs = [torch.empty((m.shape[0], 3, 3), dtype=torch.float32, device=dev) for m in ms]
    n = len(ms)
    in_ptrs = (ctypes.c_void_p * max(n, 1))(*[m.data_ptr() for m in ms])
    out_ptrs = (ctypes.c_void_p * max(n, 1))(*[r.data_ptr() for r in rs])
    rows = (ctypes.c_int64 * max(n, 1))(*[m.shape[0] for m in ms])
    with _on_device(dev):
        _check(_libh().so3_project_fwd_segments_f32(in_ptrs, out_ptrs, rows, n, _stream(dev)), "so3_project_fwd_segments_f32")
    return rs


# --------------------------------------------------------------------------------------------
# K4: metrics
# --------------------------------------------------------------------------------------------
def _angle_call(r1, r2, want_deg, want_sum, radians=False):
    dev = _require_device(r1, r2)
    a, b_ = _f32_blocks(r1), _f32_blocks(r2)
    if a.shape != b_.shape:
        raise RuntimeError(f"angle_error: shape mismatch {tuple(r1.shape)} vs {tuple(r2.shape)}")
    n = a.shape[0]
    deg = torch.empty((n,), dtype=torch.float64, device=dev) if want_deg else None
    with _on_device(dev):
        st = _stream(dev)
        sc, flag = _ZERO_POOL.take(dev, st)         # zero-filled slots: the kernel needs no init launch in front of it
        _check(_fn("so3_angle_error_v2")(a.data_ptr(), b_.data_ptr(), _ptr(deg), sc.data_ptr() if want_sum else None, flag.data_ptr(), None,
                                          _lib.PREZEROED | (_lib.RADIANS if radians else 0), n, st), "so3_angle_error")
    return deg, (sc if want_sum else None), flag


def _angle_call_f64(r1, r2, want_rows, want_sum, radians=False, geodesic=False):
    """float64 arguments (the reference casts to float64 before the product, rotation_representation.py:232-233, and returns
    the arguments' dtype from the geodesic distance): the same kernels' arithmetic on float64 data, so3_*_f64."""
    dev = _require_device(r1, r2)
    a, b_ = _f64_blocks(r1), _f64_blocks(r2)
    if a.shape != b_.shape:
        raise RuntimeError(f"angle_error: shape mismatch {tuple(r1.shape)} vs {tuple(r2.shape)}")
    n = a.shape[0]
    rows = torch.empty((n,), dtype=torch.float64, device=dev) if want_rows else None
    sc = torch.empty((2,), dtype=torch.float64, device=dev) if want_sum else None
    flag = None if geodesic else torch.empty((1,), dtype=torch.int32, device=dev)
    with _on_device(dev):
        if geodesic:
            _check(_libh().so3_geodesic_f64(a.data_ptr(), b_.data_ptr(), rows.data_ptr(), n, _stream(dev)), "so3_geodesic_f64")
        else:
            st = _stream(dev)
            ws = _workspace(dev, st) if n > _SMALL_BATCH else None          # one launch either way (above 1024 rows: the ticket finish)
            _check(_libh().so3_angle_error_v2_f64(a.data_ptr(), b_.data_ptr(), _ptr(rows), _ptr(sc), flag.data_ptr(), _ptr(ws),
                                                  _lib.RADIANS if radians else 0, n, st), "so3_angle_error_v2_f64")
    return rows, sc, flag


def _metric_backward(ctx, grad, eps: float, radians: bool, f64_math: bool, divisor: float):
    """dR1, dR2 of a metric spelling for the upstream gradient `grad` (K4b, so3_angle_bwd_*): one launch writes the gradients the
    graph needs.  An upstream gradient that autograd EXPANDED from one element (the backward of .mean() / .sum() on the per-row
    result) travels as that one element; a 0-dim one (geodesic's own reductions) likewise -- a device pointer, no host sync."""
    _no_double_backward(grad)
    a, b_ = ctx.saved_tensors
    need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    (shape1, dtype1), (shape2, dtype2) = ctx.meta
    if not (need1 or need2):
        return None, None
    dev = a.device
    n = a.shape[0]
    data64 = a.dtype is torch.float64
    g_dtype = torch.float64 if (data64 or f64_math) else torch.float32
    if grad.dim() == 0 or (grad.dim() == 1 and n > 1 and grad.stride(0) == 0):
        g = grad.reshape(-1)[:1]
        scalar = True
    else:
        g = grad.reshape(-1)
        scalar = False
        if g.shape[0] != n:
            raise RuntimeError(f"metric backward: {g.shape[0]} upstream gradients for {n} rows")
    if g.dtype is not g_dtype:
        g = g.to(g_dtype)
    if not g.is_contiguous():
        g = g.contiguous()
    d1 = torch.empty_like(a) if need1 else None
    d2 = torch.empty_like(a) if need2 else None
    if n > 0:
        flags = (_lib.RADIANS if radians else 0) | (_lib.GRAD_SCALAR if scalar else 0)
        if data64:
            _launch(dev, "so3_angle_bwd_f64", a.data_ptr(), b_.data_ptr(), g.data_ptr(), divisor, eps, flags, _ptr(d1), _ptr(d2), n)
        else:
            _launch(dev, "so3_angle_bwd_f32", a.data_ptr(), b_.data_ptr(), g.data_ptr(), divisor, eps, flags | (_lib.F64_MATH if f64_math else 0),
                    _ptr(d1), _ptr(d2), n)
    return _grad_to(d1, dtype1, shape1), _grad_to(d2, dtype2, shape2)


def _save_metric_inputs(ctx, r1, r2, f64: bool):
    """The (B,9) blocks the backward reads (the arguments themselves when they are contiguous float32 / float64 already)."""
    blocks = _f64_blocks if f64 else _f32_blocks
    a, b_ = blocks(r1), blocks(r2)
    ctx.save_for_backward(a, b_)
    ctx.meta = ((r1.shape, r1.dtype), (r2.shape, r2.dtype))
    return a, b_


class _AngleError(torch.autograd.Function):
    """angle_error as a graph node: the reference's function is plain differentiable tensor code (rotation_representation.py:230-242)."""

    @staticmethod
    def forward(ctx, r1, r2, check):
        f64 = _is_f64(r1, r2)
        a, b_ = _save_metric_inputs(ctx, r1, r2, f64)
        deg, _, flag = (_angle_call_f64 if f64 else _angle_call)(a, b_, True, False)
        if check and int(flag.item()) != 0:
            raise ValueError(_RANGE_MSG)
        return deg

    @staticmethod
    def backward(ctx, grad_deg):
        return (*_metric_backward(ctx, grad_deg, 0.0, False, True, 1.0), None)


def angle_error(t_R1: torch.Tensor, t_R2: torch.Tensor, check: bool = True) -> torch.Tensor:
    """Geodesic angle between rotations, float64 degrees, shape (B,).

    Raises ValueError("angle out of range, ...") when any cosine is outside [-1.1, 1.1], exactly as
    the reference does; that needs one device->host read (the reference's two `torch.any` cost two).
    `check=False` skips the read (and the raise) for benchmarking / graph capture.

    float64 arguments (the reference casts to float64 before the product, :232-233): K4 reads float32 data, so
    double tensors go to its float64 twin (so3_angle_error_v2_f64) instead of being rounded.

    Differentiable with respect to both arguments, like the reference's tensor code (K4b, so3_angle_bwd_*: the float64
    expression's gradient, rounded once to the argument's dtype; rows on the clamp get 0, as torch.clamp's backward gives).
    """
    if _wants_grad(t_R1, t_R2):
        _require_device(t_R1, t_R2)
        return _AngleError.apply(t_R1, t_R2, check)
    if _is_f64(t_R1, t_R2):
        deg, _, flag = _angle_call_f64(t_R1, t_R2, True, False)
    else:
        deg, _, flag = _angle_call(t_R1, t_R2, True, False)
    if check and int(flag.item()) != 0:
        raise ValueError(_RANGE_MSG)
    return deg


def angle_error_sum_count(t_R1: torch.Tensor, t_R2: torch.Tensor, check: bool = True) -> torch.Tensor:
    """Device tensor of two float64: (sum of angles in degrees, row count), reduced on the device.

    This pair is what one all-reduce sums across GPUs (poseestimation_amd.distributed); the
    per-row vector is never materialised."""
    if _wants_grad(t_R1, t_R2):
        _warn_once("angle_error_sum_count", "angle_error_sum_count is an evaluation call: the (sum, count) pair carries no gradient although an "
                                            "argument requires grad.  angle_error(...).sum() is the differentiable spelling.")
    _, sc, flag = (_angle_call_f64 if _is_f64(t_R1, t_R2) else _angle_call)(t_R1, t_R2, False, True)
    if check and int(flag.item()) != 0:
        raise ValueError(_RANGE_MSG)
    return sc


def head_angle_error(x: torch.Tensor, R_true: torch.Tensor, reduce: str = "none", check: bool = True, return_rotation: bool = False,
                     exact: bool = False):
    """Fused `angle_error(symmetric_orthogonalization(x), R_true)` (3D-Pose/main.py:60-62): one launch that reads
    x and R_true (72 B per row) and writes only what is asked for.

    reduce="none": (B,) float64 degrees;  reduce="mean": 0-dim float64 mean;  reduce="sum_count": the (sum, count)
    pair for a multi-GPU all-reduce.  return_rotation=True also returns R.  Not differentiable (evaluation path).

    Arithmetic.  reduce="none" gives, row for row, what `angle_error` gives on the materialised rotation (the reference's
    float64 expression, rotation_representation.py:232-241; equal to 1e-9 degrees).  The reduced forms of a batch above 1024
    rows evaluate the same expression -- trace, cosine, clamp, acos -- in float32 for every row whose cosine is at least
    5e-7 away from +-1 and in float64 for the rows inside that band (angles within 0.057 degrees of 0 or 180), and sum in
    float64: the result differs from `angle_error(...).mean()` by the float32 trace's round-off, at most 2e-7 / sin(theta) rad
    per row and without bias -- 3e-8 degrees on the mean of 1M Haar-distributed pairs, below 2e-6 degrees when every pair is
    0.3 degrees apart (the reference's own sensitivity to the 1e-7 of orthonormality defect its float32 inputs carry is larger).
    exact=True runs the float64 expression on every row (20 % slower at 1M rows).  The range check is the reference's."""
    if reduce not in ("none", "mean", "sum_count"):
        raise ValueError("reduce must be 'none', 'mean' or 'sum_count'")
    dev = _require_device(x, R_true)
    if _wants_grad(x, R_true):
        _warn_once("head_angle_error",
                   "head_angle_error is an evaluation call: its result carries no gradient although an argument requires grad.  "
                   "angle_error(symmetric_orthogonalization(x), R_true) and geodesic(...) are the differentiable spellings.")
    m = _head_input(x.detach())
    if m.dtype != torch.float32:
        m = m.float()
    t = _f32_blocks(R_true.detach())
    n = m.shape[0]
    if t.shape[0] != n:
        raise RuntimeError(f"head_angle_error: {n} predictions vs {t.shape[0]} targets")
    want_deg = reduce == "none"
    # the fused kernel handles whole 64-row units of 16-byte aligned arrays; anything else goes K1 -> R -> K4
    need_r = return_rotation or (n % 64 != 0) or (m.data_ptr() % 16 != 0) or (t.data_ptr() % 16 != 0)
    r = torch.empty((n, 3, 3), dtype=torch.float32, device=dev) if need_r else None
    deg = torch.empty((n,), dtype=torch.float64, device=dev) if want_deg else None
    with _on_device(dev):
        st = _stream(dev)
        sc, flag = _ZERO_POOL.take(dev, st)         # zero-filled slots: the kernel needs no init launch in front of it
        if want_deg:
            sc = None
        _check(_fn("so3_project_angle_error_v2_f32")(_ptr(m), _ptr(t), _ptr(r), _ptr(deg), _ptr(sc), _ptr(flag), None,
                                                      _lib.PREZEROED | (_lib.EXACT_F64 if exact else 0), n, st), "so3_project_angle_error_f32")
    if check and int(flag.item()) != 0:
        raise ValueError(_RANGE_MSG)
    out = deg if want_deg else (sc if reduce == "sum_count" else sc[0] / sc[1])
    return (out, r) if return_rotation else out


def _geodesic_rows(a, b_, dev):
    """K4' on (B,9) float32 / float64 blocks: radians, hard clamp."""
    if a.dtype is torch.float64:
        return _angle_call_f64(a, b_, True, False, geodesic=True)[0]
    n = a.shape[0]
    theta = torch.empty((n,), dtype=torch.float32, device=dev)
    _launch(dev, "so3_geodesic_f32", _ptr(a), _ptr(b_), _ptr(theta), n)
    return theta


class _GeodesicDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m1, m2):
        a, b_ = _save_metric_inputs(ctx, m1, m2, _is_f64(m1, m2))
        return _geodesic_rows(a, b_, a.device)

    @staticmethod
    def backward(ctx, grad_theta):
        return _metric_backward(ctx, grad_theta, 0.0, True, False, 1.0)


def compute_geodesic_distance_from_two_matrices(m1: torch.Tensor, m2: torch.Tensor) -> torch.Tensor:
    """Geodesic distance in radians, tr(m1 m2^T), hard clamp to [-1, 1]; shape (B,); the arguments' dtype as the
    reference (rotation_representation.py:209-227): float32 through K4', float64 through so3_geodesic_f64.
    Differentiable with respect to both arguments (K4b; a row on the clamp gets 0, as torch.min / torch.max's backward gives)."""
    dev = _require_device(m1, m2)
    f64 = _is_f64(m1, m2)
    if not f64 and _as_blocks(m1).shape != _as_blocks(m2).shape:
        raise RuntimeError(f"geodesic: shape mismatch {tuple(m1.shape)} vs {tuple(m2.shape)}")
    if _wants_grad(m1, m2):
        return _GeodesicDistance.apply(m1, m2)
    if f64:
        return _angle_call_f64(m1, m2, True, False, geodesic=True)[0]
    return _geodesic_rows(_f32_blocks(m1), _f32_blocks(m2), dev)


def _geodesic_eps(a, b_, reduction, dev):
    """geodesic(...)'s launch on (B,9) blocks: float32 through so3_geodesic_eps_f32, float64 through its twin."""
    n = a.shape[0]
    dt = a.dtype
    f64 = dt is torch.float64
    theta = torch.empty((n,), dtype=dt, device=dev) if reduction == "none" else None
    acc = None if reduction == "none" else torch.empty((1,), dtype=torch.float64, device=dev)
    out = None if reduction == "none" else torch.empty((), dtype=dt, device=dev)
    with _on_device(dev):
        st = _stream(dev)
        if f64:
            _check(_libh().so3_geodesic_eps_f64(_ptr(a), _ptr(b_), _ptr(theta), _ptr(acc), _ptr(out), 1 if reduction == "mean" else 0, 1e-7, n, st),
                   "so3_geodesic_eps_f64")
        else:
            ws = _workspace(dev, st) if reduction != "none" else None           # the kernel's last workgroup writes the reduced value
            _check(_libh().so3_geodesic_eps_f32(_ptr(a), _ptr(b_), _ptr(theta), _ptr(acc), _ptr(out), 1 if reduction == "mean" else 0, 1e-7,
                                                _ptr(ws), n, st), "so3_geodesic_eps_f32")
    return theta if reduction == "none" else out


class _Geodesic(torch.autograd.Function):
    """geodesic(R1, R2, reduction) as a graph node: the use its eps was written for (point_cloud/main.py:64)."""

    @staticmethod
    def forward(ctx, r1, r2, reduction):
        a, b_ = _save_metric_inputs(ctx, r1, r2, _is_f64(r1, r2))
        ctx.divisor = float(a.shape[0]) if reduction == "mean" else 1.0
        return _geodesic_eps(a, b_, reduction, a.device)

    @staticmethod
    def backward(ctx, grad):
        if ctx.divisor == 0.0:                        # the mean of no rows: no rows to send a gradient to
            (s1, d1), (s2, d2) = ctx.meta
            a, _ = ctx.saved_tensors
            return (torch.zeros(s1, dtype=d1, device=a.device) if ctx.needs_input_grad[0] else None,
                    torch.zeros(s2, dtype=d2, device=a.device) if ctx.needs_input_grad[1] else None, None)
        return (*_metric_backward(ctx, grad, 1e-7, True, False, ctx.divisor), None)


def geodesic(R1: torch.Tensor, R2: torch.Tensor, reduction: str = "mean"):
    """point_cloud/main.py:61-73: acos(clamp((tr(R1 R2^T) - 1)/2, -1 + 1e-7, 1 - 1e-7)), radians, in the arguments' dtype (float32
    on the hot path; float64 arguments go to the float64 twin);
    reduction "none" -> (B,), "mean" / "sum" -> 0-dim; any other string returns None, as the reference's if-chain does.
    Angles and their sum leave one launch (float64 accumulation; the reference's float32 .mean() agrees to its own round-off).
    Differentiable with respect to both arguments (K4b, so3_angle_bwd_*): one launch for dR1 and dR2, the reduction's 1/B folded in."""
    dev = _require_device(R1, R2)
    f64 = _is_f64(R1, R2)
    blocks = _f64_blocks if f64 else _f32_blocks
    if _as_blocks(R1).shape != _as_blocks(R2).shape:
        raise RuntimeError(f"geodesic: shape mismatch {tuple(R1.shape)} vs {tuple(R2.shape)}")
    if reduction not in ("none", "mean", "sum"):
        return None
    if _wants_grad(R1, R2):
        return _Geodesic.apply(R1, R2, reduction)
    return _geodesic_eps(blocks(R1), blocks(R2), reduction, dev)


# --------------------------------------------------------------------------------------------
# K3: loss
# --------------------------------------------------------------------------------------------
class _LossFrobenius(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r_pred, r_true):
        dev = _require_device(r_pred, r_true)
        f64 = r_pred.dtype is torch.float64 or r_true.dtype is torch.float64      # torch's promotion: the loss is float64 then
        blocks = _f64_blocks if f64 else _f32_blocks
        p, t = blocks(r_pred), blocks(r_true)
        if p.shape != t.shape:
            raise RuntimeError(f"loss_frobenius: shape mismatch {tuple(r_pred.shape)} vs {tuple(r_true.shape)}")
        b = p.shape[0]
        need_grad = r_pred.requires_grad or r_true.requires_grad
        g = torch.empty_like(p) if need_grad else None
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float64 if f64 else torch.float32, device=dev)       # the mean is written by the kernel
        with _on_device(dev):
            st = _stream(dev)
            if f64:
                ws = _workspace(dev, st) if b > _SMALL_BATCH else None
                _check(_libh().so3_frob_loss_v2_f64(p.data_ptr(), t.data_ptr(), _ptr(g), loss_sum.data_ptr(), loss.data_ptr(), _ptr(ws), 0, b, st),
                       "so3_frob_loss_v2_f64")
            else:
                ws = _workspace(dev, st) if b > _SMALL_BATCH else None
                _check(_fn("so3_frob_loss_v2_f32")(p.data_ptr(), t.data_ptr(), _ptr(g), loss_sum.data_ptr(), loss.data_ptr(), _ptr(ws), 0, b, st),
                       "so3_frob_loss_f32")
        ctx.g = g
        ctx.shapes = (r_pred.shape, r_true.shape, r_pred.dtype, r_true.dtype)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if ctx.g is None:
            return None, None
        sp, st, dp, dt = ctx.shapes
        g = ctx.g * grad_loss
        gp = g.to(dp).view(sp) if ctx.needs_input_grad[0] else None
        gt = (-g).to(dt).view(st) if ctx.needs_input_grad[1] else None
        return gp, gt


def loss_frobenius(R_pred: torch.Tensor, R_true: torch.Tensor) -> torch.Tensor:
    """mean_b ||R_true - R_pred||_F (not squared), differentiable w.r.t. both arguments.

    Stand-alone form for callers that already hold R_pred (one kernel for the loss and its gradient).
    A training step should use `frobenius_head`, which fuses head, loss and backward into one launch.

    Returns the arguments' dtype as the reference (3D-Pose/loss.py:7-11): float32 through K3'; if either argument is
    float64 (e.g. the float64 head's output) its float64 twin, so3_frob_loss_v2_f64."""
    node = _node()
    if node is not None and type(R_pred) is torch.Tensor and type(R_true) is torch.Tensor and R_pred.is_cuda:
        dev = R_pred.device
        st = _stream(dev)
        ws = 0
        if R_pred.numel() > 9 * _SMALL_BATCH:
            w = _workspace(dev, st)
            ws = w.data_ptr() if w is not None else 0
        loss = node.loss_frobenius(R_pred, R_true, st, ws)                   # the C++ node; None for what it does not cover
        if loss is not None:
            return loss
    return _LossFrobenius.apply(R_pred, R_true)


class _FrobeniusHead(torch.autograd.Function):
    """One differentiable output (the loss); the rotation, which carries no gradient, leaves through `box` instead of being a
    second output that autograd would have to wrap, mark and track."""

    @staticmethod
    def forward(ctx, x, r_true, want_r, box):
        dev = x.device if (x.is_cuda and r_true.is_cuda and x.device == r_true.device) else _require_device(x, r_true)
        m = _head_input(x)
        b = m.shape[0]
        if r_true.dtype is torch.float32 and r_true.is_contiguous() and r_true.numel() == 9 * b:
            t = r_true                                               # (B,3,3) or (B,9) as stored: only its address is needed
        else:
            t = _f32_blocks(r_true)
            if t.shape[0] != b:
                raise RuntimeError(f"frobenius_head: {b} predictions vs {t.shape[0]} targets")
        need_grad = x.requires_grad
        # d loss / d R_true = -(R - R_true) / (B ||R - R_true||_F), the loss being differentiable in both arguments
        # (3D-Pose/loss.py:7-11): it is rebuilt in backward from R and R_true (K3'), so R is kept whenever it is asked for
        ctx.true_grad = r_true.requires_grad
        want_r_user = want_r                      # the caller gets R (and may write into it)
        want_r = want_r or ctx.true_grad
        r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev) if want_r else None
        dm = torch.empty_like(m) if need_grad else None
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if b > _SMALL_BATCH or b == 0 else None
        loss = torch.empty((), dtype=torch.float32, device=dev)      # the kernel writes the float32 mean itself: no launch of ours
        fn = _fn("so3_frob_fwd_bwd_v2_bf16" if m.dtype is torch.bfloat16 else "so3_frob_fwd_bwd_v2_f32")
        with _on_device(dev):
            st = _stream(dev)
            ws = _workspace(dev, st) if b > _SMALL_BATCH else None
            _check(fn(m.data_ptr(), t.data_ptr(), _ptr(r), _ptr(dm), _ptr(loss_sum), loss.data_ptr(), _ptr(ws), 0, b, st), "so3_frob_fwd_bwd")
        ctx.dm = dm
        ctx.in_shape = x.shape
        ctx.in_dtype = x.dtype
        if ctx.true_grad:
            # the target goes through save_for_backward (an in-place edit between forward and backward then raises instead of
            # yielding a silently wrong gradient); the rotation handed to the caller leaves autograd through `box`, so backward
            # keeps a private copy of it
            ctx.save_for_backward(t)
            ctx.rt = (r.clone() if want_r_user else r, r_true.shape, r_true.dtype)
        box.append(r)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        _no_double_backward(grad_loss)
        dm = ctx.dm
        gx = gt = None
        if dm is not None and ctx.needs_input_grad[0]:
            # out of place: a second backward over the same graph (retain_graph, several losses) must see the stored gradient
            # unscaled, and the tensor handed out must not alias it.  One launch of ours (so3_scale_*) instead of torch's
            # float() / mul / to(bfloat16) chain: the upstream factor is a 0-dim float32 device tensor.
            if grad_loss.dtype is torch.float32 and grad_loss.is_cuda and dm.dtype is ctx.in_dtype:
                dev = dm.device
                gx = torch.empty_like(dm)
                fn = _fn("so3_scale_bf16" if dm.dtype is torch.bfloat16 else "so3_scale_f32")
                with _on_device(dev):
                    _check(fn(dm.data_ptr(), grad_loss.data_ptr(), gx.data_ptr(), dm.numel(), _stream(dev)), "so3_scale")
                gx = gx.view(ctx.in_shape)
            elif dm.dtype == ctx.in_dtype:
                gx = (dm * grad_loss).view(ctx.in_shape)
            else:
                gx = (dm.float() * grad_loss).to(ctx.in_dtype).view(ctx.in_shape)
        if ctx.true_grad and ctx.needs_input_grad[1]:
            r, shape, dtype = ctx.rt
            (t,) = ctx.saved_tensors
            dev = t.device
            b = t.shape[0]
            g = torch.empty_like(t)                              # d(mean loss)/dR_pred; the target's gradient is its negative
            scratch = torch.empty((1,), dtype=torch.float64, device=dev)
            with _on_device(dev):
                _check(_libh().so3_frob_loss_v2_f32(_ptr(r), _ptr(t), _ptr(g), _ptr(scratch), None, None, 0, b, _stream(dev)), "so3_frob_loss_f32")
            gt = (g * (-grad_loss)).to(dtype).view(shape)
        return gx, gt, None, None


def frobenius_head(x: torch.Tensor, R_true: torch.Tensor, return_rotation: bool = True):
    """Fused `out = symmetric_orthogonalization(x); loss = loss_frobenius(R_true, out)`.

    One kernel computes R, the loss and d(loss)/dx; `loss.backward()` then only scales the stored
    gradient.  Returns (loss, R) -- R is detached (use it for metrics) -- or loss alone.
    float64 x: the fused kernel is float32 / bfloat16 only, so the float64 head and the float64 loss are composed
    (same values and dtypes as the reference's two calls).
    """
    if x.dtype is torch.float64:
        r64 = symmetric_orthogonalization(x)
        loss64 = loss_frobenius(R_true.to(torch.float64), r64)
        return (loss64, r64.detach()) if return_rotation else loss64
    node = _node()
    if node is not None and type(x) is torch.Tensor and type(R_true) is torch.Tensor and x.is_cuda and x.dim() >= 2:
        # the C++ node: same launches, no interpreter inside forward / backward; it declines (None) what it does not cover
        dev = x.device
        st = _stream(dev)
        ws = 0
        if x.shape[0] > _SMALL_BATCH:
            w = _workspace(dev, st)
            ws = w.data_ptr() if w is not None else 0
        res = node.frobenius_head(x, R_true, return_rotation, st, ws)
        if res is not None:
            return res if return_rotation else res[0]
    box = []
    loss = _FrobeniusHead.apply(x, R_true, return_rotation, box)
    return (loss, box[0]) if return_rotation else loss


class FrobeniusHeadStep:
    """The tail of a training step -- head, Frobenius loss and d(loss)/dx (3D-Pose/main.py:60,85,90) -- for a FIXED batch
    shape, recorded once into a hipGraph and replayed: config #4 (B = 512) is launch-bound, and through autograd the
    Python and engine bookkeeping around the 5-us kernel costs twenty times the kernel.

        step = FrobeniusHeadStep(512, dtype=torch.bfloat16, device="cuda:0")
        step.x.copy_(network_output); step.r_true.copy_(targets)      # or write into them directly
        loss, dx, r = step()                                          # one graph replay; tensors are reused between calls
        network_output.backward(dx)                                   # continue into the backbone

    `x`, `r_true` are the static inputs; `loss` (0-dim float32 mean), `dx` (like x) and `r` (B,3,3) are overwritten by
    every call.  The C ABI is enqueue-only with caller-owned buffers, which is what makes it capturable."""

    def __init__(self, batch: int, dtype: torch.dtype = torch.float32, device="cuda", return_rotation: bool = True):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("FrobeniusHeadStep needs a HIP device (there is no CPU fallback)")
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("FrobeniusHeadStep: float32 or bfloat16 input")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.batch = int(batch)
        self.x = torch.zeros((self.batch, 9), dtype=dtype, device=dev)
        self.r_true = torch.eye(3, device=dev).repeat(self.batch, 1, 1)
        self.dx = torch.empty_like(self.x)
        self.r = torch.empty((self.batch, 3, 3), dtype=torch.float32, device=dev) if return_rotation else None
        self._sum = torch.empty((1,), dtype=torch.float64, device=dev)
        self.loss = torch.empty((), dtype=torch.float32, device=dev)
        lib = _libh()
        fn = lib.so3_frob_fwd_bwd_v2_bf16 if dtype == torch.bfloat16 else lib.so3_frob_fwd_bwd_v2_f32
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))

        def record():                 # the float32 mean is written by the kernel(s); no workspace inside a graph
            _check(fn(_ptr(self.x), _ptr(self.r_true), _ptr(self.r), _ptr(self.dx), _ptr(self._sum), _ptr(self.loss), None, 0, self.batch,
                      side.cuda_stream), "so3_frob_fwd_bwd")

        with torch.cuda.device(dev), torch.cuda.stream(side):
            record()                                                                 # warm-up outside the capture
            side.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph, stream=side, capture_error_mode="thread_local"):
                record()
        torch.cuda.current_stream(dev).wait_stream(side)

    def __call__(self):
        self._graph.replay()
        return self.loss, self.dx, self.r


# --------------------------------------------------------------------------------------------
# next row f2: the 6D Gram-Schmidt head
# --------------------------------------------------------------------------------------------
class _Ortho6d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses):
        dev = _require_device(poses)
        if poses.shape[-1] != 6:
            raise AssertionError("compute_rotation_matrix_from_ortho6d expects (..., 6) poses")   # reference: assert, :28
        x = poses.detach().reshape(-1, 6).contiguous().float()
        b = x.shape[0]
        r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
        _launch(dev, "so3_ortho6d_fwd_f32", _ptr(x), _ptr(r), b)
        ctx.save_for_backward(x)
        ctx.in_shape, ctx.in_dtype = poses.shape, poses.dtype
        return r.view(*poses.shape[:-1], 3, 3)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_r):
        (x,) = ctx.saved_tensors
        dev = x.device
        g = grad_r.reshape(-1, 9).contiguous().float()
        dx = torch.empty_like(x)
        _launch(dev, "so3_ortho6d_bwd_f32", _ptr(x), _ptr(g), _ptr(dx), x.shape[0])
        return dx.to(ctx.in_dtype).view(ctx.in_shape)


def compute_rotation_matrix_from_ortho6d(poses: torch.Tensor) -> torch.Tensor:
    """6D (two 3-vectors) -> rotation by Gram-Schmidt, columns (x, y, z); rotation_representation.py:21-36.
    poses: (..., 6); returns (..., 3, 3) float32, differentiable."""
    r = _row_head("ortho6d", 6, poses)
    return r if r is not None else _Ortho6d.apply(poses)


# --------------------------------------------------------------------------------------------
# next row f5: the other heads of the reference's dispatch tables
# --------------------------------------------------------------------------------------------
def _make_head(symbol: str, width: int):
    """autograd.Function over so3_<symbol>_fwd_f32 / _bwd_f32 for a (B, width) -> (B, 3, 3) head."""

    class _Head(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x_in):
            dev = _require_device(x_in)
            x = x_in.detach().contiguous().float()
            b = x.shape[0]
            r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
            _launch(dev, "so3_%s_fwd_f32" % symbol, _ptr(x), _ptr(r), b)
            ctx.save_for_backward(x)
            ctx.in_dtype = x_in.dtype
            return r

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_r):
            (x,) = ctx.saved_tensors
            dev = x.device
            g = grad_r.reshape(-1, 9).contiguous().float()
            dx = torch.empty_like(x)
            _launch(dev, "so3_%s_bwd_f32" % symbol, _ptr(x), _ptr(g), _ptr(dx), x.shape[0])
            return dx.to(ctx.in_dtype)

    _Head.__name__ = "_Head_" + symbol
    return _Head


_Quat, _Euler, _Ortho5d, _ExpMap = (_make_head(sym, n) for sym, n in (("quat", 4), ("euler", 3), ("ortho5d", 5), ("expmap", 3)))


def _batch_of(x: torch.Tensor, width: int, name: str) -> None:
    if x.dim() != 2 or x.shape[1] != width:          # the reference indexes [:, k] and .view(batch, 1): 2-D input only
        raise RuntimeError("%s expects a (batch, %d) tensor, got %s" % (name, width, tuple(x.shape)))


def compute_rotation_matrix_from_quaternion(quaternion: torch.Tensor) -> torch.Tensor:
    """(B,4) quaternion (w,x,y,z), normalised with max(|q|, 1e-8) -> (B,3,3); rotation_representation.py:137-171."""
    _batch_of(quaternion, 4, "compute_rotation_matrix_from_quaternion")
    r = _row_head("quat", 4, quaternion)
    return r if r is not None else _Quat.apply(quaternion)


def compute_rotation_matrix_from_euler(euler: torch.Tensor) -> torch.Tensor:
    """(B,3) Euler angles -> (B,3,3) in the reference's convention (c2,s2 from column 2, c3,s3 from column 1);
    rotation_representation.py:92-113."""
    _batch_of(euler, 3, "compute_rotation_matrix_from_euler")
    r = _row_head("euler", 3, euler)
    return r if r is not None else _Euler.apply(euler)


def compute_rotation_matrix_from_ortho5d(a: torch.Tensor) -> torch.Tensor:
    """(B,5) -> (B,3,3): stereographic un-projection of a[:,2:5] to a unit 4-vector, then the 6D head;
    rotation_representation.py:118-134."""
    _batch_of(a, 5, "compute_rotation_matrix_from_ortho5d")
    r = _row_head("ortho5d", 5, a)
    return r if r is not None else _Ortho5d.apply(a)


def so3_exp_map(log_rot: torch.Tensor, eps: float = 0.0001) -> torch.Tensor:
    """so(3) exponential map with PyTorch3D's clamp; rotation_representation.py:245-275."""
    if log_rot.dim() != 2 or log_rot.shape[1] != 3:
        raise ValueError("Input tensor shape has to be Nx3.")                   # reference: :255-256
    if eps != 0.0001:
        raise NotImplementedError("so3_exp_map: the kernel is built for the reference's only eps, 1e-4")
    r = _row_head("expmap", 3, log_rot)
    return r if r is not None else _ExpMap.apply(log_rot)


def vec_3d_to_SO3(x: torch.Tensor) -> torch.Tensor:
    """transform_output['3D']: (B,3) -> (B,3,3) through so3_exp_map; rotation_representation.py:309-321."""
    assert x.dim() == 2 and x.shape[1] == 3                                      # reference: assert, :316
    return so3_exp_map(x)


# Head dispatch tables, keyed like the reference's.  `transform_output` is rotation_representation.py:323-324;
# `head_functions` / `head_dimensions` are Model.func / Model.dimension of Comparison/models.py:18-19 and
# point_cloud/model_fetch.py:153-154 ("Direct" is a reshape there and has no function), with 3D-Pose/main.py:46's
# lower-case "quat" as an alias.  The SVD head is the scope of SURVEY.md section 8; the rest are its next rows f2, f5.
transform_output = {"SVD": (9, symmetric_orthogonalization), "6D": (6, compute_rotation_matrix_from_ortho6d),
                    "3D": (3, vec_3d_to_SO3)}
head_dimensions = {"SVD": 9, "6D": 6, "5D": 5, "Quat": 4, "Euler": 3, "Direct": 9}
head_functions = {"SVD": symmetric_orthogonalization, "6D": compute_rotation_matrix_from_ortho6d,
                  "5D": compute_rotation_matrix_from_ortho5d, "Quat": compute_rotation_matrix_from_quaternion,
                  "quat": compute_rotation_matrix_from_quaternion, "Euler": compute_rotation_matrix_from_euler}


# --------------------------------------------------------------------------------------------
# inverse maps: rotation matrix -> quaternion / rotation vector / Euler angles / 6D, and log(R1^T R2)
# --------------------------------------------------------------------------------------------
# GRADIENT CONVENTION (include/so3proj.h).  The backward of every inverse map returns the TANGENT-SPACE gradient at R: with
# w = (d f(R exp(hat delta)) / d delta)^T g it is dR = 1/2 R hat(w).  It does not depend on the branch the forward took, it is bounded
# for the log map up to theta = pi, and it equals the tangent projection R skew(R^T G) of any off-manifold autograd gradient G.
# Every head of this package moves R along tangent directions, so chaining an inverse map behind a head is exact.
EULER_GIMBAL_COS_FLOOR = 1e-6        # csrc: kEulerMinCos -- cos(e2) is clamped from below at this in matrix_to_euler's gradient


def _check_rotations(r: torch.Tensor, name: str) -> None:
    if not ((r.dim() == 3 and r.shape[1:] == (3, 3)) or (r.dim() == 2 and r.shape[1] == 9)):
        raise RuntimeError("%s expects (B,3,3) or (B,9) rotation matrices, got %s" % (name, tuple(r.shape)))
    if r.dtype not in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
        raise TypeError("%s: unsupported dtype %s (inputs: float32, float16, bfloat16, float64)" % (name, r.dtype))


def _rotation_blocks(r: torch.Tensor, name: str) -> torch.Tensor:
    """(B,3,3) or (B,9) of any supported dtype -> contiguous float32 (B,9) (detached)."""
    _check_rotations(r, name)
    return r.detach().reshape(-1, 9).contiguous().float()


def _make_inverse(symbol: str, width: int, name: str):
    """autograd.Function over so3_<symbol>_fwd_f32 / _bwd_f32 for a (B,3,3) -> (B, width) inverse map."""

    class _Inverse(torch.autograd.Function):
        @staticmethod
        def forward(ctx, r_in):
            dev = _require_device(r_in)
            r = _rotation_blocks(r_in, name)
            b = r.shape[0]
            y = torch.empty((b, width), dtype=torch.float32, device=dev)
            _launch(dev, "so3_%s_fwd_f32" % symbol, _ptr(r), _ptr(y), b)
            ctx.save_for_backward(r)
            ctx.in_dtype, ctx.in_shape = r_in.dtype, r_in.shape
            return y

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_y):
            (r,) = ctx.saved_tensors
            dev = r.device
            g = grad_y.reshape(-1, width).contiguous().float()
            dr = torch.empty_like(r)
            _launch(dev, "so3_%s_bwd_f32" % symbol, _ptr(r), _ptr(g), _ptr(dr), r.shape[0])
            return dr.to(ctx.in_dtype).view(ctx.in_shape)

    _Inverse.__name__ = "_Inverse_" + symbol
    return _Inverse


_MatToQuat = _make_inverse("mat_to_quat", 4, "matrix_to_quaternion")
_LogMap = _make_inverse("logmap", 3, "so3_log_map")
_MatToEuler = _make_inverse("mat_to_euler", 3, "matrix_to_euler")


def matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """(B,3,3) or (B,9) rotation matrices -> (B,4) float32 unit quaternions (w,x,y,z) with w >= 0, the order
    compute_rotation_matrix_from_quaternion reads.  Shepperd's method on the largest of (tr, r0, r4, r8), branch-free.
    Differentiable: the backward returns the tangent-space gradient 1/2 R hat(w), w = (dq/ddelta)^T g,
    dq/ddelta = 1/2 [-(x,y,z)^T ; w I + hat(x,y,z)] (see the convention above), cast back to R's dtype and shape.
    Nothing is validated on the device: a NaN row gives a NaN row."""
    return _MatToQuat.apply(R)


def so3_log_map(R: torch.Tensor) -> torch.Tensor:
    """(B,3,3) or (B,9) rotation matrices -> (B,3) float32 rotation vectors, |v| <= float32(pi): the inverse of so3_exp_map /
    vec_3d_to_SO3.  Through the quaternion (theta = 2 atan2(|xyz|, w)), so the axis survives next to theta = pi, where acos of the
    trace and (R - R^T) / (2 sin theta) lose it.  Differentiable: tangent-space gradient 1/2 R hat(J_r^-T(v) g), bounded up to pi."""
    return _LogMap.apply(R)


def matrix_to_euler(R: torch.Tensor) -> torch.Tensor:
    """(B,3,3) or (B,9) rotation matrices -> (B,3) float32 Euler angles in compute_rotation_matrix_from_euler's convention
    (e[:,2] is the middle angle, |e[:,2]| <= pi/2): (s3, c3) = (r2, r0) / |(r2, r0)| = sincos(e1), e0 = atan2(s3 r3 - c3 r5, c3 r8 - s3 r6),
    which keeps forward(inverse(R)) within rounding of R at gimbal lock, and e2 = atan2(clamp(-r1, -1, 1), |(r2, r0)|), clamped to the
    float32 just below pi/2 -- asin(-r1) for a rotation, computed from the two entries that still hold cos(e2) next to gimbal lock, where
    a float32 r1 has rounded to +-1.  At gimbal lock -- r0^2 + r2^2 below float32's smallest normal, |(r2, r0)| below about 1.1e-19 --
    cos(e2) counts as 0 and e1 = 0.
    Differentiable (tangent-space gradient); the Jacobian carries 1 / cos(e2), and cos(e2) is clamped from below at
    EULER_GIMBAL_COS_FLOOR, so the gradient is finite everywhere."""
    return _MatToEuler.apply(R)


def matrix_to_ortho6d(R: torch.Tensor) -> torch.Tensor:
    """(B,3,3) or (B,9) rotation matrices -> (B,6) float32: the first two columns, in the layout the 6D head reads
    (compute_rotation_matrix_from_ortho6d).  Plain indexing, differentiated by torch's own autograd."""
    _require_device(R)
    _check_rotations(R, "matrix_to_ortho6d")
    m = R.reshape(-1, 3, 3).float()
    return torch.cat((m[:, :, 0], m[:, :, 1]), 1)


class _RelativeLog(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r1_in, r2_in):
        dev = _require_device(r1_in, r2_in)
        r1 = _rotation_blocks(r1_in, "relative_rotation_vector")
        r2 = _rotation_blocks(r2_in, "relative_rotation_vector")
        if r1.shape != r2.shape:
            raise RuntimeError("relative_rotation_vector: batch sizes differ (%d, %d)" % (r1.shape[0], r2.shape[0]))
        b = r1.shape[0]
        v = torch.empty((b, 3), dtype=torch.float32, device=dev)
        _launch(dev, "so3_relative_log_fwd_f32", _ptr(r1), _ptr(r2), _ptr(v), b)
        ctx.save_for_backward(r1, r2)
        ctx.meta = (r1_in.dtype, r1_in.shape, r2_in.dtype, r2_in.shape)
        return v

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_v):
        r1, r2 = ctx.saved_tensors
        dev = r1.device
        g = grad_v.reshape(-1, 3).contiguous().float()
        d1 = torch.empty_like(r1) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(r2) if ctx.needs_input_grad[1] else None
        if d1 is None and d2 is None:
            return None, None
        _launch(dev, "so3_relative_log_bwd_f32", _ptr(r1), _ptr(r2), _ptr(g), _ptr(d1), _ptr(d2), r1.shape[0])
        dt1, sh1, dt2, sh2 = ctx.meta
        return _grad_to(d1, dt1, sh1), _grad_to(d2, dt2, sh2)


def relative_rotation_vector(R1: torch.Tensor, R2: torch.Tensor) -> torch.Tensor:
    """log(R1^T R2) as (B,3) float32 rotation vectors in one launch; the row norm is the geodesic angle between R1 and R2.
    Differentiable in both arguments with one backward launch (tangent-space gradients at R1 and at R2)."""
    return _RelativeLog.apply(R1, R2)


def _matrix_to_svd9(R: torch.Tensor) -> torch.Tensor:
    _require_device(R)
    _check_rotations(R, 'inverse_head_functions["SVD"]')
    return R.reshape(-1, 9).float()


# The inverse of every head: head_functions[key] (transform_output["3D"][1] for "3D") applied to inverse_head_functions[key](R) gives
# back R.  "5D" is deliberately absent: the head maps five numbers onto three degrees of freedom through a stereographic un-projection,
# and this package defines no canonical preimage for it (matrix_to_ortho6d gives the 6D one).
inverse_head_functions = {"SVD": _matrix_to_svd9, "6D": matrix_to_ortho6d, "Quat": matrix_to_quaternion, "quat": matrix_to_quaternion,
                          "Euler": matrix_to_euler, "3D": so3_log_map}


# --------------------------------------------------------------------------------------------
# the facade: the other families' public names, and the runtime's names that tests and tools read through this module
# --------------------------------------------------------------------------------------------
# Reading or mutating in place through these works as before; ASSIGNING to one here does not reach the functions that look the
# name up in their own module (patch _runtime._so3node, symmetry._capturing, ...).
from ._runtime import _STAT_WORKSPACES, _WARNED, _so3fast, _so3node  # noqa: E402,F401
from .symmetry import SymmetryTable, cyclic_symmetry, symmetric_angle_error, symmetric_loss_frobenius  # noqa: E402,F401
from .angle_statistics import STAT_FIELDS, angle_error_statistics  # noqa: E402,F401
from .clouds import (get_sampled_rotation_matrices_by_axisAngle, kabsch_rotation, kabsch_rotation_synthetic, pc_normalize,  # noqa: E402,F401
                     rigid_align, rotate_point_clouds, rotations_from_axis_angle_draws)
from .neighbors import (chamfer_distance, estimate_normals, fpfh_features, global_registration, icp_align, icp_align_plane,  # noqa: E402,F401
                        knn_gather, knn_group, knn_points, local_frames, match_features, nearest_neighbors, ransac_align)
from .pointnet import (farthest_point_sample, group_points, index_points, interpolate_features, propagate_features,  # noqa: E402,F401
                       query_ball_point, sample_and_group, sample_and_group_all, set_abstraction_group, set_abstraction_msg_group,
                       three_interpolate, three_nn)
from .pose_losses import (calculate_T_pred, cloud_diameter, compute_ADD_L1_loss, compute_ADD_loss, compute_ADD_S_loss,  # noqa: E402,F401
                          compute_disentangled_ADD_L1_loss, compute_MSSD, compute_symmetric_ADD_L1_loss, compute_symmetric_ADD_loss,
                          get_scene_parameters)
