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
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

_RANGE_MSG = "angle out of range, input probably not proper rotation matrices"   # rotation_representation.py:238-239


# --------------------------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------------------------
# The reference's real batch sizes are 64-512 (Iterative/main.py:216, UPNA/main.py:126, 3D-Pose/configs/example.yaml:3): the
# kernels then take 3-4 us and everything in this section is on the critical path.  Hence: the library handle and its entry
# points are looked up once, pointers and the stream travel as plain ints (ctypes converts them through the argtypes declared
# in _lib.py), the raw stream comes from torch's own accessor, and the device guard is a no-op on a one-GPU process.
_L = None


def _libh():
    global _L
    if _L is None:
        _L = _lib.load()
    return _L


def _optional_helper(name: str, without: str):
    """An optional host-side helper module of this package, or None -- with ONE warning on stderr saying what is lost: both
    helpers only remove host overhead (results are the same bits either way), so a missing one must not fail the import, but it
    must not go unnoticed either (_so3node is compiled against the build machine's torch; another torch on the box where it
    runs silently moved config #4's step from the C++ nodes to the Python classes in round 3)."""
    import importlib
    try:
        return importlib.import_module("." + name, __package__)
    except ImportError as exc:
        import sys
        print("[poseestimation_amd] optional helper %s is not available (%s): %s.  "
              "`python -m poseestimation_amd.build --force` rebuilds it." % (name, exc, without), file=sys.stderr)
        return None


# csrc/fastcall.c: METH_FASTCALL entry for the enqueue-only calls (ctypes: ~2.5 us per call)
_so3fast = _optional_helper("_so3fast", "every C-ABI call goes through ctypes, ~2.5 us per call slower")
_FAST = {}


def _fn(name: str):
    """The C-ABI entry point `name` as a callable taking plain ints / None (pointers, sizes, the stream) and returning the int
    status: through _so3fast when it is built, else the ctypes function (argtypes declared in _lib.py).  Integer arguments only."""
    f = _FAST.get(name)
    if f is None:
        cfn = getattr(_libh(), name)
        if _so3fast is not None:
            import ctypes
            import functools
            f = functools.partial(_so3fast.call, ctypes.cast(cfn, ctypes.c_void_p).value)
        else:
            f = cfn
        _FAST[name] = f
    return f


# csrc/autograd_node.cpp: the autograd nodes without the interpreter in forward / backward
_so3node = _optional_helper("_so3node", "the Python autograd.Function classes serve every case, ~10-25 us per training step slower at batch 512")
_NODE_BOUND = False


def _node():
    """_so3node with the C-ABI addresses handed over (once), or None."""
    global _NODE_BOUND
    if _so3node is not None and not _NODE_BOUND:
        import ctypes
        lib = _libh()
        addr = lambda name: ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
        _so3node.bind({name: addr(name) for name in (
            "so3_frob_fwd_bwd_v2_f32", "so3_frob_fwd_bwd_v2_bf16", "so3_scale_f32", "so3_scale_bf16", "so3_project_fwd_f32", "so3_project_fwd_bf16",
            "so3_project_bwd_f32", "so3_project_bwd_bf16", "so3_frob_loss_v2_f32", "so3_last_error")}, _SMALL_BATCH)
        _NODE_BOUND = True
    return _so3node


_ROW_HEADS = {}


def _row_head(symbol: str, width: int, x):
    """(..., width) -> (..., 3, 3) through the C++ node of the row-operation heads, or None when it (or its case) is not there."""
    node = _node()
    if node is None or type(x) is not torch.Tensor or not x.is_cuda:
        return None
    fns = _ROW_HEADS.get(symbol)
    if fns is None:
        import ctypes
        lib = _libh()
        fns = tuple(ctypes.cast(getattr(lib, "so3_%s_%s_f32" % (symbol, d)), ctypes.c_void_p).value for d in ("fwd", "bwd"))
        _ROW_HEADS[symbol] = fns
    return node.row_head(x, width, fns[0], fns[1], _stream(x.device))


def _require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(
                "poseestimation_amd runs on a HIP device only (tensor is on '%s'); there is no CPU "
                "fallback -- move the tensor to the MI355X with .cuda()" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} and {t.device}")
    return dev


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _NoGuard:
    __slots__ = ()

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()
_DEVICE_COUNT = None


def _on_device(dev: torch.device):
    """`with torch.cuda.device(dev)` only when dev is not already current (the context manager costs ~4 us per call)."""
    global _DEVICE_COUNT
    if _DEVICE_COUNT is None:
        _DEVICE_COUNT = torch.cuda.device_count()
    if _DEVICE_COUNT <= 1 or dev.index is None or dev.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev: torch.device) -> int:
    """The current stream of `dev` as the integer the C ABI takes (hipStream_t)."""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


_WORKSPACES = {}


def _workspace(dev: torch.device, stream: int):
    """The reduction workspace of (device, stream) -- include/so3proj.h: zero-filled once, then owned by that stream's calls.
    None while the stream is being captured into a graph (a replay may run beside eager calls: the no-workspace path then)."""
    if _capturing(dev):
        return None
    key = (dev.index, stream)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = torch.zeros((_libh().so3_reduce_workspace_bytes(),), dtype=torch.uint8, device=dev)
        _WORKSPACES[key] = ws
    return ws


def _capturing(dev: torch.device) -> bool:
    """Is the current stream OF `dev` being captured into a graph?  (torch's query looks at the current device.)"""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return torch.cuda.is_current_stream_capturing()
    with torch.cuda.device(dev):
        return torch.cuda.is_current_stream_capturing()


class _ZeroPool:
    """Zero-filled accumulator slots for the metric kernels (SO3_PREZEROED: sum_count[0] and the range flag must be 0 on entry):
    one torch.zeros per 256 calls instead of an init launch in front of every kernel.  A slot is handed out once; the tensors
    returned to the caller are views of it and keep their pool alive.
    One pool per (device, STREAM), like the reduction workspaces: the zero-fill is enqueued on the stream that was current when
    the pool was made, and a kernel on another stream could otherwise add into a slot before it has been zeroed -- or into a
    retired pool's block after the allocator handed it to someone else on the filling stream."""
    SLOTS = 256

    def __init__(self):
        self.pools = {}

    def take(self, dev: torch.device, stream: int):
        """(sum_count: 2 float64, flag: 1 int32), both zero, for a kernel enqueued on `stream` (the current stream of dev)."""
        if _capturing(dev):
            z = torch.zeros((1, 4), dtype=torch.float64, device=dev)               # a graph keeps its own (captured) zero-fill
            return z[0, :2], z[0, 2:3].view(torch.int32)[:1]
        key = (dev.index, stream)
        entry = self.pools.get(key)
        if entry is None or entry[1] >= self.SLOTS:
            with _on_device(dev):
                entry = [torch.zeros((self.SLOTS, 4), dtype=torch.float64, device=dev), 0]     # filled on `stream`: it is current
            self.pools[key] = entry
        row = entry[0][entry[1]]
        entry[1] += 1
        return row[:2], row[2:3].view(torch.int32)[:1]


_ZERO_POOL = _ZeroPool()
_SMALL_BATCH = 1024          # csrc: kSmallBatch -- up to here a reduction is one workgroup and needs no workspace


def _as_blocks(x: torch.Tensor) -> torch.Tensor:
    """x.view(-1, 3, 3) semantics (rotation_representation.py:199) -> contiguous (B, 9)."""
    if x.dim() == 2 and x.shape[1] == 9 and x.is_contiguous():
        return x
    if x.numel() % 9 != 0:
        raise RuntimeError(f"shape '[-1, 3, 3]' is invalid for input of size {x.numel()}")
    return x.reshape(-1, 9).contiguous()


def _head_input(x: torch.Tensor) -> torch.Tensor:
    """Kernel-ready (B,9) tensor: float32, bfloat16 kept as stored (math is fp32 in registers), or float64
    (its own float64 kernels, as the reference's function accepts double tensors)."""
    m = _as_blocks(x)
    dt = m.dtype
    if dt is torch.float32 or dt is torch.bfloat16 or dt is torch.float64:
        return m
    if dt is torch.float16:
        return m.float()
    raise TypeError(
        f"symmetric_orthogonalization: unsupported dtype {m.dtype} (inputs: float32, bfloat16, float16, float64)")


def _f32_blocks(t: torch.Tensor) -> torch.Tensor:
    m = _as_blocks(t)
    return m if m.dtype is torch.float32 else m.float()


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


def _no_double_backward(*grads) -> None:
    """torch's once_differentiable, at a fraction of its price (a no_grad context per call): these backward functions launch
    kernels autograd cannot see, so a backward whose result would have to be differentiated AGAIN must fail loudly.  That is
    once_differentiable's own condition -- grad mode on (create_graph=True) AND an incoming gradient that requires grad.
    create_graph=True alone (a gradient penalty on another branch of the graph) runs the kernels as always; nothing is recorded,
    the result is a constant."""
    if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in grads):
        raise RuntimeError("trying to differentiate twice a function that was marked with @once_differentiable "
                           "(poseestimation_amd kernels do not support double backward; the reference never uses it)")


def _check(code: int, what: str) -> None:
    if code != 0:
        # a call that failed may have enqueued part of its launches: the cached workspaces (include/so3proj.h: "re-zero it after a
        # call that returned an error") are dropped, the next call zero-fills fresh ones
        _WORKSPACES.clear()
        _STAT_WORKSPACES.clear()
        _lib.check(code, what)


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


def _is_f64(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in ts)


def _f64_blocks(t: torch.Tensor) -> torch.Tensor:
    m = _as_blocks(t)
    return m if m.dtype is torch.float64 else m.double()


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


_WARNED = set()


def _warn_once(key: str, message: str) -> None:
    """One warning per process and key: a metric that silently drops a gradient is how a training run goes wrong without an error."""
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(message, RuntimeWarning, stacklevel=3)


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


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
        with _on_device(dev):
            if data64:
                _check(_libh().so3_angle_bwd_f64(a.data_ptr(), b_.data_ptr(), g.data_ptr(), divisor, eps, flags, _ptr(d1), _ptr(d2), n, _stream(dev)),
                       "so3_angle_bwd_f64")
            else:
                _check(_libh().so3_angle_bwd_f32(a.data_ptr(), b_.data_ptr(), g.data_ptr(), divisor, eps, flags | (_lib.F64_MATH if f64_math else 0),
                                                 _ptr(d1), _ptr(d2), n, _stream(dev)), "so3_angle_bwd_f32")
    if d1 is not None:
        d1 = (d1 if d1.dtype is dtype1 else d1.to(dtype1)).view(shape1)
    if d2 is not None:
        d2 = (d2 if d2.dtype is dtype2 else d2.to(dtype2)).view(shape2)
    return d1, d2


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
    with _on_device(dev):
        _check(_libh().so3_geodesic_f32(_ptr(a), _ptr(b_), _ptr(theta), n, _stream(dev)), "so3_geodesic_f32")
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
    cls = None
    if table.num_classes > 1:
        if class_ids is None:
            raise ValueError(f"{what}: a table of {table.num_classes} classes needs class_ids")
        _require_device(R_pred, class_ids)
        if class_ids.dtype not in (torch.int32, torch.int64) or class_ids.dim() != 1 or class_ids.shape[0] != n:
            raise ValueError(f"{what}: class_ids must be int32 or int64 of shape ({n},), got {class_ids.dtype} {tuple(class_ids.shape)}")
        if class_ids.dtype is torch.int64:            # out-of-range ids stay out of range in int32
            class_ids = class_ids.clamp(-1, table.num_classes).int()
        cls = class_ids.contiguous()
    elif class_ids is not None:
        raise ValueError(f"{what}: class_ids given for a single-class table")
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
        with _on_device(dev):
            _check(_libh().so3_sym_angle_error_f32(p.data_ptr(), t.data_ptr(), s.data_ptr(), _ptr(cls), table.num_classes, table.K,
                                                   deg.data_ptr(), _ptr(idx), _ptr(flag), 0, n, _stream(dev)), "so3_sym_angle_error_f32")
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
    with _on_device(dev):
        _check(_libh().so3_kabsch_f32(_ptr(p), _ptr(q), _ptr(r), _ptr(h), b, n, _stream(dev)), "so3_kabsch_f32")
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
        with _on_device(dev):
            _check(_libh().so3_kabsch_bwd_f32(_ptr(p), _ptr(q), _ptr(h), _ptr(gr), _ptr(gh), _ptr(dp), _ptr(dq), b, n, _stream(dev)),
                   "so3_kabsch_bwd_f32")
        if dp is not None:
            dp = (dp if dtype_p is torch.float32 else dp.to(dtype_p)).view(shape_p)
        if dq is not None:
            dq = (dq if dtype_q is torch.float32 else dq.to(dtype_q)).view(shape_q)
        return dp, dq, None


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
    with _on_device(dev):
        _check(_libh().so3_rigid_align_f32(_ptr(p), _ptr(q), _ptr(w), _ptr(r), _ptr(t), _ptr(h), _ptr(stats), b, n, _stream(dev)),
               "so3_rigid_align_f32")
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
        with _on_device(dev):
            _check(_libh().so3_rigid_align_bwd_f32(_ptr(p), _ptr(q), _ptr(w), _ptr(h), _ptr(r), _ptr(stats), _ptr(gr), _ptr(gt), _ptr(gh),
                                                   _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), b, n, _stream(dev)), "so3_rigid_align_bwd_f32")
        for i, d in enumerate(outs):
            if d is not None:
                shape, dtype = ctx.meta[i]
                outs[i] = (d if dtype is torch.float32 else d.to(dtype)).view(shape)
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
# nearest neighbours between two clouds, and ICP on top of them
# --------------------------------------------------------------------------------------------
def _cloud_pair(name, X, Y):
    """float32 copies of a source (B,N,3) and a target (B,M,3) or shared (M,3), and the target's stride in floats (0: shared)."""
    dev = _require_device(X, Y)
    ok = X.dim() == 3 and X.shape[-1] == 3 and Y.dim() in (2, 3) and Y.shape[-1] == 3 and (Y.dim() == 2 or Y.shape[0] == X.shape[0])
    if not ok or not 1 <= X.shape[1] <= _lib.ADD_S_MAX_N or not 1 <= Y.shape[-2] <= _lib.ADD_S_MAX_N:
        raise RuntimeError("%s: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= %d, got %s and %s"
                           % (name, _lib.ADD_S_MAX_N, tuple(X.shape), tuple(Y.shape)))
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
    with _on_device(dev):
        _check(_libh().so3_nearest_f32(_ptr(x), _ptr(y), stride, _ptr(dist), _ptr(idx), b, n, m, _stream(dev)), "so3_nearest_f32")
    return dist, idx.long()


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
    if (R_init is not None and tuple(R_init.shape) != (b, 3, 3)) or (t_init is not None and tuple(t_init.shape) != (b, 3)) or \
            (weights is not None and tuple(weights.shape) != (b, n)):
        raise RuntimeError("icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = %d, N = %d, got %s"
                           % (b, n, [None if x is None else tuple(x.shape) for x in (R_init, t_init, weights)]))
    if _wants_grad(P, Q, R_init, t_init, weights):
        _warn_once("icp_align", "icp_align is not differentiable: R and t carry no gradient although an argument requires grad.  Call "
                                "rigid_align on the returned correspondences (see the docstring) for a differentiable last step.")
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
    lib = _libh()
    work = torch.empty((max(int(lib.so3_icp_workspace_bytes(b, n)) // 4, 1),), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(lib.so3_icp_f32(_ptr(p), _ptr(q), stride, _ptr(w), _ptr(t0), -1.0 if max_distance is None else float(max_distance), iterations,
                               _ptr(r), _ptr(t), _ptr(rmse), _ptr(inl), _ptr(nearest), _ptr(dist), _ptr(work), b, n, m, _stream(dev)),
               "so3_icp_f32")
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
    if (R_init is not None and tuple(R_init.shape) != (b, 3, 3)) or (t_init is not None and tuple(t_init.shape) != (b, 3)) or \
            (weights is not None and tuple(weights.shape) != (b, n)):
        raise RuntimeError("icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = %d, N = %d, got %s"
                           % (b, n, [None if x is None else tuple(x.shape) for x in (R_init, t_init, weights)]))
    if _wants_grad(P, Q, normals, R_init, t_init, weights):
        _warn_once("icp_align_plane", "icp_align_plane is not differentiable: R and t carry no gradient although an argument requires grad.  "
                                      "Call rigid_align on the returned correspondences (see icp_align's docstring) for a differentiable last step.")
    if normals is None:
        nrm = estimate_normals(q if q.dim() == 3 else q[None], int(normal_neighbors))
        nrm = (nrm if q.dim() == 3 else nrm[0]).contiguous()
    else:
        nrm = normals.detach().contiguous().float()
    t0 = None
    if R_init is not None or t_init is not None:
        r0 = R_init.detach().float() if R_init is not None else torch.eye(3, dtype=torch.float32, device=dev).expand(b, 3, 3)
        tt = t_init.detach().float() if t_init is not None else torch.zeros((b, 3), dtype=torch.float32, device=dev)
        t0 = torch.cat([r0, tt[:, :, None]], 2).contiguous()                       # (B, 3, 4): the rows (R | t)
    w = None if weights is None else weights.detach().contiguous().float()
    r = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    rmse = rmse_point = inl = solved = nearest = dist = None
    if return_info:
        rmse = torch.empty((iterations, b), dtype=torch.float32, device=dev)
        rmse_point = torch.empty((iterations, b), dtype=torch.float32, device=dev)
        inl = torch.empty((iterations, b), dtype=torch.int32, device=dev)
        solved = torch.empty((iterations, b), dtype=torch.int32, device=dev)
        nearest = torch.empty((b, n), dtype=torch.int32, device=dev)
        dist = torch.empty((b, n), dtype=torch.float32, device=dev)
    lib = _libh()
    work = torch.empty((max(int(lib.so3_icp_plane_workspace_bytes(b, n)) // 4, 1),), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(lib.so3_icp_plane_f32(_ptr(p), _ptr(q), _ptr(nrm), stride, _ptr(w), _ptr(t0), -1.0 if max_distance is None else float(max_distance),
                                     damping, iterations, _ptr(r), _ptr(t), _ptr(rmse), _ptr(rmse_point), _ptr(inl), _ptr(solved), _ptr(nearest),
                                     _ptr(dist), _ptr(work), b, n, m, _stream(dev)), "so3_icp_plane_f32")
    if return_info:
        return r, t, {"rmse": rmse, "rmse_point": rmse_point, "inliers": inl.long(), "solved": solved.bool(), "nearest": nearest.long(), "dist": dist}
    return r, t


# --------------------------------------------------------------------------------------------
# the Chamfer distance: a loss between two clouds, differentiable in both
# --------------------------------------------------------------------------------------------
def _cloud_lengths(op, error, name, lengths, b, full, dev):
    """The lengths of ragged clouds as the C ABI takes them: (B,) int32 clipped to [0, full], or None.  `op` raises `error`."""
    if lengths is None:
        return None
    _require_device(lengths)
    if lengths.device != dev or tuple(lengths.shape) != (b,) or lengths.dtype not in (torch.int32, torch.int64):
        raise error("%s: expected %s as a (B,) int32 or int64 tensor on %s for B = %d, got %s %s on %s"
                    % (op, name, dev, b, tuple(lengths.shape), lengths.dtype, lengths.device))
    return lengths.detach().clamp(0, full).to(torch.int32).contiguous()


class _Chamfer(torch.autograd.Function):
    """chamfer_distance: so3_chamfer_fwd_f32 searches both directions and leaves the (B,2) means; the reductions over them are a few
    (B,)-sized torch statements.  The backward folds the upstream gradient and those reductions into per-cloud scales on the device
    and makes one so3_chamfer_bwd_f32 call through the stored indices."""

    @staticmethod
    def forward(ctx, X, Y, x_lengths, y_lengths, squared, point_reduction, batch_reduction, single, return_nearest):
        dev = _require_device(X, Y)
        ok = X.dim() == 3 and X.shape[-1] == 3 and Y.dim() == 3 and Y.shape[-1] == 3 and Y.shape[0] == X.shape[0]
        if not ok or not 1 <= X.shape[1] <= _lib.ADD_S_MAX_N or not 1 <= Y.shape[1] <= _lib.ADD_S_MAX_N:
            raise RuntimeError("chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= %d, got %s and %s"
                               % (_lib.ADD_S_MAX_N, tuple(X.shape), tuple(Y.shape)))
        x, y = X.detach().contiguous().float(), Y.detach().contiguous().float()
        b, n, m = x.shape[0], x.shape[1], y.shape[1]
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
        lib = _libh()
        work = torch.empty((max(int(lib.so3_chamfer_workspace_bytes(b, n, m)) // 4, 1),), dtype=torch.float32, device=dev)
        with _on_device(dev):
            _check(lib.so3_chamfer_fwd_f32(_ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(dist_x), _ptr(near_x), _ptr(dist_y), _ptr(near_y), _ptr(rows),
                                           _ptr(work), flags, b, n, m, _stream(dev)), "so3_chamfer_fwd_f32")
        cham_x, cham_y = rows[:, 0], rows[:, 1]
        if point_reduction == "sum":                       # rows holds the means
            cham_x = cham_x * (float(n) if nx is None else nx)
            cham_y = cham_y * (float(m) if ny is None else ny)
        per_cloud = cham_x if single else cham_x + cham_y
        out = per_cloud.mean() if batch_reduction == "mean" else (per_cloud.sum() if batch_reduction == "sum" else per_cloud.contiguous())
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
        single = bool(flags & _lib.CHAMFER_SINGLE)
        scale_x = scale_x.contiguous()
        scale_y = None if single else scale_y.contiguous()
        dx = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if want_x else None
        dy = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if want_y else None
        with _on_device(dev):
            _check(_libh().so3_chamfer_bwd_f32(_ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(near_x), _ptr(near_y), _ptr(scale_x), _ptr(scale_y),
                                               _ptr(dx), _ptr(dy), flags, b, n, m, _stream(dev)), "so3_chamfer_bwd_f32")
        return (None if dx is None else dx.to(x_dtype), None if dy is None else dy.to(y_dtype)) + (None,) * 7


def chamfer_distance(X: torch.Tensor, Y: torch.Tensor, x_lengths: torch.Tensor = None, y_lengths: torch.Tensor = None, squared: bool = True,
                     point_reduction: str = "mean", batch_reduction: str = "mean", single_directional: bool = False,
                     return_nearest: bool = False):
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
    and info["dist_x"], info["dist_y"] float32, the per-point terms (0 in those slots); single_directional leaves the y entries out."""
    if point_reduction not in ("mean", "sum") or batch_reduction not in ("mean", "sum", None):
        raise ValueError("chamfer_distance: point_reduction is 'mean' or 'sum' and batch_reduction 'mean', 'sum' or None, got %r and %r"
                         % (point_reduction, batch_reduction))
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
        dev = _require_device(X, Y)
        ok = X.dim() == 3 and X.shape[-1] == 3 and Y.dim() in (2, 3) and Y.shape[-1] == 3 and (Y.dim() == 2 or Y.shape[0] == X.shape[0])
        if not ok or not 1 <= X.shape[1] <= _lib.ADD_S_MAX_N or not 1 <= Y.shape[-2] <= _lib.ADD_S_MAX_N:
            raise ValueError("knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= %d, got %s and %s"
                             % (_lib.ADD_S_MAX_N, tuple(X.shape), tuple(Y.shape)))
        shared = Y.dim() == 2
        if shared and ctx.needs_input_grad[1]:
            raise ValueError("knn_points: a shared (M, 3) target takes no gradient; pass Y.expand(B, M, 3) to differentiate in it")
        x, y = X.detach().contiguous().float(), Y.detach().contiguous().float()
        b, n, m = x.shape[0], x.shape[1], y.shape[-2]
        xl = _cloud_lengths("knn_points", ValueError, "x_lengths", x_lengths, b, n, dev)
        yl = _cloud_lengths("knn_points", ValueError, "y_lengths", y_lengths, b, m, dev)
        dist2 = torch.empty((b, n, k), dtype=torch.float32, device=dev)
        idx = torch.empty((b, n, k), dtype=torch.int32, device=dev)
        with _on_device(dev):
            _check(_libh().so3_knn_f32(_ptr(x), _ptr(y), 0 if shared else 3 * m, _ptr(xl), _ptr(yl), _ptr(dist2), _ptr(idx), k, b, n, m, _stream(dev)),
                   "so3_knn_f32")
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
        with _on_device(dev):
            _check(_libh().so3_knn_bwd_f32(_ptr(x), _ptr(y), _ptr(xl), _ptr(yl), _ptr(idx), _ptr(g), _ptr(dx), _ptr(dy), k, b, n, m, _stream(dev)),
                   "so3_knn_bwd_f32")
        return None if dx is None else dx.to(x_dtype), None if dy is None else dy.to(y_dtype), None, None, None


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
    with _on_device(dev):
        _check(_libh().so3_local_frames_f32(_ptr(y), 0 if points.dim() == 2 else 3 * m, _ptr(ix), _ptr(xl), _ptr(yl), _ptr(viewpoint),
                                            *(_ptr(o) for o in outs), k, b, n, m, _stream(dev)), "so3_local_frames_f32")
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
# PointNet++ sampling and grouping (reference: point_cloud/pointnet_utils.py)
# --------------------------------------------------------------------------------------------
def _cloud_f32(name, what, x, width=3):
    """A contiguous float32 copy (or the tensor itself) of a (B, N, 3) cloud on the device."""
    dev = _require_device(x)
    if x.dim() != 3 or x.shape[-1] != width or x.shape[1] < 1:
        raise RuntimeError("%s: expected %s of shape (B, N, %d) with N >= 1, got %s" % (name, what, width, tuple(x.shape)))
    return dev, x.detach().contiguous().float()


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
    with _on_device(dev):
        _check(_libh().so3_fps_f32(_ptr(x), _ptr(first), _ptr(out), b, n, npoint, _stream(dev)), "so3_fps_f32")
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
    with _on_device(dev):
        _check(_libh().so3_ball_query_f32(_ptr(x), _ptr(c), float(radius), min(nsample, 2**31 - 1), _ptr(idx), _ptr(count), b, n, s, _stream(dev)),
               "so3_ball_query_f32")
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
        with _on_device(dev):
            _check(_libh().so3_group_points_f32(_ptr(x), _ptr(c), _ptr(f), _ptr(idx32), _ptr(out), ff, cf, b, n, s, k, d, _stream(dev)),
                   "so3_group_points_f32")
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
        with _on_device(dev):
            _check(_libh().so3_group_points_bwd_f32(_ptr(g), _ptr(idx32), _ptr(gx), _ptr(gc), _ptr(gf), ff, cf, b, n, s, k, d, _stream(dev)),
                   "so3_group_points_bwd_f32")
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
    with _on_device(dev):
        _check(_libh().so3_three_nn_f32(_ptr(x), _ptr(y), _ptr(dist2), _ptr(idx), _ptr(weight), b, n, s, _stream(dev)), "so3_three_nn_f32")
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
        with _on_device(dev):
            _check(_libh().so3_three_interpolate_f32(_ptr(f), _ptr(idx32), _ptr(w32), _ptr(out), 1 if channels_first else 0, b, n, s, d, _stream(dev)),
                   "so3_three_interpolate_f32")
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
        with _on_device(dev):
            _check(_libh().so3_three_interpolate_bwd_f32(_ptr(g), _ptr(idx32), _ptr(w32), _ptr(grad), 1 if channels_first else 0, b, n, s, d,
                                                         _stream(dev)), "so3_three_interpolate_bwd_f32")
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
    with _on_device(dev):
        _check(_libh().so3_rotate_clouds_f32(_ptr(p), _ptr(r), _ptr(out), 1 if transposed else 0, b, n, _stream(dev)), "so3_rotate_clouds_f32")
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
        with _on_device(dev):
            _check(_libh().so3_rotate_clouds_bwd_f32(_ptr(p), _ptr(r), _ptr(g), _ptr(dp), _ptr(dr), 1 if transposed else 0, b, n, _stream(dev)),
                   "so3_rotate_clouds_bwd_f32")
        if dp is not None:
            dp = (dp if dtype_p is torch.float32 else dp.to(dtype_p)).view(shape_p)
        if dr is not None:
            dr = (dr if dtype_r is torch.float32 else dr.to(dtype_r)).view(shape_r)
        return dp, dr, None


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
    with _on_device(dev):
        _check(_libh().so3_pc_normalize_f32(_ptr(p), _ptr(out), _ptr(cen), _ptr(sc), b, n, _stream(dev)), "so3_pc_normalize_f32")
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
    with _on_device(dev):
        _check(_libh().so3_rotations_axis_angle_f32(_ptr(t), _ptr(a), _ptr(r), t.shape[0], _stream(dev)), "so3_rotations_axis_angle_f32")
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
    with _on_device(dev):
        _check(_libh().so3_kabsch_synth_f32(_ptr(p), _ptr(g), float(sigma), int(seed) & 0xFFFFFFFF, _ptr(r), _ptr(h), b, n, _stream(dev)),
                   "so3_kabsch_synth_f32")
    return (r, h) if return_h else r


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
        with _on_device(dev):
            _check(_libh().so3_se3_update_f32(_ptr(o), _ptr(t), _ptr(tp), fx, fy, b, _stream(dev)), "so3_se3_update_f32")
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
        with _on_device(dev):
            _check(_libh().so3_se3_update_bwd_f32(_ptr(o), _ptr(t), _ptr(g), _ptr(d), fx, fy, o.shape[0], _stream(dev)), "so3_se3_update_bwd_f32")
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


class _AddL1(torch.autograd.Function):
    """compute_ADD_L1_loss and its gradient w.r.t. the predicted pose, one launch (so3_add_l1_f32)."""

    @staticmethod
    def forward(ctx, t_gt, t_pred, points, use_batch_mean):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        want_grad = t_pred.requires_grad
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if want_grad else None
        dists = None if use_batch_mean else torch.empty((b,), dtype=torch.float32, device=dev)
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if use_batch_mean else None
        scale = 1.0 / max(b, 1) if use_batch_mean else 1.0
        with _on_device(dev):
            _check(_libh().so3_add_l1_f32(_ptr(tg), _ptr(tp), _ptr(pts), _ptr(dists), _ptr(loss_sum), _ptr(dt), scale, b, n,
                                                  _stream(dev)), "so3_add_l1_f32")
        ctx.dt, ctx.per_sample, ctx.in_dtype = dt, not use_batch_mean, t_pred.dtype
        if use_batch_mean:
            return loss_sum.to(torch.float32).mul_(1.0 / max(b, 1)).squeeze(0)
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.dt is None:
            return None, None, None, None
        g = grad_out.reshape(-1, 1, 1) if ctx.per_sample else grad_out
        return None, (ctx.dt * g).to(ctx.in_dtype), None, None


class _AddL1Disentangled(torch.autograd.Function):
    """compute_disentangled_ADD_L1_loss and its gradient, one launch (so3_add_l1_disentangled_f32)."""

    @staticmethod
    def forward(ctx, t_pred, t_gt, points):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if t_pred.requires_grad else None
        loss_sum = torch.empty((3,), dtype=torch.float64, device=dev)
        with _on_device(dev):
            _check(_libh().so3_add_l1_disentangled_f32(_ptr(tp), _ptr(tg), _ptr(pts), _ptr(loss_sum), _ptr(dt), 1.0 / max(b, 1),
                                                               b, n, _stream(dev)), "so3_add_l1_disentangled_f32")
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
    return _AddL1.apply(TCO_gt, TCO_pred, points, bool(use_batch_mean))


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


class _AddL2(torch.autograd.Function):
    """compute_ADD_loss and its gradient w.r.t. the predicted pose, one launch (so3_add_l2_f32)."""

    @staticmethod
    def forward(ctx, t_gt, t_pred, points, use_batch_mean):
        dev, b, n, tg, tp, pts = _add_l1_args(t_gt, t_pred, points)
        want_grad = t_pred.requires_grad
        dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if want_grad else None
        dists = None if use_batch_mean else torch.empty((b,), dtype=torch.float32, device=dev)
        loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if use_batch_mean else None
        scale = 1.0 / max(b, 1) if use_batch_mean else 1.0
        with _on_device(dev):
            _check(_libh().so3_add_l2_f32(_ptr(tg), _ptr(tp), _ptr(pts), _ptr(dists), _ptr(loss_sum), _ptr(dt), scale, b, n,
                                          _stream(dev)), "so3_add_l2_f32")
        ctx.dt, ctx.per_sample, ctx.in_dtype = dt, not use_batch_mean, t_pred.dtype
        if use_batch_mean:
            return loss_sum.to(torch.float32).mul_(1.0 / max(b, 1)).squeeze(0)
        return dists

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if ctx.dt is None:
            return None, None, None, None
        g = grad_out.reshape(-1, 1, 1) if ctx.per_sample else grad_out
        return None, (ctx.dt * g).to(ctx.in_dtype), None, None


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
        with _on_device(dev):
            _check(_libh().so3_add_s_fwd_f32(_ptr(tg), _ptr(tp), _ptr(pts), _ptr(point_dist), _ptr(nearest), _ptr(dists), _ptr(loss_sum),
                                             b, n, _stream(dev)), "so3_add_s_fwd_f32")
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
        with _on_device(dev):
            _check(_libh().so3_add_s_bwd_f32(_ptr(tg), _ptr(tp), _ptr(pts), _ptr(nearest), _ptr(rows), 1.0, _ptr(dt), b, n,
                                             _stream(dev)), "so3_add_s_bwd_f32")
        return None, dt.to(in_dtype), None, None, None


def compute_ADD_loss(TCO_gt: torch.Tensor, TCO_pred: torch.Tensor, points: torch.Tensor, use_batch_mean: bool = True) -> torch.Tensor:
    """The ADD metric: mean over the model points of |T_gt p - T_pred p|_2 (and over the batch; use_batch_mean=False gives (B,)).
    points: (B,N,3), or (N,3) for one model shared by the batch.  Differentiable w.r.t. TCO_pred."""
    points = _add_metric_points("compute_ADD_loss", TCO_gt, points)
    return _AddL2.apply(TCO_gt, TCO_pred, points, bool(use_batch_mean))


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
    with _on_device(dev):
        _check(_libh().so3_cloud_diameter_f32(_ptr(p), _ptr(work), _ptr(diam), b, n, _stream(dev)), "so3_cloud_diameter_f32")
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
    cls = None
    if table.num_classes > 1:
        if class_ids is None:
            raise ValueError(f"{what}: a table of {table.num_classes} classes needs class_ids")
        _require_device(t_pred, class_ids)
        if class_ids.dtype not in (torch.int32, torch.int64) or class_ids.dim() != 1 or class_ids.shape[0] != b:
            raise ValueError(f"{what}: class_ids must be int32 or int64 of shape ({b},), got {class_ids.dtype} {tuple(class_ids.shape)}")
        if class_ids.dtype is torch.int64:            # out-of-range ids stay out of range in int32
            class_ids = class_ids.clamp(-1, table.num_classes).int()
        cls = class_ids.contiguous()
    elif class_ids is not None:
        raise ValueError(f"{what}: class_ids given for a single-class table")
    s = table._on(dev)
    rows = torch.empty((b,), dtype=torch.float32, device=dev) if (want_rows or want_sum) else None
    loss_sum = torch.empty((1,), dtype=torch.float64, device=dev) if want_sum else None
    idx = torch.empty((b,), dtype=torch.int32, device=dev) if want_index else None
    dt = torch.empty((b, 4, 4), dtype=torch.float32, device=dev) if want_grad else None
    with _on_device(dev):
        _check(_libh().so3_sym_add_f32(_ptr(tg), _ptr(tp), _ptr(pts), _ptr(s), _ptr(cls), table.num_classes, table.K, _ptr(rows), _ptr(idx),
                                       _ptr(loss_sum), _ptr(dt), scale, mode, b, n, _stream(dev)), "so3_sym_add_f32")
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


# --------------------------------------------------------------------------------------------
# next row f3: per-class evaluation statistics
# --------------------------------------------------------------------------------------------
STAT_FIELDS = ("count", "mean", "std", "max", "median", "acc30", "acc15", "acc7.5")
_STAT_WORKSPACES = {}


def angle_error_statistics(angles: torch.Tensor, class_ids: torch.Tensor = None, num_classes: int = 1) -> dict:
    """Device-side replacement of the numpy block in 3D-Pose/test_per_class.py:174-216.

    angles: (B,) degrees (e.g. `angle_error(...)`), not negative (-0.0 counts as +0.0; negative angles are outside the contract);
    class_ids: optional (B,) integer ids in [0, num_classes) -- rows with other ids, int64 ids beyond int32 included, are ignored.
    Returns {"count","mean","std","max","median","acc30","acc15","acc7.5"} -> (num_classes,) float64 tensors;
    median is exact (radix select), std is numpy's population std by the one-pass formula (include/so3proj.h bounds its error: on a
    distribution much narrower than its mean no digit of it need be right), acc* are (x < t).sum()/len(x).
    As numpy: an empty class has count 0 and NaN elsewhere; a class holding a NaN has NaN for mean, std, max and median; a class
    holding +inf has mean = max = +inf and std = NaN."""
    dev = _require_device(angles)
    a = angles.detach().reshape(-1).contiguous().double()
    c = None
    if class_ids is not None:
        _require_device(class_ids)
        c = class_ids.detach().reshape(-1)
        if c.dtype is torch.int64:                    # out-of-range ids stay out of range in int32
            c = c.clamp(-1, num_classes)
        c = c.contiguous().to(torch.int32)
        if c.numel() != a.numel():
            raise RuntimeError("angle_error_statistics: angles and class_ids differ in length")
    lib = _libh()
    stats = torch.empty((num_classes, len(STAT_FIELDS)), dtype=torch.float64, device=dev)
    with _on_device(dev):
        st = _stream(dev)
        # the statistics' workspace of (device, stream): zero-filled once, every call leaves it usable (include/so3proj.h) -- 10 MB kept
        # per stream that ever asked; a fresh zero-filled one while the stream is being captured (a replay may run beside eager calls)
        key = (dev.index, st)
        work = None if _capturing(dev) else _STAT_WORKSPACES.get(key)
        if work is None:
            work = torch.zeros((lib.so3_angle_stats_workspace_bytes(),), dtype=torch.uint8, device=dev)
            if not _capturing(dev):
                _STAT_WORKSPACES[key] = work
        code = lib.so3_angle_stats(_ptr(a), _ptr(c), num_classes, _ptr(stats), _ptr(work), a.numel(), st)
        if code != 0:
            # include/so3proj.h: a workspace is to be re-zeroed after a call that returned an error -- a refused call may have
            # enqueued its first launch: the cached one is dropped, the next call starts from a fresh zero-filled one
            _STAT_WORKSPACES.pop(key, None)
            _check(code, "so3_angle_stats")
    return {name: stats[:, i] for i, name in enumerate(STAT_FIELDS)}


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
        with _on_device(dev):
            _check(_libh().so3_ortho6d_fwd_f32(_ptr(x), _ptr(r), b, _stream(dev)), "so3_ortho6d_fwd_f32")
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
        with _on_device(dev):
            _check(_libh().so3_ortho6d_bwd_f32(_ptr(x), _ptr(g), _ptr(dx), x.shape[0], _stream(dev)), "so3_ortho6d_bwd_f32")
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
            with _on_device(dev):
                _check(getattr(_lib.load(), "so3_%s_fwd_f32" % symbol)(_ptr(x), _ptr(r), b, _stream(dev)), "so3_%s_fwd_f32" % symbol)
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
            with _on_device(dev):
                _check(getattr(_lib.load(), "so3_%s_bwd_f32" % symbol)(_ptr(x), _ptr(g), _ptr(dx), x.shape[0], _stream(dev)), "so3_%s_bwd_f32" % symbol)
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
            with _on_device(dev):
                _check(getattr(_lib.load(), "so3_%s_fwd_f32" % symbol)(_ptr(r), _ptr(y), b, _stream(dev)), "so3_%s_fwd_f32" % symbol)
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
            with _on_device(dev):
                _check(getattr(_lib.load(), "so3_%s_bwd_f32" % symbol)(_ptr(r), _ptr(g), _ptr(dr), r.shape[0], _stream(dev)), "so3_%s_bwd_f32" % symbol)
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
    a float32 r1 has rounded to +-1.  At exact gimbal lock e1 = 0.
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
        with _on_device(dev):
            _check(_lib.load().so3_relative_log_fwd_f32(_ptr(r1), _ptr(r2), _ptr(v), b, _stream(dev)), "so3_relative_log_fwd_f32")
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
        with _on_device(dev):
            _check(_lib.load().so3_relative_log_bwd_f32(_ptr(r1), _ptr(r2), _ptr(g), _ptr(d1), _ptr(d2), r1.shape[0], _stream(dev)),
                   "so3_relative_log_bwd_f32")
        dt1, sh1, dt2, sh2 = ctx.meta
        return (d1.to(dt1).view(sh1) if d1 is not None else None, d2.to(dt2).view(sh2) if d2 is not None else None)


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
