"""The runtime under every module of the Python mirror: the library handle, the two optional host-side helpers, the stream and the
device guard, the reduction workspaces and the zero pool, status checking, the once-per-process warnings, and the small tensor
preparers several families share.

All of the mirror's process-wide state lives here and nowhere else.  The dicts and sets (_FAST, _ROW_HEADS, _WORKSPACES,
_STAT_WORKSPACES, _WARNED, _ZERO_POOL.pools) are only ever mutated in place, so a name bound from this module elsewhere is the same
object; _L, _NODE_BOUND and _DEVICE_COUNT are rebound, and only by the functions of this module.  The family modules bind what they
use by name (`from ._runtime import _ptr, _stream, ...`): a call costs one global lookup, as it did when all of this was one file.
The optional-helper notices are printed by this module's import, once per process.
"""
from __future__ import annotations

import torch

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


def _no_double_backward(*grads) -> None:
    """torch's once_differentiable, at a fraction of its price (a no_grad context per call): these backward functions launch
    kernels autograd cannot see, so a backward whose result would have to be differentiated AGAIN must fail loudly.  That is
    once_differentiable's own condition -- grad mode on (create_graph=True) AND an incoming gradient that requires grad.
    create_graph=True alone (a gradient penalty on another branch of the graph) runs the kernels as always; nothing is recorded,
    the result is a constant."""
    if torch.is_grad_enabled() and any(g is not None and g.requires_grad for g in grads):
        raise RuntimeError("trying to differentiate twice a function that was marked with @once_differentiable "
                           "(poseestimation_amd kernels do not support double backward; the reference never uses it)")


_STAT_WORKSPACES = {}        # angle_error_statistics' workspaces by (device, stream); they live here because _check drops them


def _check(code: int, what: str) -> None:
    if code != 0:
        # a call that failed may have enqueued part of its launches: the cached workspaces (include/so3proj.h: "re-zero it after a
        # call that returned an error") are dropped, the next call zero-fills fresh ones
        _WORKSPACES.clear()
        _STAT_WORKSPACES.clear()
        _lib.check(code, what)


def _launch(dev: torch.device, name: str, *args) -> None:
    """The cold paths' launch: the C-ABI entry `name`, whose last parameter is the stream, called with (*args, dev's current stream)
    under the device guard, and its status checked.  The hot path of config #4 spells this out instead (it goes through _fn)."""
    with _on_device(dev):
        _check(getattr(_libh(), name)(*args, _stream(dev)), name)


def _grad_to(d, dtype, shape=None):
    """A kernel's gradient, or None, as backward returns it: in the argument's dtype and, where given, its shape."""
    if d is None:
        return None
    d = d.to(dtype)
    return d if shape is None else d.view(shape)


def _is_f64(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.dtype == torch.float64 for t in ts)


def _f64_blocks(t: torch.Tensor) -> torch.Tensor:
    m = _as_blocks(t)
    return m if m.dtype is torch.float64 else m.double()


_WARNED = set()


def _warn_once(key: str, message: str) -> None:
    """One warning per process and key: a metric that silently drops a gradient is how a training run goes wrong without an error."""
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(message, RuntimeWarning, stacklevel=3)


def _wants_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _cloud_lengths(op, error, name, lengths, b, full, dev):
    """The lengths of ragged clouds as the C ABI takes them: (B,) int32 clipped to [0, full], or None.  `op` raises `error`."""
    if lengths is None:
        return None
    _require_device(lengths)
    if lengths.device != dev or tuple(lengths.shape) != (b,) or lengths.dtype not in (torch.int32, torch.int64):
        raise error("%s: expected %s as a (B,) int32 or int64 tensor on %s for B = %d, got %s %s on %s"
                    % (op, name, dev, b, tuple(lengths.shape), lengths.dtype, lengths.device))
    return lengths.detach().clamp(0, full).to(torch.int32).contiguous()


def _cloud_f32(name, what, x, width=3):
    """A contiguous float32 copy (or the tensor itself) of a (B, N, 3) cloud on the device."""
    dev = _require_device(x)
    if x.dim() != 3 or x.shape[-1] != width or x.shape[1] < 1:
        raise RuntimeError("%s: expected %s of shape (B, N, %d) with N >= 1, got %s" % (name, what, width, tuple(x.shape)))
    return dev, x.detach().contiguous().float()
