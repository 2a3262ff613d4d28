"""Per-class evaluation statistics of the angle errors.  One family of the Python mirror; rotation_representation re-exports its
public names.  (Not called `statistics`: that is a module of the standard library.)"""
from __future__ import annotations

import torch

from ._runtime import _STAT_WORKSPACES, _capturing, _check, _libh, _on_device, _ptr, _require_device, _stream

# --------------------------------------------------------------------------------------------
# next row f3: per-class evaluation statistics
# --------------------------------------------------------------------------------------------
STAT_FIELDS = ("count", "mean", "std", "max", "median", "acc30", "acc15", "acc7.5")


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
