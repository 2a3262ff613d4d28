"""Shared by tests/test_pointnet_host.py, tests/test_gpu_pointnet.py and tools/gen_golden.py (G22): farthest-point sampling and ball
query restated in numpy from their DEFINITION (include/so3proj.h), and the fixture's layout.

    d(j, c) = ((dx * dx) + (dy * dy)) + (dz * dz),  dx = x_j - c_x, ...: float32 arrays, so numpy rounds every operation on its own
    fps:   dist = 1e10;  out[0] = start;  repeat:  dist = where(d(., centre) < dist, d, dist);  next = the FIRST argmax of dist
    ball:  member_j = not (d(j, c) > r * r), the product rounded to float32;  the first `width` = min(nsample, N) members in
           ascending j, the rest of the row repeats the first member, a row without a member holds N;  count = the members, unclipped
The float32 sequence is exact: the kernels and the host model must reproduce it bit for bit.  dtype=np.float64 evaluates the same
expressions in float64 (the float32 inputs widened): the answer the fixture's near_boundary mask is measured against."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_pointnet.npz")
FPS_INIT = np.float32(1e10)
FPS_MAX_N = 16384
BOUNDARY_REL = 1e-5                  # near_boundary: some j with | |c - x_j|^2 - r^2 | <= BOUNDARY_REL * r^2 in float64
BOUNDARY_CAP = 0.01                  # at most this share of a case's rows may be near the boundary
FPS_CASES = ((2, 1024, 512), (2, 512, 128), (3, 300, 77))                      # (B, N, npoint)
BALL_CASES = ((1024, 512, 0.1, 32), (1024, 512, 0.2, 64), (512, 128, 0.4, 64), (512, 128, 0.8, 128))      # (N, S, radius, nsample): the reference model's


def dist2(xyz, c, dtype=np.float32):
    """xyz (..., N, 3), c (..., 3) -> (..., N): the defined distance of every point to the centre."""
    x, c = np.asarray(xyz, dtype), np.asarray(c, dtype)[..., None, :]
    dx, dy, dz = x[..., 0] - c[..., 0], x[..., 1] - c[..., 1], x[..., 2] - c[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def fps(xyz, npoint, start):
    """xyz (B, N, 3) float32, start (B,) or an int -> (B, npoint) int64."""
    xyz = np.asarray(xyz, np.float32)
    b, n, _ = xyz.shape
    cur = np.broadcast_to(np.asarray(start, np.int64), (b,)).copy()
    assert (cur >= 0).all() and (cur < n).all()
    dist = np.full((b, n), FPS_INIT, np.float32)
    out = np.zeros((b, npoint), np.int64)
    rows = np.arange(b)
    for i in range(npoint):
        out[:, i] = cur
        d = dist2(xyz, xyz[rows, cur])
        dist = np.where(d < dist, d, dist)
        cur = dist.argmax(1)                                   # numpy: the first of equal maxima
    return out


def ball_query(radius, nsample, xyz, centres, dtype=np.float32, rows_per_pass=1 << 14):
    """xyz (B, N, 3), centres (B, S, 3) float32 -> (idx (B, S, min(nsample, N)) int64, count (B, S) int64)."""
    xyz, centres = np.asarray(xyz, np.float32), np.asarray(centres, np.float32)
    b, n, _ = xyz.shape
    s = centres.shape[1]
    width = min(int(nsample), n)
    r2 = np.float32(radius) * np.float32(radius) if dtype == np.float32 else np.float64(radius) ** 2
    idx, count = np.empty((b, s, width), np.int64), np.empty((b, s), np.int64)
    step = max(1, rows_per_pass // n)
    for bb in range(b):
        for s0 in range(0, s, step):
            c = centres[bb, s0:s0 + step]
            member = ~(dist2(xyz[bb][None], c, dtype) > r2)                              # (rows, N)
            cnt = member.sum(1)
            order = np.argsort(~member, axis=1, kind="stable")[:, :width]               # the members first, in ascending j
            first = np.where(cnt > 0, order[:, 0], n)
            idx[bb, s0:s0 + step] = np.where(np.arange(width)[None] < cnt[:, None], order, first[:, None])
            count[bb, s0:s0 + step] = cnt
    return idx, count


def near_boundary(radius, xyz, centres):
    """(B, S) bool: the rows whose ball has a point within BOUNDARY_REL * r^2 of its surface (float64, squared distances)."""
    xyz, centres = np.asarray(xyz, np.float32), np.asarray(centres, np.float32)
    r2 = np.float64(radius) ** 2
    return np.stack([(np.abs(dist2(xyz[b][None], centres[b], np.float64) - r2) <= BOUNDARY_REL * r2).any(1) for b in range(len(xyz))])


def row_properties(idx, n):
    """Every row: in range; either all N, or strictly ascending members followed by repeats of the first."""
    idx = np.asarray(idx, np.int64).reshape(-1, np.shape(idx)[-1])
    assert idx.min() >= 0 and idx.max() <= n
    empty = idx[:, 0] == n
    assert (idx[empty] == n).all() and (idx[~empty] < n).all()
    rows = idx[~empty]
    up = np.diff(rows, axis=1) > 0
    assert (up[:, 1:] <= up[:, :-1]).all()                                               # once a row stops ascending it never resumes
    assert ((rows[:, 1:] == rows[:, :1]) | up).all()                                      # a slot that does not ascend repeats the first


def gather(xyz, idx):
    return np.stack([x[i] for x, i in zip(np.asarray(xyz), np.asarray(idx, np.int64))])


def g22():
    return np.load(GOLDEN, allow_pickle=False)


def cases(z):
    """The fixture as a list of dicts: kind "fps" (xyz, start, npoint, idx) or "ball" (xyz, centres, radius, nsample, idx, near)."""
    out = []
    clouds = {1024: z["cloud0"], 512: gather(z["cloud0"], z["fps0_idx"]), 300: z["cloud2"]}
    for k, (b, n, npoint) in enumerate(FPS_CASES):
        idx = z["fps%d_idx" % k].astype(np.int64)
        assert idx.shape == (b, npoint) and clouds[n].shape == (b, n, 3)
        out.append({"kind": "fps", "name": "fps %dx%d->%d" % (b, n, npoint), "xyz": clouds[n], "start": idx[:, 0].copy(), "npoint": npoint, "idx": idx})
    centres = {1024: clouds[512], 512: gather(clouds[512], z["fps1_idx"])}              # the FPS-chosen centres of each level
    for k, (n, s, radius, nsample) in enumerate(BALL_CASES):
        assert centres[n].shape == (2, s, 3)
        out.append({"kind": "ball", "name": "ball N=%d S=%d r=%g K=%d" % (n, s, radius, nsample), "xyz": clouds[n], "centres": centres[n],
                    "radius": radius, "nsample": nsample, "idx": z["ball%d_idx" % k].astype(np.int64), "near": z["ball%d_near" % k]})
    return out
