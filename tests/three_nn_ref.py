"""Shared by tests/test_three_nn_host.py, tests/test_gpu_three_nn.py and tools/gen_golden.py (G24): three_nn and three_interpolate
restated in numpy from their DEFINITION (include/so3proj.h), and the fixture's layout.

    d(n, s) = ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences: float32 arrays, so numpy rounds every operation on its own
    neighbours: the three smallest d, among equal d the lower index first = the first three of a STABLE argsort along s;
                S < 3: the real neighbours first, the other slots repeat slot 0's index with d = +inf
    weights:    r_k = 1 / (d_k + 1e-8) in float32 (0 for a padded slot), w_k = r_k / ((r_0 + r_1) + r_2)
These three are exact: the kernels and the host model must reproduce them bit for bit.  So are the interpolation and its backward, whose
order of operations is part of the definition (so3_device.h: three_interp, three_interp_bwd_add); interpolate32 and backward32 restate
them through tests/f32_exact.py's fma32, and the host model and the device are held to those bits:
    out = fma(w2, f2, fma(w1, f1, w0 * f0)),    grad_feat[s] = h fused multiply-adds from +0 in ascending (n, k).
The float64 evaluation FROM the float32 d and w stays beside them as the check that the defined order is an accurate one:
    out:  three roundings on float32 inputs, each at most 2^-24 relative of a partial result no larger than sum_k w_k |f_k|
          -> 3 * 2^-24 * sum_k |w_k f_k| to first order.  INTERP_ULPS = 8 is the issue's constant (two products and two sums, without
          fused operations); the fused order is inside it.
    grad_feat[s]: h roundings, each at most 2^-24 of a partial sum no larger than sum |w g| -> h * 2^-24 * sum |w g|; the bound used
          is (h + 2)."""
import os

import numpy as np

from f32_exact import fma32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_three_nn.npz")
EPS = np.float32(1e-8)
U = 2.0 ** -24
INTERP_ULPS = 8
TIE_GAP = 2e-6                       # near_tie: two adjacent distances among a row's four smallest differ by at most this (float64)
ZERO_DIST = 1e-4                     # near_zero: a row's smallest distance is at most this (float64)
MASK_CAP = 0.01
D_FIXTURE = 16
CASES = (("disjoint", 2, 1024, 512), ("disjoint", 2, 512, 128), ("disjoint", 3, 300, 77), ("subset", 2, 1024, 512), ("single", 2, 128, 1))


def dist2(xyz1, xyz2, dtype=np.float32):
    """xyz1 (B, N, 3), xyz2 (B, S, 3) -> (B, N, S): the defined distance."""
    a, b = np.asarray(xyz1, dtype)[:, :, None, :], np.asarray(xyz2, dtype)[:, None, :, :]
    dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    return ((dx * dx) + (dy * dy)) + (dz * dz)


def three_nn(xyz1, xyz2, rows_per_pass=1 << 22):
    """-> dist2 (B, N, 3) float32, idx (B, N, 3) int64, weight (B, N, 3) float32."""
    xyz1, xyz2 = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    b, n, s = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    real = min(3, s)
    d3, idx = np.full((b, n, 3), np.inf, np.float32), np.zeros((b, n, 3), np.int64)
    step = max(1, rows_per_pass // s)
    for n0 in range(0, n, step):
        d = dist2(xyz1[:, n0:n0 + step], xyz2)
        order = np.argsort(d, axis=-1, kind="stable")[..., :real]
        idx[:, n0:n0 + step, :real] = order
        d3[:, n0:n0 + step, :real] = np.take_along_axis(d, order, -1)
    idx[..., real:] = idx[..., :1]
    return d3, idx, weights(d3, s)


def weights(d3, s):
    d3 = np.asarray(d3, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.float32(1.0) / (d3 + EPS)
        r[..., min(3, s):] = np.float32(0.0)
        total = (r[..., 0] + r[..., 1]) + r[..., 2]
        return (r / total[..., None]).astype(np.float32)


def _gather(feat, idx, channels_first):
    """feat (B, S, D) or (B, D, S) -> (B, N, 3, D) float64."""
    f = np.asarray(feat, np.float64)
    f = f.transpose(0, 2, 1) if channels_first else f
    return np.stack([fb[ib] for fb, ib in zip(f, np.asarray(idx, np.int64))])


def interpolate(feat, idx, weight, channels_first=False):
    """-> (out float64, bound float64), both (B, N, D), or (B, D, N) with channels_first."""
    g = _gather(feat, idx, channels_first)
    w = np.asarray(weight, np.float64)[..., None]
    out, bound = (w * g).sum(2), INTERP_ULPS * U * np.abs(w * g).sum(2)
    return (out.transpose(0, 2, 1), bound.transpose(0, 2, 1)) if channels_first else (out, bound)


def backward(grad_out, idx, weight, s, channels_first=False):
    """-> (grad_feat float64, bound float64, hits (B, S) int64); grad_feat is (B, S, D), or (B, D, S) with channels_first."""
    g = np.asarray(grad_out, np.float64)
    g = g.transpose(0, 2, 1) if channels_first else g                              # (B, N, D)
    idx, w = np.asarray(idx, np.int64), np.asarray(weight, np.float64)
    b, n, d = g.shape
    grad, mag, hits = np.zeros((b, s, d)), np.zeros((b, s, d)), np.zeros((b, s), np.int64)
    for bb in range(b):
        for k in range(3):
            np.add.at(grad[bb], idx[bb, :, k], w[bb, :, k, None] * g[bb])
            np.add.at(mag[bb], idx[bb, :, k], np.abs(w[bb, :, k, None] * g[bb]))
            np.add.at(hits[bb], idx[bb, :, k], 1)
    bound = (hits[..., None] + 2) * U * mag
    return (grad.transpose(0, 2, 1), bound.transpose(0, 2, 1), hits) if channels_first else (grad, bound, hits)


def interpolate32(feat, idx, weight, channels_first=False):
    """The DEFINED bits (so3_device.h: three_interp): out = fma(w2, f2, fma(w1, f1, w0 * f0)) in float32, the product rounded on its own.
    -> float32 (B, N, D), or (B, D, N) with channels_first."""
    f = np.asarray(feat, np.float32)
    f = f.transpose(0, 2, 1) if channels_first else f
    g = np.stack([fb[ib] for fb, ib in zip(f, np.asarray(idx, np.int64))])          # (B, N, 3, D)
    w = np.asarray(weight, np.float32)[..., None]
    out = fma32(w[:, :, 2], g[:, :, 2], fma32(w[:, :, 1], g[:, :, 1], w[:, :, 0] * g[:, :, 0]))
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if channels_first else out


def backward32(grad_out, idx, weight, s, channels_first=False):
    """The DEFINED bits (so3_device.h: three_interp_bwd_add): every known point's running sum starts at +0 and takes its hits in
    ascending (n, k) through acc = fma(w, g, acc).  One step per (n, k), all clouds and channels at once.
    -> float32 (B, S, D), or (B, D, S) with channels_first."""
    g = np.asarray(grad_out, np.float32)
    g = g.transpose(0, 2, 1) if channels_first else g                              # (B, N, D)
    idx, w = np.asarray(idx, np.int64), np.asarray(weight, np.float32)
    b, n, d = g.shape
    acc, rows = np.zeros((b, s, d), np.float32), np.arange(b)
    for nn in range(n):
        for k in range(3):
            at = idx[:, nn, k]
            acc[rows, at] = fma32(w[:, nn, k, None], g[:, nn], acc[rows, at])
    return np.ascontiguousarray(acc.transpose(0, 2, 1)) if channels_first else acc


def masks(xyz1, xyz2):
    """(near_tie, near_zero), both (B, N) bool, from float64 distances."""
    d = np.sort(dist2(xyz1, xyz2, np.float64), axis=-1)[..., :4]
    tie = (np.diff(d, axis=-1) <= TIE_GAP).any(-1) if d.shape[-1] > 1 else np.zeros(d.shape[:2], bool)
    return tie, d[..., 0] <= ZERO_DIST


def row_properties(d3, idx, s):
    """Every row: indices in [0, S), the real neighbours distinct, dist2 non-decreasing, the padded slots as defined."""
    d3, idx = np.asarray(d3), np.asarray(idx, np.int64)
    real = min(3, s)
    assert idx.min() >= 0 and idx.max() < s
    assert (np.diff(d3[..., :real], axis=-1) >= 0).all()
    for a in range(real):
        for b in range(a + 1, real):
            assert (idx[..., a] != idx[..., b]).all()
    assert (idx[..., real:] == idx[..., :1]).all() and np.isposinf(d3[..., real:]).all()


def g24():
    return np.load(GOLDEN, allow_pickle=False)


def cases(z):
    """The fixture as a list of dicts: kind, name, xyz1, xyz2, feat (B, S, D_FIXTURE), ref_idx, near_tie, near_zero; ref_out and ref_dev
    for the kinds whose values are compared with the reference (not "subset": there the reference's weights are noise)."""
    out = []
    for k, (kind, b, n, s) in enumerate(CASES):
        c = {"kind": kind, "name": "%s %dx%d<-%d" % (kind, b, n, s)}
        if kind == "subset":                                                   # the unknown cloud and the features of case 0
            c["xyz1"], c["feat"] = z["xyz1_0"], z["feat_0"]
            c["xyz2"] = np.stack([x[i] for x, i in zip(c["xyz1"], z["fps_%d" % k].astype(np.int64))])
            c["ref_negative_weights"] = int(z["ref_negative_weights_%d" % k])
        else:
            c["xyz1"], c["xyz2"], c["feat"] = z["xyz1_%d" % k], z["xyz2_%d" % k], z["feat_%d" % k]
            c["ref_out"], c["ref_dev"] = z["ref_out_%d" % k], float(z["ref_dev_%d" % k])
        c["ref_idx"] = z["ref_idx_%d" % k].astype(np.int64)
        c["near_tie"], c["near_zero"] = z["near_tie_%d" % k], z["near_zero_%d" % k]
        assert c["xyz1"].shape == (b, n, 3) and c["xyz2"].shape == (b, s, 3) and c["feat"].shape == (b, s, D_FIXTURE), c["name"]
        out.append(c)
    return out
