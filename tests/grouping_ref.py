"""Shared by tests/test_grouping_host.py, tests/test_gpu_grouping.py and tools/gen_golden.py (G25): group_points and its backward
restated in numpy from their DEFINITION (include/so3proj.h), and the fixture's layout.

    forward:   a relative coordinate is xyz[b][idx[b][s][k]][j] - centres[b][s][j], ONE float32 subtraction; a feature is a copy; a slot
               whose index lies outside [0, N) is 0 in every channel.  Exact: kernels and host model reproduce it bit for bit.
    backward:  grad_xyz / grad_feat: per point the sum of the matching channel of grad_out over the slots that selected it, plain
               additions from 0 in the ascending MEMORY order of grad_out's slots -- (s, k) channel-last, (k, s) channel-first;
               grad_centres = 0 - (the sum over ascending k of the valid slots' coordinate channels).
               backward(..., dtype=np.float32) follows that order in float32 (the host model must equal it bit for bit);
               dtype=np.float64 is the value the device is compared with, within gamma_{h-1} * sum |g| for an element with h terms,
               gamma_n = n u / (1 - n u), u = 2^-24: the bound of h - 1 additions in ANY order (Higham, Accuracy and Stability of
               Numerical Algorithms, section 4.2); the final 0 - x of grad_centres is exact."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_grouping.npz")
U = 2.0 ** -24
N_FIXTURE, S_FIXTURE, D_FIXTURE, N_ALL = 256, 64, 5, 40
RADII = ((0.2, 16), (0.4, 32))       # the Msg layer's; the single-scale layer takes the second
G_SEED = 2500                        # the seeded G: np.random.RandomState(G_SEED + i).standard_normal(T_i.shape) as float32


def gamma(n):
    n = np.maximum(np.asarray(n, np.float64), 0.0)
    return n * U / (1.0 - n * U)


def valid(idx, n):
    idx = np.asarray(idx, np.int64)
    return (idx >= 0) & (idx < n)


def forward(xyz, centres, feat, idx, channels_first=False, features_first=False):
    """xyz (B, N, 3), centres (B, S, 3), feat None / (B, N, D) / (B, D, N), idx (B, S, K) -> float32 (B, S, K, C) or (B, C, K, S)."""
    xyz, centres, idx = np.asarray(xyz, np.float32), np.asarray(centres, np.float32), np.asarray(idx, np.int64)
    ok = valid(idx, xyz.shape[1])
    safe = np.where(ok, idx, 0)
    rows = np.arange(xyz.shape[0])[:, None, None]
    parts = [xyz[rows, safe] - centres[:, :, None, :]]
    if feat is not None:
        f = np.asarray(feat, np.float32)
        f = f.transpose(0, 2, 1) if channels_first else f
        if f.shape[-1]:
            parts.append(f[rows, safe])
    out = np.concatenate(parts[::-1] if features_first else parts, -1).astype(np.float32)
    out[~ok] = np.float32(0.0)
    return np.ascontiguousarray(out.transpose(0, 3, 2, 1)) if channels_first else out


def backward(grad_out, idx, n, channels_first=False, features_first=False, dtype=np.float32):
    """grad_out in the forward's output layout -> dict: grad_xyz (B, N, 3), grad_centres (B, S, 3), grad_feat (B, N, D) or (B, D, N), all of
    `dtype`, summed in the defined order; mag_* the float64 sums of |g|; hits (B, N) and slots (B, S), the number of terms."""
    g = np.asarray(grad_out)
    g = g.transpose(0, 3, 2, 1) if channels_first else g                           # (B, S, K, C)
    idx = np.asarray(idx, np.int64)
    b, s, k, c = g.shape
    d = c - 3
    ok = valid(idx, n)
    acc, mag, hits = np.zeros((b, n, c), dtype), np.zeros((b, n, c)), np.zeros((b, n), np.int64)
    every = np.arange(b)
    order = [(ss, kk) for kk in range(k) for ss in range(s)] if channels_first else [(ss, kk) for ss in range(s) for kk in range(k)]
    for ss, kk in order:
        rows = every[ok[:, ss, kk]]
        i, term = idx[rows, ss, kk], g[rows, ss, kk]
        acc[rows, i] = acc[rows, i] + term.astype(dtype)                           # one cloud per row: no index repeats inside the update
        mag[rows, i] += np.abs(term.astype(np.float64))
        hits[rows, i] += 1
    xs = slice(d, d + 3) if features_first else slice(0, 3)
    fs = slice(0, d) if features_first else slice(3, c)
    cen, cmag = np.zeros((b, s, 3), dtype), np.zeros((b, s, 3))
    for kk in range(k):
        m = ok[:, :, kk, None]
        cen = np.where(m, cen + g[:, :, kk, xs].astype(dtype), cen)
        cmag += np.where(m, np.abs(g[:, :, kk, xs].astype(np.float64)), 0.0)
    gf, fmag = acc[..., fs], mag[..., fs]
    if channels_first:
        gf, fmag = gf.transpose(0, 2, 1), fmag.transpose(0, 2, 1)
    return {"grad_xyz": np.ascontiguousarray(acc[..., xs]), "grad_centres": (dtype(0) - cen).astype(dtype), "grad_feat": np.ascontiguousarray(gf),
            "mag_xyz": mag[..., xs], "mag_centres": cmag, "mag_feat": fmag, "hits": hits, "slots": ok.sum(-1)}


def bounds(want, channels_first=False):
    """The three elementwise bounds of a float64 backward() result, shaped as its outputs."""
    h = want["hits"]
    hf = h[:, None, :] if channels_first else h[:, :, None]
    return {"grad_xyz": gamma(h[:, :, None] - 1) * want["mag_xyz"], "grad_centres": gamma(want["slots"][:, :, None] - 1) * want["mag_centres"],
            "grad_feat": gamma(hf - 1) * want["mag_feat"]}


def seeded_g(i, shape):
    return np.random.RandomState(G_SEED + i).standard_normal(shape).astype(np.float32)


def g25():
    return np.load(GOLDEN, allow_pickle=False)


def cases(z):
    """The fixture as a dict: xyz (2, 256, 3), points (2, 256, 5) (channel-last), and per layer what the reference recorded.
    "sa": PointNetSetAbstraction(64, 0.4, 32), "msg": PointNetSetAbstractionMsg(64, [0.2, 0.4], [16, 32]), "all": group_all on 2 x 40."""
    out = {"xyz": z["xyz"], "points": z["points"], "xyz_all": z["xyz_all"], "points_all": z["points_all"]}
    for tag, nrad in (("sa", 1), ("msg", 2)):
        out[tag] = {"fps": z["fps_" + tag].astype(np.int64), "new_xyz": z["new_xyz_" + tag], "grad_xyz": z["grad_xyz_" + tag],
                    "grad_points": z["grad_points_" + tag], "idx": [z["idx_%s_%d" % (tag, i)].astype(np.int64) for i in range(nrad)],
                    "t": [z["t_%s_%d" % (tag, i)] for i in range(nrad)]}
    out["all"] = {"new_xyz": z["new_xyz_all"], "t": z["t_all"], "grad_xyz": z["grad_xyz_all"], "grad_points": z["grad_points_all"]}
    return out
