"""Shared by tests/test_icp_host.py, tests/test_gpu_icp.py and tools/gen_golden.py (G21): nearest_neighbors and icp_align restated in
float64, and the fixture's layout.

    nearest(X, Y):  d_i = min_j |x_i - y_j|,  j(i) = the first argmin  -- brute force over coordinate differences.
    One ICP iteration from the pose (R, t):  x_i = R p_i + t;  j(i), d_i = nearest(x, Q);  w'_i = w_i [d_i <= max_distance];
        (R', t') = rigid_align_ref.align64(P, Q[j], w')  (the pose stays where sum w' = 0);
        rmse = sqrt(sum w' d^2 / sum w'),  inliers = #{w' > 0}  (0 and 0 where sum w' = 0) -- at the pose the iteration started from.
The search runs on whatever device its arguments are on (the GPU test puts large batches on the GPU, in float64); the pose is solved on
the CPU by rigid_align_ref."""
import os

import numpy as np
import torch

import rigid_align_ref as ra

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_icp.npz")
SIZES = ((1, 1), (3, 7), (255, 1023), (256, 1024), (257, 1025), (1000, 2500))      # (N, M): the tile of 1024, the unroll of 8, the chunk of 256 U
SMALL_SIZES = SIZES[:2]
WEIGHTS = ("none", "random", "mask")
OFFSETS = (0.0, 10.0, 100.0)
MARGIN = 1e-4                        # no float64 d_i of a trimmed case lies within this of its max_distance
KINDS = ("search", "step", "converge", "noise")
FULL, PROPERTIES = 0, 2              # how a step's pose is checked (as rigid_align_ref: everything, or properties only where R is not unique)


def _t(a, device="cpu"):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64, device=device)


def nearest64(X, Y, device="cpu", pairs_per_pass=1 << 24):
    """X (B,N,3), Y (B,M,3) or (M,3) -> (dist (B,N) float64, idx (B,N) int64), numpy.  The first of equal candidates."""
    X, Y = _t(X, device), _t(Y, device)
    b, n, _ = X.shape
    m = Y.shape[-2]
    step = max(1, pairs_per_pass // (n * m))
    dist, idx = [], []
    for b0 in range(0, b, step):
        x = X[b0:b0 + step]
        y = Y[b0:b0 + step] if Y.dim() == 3 else Y[None]
        d2 = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
        best = d2.min(-1).values
        first = (d2 == best[..., None]).to(torch.uint8).argmax(-1)            # argmax of a 0/1 table: the first maximum
        dist.append(best.sqrt().cpu())
        idx.append(first.cpu())
    return torch.cat(dist).numpy(), torch.cat(idx).numpy()


def pose_points(P, R, t):
    return np.einsum("bij,bnj->bni", np.asarray(R, np.float64), np.asarray(P, np.float64)) + np.asarray(t, np.float64)[:, None]


def gather(Q, idx, b):
    """The target points idx (B,N) names: Q (B,M,3) or shared (M,3) -> (B,N,3) float64."""
    Q = np.asarray(Q, np.float64)
    return Q[idx] if Q.ndim == 2 else np.take_along_axis(Q, idx[:, :, None], 1)


def dist_to(P, Q, idx, R, t):
    """Float64 distances from the posed source points to the target points idx names."""
    return np.linalg.norm(pose_points(P, R, t) - gather(Q, idx, len(P)), axis=-1)


def step_from(P, Q, idx, d, R, t, w=None, max_distance=None):
    """The second half of an iteration in float64, given the correspondences idx and their distances d: the trimmed weights, then
    rigid_align on the pairs.  Returns a dict: R, t (the pose kept where sum w' = 0), rmse, inliers, stats (pbar, qbar, W), H, wp."""
    P64 = np.asarray(P, np.float64)
    b, n, _ = P64.shape
    wp = np.ones((b, n)) if w is None else np.asarray(w, np.float64).copy()
    if max_distance is not None:
        wp = wp * (d <= max_distance)
    W = wp.sum(1)
    live = W > 0
    with torch.no_grad():
        Rn, tn, H, st = (x.numpy() for x in ra.align64(_t(P64), _t(gather(Q, idx, b)), _t(wp)))
    Rn = np.where(live[:, None, None], Rn, np.asarray(R, np.float64))
    tn = np.where(live[:, None], tn, np.asarray(t, np.float64))
    rmse = np.where(live, np.sqrt((wp * d * d).sum(1) / np.where(live, W, 1.0)), 0.0)
    return {"R": Rn, "t": tn, "rmse": rmse, "inliers": (wp > 0).sum(1), "stats": st, "H": H, "wp": wp}


def icp64(P, Q, R0=None, t0=None, iterations=10, max_distance=None, w=None, device="cpu"):
    """The whole loop in float64.  Returns a dict: R, t, rmse (iterations,B), inliers (iterations,B), nearest and dist of the last search."""
    b = len(P)
    R = np.broadcast_to(np.eye(3), (b, 3, 3)).copy() if R0 is None else np.asarray(R0, np.float64)
    t = np.zeros((b, 3)) if t0 is None else np.asarray(t0, np.float64)
    rmse, inl, idx, d = [], [], None, None
    for _ in range(iterations):
        d, idx = nearest64(pose_points(P, R, t), Q, device)
        s = step_from(P, Q, idx, d, R, t, w, max_distance)
        R, t = s["R"], s["t"]
        rmse.append(s["rmse"])
        inl.append(s["inliers"])
    return {"R": R, "t": t, "rmse": np.array(rmse).reshape(iterations, b), "inliers": np.array(inl).reshape(iterations, b), "nearest": idx, "dist": d}


def runner_up_gap(P, Q, R, t, device="cpu"):
    """min over the points of (second smallest - smallest) float64 distance to DISTINCT target positions: how far the correspondences
    are from a tie."""
    X, Y = _t(pose_points(P, R, t), device), _t(Q, device)
    y = Y if Y.dim() == 3 else Y[None]
    d = ((X[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1).sqrt()
    two = d.topk(2, dim=-1, largest=False).values
    return float((two[..., 1] - two[..., 0]).min())


# ---- the fixture: arrays of case i under the prefix "c<i>_" -------------------------------------------------------------------
ARRAYS = ("P", "Q", "w", "R0", "t0", "Rgt", "tgt", "perm", "dist", "nearest", "R", "t", "rmse", "inliers")


def g21():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def cases(d):
    """The fixture's cases as dicts.  Always: kind, name, n, m, b, shared, weights, offset, iterations, max_distance (None: no trimming),
    check, P, Q; w, R0, t0 are None where the call is made without them; the float64 answers a kind has are under the names of ARRAYS."""
    out = []
    kinds, wnames = [str(s) for s in d["kind_names"]], [str(s) for s in d["weight_names"]]
    for i in range(len(d["case_kind"])):
        md = float(d["case_max_distance"][i])
        c = {"kind": kinds[int(d["case_kind"][i])], "name": str(d["case_name"][i]), "weights": wnames[int(d["case_weights"][i])],
             "offset": float(d["case_offset"][i]), "iterations": int(d["case_iterations"][i]), "max_distance": None if md < 0 else md,
             "shared": bool(d["case_shared"][i]), "check": int(d["case_check"][i])}
        for k in ARRAYS:
            c[k] = d.get("c%d_%s" % (i, k))
        c["b"], c["n"], c["m"] = c["P"].shape[0], c["P"].shape[1], c["Q"].shape[-2]
        out.append(c)
    return out
