"""Shared by tests/test_rigid_align_host.py, tests/test_gpu_rigid_align.py and tools/gen_golden.py (G20): rigid_align restated in
float64 torch, its closed-form gradients, and the fixture's layout.

For each cloud, with w_i >= 0 (all ones when weights is None):
    W = sum w_i      pbar = sum w_i p_i / W      qbar = sum w_i q_i / W
    H = sum w_i (q_i - qbar)(p_i - pbar)^T       (not divided by W)
    R = proj_SO(3)(H) = U diag(1, 1, det(U V^T)) V^T for H = U S V^T        t = qbar - R pbar
W == 0 (or N == 0): pbar = qbar = 0, H = 0, R = I, t = 0 and every gradient is 0.
Gradients for upstream gR, gt, gH, with a_i = p_i - pbar, c_i = q_i - qbar, u = R^T gt:
    dH = K2(H, gR - gt pbar^T) + gH        K2: dM = U' Bm V^T, A = U'^T G V, Bm_ij = (A_ij - A_ji) / (s'_i + s'_j)  (the signed SVD)
    dQ_i = w_i dH a_i + (w_i / W) gt       dP_i = w_i dH^T c_i - (w_i / W) u       dw_i = c_i^T dH a_i + (gt . c_i - u . a_i) / W"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_rigid_align.npz")
SIZES = (1, 2, 3, 63, 64, 65, 512, 513, 1000)
SMALL_SIZES = SIZES[:6]                       # every (weights, offset) combination; the larger sizes take a covering selection
WEIGHTS = ("none", "ones", "random", "mask", "zero")
OFFSETS = (0.0, 10.0, 100.0)
SIGMAS = (0.0, 0.01)
FAMILIES = ("haar", "reflected", "collinear", "coincident")
# how a case is checked: everything against the float64 answers; exact identity / zeros; or properties only (finite, R a rotation,
# R pbar + t = qbar) where R is not unique or badly conditioned -- H and the centroids are compared in every case
FULL, ZERO, PROPERTIES = 0, 1, 2


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def proj64(H):
    U, _, Vh = torch.linalg.svd(H)
    d = torch.linalg.det(U @ Vh)
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1))
    return U @ D @ Vh


def align64(P, Q, w=None):
    """(B,N,3), (B,N,3), None | (B,N) float64 -> R (B,3,3), t (B,3), H (B,3,3), stats (B,7) = (pbar, qbar, W).  Differentiable."""
    b, n, _ = P.shape
    if w is None:
        w = torch.ones((b, n), dtype=torch.float64)
    W = w.sum(1)
    live = W > 0
    inv = torch.where(live, 1.0 / torch.where(live, W, torch.ones_like(W)), torch.zeros_like(W))
    pbar = (w[:, :, None] * P).sum(1) * inv[:, None]
    qbar = (w[:, :, None] * Q).sum(1) * inv[:, None]
    H = torch.einsum("bn,bni,bnj->bij", w, Q - qbar[:, None], P - pbar[:, None])
    eye = torch.eye(3, dtype=torch.float64).expand(b, 3, 3)
    R = torch.where(live[:, None, None], proj64(torch.where(live[:, None, None], H, eye)), eye)
    t = qbar - torch.einsum("bij,bj->bi", R, pbar)
    return R, t, H, torch.cat([pbar, qbar, W[:, None]], 1)


def k2_64(H, G):
    """The closed form of d(proj)/dH applied to G (include/so3proj.h, K2), float64, no clamp."""
    U, S, Vh = torch.linalg.svd(H)
    d = torch.linalg.det(U @ Vh)
    sign = torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)
    Us, s = U * sign[:, None, :], S * sign
    A = Us.transpose(1, 2) @ G @ Vh.transpose(1, 2)
    den = s[:, :, None] + s[:, None, :]
    off = ~torch.eye(3, dtype=torch.bool)
    Bm = torch.where(off, (A - A.transpose(1, 2)) / torch.where(off, den, torch.ones_like(den)), torch.zeros_like(A))
    return Us @ Bm @ Vh


def grads64(P, Q, w, gR, gt, gH):
    """dP, dQ (B,N,3) and dw (B,N) by the closed form, float64.  w None: all ones (dw is then the gradient at those ones)."""
    with torch.no_grad():
        b, n, _ = P.shape
        ww = torch.ones((b, n), dtype=torch.float64) if w is None else w
        R, _, H, st = align64(P, Q, ww)
        pbar, qbar, W = st[:, :3], st[:, 3:6], st[:, 6]
        live = W > 0
        inv = torch.where(live, 1.0 / torch.where(live, W, torch.ones_like(W)), torch.zeros_like(W))
        eye = torch.eye(3, dtype=torch.float64).expand(b, 3, 3)
        g = gR - gt[:, :, None] * pbar[:, None, :]
        dH = (k2_64(torch.where(live[:, None, None], H, eye), g) + gH) * live[:, None, None]
        u = torch.einsum("bij,bi->bj", R, gt)
        a, c = P - pbar[:, None], Q - qbar[:, None]
        gti, ui = gt * inv[:, None], u * inv[:, None]
        dHa = torch.einsum("bij,bnj->bni", dH, a)
        dQ = ww[:, :, None] * (dHa + gti[:, None])
        dP = ww[:, :, None] * (torch.einsum("bij,bni->bnj", dH, c) - ui[:, None])
        dw = (c * dHa).sum(-1) + (c * gti[:, None]).sum(-1) - (a * ui[:, None]).sum(-1)
        return dP, dQ, dw


def autograd64(P, Q, w, gR, gt, gH):
    """The same three gradients by float64 autograd of (R * gR).sum() + (t * gt).sum() + (H * gH).sum() through align64."""
    b, n, _ = P.shape
    p, q = P.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    ww = (torch.ones((b, n), dtype=torch.float64) if w is None else w.clone()).requires_grad_(True)
    R, t, H, _ = align64(p, q, ww)
    ((R * gR).sum() + (t * gt).sum() + (H * gH).sum()).backward()
    return p.grad, q.grad, ww.grad


def answers(P, Q, w):
    """The float64 answers of one case from its float32 inputs (numpy in, numpy out)."""
    with torch.no_grad():
        R, t, H, st = align64(_t(P), _t(Q), None if w is None else _t(w))
    return {"R": R.numpy(), "t": t.numpy(), "H": H.numpy(), "stats": st.numpy()}


def case_grads(c):
    """Float64 (dP, dQ, dw) of a fixture case for its stored upstream gradients, as numpy."""
    return tuple(x.numpy() for x in grads64(_t(c["P"]), _t(c["Q"]), None if c["w"] is None else _t(c["w"]), _t(c["gR"]), _t(c["gt"]), _t(c["gH"])))


# ---- the fixture: cases stored back to back -----------------------------------------------------------------------------------
PER_CLOUD = ("R", "t", "H", "stats", "gR", "gt", "gH", "sigma")
PER_POINT = ("P", "Q", "w")
PER_CASE = ("family", "n", "b", "weights", "offset", "check")


def g20():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def cases(d):
    """The fixture's cases as dicts: family and weights (str), n, b, offset, check, and every array sliced and shaped (B,...) / (B,N,...).
    w is None for the weights kind "none" (the stored ones are what the answers were computed with)."""
    out = []
    c0 = p0 = 0
    fams, kinds = [str(s) for s in d["family_names"]], [str(s) for s in d["weight_names"]]
    for i in range(len(d["case_n"])):
        n, b = int(d["case_n"][i]), int(d["case_b"][i])
        case = {"family": fams[int(d["case_family"][i])], "weights": kinds[int(d["case_weights"][i])], "n": n, "b": b,
                "offset": float(d["case_offset"][i]), "check": int(d["case_check"][i])}
        for k in PER_CLOUD:
            case[k] = d[k][c0:c0 + b]
        for k in PER_POINT:
            a = d[k][p0:p0 + b * n]
            case[k] = a.reshape((b, n) + a.shape[1:])
        if case["weights"] == "none":
            case["w"] = None
        out.append(case)
        c0 += b
        p0 += b * n
    assert c0 == len(d["R"]) and p0 == len(d["P"])
    return out


def rotation_defect(R):
    """max |R^T R - I| and max |det R - 1| over a batch of float64 matrices."""
    R = np.asarray(R, np.float64)
    return float(np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max()), float(np.abs(np.linalg.det(R) - 1).max())
