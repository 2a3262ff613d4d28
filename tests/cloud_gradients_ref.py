"""Shared by tests/test_cloud_gradient_kernels_host.py and tests/test_gpu_cloud_gradient_kernels.py: the inputs, the float64 closed
forms, the checkers and the float32 restatements of the four entry points that share k_kabsch's skeleton with a backward or a pose,
    so3_rotate_clouds_bwd_f32   dP_i = R^T g_i,  dR = sum_i g_i p_i^T
    so3_kabsch_bwd_f32          dH = K2(H, gR) + gH,  dQ_i = dH p_i,  dP_i = dH^T q_i
    so3_rigid_align_f32         tests/rigid_align_ref.py
    so3_rigid_align_bwd_f32     gR' = gR - g_t pbar^T,  dH = K2(H, gR') + gH,  a_i = p_i - pbar,  c_i = q_i - qbar,  u = R^T g_t,
                                dQ_i = w_i dH a_i + (w_i / W) g_t,  dP_i = w_i dH^T c_i - (w_i / W) u,
                                dw_i = c_i^T dH a_i + (g_t . c_i - u . a_i) / W.
The backward kernels are functions of their arguments: they do not check that H belongs to P and Q.  The tests therefore hand them a
synthetic, well-conditioned H per cloud (synthetic_h), whatever N is, and the float64 references restate the closed forms from the
same float32 inputs with H, R and stats taken as given.

A checker returns FIGURES, one number per output, the largest over every point of every cloud; LIMITS-style dictionaries in the host
test say what each may reach.  Two kinds (u = 2^-24, gamma_k = k u / (1 - k u)):
  * derived bounds, figure = max error / bound, limit 1:
      rot_dP   |d dP_ic| <= gamma_3 sum_k |R_kc| |g_ik|                  (three roundings on every product's way to the result)
      rot_dR   |d dR_ac| <= gamma_k sum_i |g_ia| |p_ic|,  k = ceil(N / 64) + 6: a lane adds its ceil(N / 64) products by fma, six
               butterfly steps follow, lanes past the end add exact zeros
      kbH_dQ   gR null: dH = gH exactly, |d dQ_ia| <= gamma_3 sum_k |gH_ak| |p_ik|;  kbH_dP the same with q and gH^T
    an entry whose bound is 0 must be exactly 0 (the figure is inf otherwise);
  * figures whose limit is measured (K2 has no proven bound): figure_i = |d row_i|_inf / D_i with
      kb_dQ    D_i = (|gR|_F / gap + |gH|_F) |p_i|_2          (kb_dP: |q_i|_2)
      ra_dQ    D_i = w_i F |a_i| + (w_i / W) |g_t|,           F = |gR'|_F / gap + |gH|_F          (ra_dP: |c_i|)
      ra_dw    D_i = F |a_i| |c_i| + |g_t| (|a_i| + |c_i|) / W
    gap = s2 + s3 sign(det H) from the float64 SVD of the H supplied; a point with D_i = 0 must come back as exact zeros."""
import numpy as np
import torch

import rigid_align_ref as ref
from support import np_ptr
from test_gpu_cloud_kernels import U, _rotations, make_batch, r_reference

POINTS = (1, 2, 3, 63, 64, 65, 127, 129, 511, 512, 513, 1023, 1025, 1537, 3001)


def gamma(k):
    return k * U / (1.0 - k * U)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _T(m):
    return m.transpose(0, 2, 1)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def synthetic_h(rng, b):
    """float32 (B,3,3): H = A diag(s) B^T 10^e, A and B Haar, s = (1, U[0.6, 1], +-U[0.2, 0.4]), e in {-2 .. 2}.  The signed gap
    s2 + s3 sign(det H) is at least 0.2 s1 and about half the rows have det H < 0."""
    a, bb = _rotations(rng, b), _rotations(rng, b)
    s = np.stack([np.ones(b), rng.uniform(0.6, 1.0, b), rng.uniform(0.2, 0.4, b) * rng.choice([-1.0, 1.0], b)], 1)
    e = rng.integers(-2, 3, b).astype(np.float64)
    return np.ascontiguousarray(np.einsum("bij,bj,bkj->bik", a, s, bb) * (10.0 ** e)[:, None, None], dtype=np.float32)


_GAP = [None, None]


def signed_gap(h):
    """(s2 + s3 sign(det H), s1) from the float64 SVD; kept for the array it was last asked about (a batch's H serves several references)."""
    if _GAP[0] is not h:
        h64 = np.asarray(h, np.float64)
        s = np.linalg.svd(h64, compute_uv=False)
        _GAP[:] = [h, (s[:, 1] + s[:, 2] * np.sign(np.linalg.det(h64)), s[:, 0])]
    return _GAP[1]


def centroids(P, Q, w):
    """float32 (B,7): the float64 (pbar, qbar, W) of each cloud, rounded."""
    p, q = _f64(P), _f64(Q)
    ww = np.ones(p.shape[:2]) if w is None else _f64(w)
    W = ww.sum(1)
    st = np.concatenate([(ww[:, :, None] * p).sum(1) / W[:, None], (ww[:, :, None] * q).sum(1) / W[:, None], W[:, None]], 1)
    return np.ascontiguousarray(st, dtype=np.float32)


def bwd_inputs(b, n, seed, offset=0.0):
    """Everything the three backward entry points read, float32 numpy: make_batch's clouds and Haar R, a synthetic H, standard normal
    upstreams (G in the (B,N,3) layout, GT the same values as (B,3,N)), weights U[0.05, 1] and the stats with and without them."""
    d = make_batch(b, n, seed, offset=offset)
    rng = np.random.default_rng(seed + 7919)
    f = lambda *shape: np.ascontiguousarray(rng.standard_normal(shape), dtype=np.float32)          # noqa: E731
    out = {"P": d["P"], "Q": d["Q"], "R": d["Rgt"], "H": synthetic_h(rng, b), "gR": f(b, 3, 3), "gH": f(b, 3, 3), "gt": f(b, 3), "G": f(b, n, 3),
           "w": np.ascontiguousarray(rng.uniform(0.05, 1.0, (b, n)), dtype=np.float32)}
    out["GT"] = np.ascontiguousarray(out["G"].transpose(0, 2, 1))
    out["stats"], out["stats_w"] = centroids(out["P"], out["Q"], None), centroids(out["P"], out["Q"], out["w"])
    gap, s1 = signed_gap(out["H"])
    flipped = np.linalg.det(_f64(out["H"])) < 0
    assert (gap >= 0.19 * s1).all() and (b < 40 or (flipped.any() and not flipped.all()))          # det-flip rows are in every batch
    return out


# ---- float64 references -----------------------------------------------------------------------------------------------------------
def k2(h, g):
    with torch.no_grad():
        return ref.k2_64(_t(h), _t(g)).numpy()


def rotate_bwd_ref(P, R, G):
    """G in the (B,N,3) layout.  -> dP, dR and their bounds."""
    p, r, g = _f64(P), _f64(R), _f64(G)
    k = -(-p.shape[1] // 64) + 6
    return {"dP": g @ r, "dP_bound": gamma(3) * (np.abs(g) @ np.abs(r)),
            "dR": _T(g) @ p, "dR_bound": gamma(k) * (_T(np.abs(g)) @ np.abs(p))}


def kabsch_bwd_ref(P, Q, H, gR, gH, mutate=None):
    """gR / gH None: a null upstream.  -> dP, dQ, dH; with gR None the entrywise bounds, otherwise the per-point denominators."""
    p, q = _f64(P), _f64(Q)
    b = len(p)
    zero = np.zeros((b, 3, 3))
    gh = zero if gH is None else _f64(gH)
    out = {}
    if gR is None:
        dh = gh
        out["dQ_bound"] = gamma(3) * (np.abs(p) @ _T(np.abs(gh)))
        out["dP_bound"] = gamma(3) * (np.abs(q) @ np.abs(gh))
    else:
        dh = k2(H, gR) + gh
        gap, _ = signed_gap(H)
        F = np.linalg.norm(_f64(gR), axis=(1, 2)) / gap + np.linalg.norm(gh, axis=(1, 2))
        out["dQ_D"], out["dP_D"] = F[:, None] * np.linalg.norm(p, axis=2), F[:, None] * np.linalg.norm(q, axis=2)
    if mutate == "neighbour":
        dh = np.roll(dh, -1, axis=0)
    out["dH"] = dh
    out["dQ"] = p @ _T(dh)                                                  # dQ_i = dH p_i
    out["dP"] = q @ (dh if mutate != "untransposed" else _T(dh))            # dP_i = dH^T q_i
    return out


def rigid_bwd_ref(P, Q, w, H, R, stats, gR, gt, gH, mutate=None):
    """rigid_align_ref.grads64 with H, R and stats taken as given (every W > 0).  Null upstreams and weights are None.
    -> dP, dQ, dw and the per-point denominators."""
    p, q, r, st = _f64(P), _f64(Q), _f64(R), _f64(stats)
    b, n, _ = p.shape
    ww = np.ones((b, n)) if w is None else _f64(w)
    g_r = np.zeros((b, 3, 3)) if gR is None else _f64(gR)
    g_h = np.zeros((b, 3, 3)) if gH is None else _f64(gH)
    g_t = np.zeros((b, 3)) if gt is None else _f64(gt)
    pbar, qbar, W = st[:, :3], st[:, 3:6], st[:, 6]
    gp = g_r - (0.0 if mutate == "no_pbar_term" else 1.0) * g_t[:, :, None] * pbar[:, None, :]
    dh = g_h if (gR is None and gt is None) else k2(H, gp) + g_h
    u = np.einsum("bij,bi->bj", r, g_t) if mutate != "u_untransposed" else np.einsum("bij,bj->bi", r, g_t)
    gti, ui = g_t / W[:, None], u / W[:, None]
    if mutate == "previous_centroid":
        pbar, qbar = np.roll(pbar, 1, axis=0), np.roll(qbar, 1, axis=0)
    if mutate == "neighbour":
        dh, pbar, qbar, gti, ui = (np.roll(v, -1, axis=0) for v in (dh, pbar, qbar, gti, ui))
    a, c = p - pbar[:, None], q - qbar[:, None]
    dha = a @ _T(dh)
    dq = ww[:, :, None] * (dha + (0.0 if mutate == "no_gt_in_dq" else 1.0) * gti[:, None])
    dhc = c @ (dh if mutate != "untransposed" else _T(dh))
    dp = ww[:, :, None] * (dhc - ui[:, None])
    dw = (c * dha).sum(-1) + (0.0 if mutate == "no_inv_w_in_dw" else 1.0) * ((c * gti[:, None]).sum(-1) - (a * ui[:, None]).sum(-1))
    gap, _ = signed_gap(H)
    F = (np.linalg.norm(gp, axis=(1, 2)) / gap + np.linalg.norm(g_h, axis=(1, 2)))[:, None]
    na, nc, ng = np.linalg.norm(a, axis=2), np.linalg.norm(c, axis=2), (np.linalg.norm(g_t, axis=1) / W)[:, None]
    return {"dP": dp, "dQ": dq, "dw": dw, "dQ_D": ww * (F * na + ng), "dP_D": ww * (F * nc + ng), "dw_D": F * na * nc + ng * (na + nc)}


# ---- checkers ---------------------------------------------------------------------------------------------------------------------
def worst_ratio(err, bound):
    """max err / bound over every entry; an entry whose bound is 0 must have no error at all.  A NaN anywhere gives inf."""
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max())


def row_figure(got, want, D):
    """max over points of |got_i - want_i|_inf / D_i (rows of three, or scalars for dw)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    return worst_ratio(err.max(-1) if err.ndim == D.ndim + 1 else err, D)


def check_rotate_bwd(got, r, which=("dP", "dR")):
    fig = {}
    if "dP" in which:
        fig["rot_dP"] = worst_ratio(np.abs(got["dP"] - r["dP"]), r["dP_bound"])
    if "dR" in which:
        fig["rot_dR"] = worst_ratio(np.abs(got["dR"].reshape(-1, 3, 3) - r["dR"]), r["dR_bound"])
    return fig


def check_kabsch_bwd(got, r, which=("dP", "dQ")):
    fig = {}
    for k in which:
        if k + "_bound" in r:
            fig["kbH_" + k] = worst_ratio(np.abs(got[k] - r[k]), r[k + "_bound"])
        else:
            fig["kb_" + k] = row_figure(got[k], r[k], r[k + "_D"])
    return fig


def check_rigid_bwd(got, r, which=("dP", "dQ", "dw")):
    return {"ra_" + k: row_figure(got[k], r[k], r[k + "_D"]) for k in which}


def check_rigid_fwd(got, P, Q, w, tol):
    """so3_rigid_align_f32's (R, t, H, stats) for real clouds against rigid_align_ref in float64, every cloud.  H, the centroids, W, the
    rotation property and R pbar + t = qbar by test_rigid_align_host.figures; R by test_gpu_cloud_kernels.r_reference with the asserted
    bound on H, tol["H"] max(max |H|, 1e-3 W) per entry, in place of the dot product's.  A cloud with gap < 1e-3 s1 is left to the
    properties; `unjudged` is the number of those, which the caller caps.  N < 3: properties only."""
    import test_rigid_align_host as host
    b, n = P.shape[:2]
    want = ref.answers(P, Q, w)
    case = dict(want, b=b, n=n, check=ref.PROPERTIES)
    fig = host.figures(case, got, None, which=())
    hden = np.maximum(np.abs(want["H"]).reshape(b, -1).max(1), 1e-3 * want["stats"][:, 6])
    r_ref, rb, judged = r_reference(want["H"], tol["H"] * hden[:, None, None] * np.ones((1, 3, 3)))
    if n < 3:
        judged[:] = False
    fig["unjudged"] = float((~judged).sum())
    r_err = np.abs(got["R"] - r_ref).max(axis=(1, 2))
    fig["R/bound"] = worst_ratio(r_err[judged], rb[judged])
    return fig


# ---- float32 restatements ------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def wave_sum_model(x, y):
    """sum_i x_i y_i^T over axis 1 of float32 (B,N,3) arrays in the kernels' order: point i on lane i % 64, each lane adding its products
    by fma in index order, then the xor butterfly over the 64 lanes."""
    b, n, _ = x.shape
    trips = -(-n // 64) if n else 0
    pad = trips * 64 - n
    x = np.concatenate([x, np.zeros((b, pad, 3), np.float32)], 1).reshape(b, trips, 64, 3)
    y = np.concatenate([y, np.zeros((b, pad, 3), np.float32)], 1).reshape(b, trips, 64, 3)
    acc = np.zeros((b, 64, 3, 3), np.float32)
    for t in range(trips):
        acc = fma32(x[:, t, :, :, None], y[:, t, :, None, :], acc)
    lanes = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0]


def _mat_rows(m, v, transposed):
    """float32 (B,3,3) times (B,N,3) as the kernels chain it: fma(m2, z, fma(m1, y, m0 * x)) per output coordinate."""
    m = m.transpose(0, 2, 1) if transposed else m
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([fma32(m[:, c, 2, None], z, fma32(m[:, c, 1, None], y, m[:, c, 0, None] * x)) for c in range(3)], -1)


def rotate_bwd_model(P, R, G):
    return {"dP": _mat_rows(R, G, True), "dR": wave_sum_model(G, P)}


def kabsch_bwd_model(P, Q, H, gR, gH):
    from oracle import kernel_model
    dh = kernel_model.project_bwd(H, gR) if gR is not None else np.zeros((len(P), 3, 3), np.float32)
    if gH is not None:
        dh = dh + gH
    return {"dQ": _mat_rows(dh, P, False), "dP": _mat_rows(dh, Q, True)}


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def rigid_fwd_model(model, P, Q, w):
    """tests/host_model/rigid_align.cpp (the ctypes library `model`): the forward."""
    import ctypes
    b, n = P.shape[:2]
    P, Q, w = _c(P), _c(Q), _c(w)
    out = {"R": np.full((b, 3, 3), np.nan, np.float32), "t": np.full((b, 3), np.nan, np.float32), "H": np.full((b, 3, 3), np.nan, np.float32),
           "stats": np.full((b, 7), np.nan, np.float32)}
    model.model_rigid_align(np_ptr(P), np_ptr(Q), np_ptr(w), np_ptr(out["R"]), np_ptr(out["t"]), np_ptr(out["H"]), np_ptr(out["stats"]), ctypes.c_int64(b), ctypes.c_int32(n))
    return out


def rigid_bwd_model(model, P, Q, w, H, R, stats, gR, gt, gH):
    """tests/host_model/rigid_align.cpp: the backward, all three gradients."""
    import ctypes
    b, n = P.shape[:2]
    args = [_c(v) for v in (P, Q, w, H, R, stats, gR, gt, gH)]
    out = {"dP": np.full((b, n, 3), np.nan, np.float32), "dQ": np.full((b, n, 3), np.nan, np.float32), "dw": np.full((b, n), np.nan, np.float32)}
    model.model_rigid_align_bwd(*[np_ptr(v) for v in args], np_ptr(out["dP"]), np_ptr(out["dQ"]), np_ptr(out["dw"]), ctypes.c_int64(b), ctypes.c_int32(n))
    return out
