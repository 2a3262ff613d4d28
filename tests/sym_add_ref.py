"""Shared by tests/test_sym_add_host.py, tests/test_gpu_sym_add.py and tools/gen_golden.py (G26): so3_sym_add_f32's definition
(include/so3proj.h) restated in float64 numpy, the selected branch's gradient in closed form and through float64 autograd, and the
fixture's layout.

Notation: T = [R t; 0 0 0 1], the class's table S_0 = I, S_1, ..., S_{K-1}; candidate k poses the cloud with T_pred S_k:
  d_i^k = (R_gt - R_pred S_k) p_i + (t_gt - t_pred)
  L2:  stat_k = (1/N) sum_i |d_i^k|_2        L1:  stat_k = (1/3N) sum_i |d_i^k|_1        MAX (MSSD):  stat_k = max_i |d_i^k|_2
  dist = min_k stat_k,  index = the smallest k attaining it
Gradient of candidate k w.r.t. T_pred, u_i = d_i / |d_i| (0 at d_i = 0) for L2, sgn(d_i) for L1, c = 1/N or 1/(3N):
  dR_pred = -c (sum_i u_i p_i^T) S_k^T,   dt_pred = -c sum_i u_i,   bottom row 0."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_sym_add.npz")
L2, L1, MAX = 0, 1, 2                              # include/so3proj.h: SO3_SYM_ADD_L2, SO3_SYM_ADD_L1, SO3_SYM_ADD_MAX
MODES = {"l2": L2, "l1": L1, "max": MAX}
FAMILIES = ("haar", "near_symmetric", "exact_c4", "identical_points")
PER_CASE = ("tgt", "tpred", "pts", "S", "cls", "stat_l2", "stat_l1", "stat_max", "grad_l2", "grad_l1")


def rows_of(S, cls, b):
    """(B,K,3,3) float64: each row's candidates.  S: (C,K,3,3); cls: (B,) ints or None (one class).  A class id out of range reads class 0
    (its results are overwritten by NaN / -1: `bad_rows`)."""
    S = np.asarray(S, np.float64)
    if cls is None:
        return np.broadcast_to(S[0], (b,) + S.shape[1:])
    cls = np.asarray(cls, np.int64)
    return S[np.where((cls < 0) | (cls >= S.shape[0]), 0, cls)]


def bad_rows(S, cls, b):
    if cls is None:
        return np.zeros(b, bool)
    cls = np.asarray(cls, np.int64)
    return (cls < 0) | (cls >= np.asarray(S).shape[0])


def residuals(tgt, tpred, pts, srows):
    """(B,K,N,3) float64 residuals of every candidate."""
    tg, tp, p = (np.asarray(a, np.float64) for a in (tgt, tpred, pts))
    a = np.einsum("bil,bklj->bkij", tp[:, :3, :3], srows)
    d = tg[:, None, :3, :3] - a
    return np.einsum("bkij,bnj->bkni", d, p) + (tg[:, :3, 3] - tp[:, :3, 3])[:, None, None, :]


def stat_of(mode, d):
    """The statistic over the point axis (-2) of residuals d (..., N, 3)."""
    if mode == L1:
        return np.abs(d).sum(-1).mean(-1) / 3.0
    nrm = np.sqrt((d * d).sum(-1))
    return nrm.max(-1) if mode == MAX else nrm.mean(-1)


def stats(tgt, tpred, pts, srows, chunk=16):
    """{mode: (B,K) float64} for the three modes, in slices of the batch."""
    out = {m: [] for m in (L2, L1, MAX)}
    for lo in range(0, len(tgt), chunk):
        sl = slice(lo, lo + chunk)
        d = residuals(tgt[sl], tpred[sl], pts[sl], srows[sl])
        for m in out:
            out[m].append(stat_of(m, d))
    return {m: np.concatenate(v) for m, v in out.items()}


def grad_closed_form(mode, tgt, tpred, pts, srows, index):
    """(B,4,4) float64: d stat_index / d T_pred."""
    b, n = len(tgt), pts.shape[1]
    p = np.asarray(pts, np.float64)
    s = srows[np.arange(b), index]                                        # (B,3,3)
    d = residuals(tgt, tpred, pts, s[:, None])[:, 0]                      # (B,N,3)
    if mode == L1:
        u, c = np.sign(d), 1.0 / (3.0 * n)
    else:
        nrm = np.sqrt((d * d).sum(-1, keepdims=True))
        u, c = np.where(nrm > 0, d / np.where(nrm > 0, nrm, 1.0), 0.0), 1.0 / n
    out = np.zeros((b, 4, 4))
    out[:, :3, :3] = -c * np.einsum("bil,bjl->bij", np.einsum("bni,bnl->bil", u, p), s)
    out[:, :3, 3] = -c * u.sum(1)
    return out


def grad_autograd(mode, tgt, tpred, pts, srows, index):
    """The same by float64 autograd through candidate `index` (rows are independent: the gradient of the sum is each row's own)."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    b = len(tgt)
    tg, p, s = t(tgt), t(pts), t(srows[np.arange(b), index])
    tp = t(tpred).clone().requires_grad_(True)
    d = p @ (tg[:, :3, :3] - tp[:, :3, :3] @ s).transpose(1, 2) + (tg[:, :3, 3] - tp[:, :3, 3])[:, None, :]
    stat = d.abs().sum(-1).mean(-1) / 3.0 if mode == L1 else torch.linalg.vector_norm(d, dim=-1).mean(-1)
    stat.sum().backward()
    return tp.grad.numpy()


def answers(tgt, tpred, pts, S, cls):
    """Every float64 answer of one case from its float32 inputs: the (B,K) statistics of the three modes and, for L2 and L1, the gradient
    of the float64 winner."""
    srows = rows_of(S, cls, len(tgt))
    st = stats(tgt, tpred, pts, srows)
    out = {"stat_l2": st[L2], "stat_l1": st[L1], "stat_max": st[MAX]}
    for name, m in (("grad_l2", L2), ("grad_l1", L1)):
        out[name] = grad_closed_form(m, tgt, tpred, pts, srows, np.argmin(st[m], axis=1))
    return out


def excess(stat_all, got_dist, got_index):
    """(|dist - the float64 minimum|, the float64 statistic at the returned index minus the float64 minimum >= 0), each the largest over the rows."""
    best = stat_all.min(1)
    at = stat_all[np.arange(len(best)), got_index]
    return float(np.abs(got_dist - best).max()), float((at - best).max())


# ---- the fixture: one group of arrays per case, "<i>_<name>" ----------------------------------------------------------------------
def g26():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def cases(d):
    """The fixture's cases as dicts: family (str), b, n, K, C, cls (None for a one-class table) and PER_CASE's arrays."""
    names = [str(s) for s in d["family_names"]]
    out = []
    for i, fam in enumerate(d["case_family"]):
        c = {k: d["%d_%s" % (i, k)] for k in PER_CASE}
        c["family"] = names[int(fam)]
        c["b"], c["n"] = int(c["pts"].shape[0]), int(c["pts"].shape[1])
        c["C"], c["K"] = int(c["S"].shape[0]), int(c["S"].shape[1])
        if c["C"] == 1:
            c["cls"] = None
        out.append(c)
    return out
