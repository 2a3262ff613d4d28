"""Shared by tests/test_add_metrics_host.py, tests/test_gpu_add_metrics.py and tools/gen_golden.py (G19): the ADD / ADD-S / diameter
definitions restated in float64 torch, their closed-form gradients with respect to the estimated pose, the formulations autograd is
taken through, and the fixture's layout.

Notation: x_i = R_gt p_i + t_gt, y_j = R_pred p_j + t_pred, T = [R t; 0 0 0 1].
  ADD_b  = (1/N) sum_i |x_i - y_i|              ADDS_b = (1/N) sum_i min_j |x_i - y_j|   (outer sum over the TRUE pose)
  nearest[b,i] = the first argmin j             diam_b = max_ij |p_i - p_j|
Gradients w.r.t. T_pred, with u_i = e_i / |e_i| (0 where e_i = 0):
  ADD:   e_i = x_i - y_i,          dR = -(1/N) sum u_i p_i^T,          dt = -(1/N) sum u_i
  ADD-S: e_i = x_i - y_nearest(i), dR = -(1/N) sum u_i p_nearest(i)^T, dt = -(1/N) sum u_i      (bottom row of dT = 0)"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_add_metrics.npz")
SIZES = (1, 3, 64, 100, 256, 1000)
FAMILIES = ("haar", "small_error", "identical", "twofold", "collinear", "duplicated")


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def pose64(T, P):
    """(B,4,4), (B,N,3) -> (B,N,3): R p + t."""
    return P @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]


def add64(Tg, Tp, P):
    return (pose64(Tg, P) - pose64(Tp, P)).norm(dim=-1).mean(-1)


def adds_parts64(Tg, Tp, P):
    """per-point nearest distance (B,N), first-argmin index (B,N), from coordinate differences."""
    x, y = pose64(Tg, P), pose64(Tp, P)
    d2 = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    return d2.min(-1).values.sqrt(), torch.as_tensor(np.argmin(d2.detach().numpy(), axis=-1))      # numpy: the FIRST minimum


def adds64(Tg, Tp, P):
    return adds_parts64(Tg, Tp, P)[0].mean(-1)


def adds_through_indices64(Tg, Tp, P, idx):
    """(1/N) sum_i |x_i - y_idx(i)|: what the gradient check differentiates, with the indices the code under test returned."""
    x, y = pose64(Tg, P), pose64(Tp, P)
    ysel = torch.gather(y, 1, torch.as_tensor(np.asarray(idx), dtype=torch.int64)[:, :, None].expand(-1, -1, 3))
    return torch.linalg.vector_norm(x - ysel, dim=-1).mean(-1)


def adds_cdist64(Tg, Tp, P):
    return torch.cdist(pose64(Tg, P), pose64(Tp, P)).min(-1).values.mean(-1)


def diameter64(P):
    return ((P[:, :, None, :] - P[:, None, :, :]) ** 2).sum(-1).flatten(1).max(-1).values.sqrt()


def _closed_form(e, q):
    """dT (B,4,4) from residuals e (B,N,3) and the inner model points q (B,N,3) they were formed with."""
    n = e.shape[1]
    nrm = e.norm(dim=-1, keepdim=True)
    u = torch.where(nrm > 0, e / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(e))
    dT = torch.zeros((e.shape[0], 4, 4), dtype=torch.float64)
    dT[:, :3, :3] = -(u.transpose(1, 2) @ q) / n
    dT[:, :3, 3] = -u.sum(1) / n
    return dT


def grad_add64(Tg, Tp, P):
    return _closed_form(pose64(Tg, P) - pose64(Tp, P), P)


def grad_adds64(Tg, Tp, P, idx):
    g = torch.as_tensor(np.asarray(idx), dtype=torch.int64)[:, :, None].expand(-1, -1, 3)
    q = torch.gather(P, 1, g)
    return _closed_form(pose64(Tg, P) - torch.gather(pose64(Tp, P), 1, g), q)


def autograd_wrt_pred(fn, Tg, Tp, P, *extra):
    """d(sum_b fn_b)/dT_pred by float64 autograd: rows are independent, so this is each row's own gradient."""
    tp = Tp.clone().requires_grad_(True)
    fn(Tg, tp, P, *extra).sum().backward()
    return tp.grad


def answers(tgt, tpred, pts):
    """Every float64 answer of one case from its float32 inputs (numpy in, numpy out)."""
    Tg, Tp, P = _t(tgt), _t(tpred), _t(pts)
    pd, nn = adds_parts64(Tg, Tp, P)
    return {"add": add64(Tg, Tp, P).numpy(), "adds": pd.mean(-1).numpy(), "point_dist": pd.numpy(), "nearest": nn.numpy().astype(np.int32),
            "diam": diameter64(P).numpy(), "grad_add": grad_add64(Tg, Tp, P).numpy(), "grad_adds": grad_adds64(Tg, Tp, P, nn).numpy()}


# ---- the fixture: cases of (family, N, B) stored back to back -----------------------------------------------------------------
PER_CLOUD = ("tgt", "tpred", "add", "adds", "diam", "grad_add", "grad_adds")
PER_POINT = ("pts", "point_dist", "nearest")


def g19():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def cases(d):
    """The fixture's cases as dicts: family (str), n, b, and every array sliced and shaped (B,...) / (B,N,...)."""
    out = []
    c0 = p0 = 0
    names = [str(s) for s in d["family_names"]]
    for fam, n, b in zip(d["case_family"], d["case_n"], d["case_b"]):
        n, b = int(n), int(b)
        case = {"family": names[int(fam)], "n": n, "b": b}
        for k in PER_CLOUD:
            case[k] = d[k][c0:c0 + b]
        for k in PER_POINT:
            a = d[k][p0:p0 + b * n]
            case[k] = a.reshape((b, n) + a.shape[1:])
        out.append(case)
        c0 += b
        p0 += b * n
    assert c0 == len(d["tgt"]) and p0 == len(d["pts"])
    return out


def index_excess(case, idx):
    """For every point: the float64 distance to the returned neighbour minus the float64 minimum (>= 0; bounded by the per-point
    tolerance -- near-ties may legitimately resolve differently in float32)."""
    x, y = pose64(_t(case["tgt"]), _t(case["pts"])), pose64(_t(case["tpred"]), _t(case["pts"]))
    g = torch.as_tensor(np.asarray(idx), dtype=torch.int64)[:, :, None].expand(-1, -1, 3)
    return ((x - torch.gather(y, 1, g)).norm(dim=-1) - _t(case["point_dist"])).numpy()
