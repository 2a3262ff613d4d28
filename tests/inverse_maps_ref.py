"""Shared by tests/test_inverse_maps_host.py and tests/test_gpu_inverse_maps.py: the G18 fixture, a float64 restatement of the inverse
maps' definitions in torch (autograd gives the reference gradients), the tangent projection, and the error measures both files bound."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_inverse_maps.npz")
PI32 = float(np.float32(np.pi))


def g18():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


# ---- the definitions, float64 torch -----------------------------------------------------------------------------------------
def quat64(R):
    """Shepperd on the largest of (tr, r0, r4, r8), normalised, w >= 0; (B,3,3) -> (B,4) (w,x,y,z)."""
    r = R.reshape(-1, 9)
    tr = r[:, 0] + r[:, 4] + r[:, 8]
    k = torch.stack([tr, r[:, 0], r[:, 4], r[:, 8]], 1).argmax(1)
    a0, a1, a2 = r[:, 7] - r[:, 5], r[:, 2] - r[:, 6], r[:, 3] - r[:, 1]
    s01, s02, s12 = r[:, 1] + r[:, 3], r[:, 2] + r[:, 6], r[:, 5] + r[:, 7]
    cand = torch.stack([torch.stack([1 + tr, a0, a1, a2], 1),
                        torch.stack([a0, 1 + r[:, 0] - r[:, 4] - r[:, 8], s01, s02], 1),
                        torch.stack([a1, s01, 1 - r[:, 0] + r[:, 4] - r[:, 8], s12], 1),
                        torch.stack([a2, s02, s12, 1 - r[:, 0] - r[:, 4] + r[:, 8]], 1)], 1)
    t = cand[torch.arange(len(k), device=k.device), k]
    q = t / t.norm(dim=1, keepdim=True)
    return torch.where(q[:, :1] < 0, -q, q)


def log64(R):
    q = quat64(R)
    n2 = (q[:, 1:] ** 2).sum(1, keepdim=True)
    zero = n2 == 0                                   # theta = 0: theta / n -> 2 / w (and autograd must not meet 0 / 0)
    n = torch.where(zero, torch.ones_like(n2), n2).sqrt()
    theta = 2 * torch.atan2(n, q[:, :1])
    return torch.where(zero, 2 / torch.where(zero, q[:, :1], torch.ones_like(n2)), theta / n) * q[:, 1:]


def euler64(R):
    r = R.reshape(-1, 9)
    e2 = torch.asin(torch.clamp(-r[:, 1], -1, 1))
    e1 = torch.atan2(r[:, 2], r[:, 0])
    s3, c3 = torch.sin(e1), torch.cos(e1)
    e0 = torch.atan2(s3 * r[:, 3] - c3 * r[:, 5], c3 * r[:, 8] - s3 * r[:, 6])
    return torch.stack([e0, e1, e2], 1)


def rel64(R1, R2):
    return log64(R1.transpose(1, 2) @ R2)


def tangent(R, G):
    """R skew(R^T G): the tangent projection of an off-manifold gradient."""
    a = R.transpose(1, 2) @ G
    return R @ (0.5 * (a - a.transpose(1, 2)))


def autograd_tangent(fn, g, *rs):
    """Tangent-projected float64 autograd gradients of <g, fn(*rs)> with respect to every rotation in rs ((B,3,3) float64 arrays)."""
    xs = [torch.as_tensor(np.asarray(r, np.float64).reshape(-1, 3, 3)).clone().requires_grad_(True) for r in rs]
    (fn(*xs) * torch.as_tensor(np.asarray(g, np.float64))).sum().backward()
    return [tangent(x.detach(), x.grad).numpy() for x in xs]


def autograd_tangent_t(fn, g, *rs):
    """The same on torch tensors of any device: float64 tangent-projected gradients, as (B,3,3) tensors."""
    xs = [r.detach().double().reshape(-1, 3, 3).clone().requires_grad_(True) for r in rs]
    (fn(*xs) * g.detach().double()).sum().backward()
    return [tangent(x.detach(), x.grad) for x in xs]


# ---- masks and error measures -------------------------------------------------------------------------------------------
def exemptions(d):
    """Rows whose value is compared up to sign (quaternion, rotation vector) or through closure only (Euler)."""
    theta = np.linalg.norm(d["rotvec"], axis=1)
    return {"quat": np.abs(d["quat"][:, 0]) < 1e-3, "rotvec": np.pi - theta < 1e-3,
            "euler": np.abs(np.abs(d["euler"][:, 2]) - np.pi / 2) < 1e-2}


def up_to_sign_error(got, want, free):
    """max |got - want| per row; rows in `free` take the better of the two signs."""
    got = np.asarray(got, np.float64)
    e = np.abs(got - want).max(1)
    return np.where(free, np.minimum(e, np.abs(got + want).max(1)), e)


def angle_wrap_error(got, want):
    """Euler triples: differences modulo 2 pi (e0, e1 are angles on a circle)."""
    dlt = np.asarray(got, np.float64) - want
    return np.abs((dlt + np.pi) % (2 * np.pi) - np.pi).max(1)


def rel_grad_error(got, want):
    """max |got - want| per row over max(1, max |want|) of the row: relative where the gradient is large (Euler's 1 / c2)."""
    got = np.asarray(got, np.float64).reshape(len(want), -1)
    want = want.reshape(len(want), -1)
    return np.abs(got - want).max(1) / np.maximum(1.0, np.abs(want).max(1))
