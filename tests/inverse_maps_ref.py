"""Shared by tests/test_inverse_maps_host.py, tests/test_gpu_inverse_maps.py and tests/test_gpu_inverse_maps_rows.py: the G18 fixture, a
float64 restatement of the inverse maps' definitions in torch (autograd gives the reference gradients), the tangent projection, the
error measures the files bound, and -- for the row-by-row tests -- the Euler maps' definition as the kernel documents it
(euler_def64, euler_grad_def64), the edge families (edge_rows) and the float64 answers of every map on G18 plus the edge rows (rows)."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_inverse_maps.npz")
PI32 = float(np.float32(np.pi))
EULER_MAX_MIDDLE = float(np.float32(1.57079625))     # csrc: kEulerMaxMiddle, the float32 below pi / 2
EULER_MIN_COS = 1e-6                                 # csrc: kEulerMinCos, the floor of cos(e2) in the Euler gradient
FLT_MIN = 2.0**-126                                  # float32's smallest normal: r0^2 + r2^2 below it (in float32) is gimbal lock


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


# ---- the Euler maps as the kernel documents them (csrc/so3_rows.h: OpMatToEuler), float64 -------------------------------------------
def _h32(r):
    """r0^2 + r2^2 as the kernel forms it in float32, fma(r2, r2, r0 * r0): the product rounded to float32, r2^2 exact in float64,
    the sum rounded once more (float64 first: a double rounding could move a tie by one ulp, and no row is judged that near
    FLT_MIN).  The rows are float32 numbers held in float64, so the cast back is exact."""
    a = r.detach().cpu().numpy()
    r0, r2 = a[:, 0].astype(np.float32), a[:, 2].astype(np.float64)
    with np.errstate(under="ignore", invalid="ignore"):
        return (r2 * r2 + (r0 * r0).astype(np.float64)).astype(np.float32)


def _euler_parts(R):
    """(s2, c2, s3, c3, lock).  GIMBAL LOCK is h = r0^2 + r2^2 below float32's smallest normal, h formed in float32 (false for a NaN
    row); there c2 = 0 and (s3, c3) = (0, 1).  Elsewhere c2 = |(r0, r2)| and (s3, c3) = (r2, r0) / c2."""
    r = R.reshape(-1, 9)
    lock = torch.as_tensor(_h32(r) < FLT_MIN, device=r.device)
    one, zero = torch.ones_like(r[:, 0]), torch.zeros_like(r[:, 0])
    c2 = torch.where(lock, zero, torch.where(lock, one, r[:, 0] ** 2 + r[:, 2] ** 2).sqrt())
    inv = 1 / torch.where(lock, one, c2)
    return torch.clamp(-r[:, 1], -1, 1), c2, torch.where(lock, zero, r[:, 2] * inv), torch.where(lock, one, r[:, 0] * inv), lock


def euler_def64(R):
    """e2 = atan2(s2, c2) clamped to +-kEulerMaxMiddle, e1 = atan2(s3, c3), e0 = atan2(s3 r3 - c3 r5, c3 r8 - s3 r6)."""
    r = R.reshape(-1, 9)
    s2, c2, s3, c3, _ = _euler_parts(R)
    e0 = torch.atan2(s3 * r[:, 3] - c3 * r[:, 5], c3 * r[:, 8] - s3 * r[:, 6])
    e2 = torch.clamp(torch.atan2(s2, c2), -EULER_MAX_MIDDLE, EULER_MAX_MIDDLE)
    return torch.stack([e0, torch.atan2(s3, c3), e2], 1)


def hat_gradient(R, w):
    """dR = 1/2 R hat(w): row i of R crossed with w / 2; (B,3,3), (B,3) -> (B,3,3)."""
    return torch.cross(R.reshape(-1, 3, 3), 0.5 * w[:, None, :].expand(-1, 3, -1), dim=2)


def euler_grad_def64(R, g, floor=EULER_MIN_COS):
    """p = (g0 + g1 s2) / max(c2, floor),  w = (c3 p - s3 g2, g1, s3 p + c3 g2),  dR = 1/2 R hat(w); at lock c2 = 0, (s3, c3) = (0, 1)."""
    s2, c2, s3, c3, _ = _euler_parts(R)
    p = (g[:, 0] + g[:, 1] * s2) / torch.clamp_min(c2, floor)
    return hat_gradient(R, torch.stack([c3 * p - s3 * g[:, 2], g[:, 1], s3 * p + c3 * g[:, 2]], 1))


def rel_grad_def64(R1, R2, g, branch=1.0):
    """The relative log's gradients in closed form at v = branch * log64(R1^T R2): w2 = g - 1/2 v x g + c v x (v x g),
    w1 = -(g + 1/2 v x g + c v x (v x g)), c = (1 - (theta / 2) cot(theta / 2)) / theta^2 (its series below theta = 1e-2);
    -> (dR1, dR2).  branch = -1 is the other side of the cut theta = pi, where log(D^T) = -log(D) fails."""
    v = branch * rel64(R1, R2)
    t2 = (v * v).sum(1, keepdim=True)
    th = torch.where(t2 > 1e-4, t2, torch.ones_like(t2)).sqrt()
    c = torch.where(t2 > 1e-4, (1 - 0.5 * th / torch.tan(0.5 * th)) / th ** 2, 1 / 12 + t2 / 720 + t2 * t2 / 30240)
    vg = torch.cross(v, g, dim=1)
    even = g + c * torch.cross(v, vg, dim=1)
    return hat_gradient(R1, -(even + 0.5 * vg)), hat_gradient(R2, even - 0.5 * vg)


# ---- the edge families ----------------------------------------------------------------------------------------------------------
EDGE_FAMILIES = ["euler_floor", "euler_underflow", "log_small", "rel_residual", "rel_cut"]
EULER_FLOOR_DELTAS = [1e-2, 1e-3, 3.5e-4, 1e-5, 1.01e-6, 0.99e-6, 1e-8, 1e-12, 1e-16]
EULER_UNDERFLOW_DELTAS = [1e-19, 1e-20, 1e-22, 1e-30]
LOG_SMALL_THETAS = [1e-30, 1e-20, 1e-12, 1e-9, 1e-7, 1e-5, 1e-3, 1e-2]
REL_RESIDUALS = [0.0, 1e-7, 1e-5, 1e-3, 1e-2]
REL_CUT_GAPS = [0.0, 1e-7, 1e-5, 1e-3]
EDGE_SEED = 1808


def _near_lock(e0, r0, r2, sign):
    """X(e0) Z(e2) Y(e1) with cos(e2) (cos e1, sin e1) = (r0, r2) given in float64 and sin(e2) = sign sqrt(1 - r0^2 - r2^2):
    oracle/so3_oracle.py's euler_torch on sines and cosines, so that c2 = 1e-30 is not lost in cos(pi / 2 - 1e-30)."""
    c2 = np.hypot(r0, r2)
    c3, s3 = (r0 / c2, r2 / c2) if c2 > 0 else (1.0, 0.0)
    s2 = sign * np.sqrt(1 - c2 * c2)
    c1, s1 = np.cos(e0), np.sin(e0)
    return [[r0, -s2, r2], [c1 * s2 * c3 + s1 * s3, c1 * c2, c1 * s2 * s3 - s1 * c3], [s1 * s2 * c3 - c1 * s3, s1 * c2, s1 * s2 * s3 + c1 * c3]]


def exp64(v):
    """Rodrigues in float64, (B,3) -> (B,3,3): I + (sin t / t) K + (2 sin^2(t / 2) / t^2) K^2, no cancellation at any t."""
    v = np.asarray(v, np.float64)
    t = np.linalg.norm(v, axis=1)
    safe = np.where(t > 0, t, 1.0)
    a = np.where(t > 0, np.sin(safe) / safe, 1.0)[:, None, None]
    b = np.where(t > 0, 2 * np.sin(0.5 * safe) ** 2 / safe ** 2, 0.5)[:, None, None]
    k = np.zeros((len(v), 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    return np.eye(3) + a * k + b * (k @ k)


def _axes(rng, n):
    """The three coordinate axes, both ways round, then random unit vectors: n in all."""
    a = rng.standard_normal((n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    a[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    return a


@functools.lru_cache(maxsize=None)
def edge_rows():
    """The rows G18 does not hold, built in float64 and rounded to float32: r (n,3,3), the second rotation r2 of the relative maps
    (n,3,3), g (n,4), family (index into EDGE_FAMILIES).  The rel_* families are pairs (r, r2) = (R1, R1 exp(.)); every other family's
    r2 is a rotation of G18's `random` family.  Every map runs on every row."""
    rng = np.random.default_rng(EDGE_SEED)
    d = g18()
    pool = d["r"][d["family"] == list(d["family_names"]).index("random")].astype(np.float64)
    dirs = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)] + [(np.cos(a), np.sin(a)) for a in (0.7, 2.3, -2.0, -0.4)]
    r, r2, fam = [], [], []

    def add(name, mats, seconds=None):
        mats = np.asarray(mats, np.float64).reshape(-1, 3, 3)
        r.append(mats)
        r2.append(pool[rng.integers(0, len(pool), len(mats))] if seconds is None else seconds)
        fam.append(np.full(len(mats), EDGE_FAMILIES.index(name)))

    for name, deltas in (("euler_floor", EULER_FLOOR_DELTAS + [0.0]), ("euler_underflow", EULER_UNDERFLOW_DELTAS)):
        add(name, [_near_lock(e0, dl * c, dl * s, sign) for dl in deltas for c, s in (dirs if dl > 0 else dirs[:1])
                   for sign in (1.0, -1.0) for e0 in rng.uniform(-np.pi, np.pi, 3 if dl > 0 else 8)])
    # r0 or r2 itself a float32 denormal (below 1.18e-38), the other component large, small, zero or denormal too
    add("euler_underflow", [_near_lock(e0, a, b, sign) for a, b in ((1e-40, 1e-10), (1e-10, -1e-40), (-1e-42, 1e-3), (1e-40, 0.0), (0.0, -1e-42), (1e-40, 1e-40))
                            for sign in (1.0, -1.0) for e0 in rng.uniform(-np.pi, np.pi, 2)])
    add("log_small", np.concatenate([exp64(t * _axes(rng, 30)) for t in LOG_SMALL_THETAS]))
    for name, vs in (("rel_residual", [t * _axes(rng, 50) for t in REL_RESIDUALS]), ("rel_cut", [(np.pi - gap) * _axes(rng, 60) for gap in REL_CUT_GAPS])):
        first = pool[rng.integers(0, len(pool), sum(len(v) for v in vs))]
        add(name, first, first @ exp64(np.concatenate(vs)))
    r, r2 = np.concatenate(r).astype(np.float32), np.concatenate(r2).astype(np.float32)
    return dict(r=r, r2=r2, g=rng.standard_normal((len(r), 4)).astype(np.float32), family=np.concatenate(fam))


@functools.lru_cache(maxsize=None)
def rows():
    """G18 and the edge rows as one table, with the float64 answer of every map on the SAME float32 rows -- computed once, gathered by
    index wherever a test tiles the table, never recomputed.  r, r2 (n,9) float32, g (n,4) float32 (G18's own g, the edge rows'
    seeded one), fam / names, and `want`: value of each map and the tangent-space gradient of each map under g, float64."""
    d, e = g18(), edge_rows()
    names = [str(s) for s in d["family_names"]] + EDGE_FAMILIES
    r = np.concatenate([d["r"], e["r"]]).reshape(-1, 9)
    r2 = np.concatenate([d["r"][d["perm"]], e["r2"]]).reshape(-1, 9)
    g = np.concatenate([d["g"].astype(np.float32), e["g"]])
    fam = np.concatenate([d["family"].astype(np.int64), len(d["family_names"]) + e["family"]])
    t, t2 = (torch.as_tensor(a.astype(np.float64)) for a in (r.reshape(-1, 3, 3), r2.reshape(-1, 3, 3)))
    want = dict(quat=quat64(t), log=log64(t), euler=euler_def64(t), rel=rel64(t, t2))
    want["rel_other"] = -want["rel"]
    want = {k: v.numpy().reshape(len(r), -1) for k, v in want.items()}
    want.update(_gradients(r, r2, g))
    return dict(r=r, r2=r2, g=g, fam=fam, names=names, want=want)


def _gradients(r, r2, g):
    """The float64 tangent-space gradient of every map under g (n,4), on both branches for the relative maps."""
    t, t2, g4 = (torch.as_tensor(a.astype(np.float64)) for a in (r.reshape(-1, 3, 3), r2.reshape(-1, 3, 3), g))
    g3 = g4[:, :3]
    want = dict(euler_grad=euler_grad_def64(t, g3))
    (want["quat_grad"],) = autograd_tangent_t(quat64, g4, t)
    (want["log_grad"],) = autograd_tangent_t(log64, g3, t)
    want["rel_grad1"], want["rel_grad2"] = autograd_tangent_t(rel64, g3, t, t2)
    want["rel_grad1_other"], want["rel_grad2_other"] = rel_grad_def64(t, t2, g3, -1.0)
    return {k: v.numpy().reshape(len(r), -1) for k, v in want.items()}


G_DRAWS = 8


@functools.lru_cache(maxsize=None)
def redrawn(k):
    """rows() under another seeded g, draw k = 1 .. G_DRAWS (draw 0 is rows() itself): the same rows and values, the gradients' answers
    for that g.  A family's largest gradient error depends on g as much as on the row -- theta_pi_coordinate_axis has three rows -- so the
    host figures behind the bounds are taken over all the draws; the GPU tests run draw 0."""
    if k == 0:
        return rows()
    t = dict(rows())
    t["g"] = np.random.default_rng([EDGE_SEED, k]).standard_normal(t["g"].shape).astype(np.float32)
    t["want"] = dict(t["want"], **_gradients(t["r"], t["r2"], t["g"]))
    return t


# ---- the row-by-row error measures ------------------------------------------------------------------------------------------------
RELATIVE_FAMILIES = ("theta_small", "log_small")      # rotation vectors of 1e-30 .. 1e-2: an absolute bound sized at theta = pi says nothing


def value_error(got, want, circle=()):
    """max |got - want| per row; the columns in `circle` are angles, compared modulo 2 pi (-pi and pi are one angle)."""
    dlt = np.abs(np.asarray(got, np.float64).reshape(want.shape) - want)
    for c in circle:
        dlt[:, c] = np.minimum(dlt[:, c], np.abs(2 * np.pi - dlt[:, c]))
    return dlt.max(1)


def relative_value_error(got, want):
    """max |got - want| / max |want| per row; a row whose answer is exactly 0 must be exactly 0 (error 0), and is inf otherwise."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    num, den = np.abs(got - want).max(1), np.abs(want).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


CUT_BAND = 1e-6


def on_cut(table):
    """Rows of the relative maps ON the cut theta = pi: pi - |log64(R1^T R2)| < CUT_BAND.  The kernel forms D = R1^T R2 in float32;
    each entry carries up to 3 x 2^-24 of rounding, the antisymmetric part (a difference of two entries) up to 3.6e-7, and its sign --
    2 sin(theta) times the axis -- picks the side of the cut.  Where 2 (pi - theta) is below that, no float64 evaluation on the inputs
    says which side float32 lands on: both are the definition's answer to the precision of D, and such a row is held to the NEARER of
    the float64 answers at v and at -v, value and gradients alike.  The band is a few times 1.8e-7; the table's rows are within
    3e-7 of the cut or at least 1e-5 from it."""
    return np.pi - np.linalg.norm(table["want"]["rel"], axis=1) < CUT_BAND


def cut_branch(check, got, table, index=None):
    """For the rows on the cut: True where `got` is nearer the float64 answer at -v than the one at v."""
    pick = (lambda a: a) if index is None else (lambda a: a[index])
    measure = value_error if check == "rel" else rel_grad_error
    return pick(on_cut(table)) & (measure(got, pick(table["want"][check + "_other"])) < measure(got, pick(table["want"][check])))


CHECKS = ("quat", "log", "euler", "rel", "quat_grad", "log_grad", "euler_grad", "rel_grad1", "rel_grad2")


def row_error(check, got, table, index=None):
    """The figure of every row for one check of rows()' table (`index`: the rows of the table that `got` holds, in order).  Values
    are max |difference| (Euler's e0 and e1 modulo 2 pi); the log map's value on RELATIVE_FAMILIES is relative to the answer;
    gradients are max |difference| over max(1, max |answer|) of the row."""
    pick = (lambda a: a) if index is None else (lambda a: a[index])
    want = pick(table["want"][check])
    if check.startswith("rel"):
        measure = value_error if check == "rel" else rel_grad_error
        e = measure(got, want)
        return np.where(pick(on_cut(table)), np.minimum(e, measure(got, pick(table["want"][check + "_other"]))), e)
    if check.endswith("_grad"):
        return rel_grad_error(got, want)
    if check == "log":
        fam = table["fam"] if index is None else table["fam"][index]
        relative = np.isin(fam, [table["names"].index(n) for n in RELATIVE_FAMILIES])
        return np.where(relative, relative_value_error(got, want), value_error(got, want))
    return value_error(got, want, circle=(0, 1) if check == "euler" else ())


def row_bound(check, bounds, table, index=None):
    """The bound of every row: its family's entry of bounds[check] (tests/test_inverse_maps_host.py: ROW_TOL)."""
    per_family = np.array([bounds[check][n] for n in table["names"]])
    return per_family[table["fam"] if index is None else table["fam"][index]]
