"""Edge families for the forward rotation heads (so3_quat_*, so3_euler_*, so3_ortho5d_*, so3_expmap_*, so3_ortho6d_*, so3_se3_update_*,
so3_rotations_axis_angle_f32), their float64 answers and the bounds every row is judged by.  No GPU: tests/test_heads_host.py runs the
float32 host model of the very templates on these rows, tests/test_gpu_heads.py the kernels on tilings of them (answers gathered).

Everything is built once from SEED.  data(op) holds, for the op's families one after the other: the float32 input `x` (se3_update: `x` is
the network output (n,12) and `t` is T_init (n,16)), the float64 forward answer `r64` ON THE FLOAT32-ROUNDED INPUT, a fixed upstream `g`,
the float64 gradient `dx64` (oracle/so3_oracle.py: head_backward_np, ortho6d_backward_np, se3_update_backward_np), and per row:

    cond    the forward condition number:  1 (quat, euler);  max(1, t), t = |v| (expmap);  1 / sin of the angle between the two
            Gram-Schmidt vectors in float64 (6D: the two halves; 5D: the un-projected pair x_raw, y_raw);  s1 / gap (se3 update);
    gunit   the unit of each gradient component.  The issue states the backward bound as C u |G|_1 cond.  That cannot hold for a head
            that does not depend on its input's scale: its gradient is homogeneous of degree -1 in the input (at |q| = 1e-9 it is
            1e8 |G|, and the float32 rounding of the answer alone is 1e8 u |G|).  The bound is therefore stated in the gradient's
            natural unit -- an explicit function of the INPUT, never of the gradient under test or of its reference value:
                quat     1 / max(|q|, 1e-8)
                6D       1 / (|a| sin) for d/da,  1 / (|b| sin) for d/db: z = w / |w| with |w| = |b| sin, so the Jacobian itself is of
                         that size and its float32 error is u cond RELATIVE to it.  (With 1 / |a|, 1 / |b| alone the host model needs
                         C = 0.2 / sin on the nearly parallel families: 203 at sine 1e-3, 18117 at 1e-5 -- the finding, not a constant.)
                5D       1 / |x_raw| for d/da[0:2];  k (1 / |v| + (s + 1) / (2 s |x_raw|)) for d/da[2:5]  (v = a[2:5] * scale, s = |v|^2,
                         k = 1 + sqrt 2).  This is the chain rule on the head's DEFINITION, not a reading of the kernel: the head is the
                         6D head of (x_raw, y_raw) with x_raw = (a0, a1, (s - 1) / (2 |v|)) and y_raw = v / |v|.  The 6D head's Jacobian
                         is of size 1 / (|first| sin) in its first vector and 1 / (|second| sin) in its second (above; sin is `cond`),
                         |y_raw| = 1;  d y_raw / dv = (I - y y^T) / |v| has norm 1 / |v|;  d x_raw.z / dv = v (s + 1) / (2 s |v|) has
                         norm (s + 1) / (2 s);  v = a[2:5] * scale contributes at most k.  Summing the two paths gives the unit.
                euler, expmap   1
            It stays absolute in the issue's sense: a gradient that cancels to nothing (the exp map at 2 pi) is still judged by
            u |G|_1 cond gunit, not by its own size.

BOUNDS (u = 2^-24, every row, no quantiles):
    forward    max_ij |R - R64|            <=  C_FWD[op] u cond
    backward   max_k |dx_k - dx64_k| / gunit_k  <=  C_BWD[op] u |G|_1 cond
    se3 update: the rotation block max |.| gap / s1-scaled as test_g8 does (rows with gap < SE3_MIN_GAP have no defined rotation: their
    block is judged for being a rotation only), the translation column relative to max(1, |t|); backward with the scaling of
    tests/test_kernel_model.py (min(1, s1 gap^2) / max(1, max |dref|)).
    The one exclusion is the exp map's kink: a row with | |v|^2 - 1e-4 | <= 4 u 1e-4 may take the clamp's other side in float32, and
    passes if its gradient matches the float64 gradient of either side (`dx64_alt`).  Only the `straddle` family has such rows
    (asserted below).

C = 4 x the largest figure the float32 host model (oracle/kernel_model.cpp, libm's correctly rounded sqrt and division) reaches on
these families; the margin covers the device's 1-ulp v_rsq_f32 / v_rcp_f32 / v_sqrt_f32 and its fma contraction.  The measured value
stands beside each constant (tests/test_heads_host.py prints and re-asserts them).  No C may exceed 64.

OUTSIDE THE RANGE (outside(op)): rows whose squared norm underflows to 0 or overflows to inf in float32.  What the kernels return
there is pinned as it is (include/so3proj.h, "input range of the heads"): NaN in fixed slots (5D), or the identity for an overflowing
quaternion -- in that row only.  The 6D head has no such rows: it prescales its halves (so3_rows.h: pow2_prescaled).
"""
import functools
import math

import numpy as np
import torch

from oracle import so3_oracle as so

U = 2.0**-24
SEED = 23
ROWS = 128                                   # rows per family
FX = FY = 50 / (36 / 320)
QUAT_MIN_NORM = so.QUAT_MIN_NORM             # float32(1e-8), as the reference's FloatTensor([1e-8]) and the kernel's 1e-8f
EXPMAP_EPS = 1e-4
KINK_BAND = 4 * U * EXPMAP_EPS               # | |v|^2 - 1e-4 | within it: either side of the clamp
SE3_MIN_GAP = 1e-4                           # below it float32 cannot tell s2 from -+s3: the rotation is not defined

#                  measured on the host model        bound (4 x)
# (on the MI355X, all sizes of tests/test_gpu_heads.py: forward 10.09 / 2.03 / 3.60 / 2.79 / 3.63 / 11.98, backward 5.34 / 1.06 / 1.89 / 1.20 / 6.08 / 7.50,
#  sampler 3.92, in the order of the dictionaries below)
HOST_FWD = {"quat": 8.65, "euler": 1.80, "expmap": 3.61, "ortho6d": 3.11, "ortho5d": 3.63, "se3_update": 10.67}
HOST_BWD = {"quat": 5.86, "euler": 1.06, "expmap": 1.77, "ortho6d": 1.55, "ortho5d": 7.10, "se3_update": 7.51}
HOST_SAMPLER = 3.66                          # the float32 restatement sampler_f32() below (the sampler is not a row operation)
C_FWD = {k: 4 * v for k, v in HOST_FWD.items()}
C_BWD = {k: 4 * v for k, v in HOST_BWD.items()}
C_SAMPLER = 4 * HOST_SAMPLER
assert max(max(C_FWD.values()), max(C_BWD.values()), C_SAMPLER) <= 64

WIDTH = {"quat": 4, "euler": 3, "ortho5d": 5, "expmap": 3, "ortho6d": 6, "se3_update": 12}
OUT_WIDTH = {"quat": 9, "euler": 9, "ortho5d": 9, "expmap": 9, "ortho6d": 9, "se3_update": 16}
OPS = tuple(WIDTH)
K0, K2 = math.sqrt(2.0) + 1.0, math.sqrt(2.0)


def _unit(rng, n, k):
    v = rng.standard_normal((n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rot(rng, n):
    return so.symmetric_orthogonalization_np(rng.standard_normal((n, 9)))


def _sin_between(a, b):
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


# ---- the families ---------------------------------------------------------------------------------------------------------------
def _quat_families(rng):
    fams = {}
    for label, s in (("zero", 0.0), ("1e-25", 1e-25), ("1e-9", 1e-9), ("0.99e-8", 0.99e-8), ("1.01e-8", 1.01e-8), ("1e-6", 1e-6), ("one", 1.0),
                     ("1e10", 1e10), ("1e18", 1e18)):
        fams[label] = _unit(rng, ROWS, 4) * s
    one = np.zeros((ROWS, 4))
    one[np.arange(ROWS), np.arange(ROWS) % 4] = np.where(rng.random(ROWS) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 6, ROWS)
    one[0] = (2.0, 0.0, 0.0, 0.0)
    fams["one_component"] = one
    return fams


def _euler_families(rng):
    fams = {"pm%g" % s: rng.uniform(-s, s, (ROWS, 3)) for s in (1.0, 100.0, 1e4, 1e6)}
    lock = rng.uniform(-np.pi, np.pi, (ROWS, 3))
    lock[:, 2] = np.where(np.arange(ROWS) % 2 == 0, 1.0, -1.0) * float(np.float32(np.pi / 2))
    fams["e2_half_pi"] = lock
    fams["zero"] = np.zeros((ROWS, 3))
    return fams


def _expmap_families(rng):
    t = {
        "zero": np.zeros(ROWS),
        "below_clamp": 10.0 ** rng.uniform(-6, math.log10(0.0099), ROWS),
        "straddle": 0.01 * np.sqrt(1 + rng.uniform(-1e-6, 1e-6, ROWS)),
        "0.01_to_1": rng.uniform(0.0101, 0.99, ROWS),
        "around_1": rng.uniform(0.99, 1.01, ROWS),
        "1_to_3": rng.uniform(1.01, 3.0, ROWS),
        "near_pi": np.pi + rng.uniform(-1e-3, 1e-3, ROWS),
        "near_2pi": 2 * np.pi + rng.uniform(-1e-3, 1e-3, ROWS),
        "50_to_100": rng.uniform(50, 100, ROWS),
        "5e3_to_1e4": rng.uniform(5e3, 1e4, ROWS),
    }
    return {k: _unit(rng, ROWS, 3) * v[:, None] for k, v in t.items()}


def _ortho6d_families(rng):
    fams = {}
    scales = (1e-18, 1e-12, 1.0, 1e15, 1e18)
    for sa in scales:
        for sb in scales:
            a = _unit(rng, ROWS, 3) * rng.uniform(0.5, 2, (ROWS, 1)) * sa
            b = _unit(rng, ROWS, 3) * rng.uniform(0.5, 2, (ROWS, 1)) * sb
            fams["a%g_b%g" % (sa, sb)] = np.concatenate((a, b), 1)
    # beyond the issue's set: since the head prescales both halves by a power of two these magnitudes are in range (the backward
    # wherever 1 / |a| and 1 / |b| are float32 numbers); 1e-24 and 1e20 used to square to 0 and inf
    for sa, sb in ((1e-24, 1e-24), (1e20, 1e20), (1e-30, 1e30), (1e30, 1e-30)):
        a = _unit(rng, ROWS, 3) * rng.uniform(0.5, 2, (ROWS, 1)) * sa
        b = _unit(rng, ROWS, 3) * rng.uniform(0.5, 2, (ROWS, 1)) * sb
        fams["a%g_b%g" % (sa, sb)] = np.concatenate((a, b), 1)
    for sine in (1e-1, 1e-3, 1e-5):
        a = _unit(rng, ROWS, 3)
        p = np.cross(a, _unit(rng, ROWS, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        b = (math.sqrt(1 - sine * sine) * a + sine * p) * rng.uniform(0.5, 2, (ROWS, 1))
        fams["parallel_%g" % sine] = np.concatenate((a * rng.uniform(0.5, 2, (ROWS, 1)), b), 1)
    return fams


def _ortho5d_families(rng):
    fams = {}
    for s in (1e-10, 1e-3, 1.0, 1e3, 1e10):
        a = rng.standard_normal((ROWS, 5))
        a[:, 2:] *= s
        fams["tail_%g" % s] = a
        a = rng.standard_normal((ROWS, 5))
        a[:, :2] *= s
        fams["head_%g" % s] = a
    return fams


def _se3_families(rng):
    def base():
        out = rng.standard_normal((ROWS, 12))
        out[:, 9:11] *= 20.0
        out[:, 11] = 1.0 + 0.1 * rng.standard_normal(ROWS)
        t = np.zeros((ROWS, 4, 4))
        t[:, :3, :3] = _rot(rng, ROWS)
        t[:, :3, 3] = [0.0, 0.0, 2.5] + 0.3 * rng.standard_normal((ROWS, 3))
        t[:, 3, 3] = 1.0
        return out, t

    fams = {"g8_like": base()}
    out, t = base()                                                   # tools/stress_families.py: reflection, rank one, ties
    out[:, :9] = (_rot(rng, ROWS) @ np.diag([1.0, 1.0, -1.0]) + 0.1 * rng.standard_normal((ROWS, 3, 3))).reshape(ROWS, 9)
    fams["reflection"] = (out, t)
    out, t = base()
    out[:, :9] = (rng.standard_normal((ROWS, 3, 1)) @ rng.standard_normal((ROWS, 1, 3))).reshape(ROWS, 9)
    fams["rank_one"] = (out, t)
    out, t = base()
    d = np.ones((ROWS, 3))
    d[:, 1] = 1 - 1e-3 * rng.random(ROWS)
    d[:, 2] = 1 - 2e-3 * rng.random(ROWS)
    out[:, :9] = ((_rot(rng, ROWS) * d[:, None, :]) @ _rot(rng, ROWS)).reshape(ROWS, 9)
    fams["ties"] = (out, t)
    for zk in (0.05, 2.5, 50.0):
        out, t = base()
        t[:, 2, 3] = zk
        fams["zk_%g" % zk] = (out, t)
    for vz in (0.5, 1.0, 2.0):
        out, t = base()
        out[:, 11] = vz
        fams["vz_%g" % vz] = (out, t)
    return {k: (o, t.reshape(ROWS, 16)) for k, (o, t) in fams.items()}


_FAMILIES = {"quat": _quat_families, "euler": _euler_families, "expmap": _expmap_families, "ortho6d": _ortho6d_families,
             "ortho5d": _ortho5d_families, "se3_update": _se3_families}


def expmap_backward_np(v, g, clamped):
    """The exp map's float64 gradient with the clamp's side GIVEN per row (clamped: theta is the constant sqrt(1e-4), no gradient through
    it) -- the two answers a row inside KINK_BAND may take."""
    vt = torch.as_tensor(np.asarray(v, np.float64)).clone().requires_grad_(True)
    nrms = (vt * vt).sum(1)
    ang = torch.where(torch.as_tensor(np.asarray(clamped, bool)), torch.full_like(nrms, EXPMAP_EPS), nrms).sqrt()
    inv = 1.0 / ang
    fac1, fac2 = inv * ang.sin(), inv * inv * (1.0 - ang.cos())
    x, y, z = vt.unbind(1)
    zero = torch.zeros_like(x)
    k = torch.stack((torch.stack((zero, -z, y), 1), torch.stack((z, zero, -x), 1), torch.stack((-y, x, zero), 1)), 1)
    r = fac1[:, None, None] * k + fac2[:, None, None] * torch.bmm(k, k) + torch.eye(3, dtype=torch.float64)[None]
    r.backward(torch.as_tensor(np.asarray(g, np.float64).reshape(-1, 3, 3)))
    return vt.grad.numpy()


def _quat_clamped_backward_np(q, g):
    qt = torch.as_tensor(np.asarray(q, np.float64)).clone().requires_grad_(True)
    w, x, y, z = (qt / QUAT_MIN_NORM).unbind(1)
    r = torch.stack((1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w, 2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z,
                     2 * y * z - 2 * x * w, 2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y), 1)
    r.backward(torch.as_tensor(np.asarray(g, np.float64).reshape(-1, 9)))
    return qt.grad.numpy()


def ortho5d_pair(a):
    """The un-projected pair (x_raw, y_raw) of the 5D head in float64, |v| and s = |v|^2."""
    a = np.asarray(a, np.float64)
    v = a[:, 2:5] * [K0, K0, K2]
    s = (v * v).sum(1)
    nv = np.sqrt(s)
    return np.stack((a[:, 0], a[:, 1], (s - 1) / (2 * nv)), 1), v / nv[:, None], nv, s


def se3_gap(out):
    """(s1, gap) of out[:, :9] in float64: gap = (s2 + s3) / s1 without a flip, (s2 - s3) / s1 with one."""
    _, s, d = so.symmetric_orthogonalization_np(np.asarray(out, np.float64)[:, :9], return_parts=True)
    return s[:, 0], np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]


@functools.lru_cache(maxsize=None)
def data(op):
    rng = np.random.default_rng([SEED, OPS.index(op)])
    fams = _FAMILIES[op](rng)
    names = list(fams)
    fam = np.repeat(np.arange(len(names)), ROWS)
    d = dict(names=names, fam=fam)
    if op == "se3_update":
        x = np.concatenate([fams[k][0] for k in names]).astype(np.float32)
        t = np.concatenate([fams[k][1] for k in names]).astype(np.float32)
        d["t"] = t
    else:
        x = np.concatenate([fams[k] for k in names]).astype(np.float32)
    n = len(x)
    d["x"] = x
    x64 = x.astype(np.float64)
    g = rng.standard_normal((n, OUT_WIDTH[op])).astype(np.float32)
    d["g"] = g
    one = np.ones(n)
    if op == "ortho6d":
        d["r64"] = so.ortho6d_np(x64).reshape(n, 9)
        d["dx64"] = so.ortho6d_backward_np(x64, g)
        d["cond"] = 1 / _sin_between(x64[:, :3], x64[:, 3:])
        d["gunit"] = np.repeat(np.stack((1 / np.linalg.norm(x64[:, :3], axis=1), 1 / np.linalg.norm(x64[:, 3:], axis=1)), 1), 3, axis=1) * d["cond"][:, None]
    elif op == "se3_update":
        t64 = d["t"].astype(np.float64)
        d["r64"] = so.se3_update_np(x64, t64, FX, FY).reshape(n, 16)
        d["dx64"] = so.se3_update_backward_np(x64, t64, g, FX, FY)
        d["s1"], d["gap"] = se3_gap(x64)
        d["cond"] = 1 / d["gap"]
    else:
        d["r64"] = so.head_np(op, x64).reshape(n, 9)
        d["dx64"] = so.head_backward_np(op, x64, g)
        d["cond"], d["gunit"] = one, np.ones((n, WIDTH[op]))
        if op == "quat":
            nq = np.linalg.norm(x64, axis=1)
            assert (np.abs(nq / QUAT_MIN_NORM - 1) > 5e-3).all()                  # no row on the clamp itself
            d["gunit"] = np.repeat((1 / np.maximum(nq, QUAT_MIN_NORM))[:, None], 4, axis=1)
            # q = 0 exactly: autograd through sqrt(0) is NaN (in the reference too); under the clamp the divisor is the constant 1e-8,
            # which is what every other clamped row's autograd gives (checked here) and what the kernel computes: 0 at q = 0
            low = nq < QUAT_MIN_NORM
            const = _quat_clamped_backward_np(x64[low], g[low])
            assert np.allclose(const[nq[low] > 0], d["dx64"][low][nq[low] > 0], rtol=1e-12, atol=0)
            d["dx64"][low] = const
        elif op == "expmap":
            n2 = (x64 * x64).sum(1)
            d["cond"] = np.maximum(1.0, np.sqrt(n2))
            d["kink"] = np.abs(n2 - EXPMAP_EPS) <= KINK_BAND
            assert d["kink"].any() and (~d["kink"][fam == names.index("straddle")]).any()
            assert not d["kink"][fam != names.index("straddle")].any()          # outside the straddle family no row is in the band
            d["dx64_alt"] = d["dx64"].copy()
            d["dx64_alt"][d["kink"]] = expmap_backward_np(x64[d["kink"]], g[d["kink"]], ~(n2 < EXPMAP_EPS)[d["kink"]])
            assert np.array_equal(expmap_backward_np(x64, g, n2 < EXPMAP_EPS), d["dx64"])
        elif op == "ortho5d":
            xr, vh, nv, s = ortho5d_pair(x64)
            nx = np.linalg.norm(xr, axis=1)
            d["cond"] = 1 / _sin_between(xr, vh)
            tail = K0 * (1 / nv + (s + 1) / (2 * s * nx))
            d["gunit"] = np.stack((1 / nx, 1 / nx, tail, tail, tail), 1)
    for k, v in d.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), (op, k)
            v.setflags(write=False)
    return d


def _take(a, idx):
    return a if idx is None else a[idx]


def forward_figure(op, got, idx=None):
    """Per row: the forward error in units of u cond (compare with C_FWD[op]).  `idx`: the fixture rows `got` was computed from."""
    d = data(op)
    err = np.abs(np.asarray(got, np.float64).reshape(-1, OUT_WIDTH[op]) - _take(d["r64"], idx))
    if op != "se3_update":
        return err.max(1) / (U * _take(d["cond"], idx))
    gap, want = _take(d["gap"], idx), _take(d["r64"], idx)
    rot = np.where(gap < SE3_MIN_GAP, 0.0, err[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].max(1) * gap)
    trans = (err[:, [3, 7, 11]] / np.maximum(1.0, np.abs(want[:, [3, 7, 11]]))).max(1)
    return np.maximum(np.maximum(rot, trans), err[:, 12:].max(1)) / U


def backward_figure(op, got, idx=None):
    """Per row: the backward error in units of u |G|_1 cond gunit (compare with C_BWD[op]); inside the exp map's kink band the smaller of
    the two sides' figures."""
    d = data(op)
    got = np.asarray(got, np.float64).reshape(-1, WIDTH[op])
    want = _take(d["dx64"], idx)
    if op == "se3_update":
        s1, gap = _take(d["s1"], idx), _take(d["gap"], idx)
        return np.abs(got - want).max(1) * np.minimum(1.0, s1 * gap * gap) / np.maximum(np.abs(want).max(1), 1.0) / U
    unit = (U * np.abs(_take(d["g"], idx)).astype(np.float64).sum(1) * _take(d["cond"], idx))[:, None] * _take(d["gunit"], idx)
    fig = (np.abs(got - want) / unit).max(1)
    if op == "expmap":
        alt = (np.abs(got - _take(d["dx64_alt"], idx)) / unit).max(1)
        fig = np.where(_take(d["kink"], idx), np.minimum(fig, alt), fig)
    return fig


def se3_rotation_defect(got, idx=None):
    """max |R^T R - I| of the rotation block of T_pred, per row (what is asked of rows without a gap)."""
    r = np.asarray(got, np.float64).reshape(-1, 4, 4)[:, :3, :3]
    return np.abs(np.einsum("bji,bjk->bik", r, r) - np.eye(3)).reshape(len(r), 9).max(1)


def tile_period(m):
    """The tiling's period: the smallest prime above m.  A prime period shares no factor with the rows of one pass of an engine's grid
    (CUs x 4 x WPS x NPL x 64; tests/test_gpu_heads.py asserts it), so row p and row p - k * pass never hold the same fixture row: a
    round that reads another round's input returns another row's answer.  (Tiled with period m itself, the Euler fixture's 768 rows and
    the 6D fixture's 4096 divide a pass exactly, and a stale round would have gone unseen.)"""
    p = m + 1
    while any(p % q == 0 for q in range(2, int(math.isqrt(p)) + 1)):
        p += 1
    return p


def tile_index(n, m):
    """n fixture-row numbers: position i holds row ((i * stride) mod P) mod m with P = tile_period(m) and a stride coprime to P.  Every
    block of P positions holds every fixture row (the first P - m rows twice); copies of a position's row sit exactly P apart."""
    period = tile_period(m)
    stride = next(q for q in (929, 937, 941, 947, 953) if q % period != 0)
    return ((np.arange(n, dtype=np.int64) * stride) % period) % m


# ---- outside the range ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def outside(op):
    """Rows beyond the documented range -- the float32 squared norm is exactly 0 (inputs of 1e-24) or inf (1e20) on the host and on the
    device alike -- with what the forward kernel returns there: `nan` marks the slots that are NaN, `value` gives the others (NaN where
    the slot is not pinned).  Magnitudes between the range and these (1e-21, 1e19) give a subnormal squared norm, where v_rsq_f32 and libm
    differ: nothing is pinned there but that the row stays in its row."""
    rng = np.random.default_rng([SEED, 99, OPS.index(op)])
    n = 16
    if op == "quat":                                           # |q|^2 = inf: 1 / |q| = 0, n = 0, R = I exactly (|q| = 0 is IN range: also I)
        x = _unit(rng, n, 4) * 1e20
        return dict(x=x.astype(np.float32), nan=np.zeros((n, 9), bool), value=np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    if op == "ortho5d":
        lo = rng.standard_normal((n // 2, 5))
        lo[:, 2:] *= 1e-24                                     # s = 0: x_raw.z = -inf, x = (0, 0, NaN)
        hi = rng.standard_normal((n // 2, 5))
        hi[:, 2:] *= 1e20                                      # s = inf: x_raw.z = inf * 0 = NaN: every slot
        nan = np.ones((n, 9), bool)
        nan[: n // 2, [0, 3]] = False
        value = np.full((n, 9), np.nan)
        value[: n // 2, [0, 3]] = 0.0
        return dict(x=np.concatenate((lo, hi)).astype(np.float32), nan=nan, value=value)
    raise KeyError(op)                                         # euler, expmap, ortho6d, se3_update: every finite float32 input is in range


OUTSIDE_OPS = ("quat", "ortho5d")


def outside_matches(op, got):
    o = outside(op)
    got = np.asarray(got, np.float64).reshape(-1, 9)
    pinned = ~np.isnan(o["value"])
    return bool(np.array_equal(np.isnan(got), o["nan"]) and np.array_equal(got[pinned], o["value"][pinned]))


# ---- the axis-angle sampler (so3_rotations_axis_angle_f32: point_cloud/prepare.py:21-49 for given draws) -------------------------------
@functools.lru_cache(maxsize=None)
def sampler():
    rng = np.random.default_rng([SEED, 77])
    per = 16
    theta, axis, names = [], [], []
    for th in (0.0, np.pi / 2, np.pi, 1e4):
        for nrm in (0.0, 1e-9, 1.0, 1e10):
            theta.append(np.full(per, th))
            axis.append(_unit(rng, per, 3) * nrm)
            names.append("theta%g_axis%g" % (th, nrm))
    theta, axis = np.concatenate(theta).astype(np.float32), np.concatenate(axis).astype(np.float32)
    r64 = so.rotations_from_draws_np(theta.astype(np.float64), axis.astype(np.float64)).reshape(-1, 9)
    return dict(theta=theta, axis=axis, r64=r64, names=names, fam=np.repeat(np.arange(16), per))


def sampler_f32(theta, axis):
    """k_rotations_axis_angle's arithmetic restated operation for operation in numpy float32 (the kernel is not a row operation of the host
    model): what HOST_SAMPLER is measured on."""
    f = np.float32
    t, a = np.asarray(theta, f), np.asarray(axis, f)
    mag = np.maximum(np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]), f(1e-8))
    ax, ay, az = a[:, 0] / mag, a[:, 1] / mag, a[:, 2] / mag
    sn, qw = np.sin(t), np.cos(t)
    qx, qy, qz = ax * sn, ay * sn, az * sn
    xx, yy, zz, xy, xz, yz, xw, yw, zw = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qx * qw, qy * qw, qz * qw
    one, two = f(1), f(2)
    out = np.stack((one - two * yy - two * zz, two * xy - two * zw, two * xz + two * yw, two * xy + two * zw, one - two * xx - two * zz, two * yz - two * xw,
                    two * xz - two * yw, two * yz + two * xw, one - two * xx - two * yy), 1)
    assert out.dtype == np.float32
    return out


def sampler_figure(got, idx=None):
    return np.abs(np.asarray(got, np.float64).reshape(-1, 9) - _take(sampler()["r64"], idx)).max(1) / U
