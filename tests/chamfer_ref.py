"""The Chamfer distance restated in float64 numpy (no reference code exists for it): the definition chamfer_distance and
so3_chamfer_fwd_f32 / so3_chamfer_bwd_f32 are held to, the generator and the reader of tests/golden/g27_chamfer.npz, and the figures
tests/test_chamfer_host.py and tests/test_gpu_chamfer.py share.  TEST INFRASTRUCTURE ONLY.

    n_b = clip(x_lengths[b], 0, N),  m_b = clip(y_lengths[b], 0, M);   j(i) = the first argmin over j < m_b of |x_i - y_j|^2,
    i(j) = the first argmin over i < n_b of |y_j - x_i|^2;   e = d^2 (squared) or d;   rows[b] = (mean_{i<n_b} e_i, mean_{j<m_b} e_j),
    (0, 0) when n_b == 0 or m_b == 0;   a padded slot has dist 0, nearest -1 and a zero gradient row.
    dX[b,i] = a_b phi(x_i - y_j(i)) + sum_{j<m_b, i(j)=i} c_b phi(x_i - y_j),  phi(v) = 2v or v/|v| (0 at 0);  dY the mirror image.

The search's and the squared gradient's order of operations is part of the definition (so3_device.h), so search32 and grad32 below
restate their float32 BITS through tests/f32_exact.py: the host model and the device are held to them by equality -- nearest_x /
nearest_y in both flavours, the squared dist and the squared dX / dY.  The unsquared terms pass through 1-ulp instructions and rows
through a butterfly whose shape follows the device, so those stay on the float64 figures, which the exact outputs keep beside the
equality.  Against FLOAT64 the search is discontinuous, so there indices are never compared outside the exact families; the figures are
  search   e64(point, RETURNED neighbour) - the float64 minimum, over the live points of both directions
  dist     |returned dist - e64(point, returned neighbour)|
  rows     |rows - float64 rows| / |float64 rows|;  a float64 row of exactly 0 must be returned as exactly 0 (else inf)
  loss     the same for the per-cloud loss rows[b][0] + rows[b][1] the Python surface returns
  grad     |dX - dX64| / A  with dX64 the closed form in float64 through the RETURNED indices and A the same sum over the absolute
           values of its terms (the scale the rounding errors of the chain have); A == 0 must come back as exactly 0 (else inf)
  exact    0 or inf: padded slots, empty clouds, and what an exact family promises."""
import os

import numpy as np

from f32_exact import first_argmin32, fma32, pair_dist2_32
from support import lengths_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_chamfer.npz")
SIZES = [(1, 1), (3, 7), (255, 1023), (256, 1024), (257, 1025), (1000, 2500)]
B = 4                                   # clouds per geometry: ragged gives cloud 0 n_b = 0, cloud 1 m_b = 0, cloud 2 m_b = 1
MIN_DISTANCE = 1e-3                     # no non-zero nearest distance of the fixture lies below it (the unsquared gradient's singularity)
FAMILIES = ("random", "subset", "many_to_one")


def scales(b):
    """The per-cloud gradient scales (a_b, c_b) the gradient checks use: float32-exact, both signs."""
    k = np.arange(b, dtype=np.float64)
    return (0.75 + 0.5 * k).astype(np.float32), (-1.25 + 0.25 * k).astype(np.float32)


def _search(P, Q):
    """Per point of P (n,3) the squared float64 distance to the closest point of Q (m,3) and the first argmin."""
    d2 = np.empty(len(P))
    idx = np.empty(len(P), np.int64)
    for s in range(0, len(P), 256):
        blk = ((P[s:s + 256, None, :] - Q[None, :, :]) ** 2).sum(-1)
        idx[s:s + 256] = blk.argmin(1)
        d2[s:s + 256] = blk[np.arange(len(blk)), idx[s:s + 256]]
    return d2, idx


def term(d2, squared):
    return d2 if squared else np.sqrt(d2)


def chamfer64(X, Y, x_lengths=None, y_lengths=None, squared=True):
    """The forward in float64: dist_x (B,N), nearest_x (B,N) int64, dist_y, nearest_y, rows (B,2) the means, sums (B,2)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    b, n, m = X.shape[0], X.shape[1], Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    out = {"dist_x": np.zeros((b, n)), "nearest_x": np.full((b, n), -1, np.int64), "dist_y": np.zeros((b, m)),
           "nearest_y": np.full((b, m), -1, np.int64), "rows": np.zeros((b, 2)), "sums": np.zeros((b, 2))}
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        d2, idx = _search(X[k, :nb], Y[k, :mb])
        out["dist_x"][k, :nb], out["nearest_x"][k, :nb] = term(d2, squared), idx
        d2, idx = _search(Y[k, :mb], X[k, :nb])
        out["dist_y"][k, :mb], out["nearest_y"][k, :mb] = term(d2, squared), idx
        out["sums"][k] = out["dist_x"][k].sum(), out["dist_y"][k].sum()
        out["rows"][k] = out["sums"][k] / (nb, mb)
    return out


def loss64(fwd, x_lengths, y_lengths, n, m, point_reduction="mean", batch_reduction="mean", single=False):
    per = fwd["rows"] if point_reduction == "mean" else fwd["sums"]
    per = per[:, 0] if single else per[:, 0] + per[:, 1]
    return per.mean() if batch_reduction == "mean" else (per.sum() if batch_reduction == "sum" else per)


def fold_scales(g, b, n, m, x_lengths, y_lengths, point_reduction, batch_reduction):
    """The upstream gradient g (a scalar, or (B,) for batch_reduction None) folded into the per-cloud scales (a_b, c_b), float64."""
    g = np.broadcast_to(np.asarray(g, np.float64), (b,)) * (1.0 / b if batch_reduction == "mean" else 1.0)
    if point_reduction == "sum":
        return g.copy(), g.copy()
    return g / np.maximum(lengths_of(x_lengths, b, n), 1), g / np.maximum(lengths_of(y_lengths, b, m), 1)


def phi(v, squared):
    if squared:
        return 2.0 * v
    r = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(r > 0, v / np.where(r > 0, r, 1.0), 0.0)


def e_through(P, Q, idx, squared):
    """e64 of every point of P (n,3) against the point of Q its index names."""
    return term(((P - Q[idx]) ** 2).sum(-1), squared)


def grad64(X, Y, x_lengths, y_lengths, nearest_x, nearest_y, scale_x, scale_y, squared=True):
    """The closed-form gradient in float64 through the given indices: dX, dY and the sums of their terms' absolute values AX, AY.
    scale_y None: the x direction alone (dY then holds the x direction's hits)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    b, n, m = X.shape[0], X.shape[1], Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    dX, dY, AX, AY = np.zeros_like(X), np.zeros_like(Y), np.zeros_like(X), np.zeros_like(Y)
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        j = np.asarray(nearest_x[k, :nb], np.int64)
        assert j.min() >= 0 and j.max() < mb
        t = float(scale_x[k]) * phi(X[k, :nb] - Y[k, j], squared)
        dX[k, :nb] += t
        AX[k, :nb] += np.abs(t)
        np.add.at(dY[k], j, -t)
        np.add.at(AY[k], j, np.abs(t))
        if scale_y is not None:
            i = np.asarray(nearest_y[k, :mb], np.int64)
            assert i.min() >= 0 and i.max() < nb
            t = float(scale_y[k]) * phi(Y[k, :mb] - X[k, i], squared)
            dY[k, :mb] += t
            AY[k, :mb] += np.abs(t)
            np.add.at(dX[k], i, -t)
            np.add.at(AX[k], i, np.abs(t))
    return dX, dY, AX, AY


# ---- the defined float32 bits (so3_device.h: add_s_pair, chamfer_own, chamfer_hit), through tests/f32_exact.py ------------------------
SEARCH32_PAIRS = 1 << 20                # pairs per numpy pass of search32


def _search32(P, Q, pl, ql):
    """P (b,n,3) searches Q (b,m,3) over the live prefixes pl, ql (b,): d2 (b,n) float32 and the first argmin (b,n), 0 / -1 in the
    slots past pl and in clouds with an empty side."""
    b, n, m = P.shape[0], P.shape[1], Q.shape[1]
    d2, idx = np.zeros((b, n), np.float32), np.full((b, n), -1, np.int64)
    rows = max(1, SEARCH32_PAIRS // m)                          # a pass is some rows of some clouds, all m candidates of each
    step = max(1, rows // n)
    for k in range(0, b, step):
        q = Q[k:k + step, None, :, :]
        past = np.arange(m)[None, None, :] >= ql[k:k + step, None, None]
        for lo in range(0, n, rows):
            p = P[k:k + step, lo:lo + rows, None, :]
            d = pair_dist2_32(p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2])
            d[np.broadcast_to(past, d.shape)] = np.inf
            at = first_argmin32(d)
            idx[k:k + step, lo:lo + rows], d2[k:k + step, lo:lo + rows] = at, np.take_along_axis(d, at[..., None], -1)[..., 0]
    dead = (np.arange(n)[None, :] >= pl[:, None]) | (ql[:, None] == 0)
    d2[dead], idx[dead] = 0, -1
    return d2, idx


def search32(X, Y, x_lengths=None, y_lengths=None, single=False):
    """The squared flavour's forward, bit for bit: dist_x, nearest_x (and dist_y, nearest_y) as so3_chamfer_fwd_f32 defines them --
    d^2 = fma(dz, dz, fma(dy, dy, dx * dx)) from float32 coordinate differences, the first of equal candidates, a padded slot 0 / -1.
    The indices are the unsquared flavour's too (its term is the root of the same minimum)."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    b, n, m = X.shape[0], X.shape[1], Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    out = {}
    out["dist_x"], out["nearest_x"] = _search32(X, Y, nl, ml)
    if not single:
        out["dist_y"], out["nearest_y"] = _search32(Y, X, ml, nl)
    return out


def _chain32(P, Q, pl, ql, near_own, near_hit, s_own, s_hit):
    """One cloud, one side (so3_device.h's chain): acc = s_own * (2 (p_i - q_near_own(i))) as one rounded product (+0 without an own
    term), then acc = fma(s_hit, 2 (p_i - q_j), acc) over the j < ql with near_hit[j] == i in ascending j.  The r-th hit of every
    owner is one numpy step."""
    out = np.zeros_like(P)
    if pl == 0 or ql == 0:
        return out
    acc = np.zeros((pl, 3), np.float32)
    if s_own is not None:
        j = np.clip(np.asarray(near_own[:pl], np.int64), 0, ql - 1)
        acc = np.float32(s_own) * (np.float32(2) * (P[:pl] - Q[j]))
    if s_hit is not None:
        owner = np.asarray(near_hit[:ql], np.int64)
        j = np.flatnonzero((owner >= 0) & (owner < pl))
        j = j[np.argsort(owner[j], kind="stable")]                     # by owner, ascending j within an owner
        o = owner[j]
        rank = np.arange(len(j)) - np.searchsorted(o, o, side="left")  # the hit's place in its owner's chain
        for r in range(int(rank.max()) + 1 if len(j) else 0):
            at = rank == r
            oo, jj = o[at], j[at]
            acc[oo] = fma32(np.float32(s_hit), np.float32(2) * (P[oo] - Q[jj]), acc[oo])
    out[:pl] = acc
    return out


def grad32(X, Y, x_lengths, y_lengths, nearest_x, nearest_y, scale_x, scale_y, clouds=None):
    """The squared flavour's gradients, bit for bit, through the GIVEN indices and the float32 scales: (dX, dY) float32.  scale_y None:
    the x direction alone (dY's chains then start at +0 and hold the x direction's hits).  clouds: restate these alone (the others 0)."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    b, n, m = X.shape[0], X.shape[1], Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    dX, dY = np.zeros_like(X), np.zeros_like(Y)
    for k in range(b) if clouds is None else clouds:
        sx, sy = scale_x[k], None if scale_y is None else scale_y[k]
        iy = None if scale_y is None else nearest_y[k]
        dX[k] = _chain32(X[k], Y[k], int(nl[k]), int(ml[k]), nearest_x[k], iy, sx, sy)
        dY[k] = _chain32(Y[k], X[k], int(ml[k]), int(nl[k]), iy, nearest_x[k], sy, sx)
    return dX, dY


def small_last_hit_case(seed=2750):
    """G27's many-to-one geometry on fresh points (squared, full lengths), with the LAST of the 2500 hits on x_0 made small: y_2499 lies
    1e-6 from x_0, so its term in dX[0]'s chain is about 1e-7 of the sum of the chain's absolute terms -- a tenth of what the float64
    figure's bound lets pass -- and still tens of ulps of the running sum.  It sits in the last, partial 64-entry block of the scan."""
    rng = np.random.default_rng(seed)
    n, m = 257, 2500
    d = rng.standard_normal((m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = d * rng.uniform(2e-3, 9e-3, (m, 1))
    Y[-1] = d[-1] * 1e-6
    X = rng.standard_normal((n, 3))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[0] = 0
    return {"name": "many_to_one, the last hit a small one", "family": "fresh", "X": X[None].astype(np.float32), "Y": Y[None].astype(np.float32),
            "x_lengths": None, "y_lengths": None, "squared": True, "b": 1, "n": n, "m": m}


def min_nonzero_distance(X, Y, x_lengths=None, y_lengths=None):
    """The smallest non-zero float64 nearest-neighbour distance of either direction (inf when there is none)."""
    f = chamfer64(X, Y, x_lengths, y_lengths, squared=False)
    d = np.concatenate([f["dist_x"].ravel(), f["dist_y"].ravel()])
    return d[d > 0].min() if (d > 0).any() else np.inf


# ---- the figures -----------------------------------------------------------------------------------------------------------------
def _relative(got, want, scale):
    """max |got - want| / scale where scale > 0; where scale == 0 the value must be exactly 0."""
    got, want, scale = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64)
    live = scale > 0
    if (got[~live] != 0).any() or not np.isfinite(got).all():
        return np.inf
    return float((np.abs(got - want)[live] / scale[live]).max()) if live.any() else 0.0


def forward_figures(X, Y, x_lengths, y_lengths, squared, got, single=False, want=None):
    """got: dist_x, nearest_x, rows (B,2) and, unless single, dist_y, nearest_y.  want: chamfer64's answer when it is at hand."""
    X64, Y64 = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    b, n, m = X64.shape[0], X64.shape[1], Y64.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    if want is None:
        want = chamfer64(X, Y, x_lengths, y_lengths, squared)
    f = {"search": 0.0, "dist": 0.0, "exact": 0.0}
    for side, P, Q, pl, ql in (("x", X64, Y64, nl, ml),) + (() if single else (("y", Y64, X64, ml, nl),)):
        dist, near = np.asarray(got["dist_" + side], np.float64), np.asarray(got["nearest_" + side], np.int64)
        for k in range(b):
            pb, qb = (int(pl[k]), int(ql[k])) if pl[k] > 0 and ql[k] > 0 else (0, 0)
            if (dist[k, pb:] != 0).any() or (near[k, pb:] != -1).any():                 # padded slots, empty clouds
                f["exact"] = np.inf
            if pb == 0:
                continue
            if near[k, :pb].min() < 0 or near[k, :pb].max() >= qb:
                f["exact"] = np.inf
                continue
            e = e_through(P[k, :pb], Q[k], near[k, :pb], squared)
            f["search"] = max(f["search"], float((e - want["dist_" + side][k, :pb]).max()))
            f["dist"] = max(f["dist"], float(np.abs(dist[k, :pb] - e).max()))
    ref = want["rows"].copy()
    if single:
        ref[:, 1] = 0
    if "rows" in got:
        f["rows"] = _relative(got["rows"], ref, np.abs(ref))
    if "loss" in got:                                    # the Python surface's per-cloud loss: the sum of the two rows
        f["loss"] = _relative(got["loss"], ref.sum(1), np.abs(ref.sum(1)))
    return f


def gradient_figures(X, Y, x_lengths, y_lengths, squared, nearest_x, nearest_y, scale_x, scale_y, dX, dY):
    """Both gradients against float64 through the RETURNED indices (dX or dY None: not asked for)."""
    wx, wy, ax, ay = grad64(X, Y, x_lengths, y_lengths, nearest_x, nearest_y, scale_x, scale_y, squared)
    f = {"grad": 0.0}
    if dX is not None:
        f["grad"] = max(f["grad"], _relative(dX, wx, ax))
    if dY is not None:
        f["grad"] = max(f["grad"], _relative(dY, wy, ay))
    return f


# ---- G27 -----------------------------------------------------------------------------------------------------------------------
def _ball(rng, n):
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(0, 1, (n, 1)) ** (1 / 3)


def generate(seed=27):
    """The arrays of g27_chamfer.npz (tools/gen_golden.py g27 saves them).  Per geometry g: X, Y float32 in the unit ball, the ragged
    lengths, and per (g, lengths) the float64 search's indices and rows (squared and unsquared)."""
    rng = np.random.default_rng(seed)
    out, names = {}, []

    def add(name, family, X, Y, xl, yl):
        X, Y = X.astype(np.float32), Y.astype(np.float32)
        assert np.abs(X).max() <= 1 and np.abs(Y).max() <= 1
        out[name + "/X"], out[name + "/Y"] = X, Y
        names.append(name)
        out[name + "/family"] = np.int32(FAMILIES.index(family))
        for tag, a, c in (("full", None, None),) + ((("ragged", xl, yl),) if xl is not None else ()):
            assert min_nonzero_distance(X, Y, a, c) >= MIN_DISTANCE, (name, tag)
            if a is not None:
                out[name + "/x_lengths"], out[name + "/y_lengths"] = a.astype(np.int32), c.astype(np.int32)
            for squared in (True, False):
                f = chamfer64(X, Y, a, c, squared)
                out["%s/%s/rows_%s" % (name, tag, "sq" if squared else "l2")] = f["rows"]
            out["%s/%s/nearest_x" % (name, tag)] = f["nearest_x"].astype(np.int32)
            out["%s/%s/nearest_y" % (name, tag)] = f["nearest_y"].astype(np.int32)

    for n, m in SIZES:
        X = np.stack([_ball(rng, n) for _ in range(B)])
        Y = np.stack([_ball(rng, m) for _ in range(B)])
        xl = np.array([0, max(n // 2, 1), n, rng.integers(1, n + 1)])
        yl = np.array([max(m // 3, 1), 0, 1, rng.integers(1, m + 1)])
        add("random_%dx%d" % (n, m), "random", X, Y, xl, yl)
    # X is a subset of Y, and Y holds every point of X twice: the x direction is exactly 0 and returns the FIRST duplicate
    n, m = 300, 700
    Y = np.stack([_ball(rng, m) for _ in range(2)]).astype(np.float32)
    pick = np.stack([rng.permutation(m // 2)[:n] for _ in range(2)])
    for k in range(2):
        Y[k, m // 2:] = Y[k, :m // 2]                                  # the second half repeats the first
    X = np.stack([Y[k, pick[k]] for k in range(2)])
    add("subset_%dx%d" % (n, m), "subset", X, Y, None, None)
    out["subset_%dx%d/pick" % (n, m)] = pick.astype(np.int32)
    # many-to-one: every y lies within 1e-2 of x_0 = 0 (no closer than 2e-3), the other x are one unit away
    n, m = 257, 2500
    x0 = np.zeros(3)
    d = rng.standard_normal((m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = (x0 + d * rng.uniform(2e-3, 9e-3, (m, 1)))[None]
    far = rng.standard_normal((n, 3))
    far /= np.linalg.norm(far, axis=1, keepdims=True)
    X = (x0 + far)[None].copy()                                        # one unit away
    X[0, 0] = x0
    add("many_to_one_%dx%d" % (n, m), "many_to_one", X, Y, None, None)
    out["names"] = np.array(names)
    return out


def g27():
    return np.load(GOLDEN)


def cases(z):
    """One dict per (geometry, lengths, squared): name, family, X, Y, x_lengths, y_lengths (None: full), squared, n, m, b, and the
    fixture's float64 answers nearest_x, nearest_y, rows."""
    out = []
    for name in [str(s) for s in z["names"]]:
        X, Y = z[name + "/X"], z[name + "/Y"]
        for tag in ("full", "ragged"):
            if tag == "ragged" and name + "/x_lengths" not in z.files:
                continue
            xl, yl = (z[name + "/x_lengths"], z[name + "/y_lengths"]) if tag == "ragged" else (None, None)
            for squared in (True, False):
                out.append({"name": "%s/%s/%s" % (name, tag, "sq" if squared else "l2"), "geometry": name, "lengths": tag,
                            "family": FAMILIES[int(z[name + "/family"])], "X": X, "Y": Y, "x_lengths": xl, "y_lengths": yl, "squared": squared,
                            "b": X.shape[0], "n": X.shape[1], "m": Y.shape[1], "nearest_x": z["%s/%s/nearest_x" % (name, tag)],
                            "nearest_y": z["%s/%s/nearest_y" % (name, tag)], "rows": z["%s/%s/rows_%s" % (name, tag, "sq" if squared else "l2")],
                            "pick": z[name + "/pick"] if name + "/pick" in z.files else None})
    return out
