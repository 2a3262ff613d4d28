"""Chamfer's normal term restated in numpy (no reference code exists for it): the definition chamfer_distance(x_normals=, y_normals=)
and so3_chamfer_normals_fwd_f32 / so3_chamfer_normals_bwd_f32 are held to (include/so3proj.h), the generator and the reader of
tests/golden/g31_chamfer_normals.npz, and the figures tests/test_chamfer_normals_host.py and tests/test_gpu_chamfer_normals.py share.
TEST INFRASTRUCTURE ONLY.

    A pair is a point's own normal a and the normal b of the point its search returned (direction x: nx_i, ny_j(i); y: ny_j, nx_i(j)).
    c = a.b / (|a| |b|);  the pair is FLAT when the float32 chain a.a or b.b is not in (0, inf): c = 0, t = 1, no gradient;
    t = 1 - |c| (signed: 1 - c);  rows_n[b] = (mean_{i<n_b} t_i, mean_{j<m_b} t_j), (0, 0) with an empty side;
    psi(a, b) = dt/da = -sigma (b / |b| - c a / |a|) / |a|,  sigma = sgn(c) (signed: 1);
    dNX[b,i] = s_x[b] psi(nx_i, ny_j(i)) + sum_{j<m_b, i(j)=i} s_y[b] psi(nx_i, ny_j),  dNY the mirror image.

normals64 is that in float64 through GIVEN indices; normals32 the defined order of operations in float32 (so3_device.h:
chamfer_cosine, chamfer_normal_psi, chamfer_normal_own, chamfer_hit) with 1 / sqrt correctly rounded, which is what the host model
computes -- the device's v_rsq_f32 is a 1-ulp instruction, so the device is held to the float64 figures only:
  term     |returned t - t64(pair through the RETURNED index)|: absolute, t lies in [0, 2] and near 0 where a relative figure means nothing
  rows_n   |rows_n - the float64 mean of those t64|: absolute;  loss_n: the same for the per-cloud sum of the two rows the surface returns
  grad     |dN - dN64| / (sum over the chain of |coefficient| / |a_owner|): every |psi| <= 1 / |a|, and near |c| = 1 psi cancels to
           about zero, so a figure relative to |psi| itself is unbounded; an owner without a live pair must get exactly 0 (else inf)
  exact    0 or inf: padded slots, empty clouds, flat pairs, and what an exact family promises.
Condition on the inputs (asserted by the generator and again by the host test): through the float64 indices no pair has
0 < |c64| < MIN_COSINE, which keeps sgn(c) the same in float32 and float64; the generator redraws an offending normal."""
import os

import numpy as np

import chamfer_ref as cref
from f32_exact import fma32
from support import lengths_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_chamfer_normals.npz")
SIZES = [(1, 1), (3, 7), (255, 1023), (256, 1024), (257, 1025)]
B = 4                                   # clouds per random geometry: ragged gives cloud 0 n_b = 0, cloud 1 m_b = 0, cloud 2 m_b = 1
MIN_COSINE = 1e-5
FAMILIES = ("random", "sphere", "flipped", "subset", "orthogonal", "degenerate", "many_to_one")
scales = cref.scales                    # the per-cloud gradient scales (float32-exact, both signs)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def dot32(a, b):
    """The defined chain fma(az, bz, fma(ay, by, ax * bx)) in float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def flat(a, b):
    """The definition's flat pairs: decided on the float32 chains, as the kernels decide them."""
    with np.errstate(invalid="ignore"):
        saa, sbb = dot32(a, a), dot32(b, b)
        return ~((saa > 0) & (saa < np.inf) & (sbb > 0) & (sbb < np.inf))


def cosine64(a, b):
    """(c, |a|, |b|, flat) of float32 normals a, b (..., 3) in float64; c = 0 and lengths of 1 where the pair is flat."""
    fl = flat(a, b)
    a64, b64 = np.where(fl[..., None], 1.0, np.asarray(a, np.float64)), np.where(fl[..., None], 1.0, np.asarray(b, np.float64))
    la, lb = np.linalg.norm(a64, axis=-1), np.linalg.norm(b64, axis=-1)
    c = np.where(fl, 0.0, (a64 * b64).sum(-1) / (la * lb))
    return c, la, lb, fl


def term64(a, b, signed):
    c = cosine64(a, b)[0]
    return 1.0 - (c if signed else np.abs(c))


def psi64(a, b, signed):
    c, la, lb, fl = cosine64(a, b)
    sigma = np.ones_like(c) if signed else np.sign(c)
    a64, b64 = np.where(fl[..., None], 1.0, np.asarray(a, np.float64)), np.where(fl[..., None], 1.0, np.asarray(b, np.float64))
    psi = -(sigma / la)[..., None] * (b64 / lb[..., None] - c[..., None] * a64 / la[..., None])
    return np.where(fl[..., None], 0.0, psi)


def normals64(NX, NY, x_lengths, y_lengths, nearest_x, nearest_y, signed=False, scale_x=None, scale_y=None):
    """Terms, rows and (with scale_x) the gradient in float64 through the GIVEN indices.  nearest_y None: the x direction alone (term_y,
    rows_n[:, 1] are 0 and dNY holds the x direction's hits).  SX, SY: the grad figure's scale per normal."""
    NX, NY = np.asarray(NX, np.float32), np.asarray(NY, np.float32)
    b, n, m = NX.shape[0], NX.shape[1], NY.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    out = {"term_x": np.zeros((b, n)), "term_y": np.zeros((b, m)), "rows_n": np.zeros((b, 2)), "sums_n": np.zeros((b, 2)),
           "dNX": np.zeros((b, n, 3)), "dNY": np.zeros((b, m, 3)), "SX": np.zeros((b, n, 1)), "SY": np.zeros((b, m, 1))}
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        sides = [("x", NX[k, :nb], NY[k], np.asarray(nearest_x[k, :nb], np.int64), mb, "dNX", "dNY", "SX", "SY", scale_x, 0)]
        if nearest_y is not None:
            sides.append(("y", NY[k, :mb], NX[k], np.asarray(nearest_y[k, :mb], np.int64), nb, "dNY", "dNX", "SY", "SX", scale_y, 1))
        for side, own, other, idx, lim, d_own, d_hit, s_own, s_hit, scale, col in sides:
            assert idx.min() >= 0 and idx.max() < lim
            t = term64(own, other[idx], signed)
            out["term_" + side][k, :len(own)] = t
            out["sums_n"][k, col] = t.sum()
            out["rows_n"][k, col] = t.sum() / len(own)
            if scale is None:
                continue
            s = float(scale[k])
            fl = flat(own, other[idx])
            with np.errstate(invalid="ignore", over="ignore"):
                la, lb = np.linalg.norm(own.astype(np.float64), axis=-1), np.linalg.norm(other[idx].astype(np.float64), axis=-1)
            out[d_own][k, :len(own)] += s * psi64(own, other[idx], signed)
            out[s_own][k, :len(own), 0] += np.where(fl, 0.0, abs(s) / np.where(fl, 1.0, la))
            np.add.at(out[d_hit][k], idx, s * psi64(other[idx], own, signed))
            np.add.at(out[s_hit][k, :, 0], idx, np.where(fl, 0.0, abs(s) / np.where(fl, 1.0, lb)))
    return out


# ---- the defined order in float32 (so3_device.h), 1 / sqrt correctly rounded ------------------------------------------------------
def cosine32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    fl = flat(a, b)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        saa, sbb, sab = dot32(a, a), dot32(b, b), dot32(a, b)
        one = np.float32(1)
        ra = np.where(fl, np.float32(0), one / np.sqrt(np.where(fl, one, saa))).astype(np.float32)
        rb = np.where(fl, np.float32(0), one / np.sqrt(np.where(fl, one, sbb))).astype(np.float32)
        c = np.where(fl, np.float32(0), (np.where(fl, np.float32(0), sab) * ra) * rb).astype(np.float32)
    return c, ra, rb, fl


def term32(a, b, signed):
    c = cosine32(a, b)[0]
    return (np.float32(1) - (c if signed else np.abs(c))).astype(np.float32)


def psi32(a, b, signed):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    c, ra, rb, fl = cosine32(a, b)
    sigma = np.ones_like(c) if signed else np.sign(c).astype(np.float32)
    g = (-sigma * ra).astype(np.float32)
    safe_a, safe_b = np.where(fl[..., None], np.float32(0), a), np.where(fl[..., None], np.float32(0), b)
    u = g[..., None] * fma32(-c[..., None], safe_a * ra[..., None], safe_b * rb[..., None])
    return np.where(fl[..., None], np.float32(0), u).astype(np.float32)


def _chain32(P, Q, pl, ql, near_own, near_hit, s_own, s_hit, signed):
    """One cloud, one side: acc = s_own * psi(p_i, q_near_own(i)) as one rounded product (+0 without an own term), then
    acc = fma(s_hit, psi(p_i, q_j), acc) over the j < ql with near_hit[j] == i in ascending j (chamfer_ref._chain32's walk)."""
    out = np.zeros_like(P)
    if pl == 0 or ql == 0:
        return out
    acc = np.zeros((pl, 3), np.float32)
    if s_own is not None:
        j = np.clip(np.asarray(near_own[:pl], np.int64), 0, ql - 1)
        acc = (np.float32(s_own) * psi32(P[:pl], Q[j], signed)).astype(np.float32)
    if s_hit is not None:
        owner = np.asarray(near_hit[:ql], np.int64)
        j = np.flatnonzero((owner >= 0) & (owner < pl))
        j = j[np.argsort(owner[j], kind="stable")]
        o = owner[j]
        rank = np.arange(len(j)) - np.searchsorted(o, o, side="left")
        for r in range(int(rank.max()) + 1 if len(j) else 0):
            at = rank == r
            oo, jj = o[at], j[at]
            acc[oo] = fma32(np.float32(s_hit), psi32(P[oo], Q[jj], signed), acc[oo])
    out[:pl] = acc
    return out


def normals32(NX, NY, x_lengths, y_lengths, nearest_x, nearest_y, signed=False, scale_x=None, scale_y=None):
    """term_x, term_y and (with scale_x) dNX, dNY in the defined float32 order through the GIVEN indices; nearest_y None: the x
    direction alone."""
    NX, NY = np.asarray(NX, np.float32), np.asarray(NY, np.float32)
    b, n, m = NX.shape[0], NX.shape[1], NY.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    out = {"term_x": np.zeros((b, n), np.float32), "term_y": np.zeros((b, m), np.float32), "dNX": np.zeros_like(NX), "dNY": np.zeros_like(NY)}
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        ix = np.clip(np.asarray(nearest_x[k, :nb], np.int64), 0, mb - 1)
        out["term_x"][k, :nb] = term32(NX[k, :nb], NY[k, ix], signed)
        iy = None
        if nearest_y is not None:
            iy = nearest_y[k]
            out["term_y"][k, :mb] = term32(NY[k, :mb], NX[k, np.clip(np.asarray(iy[:mb], np.int64), 0, nb - 1)], signed)
        if scale_x is not None:
            sx, sy = scale_x[k], None if nearest_y is None else scale_y[k]
            out["dNX"][k] = _chain32(NX[k], NY[k], nb, mb, nearest_x[k], iy, sx, sy, signed)
            out["dNY"][k] = _chain32(NY[k], NX[k], mb, nb, iy, nearest_x[k], sy, sx, signed)
    return out


# ---- the figures -----------------------------------------------------------------------------------------------------------------
def figures(c, got, signed, single=False):
    """The figures of one fixture case for the results `got`: nearest_x (nearest_y), term_x (term_y), rows_n or loss_n (the per-cloud
    sum of the two rows), and dNX / dNY for the scales got["scale_x"], got["scale_y"] (default: scales(b)); an entry may be missing."""
    b, n, m = c["b"], c["n"], c["m"]
    nl, ml = lengths_of(c["x_lengths"], b, n), lengths_of(c["y_lengths"], b, m)
    sx, sy = got.get("scale_x", scales(b)[0]), got.get("scale_y", scales(b)[1])
    f = {"term": 0.0, "rows_n": 0.0, "grad": 0.0, "exact": 0.0}
    near_x, near_y = np.asarray(got["nearest_x"], np.int64), None if single else np.asarray(got["nearest_y"], np.int64)
    for side, near, pl, ql in (("x", near_x, nl, ml),) + (() if single else (("y", near_y, ml, nl),)):
        for k in range(b):
            pb, qb = (int(pl[k]), int(ql[k])) if pl[k] > 0 and ql[k] > 0 else (0, 0)
            if (near[k, pb:] != -1).any() or (pb and (near[k, :pb].min() < 0 or near[k, :pb].max() >= qb)):
                f["exact"] = np.inf
                return f
            if "term_" + side in got and (np.asarray(got["term_" + side])[k, pb:] != 0).any():        # padded slots, empty clouds
                f["exact"] = np.inf
    want = normals64(c["NX"], c["NY"], c["x_lengths"], c["y_lengths"], near_x, near_y, signed, sx, None if single else sy)
    for side in ("x",) if single else ("x", "y"):
        if "term_" + side in got:
            t = np.asarray(got["term_" + side], np.float64)
            f["term"] = max(f["term"], float(np.abs(t - want["term_" + side]).max()) if np.isfinite(t).all() else np.inf)
    if "rows_n" in got:
        r = np.asarray(got["rows_n"], np.float64)
        f["rows_n"] = float(np.abs(r - want["rows_n"]).max()) if np.isfinite(r).all() else np.inf
        if single and (r[:, 1] != 0).any():
            f["exact"] = np.inf
    if "loss_n" in got:
        r = np.asarray(got["loss_n"], np.float64)
        f["loss_n"] = float(np.abs(r - want["rows_n"].sum(1)).max()) if np.isfinite(r).all() else np.inf
    for key, scale in (("dNX", "SX"), ("dNY", "SY")):
        if got.get(key) is not None:
            f["grad"] = max(f["grad"], cref._relative(got[key], want[key], np.broadcast_to(want[scale], want[key].shape)))
    return f


# ---- G31 -----------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _random_normals(rng, n):
    return (_unit(rng, n) * 2.0 ** rng.uniform(-10, 10, (n, 1))).astype(np.float32)


def small_cosines(NX, NY, x_lengths, y_lengths, nearest_x, nearest_y):
    """The pairs (direction, cloud, point) whose float64 cosine through the given indices lies in (0, MIN_COSINE)."""
    b, n, m = NX.shape[0], NX.shape[1], NY.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    bad = []
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        for side, own, other, idx in (("x", NX[k, :nb], NY[k], nearest_x[k, :nb]), ("y", NY[k, :mb], NX[k], nearest_y[k, :mb])):
            c = np.abs(cosine64(own, other[np.asarray(idx, np.int64)])[0])
            bad += [(side, k, int(i)) for i in np.flatnonzero((c > 0) & (c < MIN_COSINE))]
    return bad


def axis_normals(count, axes, shift):
    """Axis-aligned normals of power-of-two length and both signs, a formula of the index: point i lies along axes[i % len(axes)]."""
    i = np.arange(count) + shift
    out = np.zeros((count, 3), np.float32)
    out[np.arange(count), np.asarray(axes)[i % len(axes)]] = (np.where(i % 2 == 0, 1.0, -1.0) * 2.0 ** (i % 21 - 10)).astype(np.float32)
    return out


def derive(family, NX, NY):
    """The normals of a family that shares another geometry's arrays (a formula, nothing stored): flipped negates every second ny;
    orthogonal puts NX along x and NY along y or z; degenerate zeroes every third normal and fills the LAST cloud's normals with NaN
    and infinities (one component of every fifth / seventh)."""
    NX, NY = NX.copy(), NY.copy()
    if family == "flipped":
        NY[:, 1::2] = -NY[:, 1::2]
    elif family == "orthogonal":
        NX[:] = axis_normals(NX.shape[1], (0,), 0)[None]
        NY[:] = axis_normals(NY.shape[1], (1, 2), 3)[None]
    elif family == "degenerate":
        NX[:, 0::3], NY[:, 1::3] = 0, 0
        NX[-1, 1::5, 0], NX[-1, 2::7, 1] = np.nan, np.inf
        NY[-1, 0::5, 2], NY[-1, 3::7, 0] = -np.inf, np.nan
    return NX, NY


def generate(seed=31):
    """The arrays of g31_chamfer_normals.npz (tools/gen_golden.py g31 saves them).  Per stored geometry: X, Y, NX, NY float32 (the
    sphere's normals are its points' directions and are not stored), the ragged lengths, and per (geometry, lengths) the float64
    search's indices as int16.  The flipped, orthogonal and degenerate families share a stored geometry's arrays (derive)."""
    rng = np.random.default_rng(seed)
    out, names, redraws = {}, [], 0

    def add(name, family, X, Y, NX, NY, xl=None, yl=None, store_normals=True):
        nonlocal redraws
        X, Y = X.astype(np.float32), Y.astype(np.float32)
        variants = (("full", None, None),) + ((("ragged", xl, yl),) if xl is not None else ())
        found = {tag: cref.chamfer64(X, Y, a, c) for tag, a, c in variants}
        while store_normals:                                                        # the cosine condition: redraw an offending normal
            bad = [p for tag, a, c in variants for p in small_cosines(NX, NY, a, c, found[tag]["nearest_x"], found[tag]["nearest_y"])]
            if not bad:
                break
            for side, k, i in bad:
                (NX if side == "x" else NY)[k, i] = _random_normals(rng, 1)[0]
                redraws += 1
        out[name + "/X"], out[name + "/Y"] = X, Y
        if store_normals:
            out[name + "/NX"], out[name + "/NY"] = NX, NY
        out[name + "/family"] = np.int32(FAMILIES.index(family))
        names.append(name)
        for tag, a, c in variants:
            if a is not None:
                out[name + "/x_lengths"], out[name + "/y_lengths"] = a.astype(np.int32), c.astype(np.int32)
            out["%s/%s/nearest_x" % (name, tag)] = found[tag]["nearest_x"].astype(np.int16)
            out["%s/%s/nearest_y" % (name, tag)] = found[tag]["nearest_y"].astype(np.int16)

    for n, m in SIZES:
        X = np.stack([cref._ball(rng, n) for _ in range(B)])
        Y = np.stack([cref._ball(rng, m) for _ in range(B)])
        xl = np.array([0, max(n // 2, 1), n, rng.integers(1, n + 1)])
        yl = np.array([max(m // 3, 1), 0, 1, rng.integers(1, m + 1)])
        add("random_%dx%d" % (n, m), "random", X, Y, np.stack([_random_normals(rng, n) for _ in range(B)]),
            np.stack([_random_normals(rng, m) for _ in range(B)]), xl, yl)
    # sphere: Y on the unit sphere, X a noisy copy of some of it; the normals are radial (the points' own directions, not stored)
    n, m = 257, 1025
    Y = _unit(rng, m)[None]
    X = Y[:, rng.permutation(m)[:n]] + 1e-3 * rng.standard_normal((1, n, 3))
    add("sphere_%dx%d" % (n, m), "sphere", X, Y, None, None, store_normals=False)
    # subset: X inside Y, every point twice in Y with DIFFERENT normals on the two copies: the first-index tie rule shows in term_x
    n, m = 100, 300
    Y = cref._ball(rng, m)[None].astype(np.float32)
    Y[0, m // 2:] = Y[0, :m // 2]
    pick = rng.permutation(m // 2)[:n][None]
    add("subset_%dx%d" % (n, m), "subset", Y[:, pick[0]], Y, _random_normals(rng, n)[None], _random_normals(rng, m)[None])
    out["subset_%dx%d/pick" % (n, m)] = pick.astype(np.int16)
    # many-to-one: every y lies within 1e-2 of x_0 = 0 (no closer than 2e-3), the other x are one unit away
    n, m = 65, 1025
    Y = (_unit(rng, m) * rng.uniform(2e-3, 9e-3, (m, 1)))[None]
    X = _unit(rng, n)[None].copy()
    X[0, 0] = 0
    add("many_to_one_%dx%d" % (n, m), "many_to_one", X, Y, _random_normals(rng, n)[None], _random_normals(rng, m)[None])
    out["names"] = np.array(names)
    out["redraws"] = np.int32(redraws)
    return out


SHARED = (("flipped", "sphere_257x1025"), ("orthogonal", "random_257x1025"), ("degenerate", "random_256x1024"))


def g31():
    return np.load(GOLDEN)


def cases(z):
    """One dict per (family, geometry, lengths): name, family, geometry, lengths, X, Y, NX, NY, x_lengths, y_lengths (None: full), b, n,
    m, the fixture's float64 indices nearest_x, nearest_y (int64) and pick (the subset family's)."""
    out = []
    stored = [(FAMILIES[int(z[name + "/family"])], name) for name in (str(s) for s in z["names"])]
    for family, name in stored + list(SHARED):
        X, Y = z[name + "/X"], z[name + "/Y"]
        if name + "/NX" in z.files:
            NX, NY = z[name + "/NX"], z[name + "/NY"]
        else:                                              # the sphere: radial normals
            NX, NY = (X / np.linalg.norm(X.astype(np.float64), axis=-1, keepdims=True)).astype(np.float32), Y.copy()
        NX, NY = derive(family, NX, NY)
        for tag in ("full", "ragged"):
            if tag == "ragged" and name + "/x_lengths" not in z.files:
                continue
            xl, yl = (z[name + "/x_lengths"], z[name + "/y_lengths"]) if tag == "ragged" else (None, None)
            out.append({"name": "%s:%s/%s" % (family, name, tag), "family": family, "geometry": name, "lengths": tag, "X": X, "Y": Y, "NX": NX,
                        "NY": NY, "x_lengths": xl, "y_lengths": yl, "b": X.shape[0], "n": X.shape[1], "m": Y.shape[1],
                        "nearest_x": z["%s/%s/nearest_x" % (name, tag)].astype(np.int64),
                        "nearest_y": z["%s/%s/nearest_y" % (name, tag)].astype(np.int64),
                        "pick": z[name + "/pick"].astype(np.int64) if name + "/pick" in z.files else None})
    return out
