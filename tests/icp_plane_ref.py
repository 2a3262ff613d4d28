"""Shared by tests/test_icp_plane_host.py, tests/test_gpu_icp_plane.py and tools/gen_golden.py (G30): icp_align_plane restated in float64
with a numpy solve, and the fixture's layout.

    One iteration from the pose (R, t):  x_i = R p_i + t;  j(i), d_i = icp_ref.nearest64(x, Q);  n_i = normals[j(i)];
        w'_i = w_i [d_i <= max_distance] [n_i != 0];  c = x_0;  a_i = x_i - c;  e_i = x_i - q_j(i);  r_i = n_i . e_i;  J_i = (a_i x n_i, n_i);
        A = sum w' J J^T with its diagonal scaled by (1 + damping),  g = sum w' J r,  delta = -A^-1 g = (omega, v);
        dR = cayley64(omega),  R' = the rotation closest to dR R (an initial pose need not be orthogonal to the last bit),  t' = dR (t - c) + c + v;
        rmse = sqrt(sum w' r^2 / sum w'),  rmse_point = sqrt(sum w' d^2 / sum w'),  inliers = #{w' > 0} -- at the pose the iteration started from.
    With damping > 0 a column whose diagonal entry is exactly 0 (J_k = 0 on every inlier, hence g_k = 0) is left out: delta_k = 0.
A step is UNIQUE when it has at least 6 inliers and the equilibrated condition number cond(D A D), D = diag(A)^-1/2, is at most
COND_MAX; only unique steps are compared as numbers, the others are held to properties (include/so3proj.h calls them unsolved when a
float32 pivot fails, which is the implementation's own, coarser, view of the same thing)."""
import os

import numpy as np

import icp_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_icp_plane.npz")
SIZES = icp_ref.SIZES
SMALL_SIZES = icp_ref.SMALL_SIZES
WEIGHTS = icp_ref.WEIGHTS
OFFSETS = icp_ref.OFFSETS
MARGIN = icp_ref.MARGIN
COND_MAX = 1e3
MIN_INLIERS = 6
KINDS = ("step", "degenerate", "converge", "compare")
AXES = {"ellipsoid": (1.0, 0.7, 0.5), "blob": (0.9, 0.8, 0.45)}

nearest64, pose_points, gather, dist_to = icp_ref.nearest64, icp_ref.pose_points, icp_ref.gather, icp_ref.dist_to


def hat(h):
    return np.array([[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]])


def cayley64(omega):
    """I + (2 / (1 + s)) (hat(h) + hat(h)^2), h = omega / 2, s = |h|^2: the rotation of the quaternion (1, h)."""
    h = np.asarray(omega, np.float64) / 2
    K = hat(h)
    return np.eye(3) + (2.0 / (1.0 + h @ h)) * (K + K @ K)


def project64(M):
    """The rotation closest to M (the SVD projection)."""
    u, _, vt = np.linalg.svd(M)
    return u @ np.diag([1.0, 1.0, np.linalg.det(u @ vt)]) @ vt


def ellipsoid_normals(Q, centre, axes, zero_every=0):
    """The analytic normals of the ellipsoid with these semi-axes about `centre` at the directions of the float32 points Q, in float64
    (division and square root only), rounded to float32.  zero_every = k > 0 zeroes the rows j % k == 1."""
    g = (np.asarray(Q, np.float64) - np.asarray(centre, np.float64)) / np.asarray(axes, np.float64) ** 2
    n = g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-300)
    if zero_every:
        n[..., 1::zero_every, :] = 0.0
    return n.astype(np.float32)


def equilibrated_cond(A):
    d = np.sqrt(np.diag(A))
    if (d <= 0).any() or not np.isfinite(A).all():
        return np.inf
    return float(np.linalg.cond(A / np.outer(d, d)))


def step_from(P, Q, Nrm, idx, d, R, t, w=None, max_distance=None, damping=0.0):
    """The second half of an iteration in float64, given the correspondences idx and their distances d.  Returns a dict of per-cloud
    arrays: R, t (kept where the step is not live or cond is infinite), rmse, rmse_point, inliers, W, cond, unique, wp, A (B,6,6, damped),
    g (B,6), pbar, qbar (weighted centroids of the posed source and the matched target: the scale of the translation's norm)."""
    P64 = np.asarray(P, np.float64)
    b, n, _ = P64.shape
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    X = pose_points(P64, R, t)
    Qj, Nj = gather(Q, idx, b), gather(Nrm, idx, b)
    wp = np.ones((b, n)) if w is None else np.asarray(w, np.float64).copy()
    if max_distance is not None:
        wp = wp * (d <= max_distance)
    wp = wp * (Nj != 0).any(-1)
    out = {k: [] for k in ("R", "t", "rmse", "rmse_point", "inliers", "W", "cond", "unique", "A", "g", "pbar", "qbar")}
    for k in range(b):
        c = X[k, 0]
        a, e = X[k] - c, X[k] - Qj[k]
        r = (Nj[k] * e).sum(-1)
        J = np.concatenate([np.cross(a, Nj[k]), Nj[k]], 1)
        W = wp[k].sum()
        A = np.einsum("i,ik,il->kl", wp[k], J, J)
        A[np.diag_indices(6)] *= 1.0 + damping
        g = (wp[k] * r) @ J
        keep = np.ones(6, bool) if damping == 0 else np.diag(A) != 0
        live = W > 0
        cond = equilibrated_cond(A[np.ix_(keep, keep)]) if live and keep.any() else np.inf
        Rn, tn = R[k], t[k]
        if live and cond < 1e12:
            delta = np.zeros(6)
            delta[keep] = -np.linalg.solve(A[np.ix_(keep, keep)], g[keep])
            dR = cayley64(delta[:3])
            Rn, tn = project64(dR @ R[k]), dR @ (t[k] - c) + c + delta[3:]
        inl = int((wp[k] > 0).sum())
        out["R"].append(Rn); out["t"].append(tn); out["W"].append(W); out["cond"].append(cond); out["A"].append(A); out["g"].append(g)      # noqa: E702
        out["rmse"].append(np.sqrt((wp[k] * r * r).sum() / W) if live else 0.0)
        out["rmse_point"].append(np.sqrt((wp[k] * d[k] ** 2).sum() / W) if live else 0.0)
        out["inliers"].append(inl)
        out["unique"].append(bool(live and inl >= MIN_INLIERS and cond <= COND_MAX))
        out["pbar"].append(wp[k] @ X[k] / W if live else np.zeros(3))
        out["qbar"].append(wp[k] @ Qj[k] / W if live else np.zeros(3))
    res = {k: np.array(v) for k, v in out.items()}
    res["wp"] = wp
    return res


def icp_plane64(P, Q, Nrm, R0=None, t0=None, iterations=10, max_distance=None, w=None, damping=0.0, device="cpu"):
    """The whole loop in float64: R, t, rmse, rmse_point, inliers, unique (iterations,B), nearest and dist of the last search."""
    b = len(P)
    R = np.broadcast_to(np.eye(3), (b, 3, 3)).copy() if R0 is None else np.asarray(R0, np.float64)
    t = np.zeros((b, 3)) if t0 is None else np.asarray(t0, np.float64)
    hist = {k: [] for k in ("rmse", "rmse_point", "inliers", "unique", "cond")}
    idx = d = None
    for _ in range(iterations):
        d, idx = nearest64(pose_points(P, R, t), Q, device)
        s = step_from(P, Q, Nrm, idx, d, R, t, w, max_distance, damping)
        R, t = s["R"], s["t"]
        for k in hist:
            hist[k].append(s[k])
    return {"R": R, "t": t, "nearest": idx, "dist": d, **{k: np.array(v).reshape(iterations, b) for k, v in hist.items()}}


def plane_rmse64(P, Q, Nrm, R, t, device="cpu"):
    """The float64 point-to-plane rmse of a pose (B,): unweighted, untrimmed, over the float64 nearest neighbours -- the judge of the
    comparison case, for poses from any method."""
    X = pose_points(P, R, t)
    _, idx = nearest64(X, Q, device)
    r = (gather(Nrm, idx, len(X)) * (X - gather(Q, idx, len(X)))).sum(-1)
    return np.sqrt((r * r).mean(1))


# ---- the fixture: arrays of case i under the prefix "c<i>_" -------------------------------------------------------------------
ARRAYS = ("P", "Q", "Nrm", "w", "R0", "t0", "Rgt", "tgt", "R", "t", "rmse", "rmse_point", "inliers", "cond", "unique", "plateau")      # and "perm"


def g30():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def cases(d):
    """The fixture's cases as dicts.  Always: kind, name, n, m, b, shared, weights, offset, iterations, max_distance (None: no trimming),
    damping, surface, P, Q, Nrm (stored, or the analytic normals of the case's ellipsoid about its centre); w, R0, t0 are None where the
    call is made without them; the float64 answers under the names of ARRAYS."""
    out = []
    kinds, wnames = [str(s) for s in d["kind_names"]], [str(s) for s in d["weight_names"]]
    for i in range(len(d["case_kind"])):
        md = float(d["case_max_distance"][i])
        c = {"kind": kinds[int(d["case_kind"][i])], "name": str(d["case_name"][i]), "weights": wnames[int(d["case_weights"][i])],
             "offset": float(d["case_offset"][i]), "iterations": int(d["case_iterations"][i]), "max_distance": None if md < 0 else md,
             "shared": bool(d["case_shared"][i]), "damping": float(d["case_damping"][i]), "surface": str(d["case_surface"][i]),
             "zero_every": int(d["case_zero_every"][i]), "centre": d["case_centre"][i], "expect_solved": int(d["case_expect_solved"][i])}
        for k in ARRAYS + ("perm",):
            c[k] = d.get("c%d_%s" % (i, k))
        if c["Nrm"] is None:
            c["Nrm"] = ellipsoid_normals(c["Q"], c["centre"], AXES[c["surface"]], c["zero_every"])
        c["b"], c["n"], c["m"] = c["P"].shape[0], c["P"].shape[1], c["Q"].shape[-2]
        out.append(c)
    return out


# ---- the generator (tools/gen_golden.py g30) -----------------------------------------------------------------------------------
def generate(seed=30):
    """G30.  No reference code exists, so the fixture holds the inputs and the answers of this file's float64 restatement.  What the
    generator asserts about its own cases is what the tests rely on: the trimming margin of every trimmed step, that at most 5 % of
    the random steps with N >= MIN_INLIERS are not unique, that the exact plane and the exact sphere are not unique, exact
    convergence within 10 float64 iterations, and the comparison case's property (point-to-plane reaches its plateau in k iterations,
    point-to-point from the same start has not in 3 k)."""
    rng = np.random.default_rng(seed)
    cases_ = []

    def unit(*shape):
        d = rng.standard_normal(shape + (3,))
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    def surface(kind, n, centre):
        pts = unit(n) * np.array(AXES[kind])
        if kind == "blob":
            pts = pts + 0.01 * rng.standard_normal((n, 3))
        return pts + centre

    def small_motion(angle, shift, centre):
        R = cayley64(unit()[0:3] * rng.uniform(0.25 * angle, angle))
        return R, centre - R @ centre + unit() * rng.uniform(0.25 * shift, shift)

    def add(kind, name, P, Q, Nrm=None, w=None, R0=None, t0=None, iterations=1, max_distance=None, weights="none", offset=0.0, damping=0.0,
            surface_="ellipsoid", zero_every=0, centre=(0.0, 0.0, 0.0), expect_solved=-1, **answers):
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        c = dict(kind=kind, name=name, P=f32(P), Q=f32(Q), w=f32(w), R0=f32(R0), t0=f32(t0), iterations=iterations, max_distance=max_distance,
                 weights=weights, offset=offset, damping=damping, surface=surface_, zero_every=zero_every, centre=np.asarray(centre, np.float64),
                 shared=np.ndim(Q) == 2, expect_solved=expect_solved, stored_normals=Nrm is not None, **answers)
        c["Nrm"] = f32(Nrm) if Nrm is not None else ellipsoid_normals(c["Q"], c["centre"], AXES[surface_], zero_every)
        cases_.append(c)
        return c

    def start(c):
        b = len(c["P"])
        if c["R0"] is None:
            return np.broadcast_to(np.eye(3), (b, 3, 3)).copy(), np.zeros((b, 3))
        return c["R0"].astype(np.float64), c["t0"].astype(np.float64)

    # ---- single steps ---------------------------------------------------------------------------------------------------------
    random_steps = []

    def step_case(n, m, weights, trimmed, offset, axis, shared=False, b=1, kind="ellipsoid", zero_every=0, identity=False, empty=False):
        centre = offset * np.eye(3)[axis]
        q_shared = surface(kind, m, centre)
        P, Q, W, R0, T0 = [], [], [], [], []
        for _ in range(b):
            src = surface(kind, n, centre)
            if trimmed and n >= 32:                               # a quarter of the source lies off the surface, beyond the threshold
                far = rng.uniform(0, 1, n) < 0.25
                src[far] = centre + 1.4 * (src[far] - centre)
            r0, t0 = small_motion(0.05, 0.03, centre)
            P.append((src - t0) @ r0 if identity else src)        # identity start: p = R0^T (src - t0), so that the pose to find is (R0, t0)
            R0.append(r0); T0.append(t0)                          # noqa: E702
            Q.append(q_shared if shared else surface(kind, m, centre))
            W.append(None if weights == "none" else rng.uniform(0.05, 1.0, n) if weights == "random" else (rng.uniform(0, 1, n) < 0.7).astype(np.float64))
        name = "step %dx%d %s %s %s off %g%s%s%s" % (n, m, kind, weights, "trimmed" if trimmed else "all", offset, " shared" if shared else "",
                                                      " zeros" if zero_every else "", " empty" if empty else "")
        c = add("step", name, np.stack(P), q_shared if shared else np.stack(Q), None, None if weights == "none" else np.stack(W),
                None if identity else np.stack(R0), None if identity else np.stack(T0), weights=weights, offset=offset, surface_=kind,
                zero_every=zero_every, centre=centre)
        R0_, t0_ = start(c)
        d, idx = nearest64(pose_points(c["P"], R0_, t0_), c["Q"])
        if trimmed or empty:
            flat = np.sort(d.reshape(-1))
            md = None
            if empty:
                md = 0.5 * flat[0]
            else:
                for k in range(max(1, int(0.6 * len(flat))), len(flat)):
                    if flat[k] - flat[k - 1] > 4 * MARGIN:
                        md = 0.5 * (flat[k] + flat[k - 1])
                        break
                if md is None:
                    md = flat[-1] + 0.01
            c["max_distance"] = float(np.float32(md))
            assert np.abs(d - c["max_distance"]).min() > MARGIN and c["max_distance"] > MARGIN, (name, md)
        s = step_from(c["P"], c["Q"], c["Nrm"], idx, d, R0_, t0_, c["w"], c["max_distance"])
        if empty:
            assert (s["inliers"] == 0).all() and (s["rmse"] == 0).all() and np.array_equal(s["R"], R0_) and np.array_equal(s["t"], t0_)
        elif n >= MIN_INLIERS:
            random_steps.extend(s["unique"].tolist())
        c.update({k: s[k] for k in ("R", "t", "rmse", "rmse_point", "inliers", "cond", "unique")})
        print("g30 %-58s cond %s  unique %s" % (name, " ".join("%.1e" % v for v in s["cond"]), s["unique"].astype(int)))
        return c

    for n, m in SMALL_SIZES:
        for wi, wk in enumerate(WEIGHTS):
            for trimmed in (False, True):
                for ax, off in enumerate(OFFSETS):
                    step_case(n, m, wk, trimmed, off, ax, shared=(wi + ax) % 2 == 1, b=2, kind=("ellipsoid", "blob")[(wi + ax + trimmed) % 2],
                              identity=wk == "none" and off == 0.0 and not trimmed)
    for i, (n, m) in enumerate(SIZES[2:]):                         # a covering selection at the large sizes
        for j, wk in enumerate(WEIGHTS):
            shared = (i + j) % 2 == 1
            step_case(n, m, wk, (i + j) % 2 == 1, OFFSETS[(i + j) % 3], (i + j) % 3, shared=shared, b=2 if shared and n < 1000 else 1,
                      kind=("ellipsoid", "blob")[(i + j // 2) % 2], zero_every=3 if j == 1 else 0, identity=j == 0 and i == 0)
    step_case(256, 1024, "mask", False, 0.0, 0, empty=True)
    step_case(3, 7, "none", False, 10.0, 2, empty=True, b=2)
    share = 1.0 - np.mean(random_steps)
    print("g30: %d random steps with N >= %d, %.1f %% not unique" % (len(random_steps), MIN_INLIERS, 100 * share))
    assert share <= 0.05, share

    # ---- degenerate systems: the exact lattice plane (undamped and damped) and the exact sphere about its centre -----------------------
    gx, gy = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    lattice = np.stack([gx.reshape(-1) / 8.0, gy.reshape(-1) / 8.0, np.zeros(144)], 1)
    up = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (144, 3))
    picks = np.stack([rng.permutation(144)[:60] for _ in range(2)])
    above = lattice[picks] + np.array([1 / 64.0, 1 / 32.0, 1 / 8.0])          # every point an eighth above its own lattice point, far from a tie
    for damping, expect in ((0.0, 0), (0.1, 1)):
        c = add("degenerate", "plane n=(0,0,1) damping %g" % damping, above, lattice, up, damping=damping, expect_solved=expect)
        d, idx = nearest64(c["P"], c["Q"])
        assert np.array_equal(idx, picks) and np.array_equal(c["P"].astype(np.float64), above)
        s = step_from(c["P"], c["Q"], c["Nrm"], idx, d, *start(c), damping=damping)
        assert (s["unique"] == bool(expect)).all(), s["cond"]
        assert damping > 0 or (s["cond"] == np.inf).all()
        c.update({k: s[k] for k in ("R", "t", "rmse", "rmse_point", "inliers", "cond", "unique")})
    r = np.arange(-65, 66)
    a, b_, c_ = np.meshgrid(r, r, r, indexing="ij")
    on = np.stack([x[a * a + b_ * b_ + c_ * c_ == 65 * 65] for x in (a, b_, c_)], 1).astype(np.float64)      # integer points of the sphere of radius 65
    centre = np.array([0.5, -0.25, 1.0])
    sphere = centre + on / 64.0
    picks = np.stack([rng.permutation(len(on))[:80] for _ in range(2)])
    c = add("degenerate", "sphere about its centre", sphere[picks], sphere, on / 64.0, expect_solved=0, centre=centre)
    d, idx = nearest64(c["P"], c["Q"])
    assert (d == 0).all() and np.array_equal(idx, picks) and np.array_equal(c["Q"].astype(np.float64), sphere)
    s = step_from(c["P"], c["Q"], c["Nrm"], idx, d, *start(c))
    assert not s["unique"].any() and (s["cond"] > 1e12).all(), s["cond"]
    c.update({k: s[k] for k in ("R", "t", "rmse", "rmse_point", "inliers", "cond", "unique")})

    # ---- exact convergence: Q = T_gt P EXACTLY in float32 (G21's construction), ellipsoid normals in float64, forty extra targets -------
    c5, s5 = 3.0 / 5.0, 4.0 / 5.0
    rz5, rx5 = np.array([[c5, -s5, 0], [s5, c5, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0], [0, c5, -s5], [0, s5, c5]])
    r_exact = [rz5 @ rx5, (rz5 @ rx5).T, rx5 @ rz5, (rx5 @ rz5).T]
    axes = np.array(AXES["ellipsoid"])
    n, extra, quantum = 300, 40, 25 * 2.0**-14
    P, Q, NR, R0, T0, RG, TG, PERM = [], [], [], [], [], [], [], []
    for cloud in range(2):
        pts = []
        while len(pts) < n:
            cand = np.round(unit()[0:3] * axes / quantum) * quantum
            if all(np.linalg.norm(cand - o) >= 0.1 for o in pts):
                pts.append(cand)
        p = np.array(pts)
        r_gt, t_gt = r_exact[cloud], np.round(rng.uniform(-0.5, 0.5, 3) * 2**14) / 2**14
        slots = rng.permutation(n + extra)
        q, nr = np.zeros((n + extra, 3)), np.zeros((n + extra, 3))
        q[slots[:n]] = (np.round(p * 2.0**14 / 25) @ np.round(25 * r_gt).T) * 2.0**-14 + t_gt
        g = p / axes**2
        nr[slots[:n]] = (g / np.linalg.norm(g, axis=1, keepdims=True)) @ r_gt.T
        far = unit(extra)
        q[slots[n:]] = (t_gt + far * rng.uniform(1.5, 2.0, (extra, 1))).astype(np.float32)
        nr[slots[n:]] = far
        dr, dt = small_motion(0.035, 0.02, np.zeros(3))
        P.append(p); Q.append(q); NR.append(nr); R0.append(r_gt @ dr); T0.append(t_gt + dt); RG.append(r_gt); TG.append(t_gt); PERM.append(slots[:n])      # noqa: E702
    c = add("converge", "converge exact superset", np.stack(P), np.stack(Q), np.stack(NR), None, np.stack(R0), np.stack(T0), iterations=20, max_distance=0.2)
    assert np.array_equal(c["P"].astype(np.float64), np.stack(P)) and np.array_equal(c["Q"].astype(np.float64), np.stack(Q))
    ans = icp_plane64(c["P"], c["Q"], c["Nrm"], c["R0"], c["t0"], 20, 0.2)
    print("g30 converge rmse", " ".join("%.1e" % v for v in ans["rmse"][:8, 0]), " cond %.1e" % ans["cond"].max())
    assert (ans["rmse"][9:] < 1e-12).all() and np.array_equal(ans["nearest"], np.stack(PERM)) and ans["unique"].all() and (ans["inliers"] == n).all()
    assert np.abs(ans["R"] - np.stack(RG)).max() < 1e-12 and np.abs(ans["t"] - np.stack(TG)).max() < 1e-12
    c.update(Rgt=np.stack(RG), tgt=np.stack(TG), perm=np.stack(PERM).astype(np.int32), **{k: ans[k] for k in ("R", "t", "rmse", "rmse_point", "inliers")})

    # ---- the comparison case: a smooth surface, the target sampled densely and differently from the source, 0.15 rad and 0.1 off ---------
    b, n, m = 2, 300, 1000
    P, Q = np.stack([surface("ellipsoid", n, 0.0) for _ in range(b)]), np.stack([surface("ellipsoid", m, 0.0) for _ in range(b)])
    R0, T0 = np.stack([cayley64(unit()[0:3] * 0.15) for _ in range(b)]), unit(b) * 0.1
    c = add("compare", "compare 0.15 rad 0.1 off", P, Q, None, None, R0, T0)
    R0_, t0_ = start(c)
    E, R, t = [], R0_, t0_
    for _ in range(40):
        s = icp_plane64(c["P"], c["Q"], c["Nrm"], R, t, 1)
        R, t = s["R"], s["t"]
        E.append(plane_rmse64(c["P"], c["Q"], c["Nrm"], R, t))
    E = np.array(E)
    plateau = E[-1]
    k = 1 + int(np.max([np.argmax(E[:, i] <= 1.1 * plateau[i]) for i in range(b)]))
    pt = icp_ref.icp64(c["P"], c["Q"], R0_, t0_, 3 * k)
    e_point = plane_rmse64(c["P"], c["Q"], c["Nrm"], pt["R"], pt["t"])
    print("g30 compare: plateau %s reached in k = %d; point-to-point after %d: %s" % (plateau, k, 3 * k, e_point))
    assert k <= 12 and (E[k - 1] <= 1.1 * plateau).all() and (e_point > 2.0 * plateau).all(), (k, E[:, 0], e_point)
    c.update(iterations=k, plateau=plateau)

    arrays = {}
    for i, c in enumerate(cases_):
        for key in ARRAYS + ("perm",):
            if c.get(key) is not None and not (key == "Nrm" and not c["stored_normals"]):
                arrays["c%d_%s" % (i, key)] = c[key]
    wn = list(WEIGHTS)
    print("g30: %d cases" % len(cases_))
    return dict(kind_names=np.array(KINDS), weight_names=np.array(wn), case_kind=np.array([KINDS.index(c["kind"]) for c in cases_], np.int32),
                case_name=np.array([c["name"] for c in cases_]), case_weights=np.array([wn.index(c["weights"]) for c in cases_], np.int32),
                case_offset=np.array([c["offset"] for c in cases_]), case_iterations=np.array([c["iterations"] for c in cases_], np.int32),
                case_max_distance=np.array([-1.0 if c["max_distance"] is None else c["max_distance"] for c in cases_]),
                case_shared=np.array([c["shared"] for c in cases_]), case_damping=np.array([c["damping"] for c in cases_]),
                case_surface=np.array([c["surface"] for c in cases_]), case_zero_every=np.array([c["zero_every"] for c in cases_], np.int32),
                case_centre=np.array([c["centre"] for c in cases_]), case_expect_solved=np.array([c["expect_solved"] for c in cases_], np.int32), **arrays)
