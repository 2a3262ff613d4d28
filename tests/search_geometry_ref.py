"""Shared by tests/test_search_geometry_host.py and tests/test_gpu_search_geometry.py: the launch geometry of the two N^2 kernels
(k_add_s, k_icp_step) restated, the shapes that reach every work split of it, the random input families of those shapes, and the exact
(lattice) families with their expected answers.

GEOMETRY.  A work item is 256 U outer points of one cloud, U = rule(B, N, CUs); a cloud is ceil(N / (256 U)) items; at most 64 CUs
workgroups stride over the items; the inner cloud goes through LDS in tiles of 1024 points whose tail is padded to a multiple of 8
with copies of the tile's last point.  cases(cus) evaluates the rule, so the batch sizes follow the device:

    id        B                      N (ADD-S)   (N, M) (ICP / search)     what it reaches [at 256 CUs]
    G1        3                      2500        (2500, 1500)              U = 1, 10 chunks, 3 tiles, last tile 452 points + 4 pads
    G2        smallest with U = 2    1025        (1025, 1023)              [171] 3 chunks, the last with one point; tile 2: 1 point + 7 pads
    G3        smallest with U = 4    1025        (1025, 1023)              [256] 2 chunks, the last record from one real point
    G4        64 CUs + 37            7           (12, 11)                  U = 4, one chunk, items > the grid: the second trip; > 8192 rows
    G5        32 CUs + 5             1025        (1025, 1025)              U = 4, 2 chunks, items = 64 CUs + 10: second trip, multi-tile clouds
    G6-<N>    2                      1023 1024 1025 2047 2049              both sides of the tile and of the unroll (U = 1)
    G7-<N>    2                      255 256 257 1 2 9                     the chunk edge at U = 1; N below the unroll

G2, G3 and G5 share their data: G2 and G3 are the first clouds of G5's batch (the search's targets cut to M = 1023), so the same cloud
runs at U = 1 (in batches of <= 64), 2 and 4.  N = 12 at G4's ICP: with 7 points and trimming too many float64 steps would have fewer
than three inliers (uniqueness below).

RANDOM FAMILIES.  ADD-S and the diameter: the generators of tests/test_gpu_add_metrics.py (unit-sphere clouds, poses about two units
out).  ICP: targets in the unit ball, a source = a target point plus noise of at most 0.03; `posed` cases start from a motion of at
most 2 degrees and 0.02; `trimmed` cases move about 15 % of the source points 1.6 to 2 units out, so that the distances have a gap and
max_distance is chosen in a gap as tools/gen_golden.py's g21_icp does (max_distance_for).  A cloud whose float64 step is not unique
by that generator's own criterion -- fewer than 3 inliers or (s2 + s3) / s1 < 0.1 -- is judged on properties only (unique_step);
test_search_geometry_host.py asserts that this is at most 5 % of a case's clouds, and none at N >= 255.  N < 3 can never be unique:
those two G7 sizes are held to the search's checks and the step's properties.

EXACT FAMILIES.  Coordinates k 2^-6 with |k| <= 64, poses signed permutation matrices with translations on the same lattice: every
product, sum and squared distance is exact in float32, so the float64 answer IS the float32 answer and the first of equal candidates is
decided by integers (lattice_nearest).  identical: T_pred == T_gt, distinct points; ties: duplicates of point 5 at 1023, 1024 and 2048
and of point 1030 at 2047 (N = 2049: across the tiles and in the padded last tile); last_wins: the unique nearest inner point of three
outer points is point N - 1 with N = 1 mod 8, whose padded copies carry indices >= N."""
import functools

import numpy as np

import icp_ref
from f32_exact import first_argmin32, pair_dist2_32

CUS = 256                            # the device the CPU file evaluates the rule for
BLOCK, TILE, UNROLL = 256, 1024, 8
QUANTUM = 2.0 ** -6
ICP_N4, ICP_M4, ADDS_N4 = 12, 11, 7
G6_SIZES = ((1023, 2049), (1024, 1025), (1025, 1024), (2047, 1023), (2049, 2047))       # (N, M)
G7_SIZES = ((255, 1024), (256, 1023), (257, 2049), (1, 9), (2, 1), (9, 7))
IDS = ["G1", "G2", "G3", "G4", "G5"] + ["G6-%d" % n for n, _ in G6_SIZES] + ["G7-%d" % n for n, _ in G7_SIZES]
F64_PAIRS = 1 << 29                  # float64 pairs a GPU test checks per case: above it every k-th cloud (G5: every 32nd)
F32_PAIRS = 1 << 25                  # pairs a GPU test restates in float32 numpy per case (f32_sample; G5 at 256 CUs: every 512th cloud)


# ---- the geometry ---------------------------------------------------------------------------------------------------------------
def rule(b, n, cus):
    u = 4
    while u > 1 and b * ((n + BLOCK * u - 1) // (BLOCK * u)) < 2 * cus:
        u >>= 1
    return u


def chunks(n, u):
    return (n + BLOCK * u - 1) // (BLOCK * u)


def smallest_batch(n, u, cus):
    b = 1
    while rule(b, n, cus) != u:
        b += 1
        assert b <= 4 * cus, (n, u, cus)
    return b


def cases(cus):
    """id -> dict(b, n, m, n_adds, u (ICP and the N = n search), u_adds, items, cap)."""
    shapes = {"G1": (3, 2500, 1500, 2500), "G2": (smallest_batch(1025, 2, cus), 1025, 1023, 1025),
              "G3": (smallest_batch(1025, 4, cus), 1025, 1023, 1025), "G4": (64 * cus + 37, ICP_N4, ICP_M4, ADDS_N4),
              "G5": (32 * cus + 5, 1025, 1025, 1025)}
    shapes.update({"G6-%d" % n: (2, n, m, n) for n, m in G6_SIZES})
    shapes.update({"G7-%d" % n: (2, n, m, n) for n, m in G7_SIZES})
    out = {}
    for k, (b, n, m, na) in shapes.items():
        u, ua = rule(b, n, cus), rule(b, na, cus)
        out[k] = {"id": k, "b": b, "n": n, "m": m, "n_adds": na, "u": u, "u_adds": ua, "items": b * chunks(n, u),
                  "items_adds": b * chunks(na, ua), "cap": 64 * cus}
    return out


def f64_sample(b, pairs_per_cloud, budget=F64_PAIRS):
    """The clouds of a batch that are compared with float64: all of them, or every k-th (k a power of two) within `budget` pairs."""
    k = 1
    while (b + k - 1) // k * pairs_per_cloud > budget:
        k *= 2
    return np.arange(0, b, k)


# ---- the searches' defined float32 bits ---------------------------------------------------------------------------------------
def f32_sample(b, pairs_per_cloud, items, cap, budget=F32_PAIRS):
    """The clouds of a batch whose indices are compared with the float32 restatement: the first, the last and every k-th between, k the
    smallest power of two that keeps the restated pairs within `budget`.  -> (clouds, k).  Work item i of `items` is served on trip
    i // cap of the grid and a cloud's items are consecutive, so with items > cap the last cloud is a second-trip one: asserted."""
    k = 1
    while True:
        keep = np.union1d(np.arange(0, b, k), [b - 1])
        if len(keep) * pairs_per_cloud <= budget:
            break
        k *= 2
    per_cloud = items // b
    assert items == per_cloud * b and (items <= cap or ((keep + 1) * per_cloud - 1 >= cap).any()), (b, items, cap)
    return keep, k


def nearest32(X, Y, pairs_per_pass=1 << 20):
    """add_s_pair's search restated with tests/f32_exact.py: X (c,n,3) float32, Y (c,m,3) or one shared (m,3) -> (c,n) the first index
    of the smallest d^2 = fma(dz, dz, fma(dy, dy, dx * dx)), coordinate differences rounded to float32."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    c, n, m = X.shape[0], X.shape[1], Y.shape[-2]
    out = np.empty((c, n), np.int64)
    rows = max(1, pairs_per_pass // m)
    step = max(1, rows // n)
    for k in range(0, c, step):
        q = Y[None, None] if Y.ndim == 2 else Y[k:k + step, None]
        for lo in range(0, n, rows):
            p = X[k:k + step, lo:lo + rows, None, :]
            out[k:k + step, lo:lo + rows] = first_argmin32(pair_dist2_32(p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]))
    return out


# ---- ADD-S and the diameter: random input ----------------------------------------------------------------------------------------
def adds_inputs(b, n, seed):
    """(tgt, tpred, pts) float32 torch tensors on the CPU, from test_gpu_add_metrics's generators."""
    import test_gpu_add_metrics as gen
    tg, tp = gen._poses(b, "cpu", seed=seed)
    return tg, tp, gen._cloud(b, n, "cpu", seed=seed + 1)


@functools.lru_cache(maxsize=2)
def adds_shared(cus):
    """G5's batch at N = 1025; G2 and G3 take its first clouds."""
    return adds_inputs(32 * cus + 5, 1025, 505)


# ---- ICP and the search: random input --------------------------------------------------------------------------------------------
def _ball(rng, *shape):
    d = rng.standard_normal(shape + (3,))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d * rng.uniform(0, 1, shape + (1,)) ** (1 / 3)


def icp_inputs(b, n, m, seed, weighted=False, trimmed=False, posed=False):
    """dict: Q (b,m,3) own targets, Qs (m,3) one shared target, P / Ps (b,n,3) the sources for either, w, R0, t0 (None where the call
    is made without them), all float32."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Q, Qs = _ball(rng, b, m), _ball(rng, m)
    pick = np.argsort(rng.random((b, m)), axis=1)[:, :n] if n <= m else rng.integers(0, m, (b, n))
    noise = 0.03 * _ball(rng, b, n)
    P, Ps = np.take_along_axis(Q, pick[:, :, None], 1) + noise, Qs[pick] + noise
    if trimmed:
        far = rng.random((b, n)) < 0.15
        out = _ball(rng, b, n)
        out = out / np.linalg.norm(out, axis=-1, keepdims=True) * rng.uniform(1.6, 2.0, (b, n, 1))
        P, Ps = np.where(far[:, :, None], out, P), np.where(far[:, :, None], out, Ps)
    d = {"Q": f32(Q), "Qs": f32(Qs), "P": f32(P), "Ps": f32(Ps), "w": None, "R0": None, "t0": None}
    if weighted:
        d["w"] = f32(rng.uniform(0.05, 1.0, (b, n)))
    if posed:
        axis = _ball(rng, b)
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        ang = np.deg2rad(rng.uniform(0.5, 2.0, b))[:, None, None]
        K = np.zeros((b, 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
        d["R0"] = f32(np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K))
        t = _ball(rng, b)
        d["t0"] = f32(0.02 * t / np.linalg.norm(t, axis=-1, keepdims=True))
    return d


# how each id runs ICP: (weighted, trimmed, posed, iterations); the search alone runs everywhere
ICP_MODE = {"G2": (True, False, True, 1), "G3": (True, False, True, 1), "G4": (True, True, True, 2), "G5": (True, True, True, 2)}
PLAIN = (False, False, False, 1)


def icp_mode(case_id):
    return ICP_MODE.get(case_id, PLAIN)


@functools.lru_cache(maxsize=2)
def icp_shared(cus):
    """G5's batch (N = M = 1025, weighted, trimmed, posed); G2 and G3 take its first clouds with the targets cut to 1023 points."""
    return icp_inputs(32 * cus + 5, 1025, 1025, 2105, weighted=True, trimmed=True, posed=True)


def icp_case_inputs(case, cus):
    """The inputs of one geometry id."""
    k, b, n, m = case["id"], case["b"], case["n"], case["m"]
    weighted, trimmed, posed, _ = icp_mode(k)
    if k in ("G2", "G3", "G5"):
        d = icp_shared(cus)
        return {key: (None if v is None else np.ascontiguousarray(v[:m] if key == "Qs" else v[:b, :m] if key == "Q" else v[:b])) for key, v in d.items()}
    seed = 2100 + IDS.index(k)
    return icp_inputs(b, n, m, seed, weighted, trimmed, posed)


def initial64(d, b):
    if d["R0"] is None:
        return np.broadcast_to(np.eye(3), (b, 3, 3)).copy(), np.zeros((b, 3))
    return d["R0"].astype(np.float64), d["t0"].astype(np.float64)


def gaps(dists):
    """g21_icp's candidates over the float64 distances `dists`, in its order: the middle of every gap wider than 4 MARGIN above the
    60 % quantile, as float32, and last a value behind the largest distance."""
    flat = np.sort(np.ravel(dists))
    k = np.arange(max(1, int(0.6 * len(flat))), len(flat))
    wide = k[flat[k] - flat[k - 1] > 4 * icp_ref.MARGIN]
    out = [float(np.float32(0.5 * (flat[i] + flat[i - 1]))) for i in wide] + [float(np.float32(flat[-1] + 0.01))]
    return [md for md in out if np.abs(flat - md).min() > icp_ref.MARGIN and md > icp_ref.MARGIN]


def max_distance_for(P, Q, w, R0, t0, iterations, device="cpu"):
    """max_distance of a trimmed case, chosen as g21_icp chooses it: the first gap of the first search's float64 distances.  That fixture
    trims single steps; here a later iteration must keep the margin too, so a candidate whose float64 loop brings a distance within
    2 MARGIN of it gives way to the next one.  The gap between the sources near the target and those moved away always qualifies."""
    R0, t0 = np.asarray(R0, np.float64), np.asarray(t0, np.float64)
    first = icp_ref.nearest64(icp_ref.pose_points(P, R0, t0), Q, device)
    for md in gaps(first[0]):
        R, t, (d, idx), ok = R0, t0, first, True
        for it in range(iterations):
            if it > 0:
                d, idx = icp_ref.nearest64(icp_ref.pose_points(P, R, t), Q, device)
            ok = ok and np.abs(d - md).min() > 2 * icp_ref.MARGIN
            if not ok:
                break
            s = icp_ref.step_from(P, Q, idx, d, R, t, w, md)
            R, t = s["R"], s["t"]
        if ok:
            return md
    raise AssertionError("no max_distance keeps the margin")


def unique_step(s):
    """g21_icp's criterion per cloud, from icp_ref.step_from's result: at least 3 inliers and (s2 + s3) / s1 >= 0.1."""
    sv = np.linalg.svd(s["H"], compute_uv=False)
    return ((s["wp"] > 0).sum(1) >= 3) & (sv[:, 0] > 0) & ((sv[:, 1] + sv[:, 2]) / np.maximum(sv[:, 0], 1e-300) >= 0.1)


# ---- the exact families ----------------------------------------------------------------------------------------------------------
def lattice_points(rng, n, lo=-64, hi=64):
    """n DISTINCT integer triples in [lo, hi]^3."""
    side = hi - lo + 1
    code = rng.choice(side ** 3, size=n, replace=False)
    return np.stack([code // (side * side), code // side % side, code % side], 1).astype(np.int64) + lo


def lattice_pose(rng):
    """(R int (3,3) signed permutation with det +1, t int (3,)) in lattice units."""
    R = np.zeros((3, 3), np.int64)
    R[np.arange(3), rng.permutation(3)] = rng.choice([-1, 1], 3)
    if round(np.linalg.det(R)) < 0:
        R[0] = -R[0]
    return R, rng.integers(-128, 129, 3)


def pose_matrix(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t * QUANTUM
    return T


def lattice_nearest(x, y):
    """Integer points x (n,3), y (m,3) -> (d2 int (n,), the FIRST argmin (n,), the number of minimisers (n,)), exactly."""
    d2 = np.empty(len(x), np.int64)
    idx = np.empty(len(x), np.int64)
    cnt = np.empty(len(x), np.int64)
    for lo in range(0, len(x), 512):
        t = ((x[lo:lo + 512, None, :] - y[None, :, :]) ** 2).sum(-1)
        d2[lo:lo + 512], idx[lo:lo + 512] = t.min(1), t.argmin(1)
        cnt[lo:lo + 512] = (t == t.min(1)[:, None]).sum(1)
    return d2, idx, cnt


def lattice_dist(d2):
    """float64 distances of integer squared distances in lattice units."""
    return np.sqrt(d2.astype(np.float64)) * QUANTUM


TIES = {1023: 5, 1024: 5, 2048: 5, 2047: 1030}         # point -> the earlier point it duplicates (N = 2049)


def _tied(k):
    k = k.copy()
    for dup, first in TIES.items():
        k[dup] = k[first]
    return k


def _last_wins(rng, n):
    """Integer cloud (n,3) and the shift (in the object's frame) of the outer cloud: the outer points 0, n // 3 and n - 2 sit one lattice
    step from where the shift puts them next to point n - 1, and every other point is at least 8 steps from that corner."""
    k = lattice_points(rng, n, -64, 40)                     # the corner region [48, 64]^3 stays empty
    special = [0, n // 3, n - 2][:max(0, min(3, n - 1))]
    corner = np.array([56, 56, 56])
    shift = np.array([4, 0, 0])
    k[n - 1] = corner
    for i, o in zip(special, ([0, 1, 0], [0, -1, 0], [0, 0, 1])):
        k[i] = corner - shift + np.array(o)
    return k, shift, special


def exact_adds_family(name, n, b, seed):
    """dict: tgt, tpred (b,4,4), pts (b,n,3) float32; expected d2 (b,n) int (lattice units squared), nearest (b,n), count (b,n) the number
    of minimisers, special: the outer points whose answer is the family's point."""
    rng = np.random.default_rng(seed)
    base = min(b, 4)                                          # distinct clouds; the batch repeats them under different poses
    clouds, shifts, special = [], [], []
    for _ in range(base):
        if name == "last_wins":
            k, s, special = _last_wins(rng, n)
        else:
            k, s = lattice_points(rng, n), np.zeros(3, np.int64)
            if name == "ties":
                k = _tied(k)
        clouds.append(k)
        shifts.append(s)
    tg, tp, pts, d2, nn, cnt = [], [], [], [], [], []
    answers = [lattice_nearest(k + s, k) for k, s in zip(clouds, shifts)]      # in the object's frame: a pose moves both clouds alike
    for i in range(b):
        R, t = lattice_pose(rng)
        k, s = clouds[i % base], shifts[i % base]
        tp.append(pose_matrix(R, t))
        tg.append(pose_matrix(R, t + R @ s))                  # x = R (p + s) + t
        pts.append((k * QUANTUM).astype(np.float32))
        a = answers[i % base]
        d2.append(a[0]); nn.append(a[1]); cnt.append(a[2])    # noqa: E702
    return {"name": name, "n": n, "b": b, "tgt": np.stack(tg), "tpred": np.stack(tp), "pts": np.stack(pts), "d2": np.stack(d2),
            "nearest": np.stack(nn).astype(np.int32), "count": np.stack(cnt), "special": special, "ints": clouds}


def exact_search_family(name, n_or_m, seed):
    """The same for so3_nearest_f32 (no pose): X (2,n,3), Y (2,m,3) float32 and the expected d2, nearest, count.  ties: X = Y with the
    duplicates (m = 2049); last_wins: X is Y shifted, three of its points next to Y's last point."""
    rng = np.random.default_rng(seed)
    X, Y, d2, nn, cnt, special = [], [], [], [], [], []
    for _ in range(2):
        if name == "last_wins":
            k, s, special = _last_wins(rng, n_or_m)
        else:
            k, s = _tied(lattice_points(rng, n_or_m)), np.zeros(3, np.int64)
        a = lattice_nearest(k + s, k)
        X.append(((k + s) * QUANTUM).astype(np.float32)); Y.append((k * QUANTUM).astype(np.float32))      # noqa: E702
        d2.append(a[0]); nn.append(a[1]); cnt.append(a[2])    # noqa: E702
    return {"name": name, "n": n_or_m, "m": n_or_m, "X": np.stack(X), "Y": np.stack(Y), "d2": np.stack(d2), "nearest": np.stack(nn).astype(np.int32),
            "count": np.stack(cnt), "special": special}


def lattice_diameter2(k):
    """max_ij |k_i - k_j|^2 of an integer cloud, exactly."""
    best = 0
    for lo in range(0, len(k), 512):
        best = max(best, int(((k[lo:lo + 512, None, :] - k[None, :, :]) ** 2).sum(-1).max()))
    return best


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def exact_seed(name, n):
    """The seed of an exact family, so that both test files build the same clouds."""
    return 700 + 2 * (n % 97) + 200 * len(name)


EXACT_ADDS = (("identical", 2500, 3), ("ties", 2049, 2), ("last_wins", 1025, 2), ("last_wins", 2049, 2), ("last_wins", 9, 2))
EXACT_SEARCH = (("ties", 2049), ("last_wins", 1025), ("last_wins", 9))
