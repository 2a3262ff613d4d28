"""Shared by tests/test_fpfh_host.py, tests/test_gpu_fpfh.py and tools/gen_golden.py (G32): fpfh_features restated in numpy from its
DEFINITION (include/so3proj.h), the margin condition on the fixture's inputs, and the fixture's layout.  No reference code exists for
this operation; the header is the contract.

    lengths:   cloud b has n_b = clip(len[b], 0, N) points; row i of idx (B, N, K) is point i's neighbourhood in the same cloud
    pair:      slot k of row (b, i), j = idx[b, i, k]: 0 <= j < n_b, j != i, |p_j - p_i|^2 > 0, neither normal all zero,
               |dp x n1|^2 > 0, no feature NaN
    features:  d = |dp|, a1 = n_i . dp / d, a2 = n_j . dp / d; |a1| < |a2| swaps the roles (n1 = n_j, n2 = n_i, dp <- -dp, f3 = -a2),
               else n1 = n_i, n2 = n_j, f3 = a1; v = dp x n1 / |dp x n1|, w = n1 x v, f2 = v . n2, f1 = atan2(w . n2, n1 . n2)
    bins:      h(g) = min(10, max(0, floor(g))), g1 = 11 (f1 + pi) / (2 pi), g2 = 11 (f2 + 1) / 2, g3 = 11 (f3 + 1) / 2
    features64 / counts64: all of that in float64 on the stored float32 inputs.
    spfh32:    (100 c) / (float)r in float32: EXACT given the counts.
    fpfh32:    the weighted sum in the defined order (w = 1 / d2, d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of the rounded differences,
               W a chain of rounded additions, A_s a chain of fma(w, spfh_js, A_s), spfh_is + A_s / W).  EXACT: the kernel and the host
               model must reproduce it bit for bit from the same spfh and pairs.
    fpfh64:    the same sum in float64 from the float64 counts, in any order.

THE MARGIN CONDITION.  A histogram's bins are discontinuous, so float32 and float64 can only agree away from the edges.  That is a
condition on the INPUTS, not a tolerance: for every pair none of g1, g2, g3 lies within MARGIN of an integer, |dp x n1| / d does not lie
in (0, MARGIN), and where | |a1| - |a2| | < MARGIN both role assignments give the same three bins, each with the edge margin.  The
generator redraws points until no pair violates it and tests/test_fpfh_host.py asserts it again.  Under it, pairs and all counts are
compared EXACTLY.  The margin is justified by a measured figure: the largest |g32 - g64| of the float32 host model over the fixture
(MEASURED["g"]) is asserted <= MARGIN / 4.

fpfh against float64 is judged per element as |got - want| / want, and as exact 0 where want == 0 (every term is non-negative, so the
figure means something everywhere); the bound is 4 x the host model's largest figure over G32 (MEASURED["fpfh"]), the rule of the
other families.

THE BRANCH CASES (tie_case, outer_case, weight_case, below) are the opposite of the margin condition: inputs built ON the strict swap,
beyond the two clamps of the bin and on "used when w < inf", each asserting that it reaches its branch, judged exactly under undecided()."""
import functools
import os

import numpy as np

from f32_exact import fma32, pair_dist2_32
import knn_ref
from support import bits, lengths_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g32_fpfh.npz")
MAX_K = 64
BINS, SLOTS = 11, 33
MARGIN = 1e-4
INT32_MIN = -2 ** 31
SURFACE_SHAPES = [(64, 8), (257, 16), (300, 64)]                               # (N, K)
MOVED_SHAPE = (257, 16)
MOVED_GAP = 1e-3                                                              # second-best - best descriptor distance across the poses
# what the float32 host model reaches over G32 (rounded up): the largest |g32 - g64| over the pairs, and the largest relative
# deviation of fpfh from float64 ...
MEASURED = {"g": 1.2e-5, "fpfh": 7.1e-7}
# ... and the bound the device's fpfh is held to: 4 x
FPFH_BOUND = 4 * MEASURED["fpfh"]


# ---- float64 -------------------------------------------------------------------------------------------------------------
def _gather(X, normals, idx, lengths, dtype):
    idx = np.asarray(idx, np.int64)
    b, n, K = idx.shape
    nl = lengths_of(lengths, b, n)
    i = np.arange(n)[None, :, None]
    valid = (idx >= 0) & (idx < nl[:, None, None]) & (i < nl[:, None, None]) & (idx != i)
    at = np.where(valid, idx, 0)
    batch = np.arange(b)[:, None, None]
    X, normals = np.asarray(X, np.float32).astype(dtype), np.asarray(normals, np.float32).astype(dtype)
    return valid, at, X[:, :, None, :], normals[:, :, None, :], X[batch, at], normals[batch, at]


def _darboux(u, ni, nj, a1, a2, swap):
    """The three features in bins' units for one assignment of the roles, and |u x n1| = |dp x n1| / d."""
    s = swap[..., None]
    n1, n2, uu = np.where(s, nj, ni), np.where(s, ni, nj), np.where(s, -u, u)
    f3 = np.where(swap, -a2, a1)
    c = np.cross(uu, n1)
    cn = np.sqrt((c * c).sum(-1))
    v = c / cn[..., None]
    w = np.cross(n1, v)
    f2 = (v * n2).sum(-1)
    f1 = np.arctan2((w * n2).sum(-1), (n1 * n2).sum(-1))
    g = np.stack([BINS * (f1 + np.pi) / (2 * np.pi), BINS * (f2 + 1) / 2, BINS * (f3 + 1) / 2], -1)
    return g, cn


def features64(X, normals, idx, lengths=None):
    """Every slot's float64 features: pair (B, N, K), g (B, N, K, 3), the other role assignment's g_alt, cn and cn_alt = |dp x n1| / d
    of both, tie (| |a1| - |a2| | < MARGIN), valid, at (the clamped index), d2, a1, a2."""
    with np.errstate(all="ignore"):
        valid, at, pi, ni, pj, nj = _gather(X, normals, idx, lengths, np.float64)
        ni, pi = np.broadcast_to(ni, nj.shape), np.broadcast_to(pi, pj.shape)
        dp = pj - pi
        d2 = (dp * dp).sum(-1)
        u = dp / np.sqrt(d2)[..., None]
        a1, a2 = (ni * u).sum(-1), (nj * u).sum(-1)
        swap = np.abs(a1) < np.abs(a2)
        g, cn = _darboux(u, ni, nj, a1, a2, swap)
        g_alt, cn_alt = _darboux(u, ni, nj, a1, a2, ~swap)
        nonzero = (ni != 0).any(-1) & (nj != 0).any(-1)
        pair = valid & (d2 > 0) & nonzero & (cn > 0) & ~np.isnan(g).any(-1)
        tie = np.abs(np.abs(a1) - np.abs(a2)) < MARGIN
    return {"pair": pair, "g": g, "g_alt": g_alt, "cn": cn, "cn_alt": cn_alt, "tie": tie, "valid": valid, "at": at, "d2": d2, "a1": a1, "a2": a2}


def bins_of(g):
    with np.errstate(invalid="ignore"):
        return np.clip(np.floor(np.where(np.isnan(g), 0.0, g)), 0, BINS - 1).astype(np.int64)


def counts_of(pair, g):
    """-> counts (B, N, 33) int64 and r (B, N): the histogram of the pairs' bins."""
    h = bins_of(g) + np.arange(3) * BINS                                       # (B, N, K, 3) slots
    hot = (h[..., None] == np.arange(SLOTS)).any(-2) & pair[..., None]         # (B, N, K, 33)
    return hot.sum(2), pair.sum(-1)


def counts64(X, normals, idx, lengths=None):
    f = features64(X, normals, idx, lengths)
    return counts_of(f["pair"], f["g"])


def _near_edge(g):
    with np.errstate(invalid="ignore"):
        return (np.abs(g - np.round(g)) < MARGIN).any(-1)


def violations(f):
    """The slots (B, N, K) that break the margin condition, from features64's result."""
    with np.errstate(invalid="ignore"):
        own = _near_edge(f["g"]) | ((f["cn"] > 0) & (f["cn"] < MARGIN))
        other = _near_edge(f["g_alt"]) | ~(f["cn_alt"] >= MARGIN) | (bins_of(f["g"]) != bins_of(f["g_alt"])).any(-1)
    return f["pair"] & (own | (f["tie"] & other))


def _near_interior_edge(g):
    """_near_edge for the branch cases: the interior integers 1 .. 10 are the only real edges.  h() clamps at 0 and at 10, so a g at
    0, at 11 or beyond either of them lands in the outer bin in any arithmetic."""
    with np.errstate(invalid="ignore"):
        k = np.round(g)
        return ((np.abs(g - k) < MARGIN) & (k >= 1) & (k <= BINS - 1)).any(-1)


def same_normals(f, normals):
    """The slots (B, N, K) whose two normals are bit-identical."""
    nb = bits(normals)
    return (nb[:, :, None, :] == nb[np.arange(nb.shape[0])[:, None, None], f["at"]]).all(-1)


def undecided(f, normals):
    """The second acceptance rule, for the branch cases: the slots (B, N, K) that break it.  violations() with two differences: only
    the interior integers are edges (_near_interior_edge), and a swap tie is DECIDED when the two normals are bit-identical -- a1 and a2
    are then the same float32 value in any arithmetic, |a1| < |a2| is false, and the header says no swap."""
    with np.errstate(invalid="ignore"):
        own = _near_interior_edge(f["g"]) | ((f["cn"] > 0) & (f["cn"] < MARGIN))
        other = _near_interior_edge(f["g_alt"]) | ~(f["cn_alt"] >= MARGIN) | (bins_of(f["g"]) != bins_of(f["g_alt"])).any(-1)
    return f["pair"] & (own | (f["tie"] & ~same_normals(f, normals) & other))


def clean_rows(X, normals, idx, lengths=None):
    """-> (spfh_rows, fpfh_rows) (B, N) bool: the rows a non-finite point or normal cannot reach -- for spfh the rows that neither are
    nor name one, for fpfh those that in addition name no row that does.  All True for a finite cloud."""
    idx = np.asarray(idx, np.int64)
    b, n, K = idx.shape
    nl = lengths_of(lengths, b, n)
    bad = ~(np.isfinite(np.asarray(X, np.float64)).all(-1) & np.isfinite(np.asarray(normals, np.float64)).all(-1))
    valid = (idx >= 0) & (idx < nl[:, None, None])
    at, batch = np.where(valid, idx, 0), np.arange(b)[:, None, None]
    first = ~(bad | (valid & bad[batch, at]).any(-1))
    second = first & ~(valid & ~first[batch, at]).any(-1)
    return first, second


def spfh32(counts, r):
    """(100 c) / (float)r in float32, zeros where r == 0."""
    r = np.asarray(r)
    rf = np.maximum(r, 1).astype(np.float32)[..., None]
    return np.where(r[..., None] > 0, (np.float32(100) * np.asarray(counts).astype(np.float32)) / rf, np.float32(0)).astype(np.float32)


def fpfh32(X, idx, lengths, spfh, pairs):
    """-> fpfh (B, N, 33) float32: the DEFINED bits from these spfh and pairs."""
    spfh, pairs = np.asarray(spfh, np.float32), np.asarray(pairs)
    valid, at, pi, _, pj, _ = _gather(X, X, idx, lengths, np.float32)
    b, n, K = valid.shape
    batch = np.arange(b)[:, None]
    live = np.arange(n)[None, :] < lengths_of(lengths, b, n)[:, None]
    W, A = np.zeros((b, n), np.float32), np.zeros((b, n, SLOTS), np.float32)
    with np.errstate(all="ignore"):
        dp = pj - pi
        d2 = pair_dist2_32(dp[..., 0], dp[..., 1], dp[..., 2]).astype(np.float32)
        w = (np.float32(1) / d2).astype(np.float32)
        for k in range(K):
            use = valid[:, :, k] & (d2[:, :, k] > 0) & (w[:, :, k] < np.inf) & (pairs[batch, at[:, :, k]] > 0)
            wk = np.where(use, w[:, :, k], np.float32(0))                       # a skipped slot's w may be inf or NaN: keep it out of fma32
            W = np.where(use, W + wk, W)
            A = np.where(use[..., None], fma32(wk[..., None], spfh[batch, at[:, :, k]], A).astype(np.float32), A)
        mean = np.where(W[..., None] > 0, A / np.where(W > 0, W, np.float32(1))[..., None], np.float32(0)).astype(np.float32)
        out = (spfh + mean).astype(np.float32)
    return np.where(live[..., None], out, np.float32(0))


def fpfh64(X, idx, lengths, counts, r):
    """-> fpfh (B, N, 33) float64 from the float64 counts."""
    valid, at, pi, _, pj, _ = _gather(X, X, idx, lengths, np.float64)
    b, n, K = valid.shape
    batch = np.arange(b)[:, None, None]
    r = np.asarray(r)
    s = np.where(r[..., None] > 0, 100.0 * np.asarray(counts) / np.maximum(r, 1)[..., None], 0.0)
    with np.errstate(all="ignore"):
        d2 = ((pj - pi) ** 2).sum(-1)
        use = valid & (d2 > 0) & (r[batch, at] > 0)
        w = np.where(use, 1.0 / np.where(use, d2, 1.0), 0.0)
        W = w.sum(-1)
        A = (w[..., None] * s[batch, at]).sum(2)
        return s + np.where(W[..., None] > 0, A / np.where(W > 0, W, 1.0)[..., None], 0.0)


def relative_deviation(got, want, rows=None):
    """The largest |got - want| / want over the elements with want > 0 (of `rows`); where want == 0, got must be exactly 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if rows is not None:
        got, want = got[rows], want[rows]
    assert (got[want == 0] == 0).all()
    pos = want > 0
    return float((np.abs(got[pos] - want[pos]) / want[pos]).max()) if pos.any() else 0.0


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def draw_sphere(rng, count):
    """Points on the unit sphere with normals = radial + 0.2 sigma noise (exact normals put |a1| = |a2| on most pairs)."""
    p = _unit(rng.standard_normal((count, 3)))
    return p.astype(np.float32), _unit(p + 0.2 * rng.standard_normal((count, 3))).astype(np.float32)


def draw_blob(rng, count):
    """A Gaussian blob with random unit normals."""
    return (0.35 * rng.standard_normal((count, 3))).astype(np.float32), _unit(rng.standard_normal((count, 3))).astype(np.float32)


def knn_rows(X, K, lengths=None, drop_self=False):
    idx = knn_ref.knn32(X, X, K + 1 if drop_self else K, lengths, lengths)[1]
    return idx[:, :, 1:] if drop_self else idx


def settle(rng, draw, b, n, K, lengths=None, post=None, check=None, rows=None, rounds=2000):
    """Draw clouds (B, N) and redraw the points whose row breaks the condition (check: a further (B, N) mask of points to redraw)
    until none does -> X, normals, idx.  post(X, normals) re-imposes a family's structure after every draw; rows(X) the index rows."""
    X, Nr = (np.stack(a) for a in zip(*(draw(rng, n) for _ in range(b))))
    rows = rows or (lambda X: knn_rows(X, K, lengths))
    for _ in range(rounds):
        if post is not None:
            post(X, Nr)
        idx = rows(X)
        bad = violations(features64(X, Nr, idx, lengths)).any(-1)
        if check is not None:
            bad = bad | check(X, Nr, idx)
        if not bad.any():
            return X, Nr, idx
        X[bad], Nr[bad] = draw(rng, int(bad.sum()))
    raise AssertionError("the margin condition did not settle")


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.linalg.det(q)


def moved_pose(X, Nr, R, t):
    """The rigid motion applied in float64 and rounded to float32."""
    return (X.astype(np.float64) @ R.T + t).astype(np.float32), (Nr.astype(np.float64) @ R.T).astype(np.float32)


def moved_premises(Xa, Na, Xb, Nb, K):
    """The moved copy's three premises -> the (N,) mask of points that break one (empty: all hold): equal kNN rows, equal counts, and
    every point's nearest float64 descriptor in the other pose is its own with second-best - best > MOVED_GAP."""
    ia, ib = knn_ref.knn32(Xa[None], Xa[None], K)[1], knn_ref.knn32(Xb[None], Xb[None], K)[1]
    bad = (ia != ib).any(-1)[0] | (knn_ref.knn64(Xa[None], Xa[None], K)[1] != knn_ref.knn64(Xb[None], Xb[None], K)[1]).any(-1)[0] \
        | (ia != knn_ref.knn64(Xa[None], Xa[None], K)[1]).any(-1)[0]
    ca, ra = counts64(Xa[None], Na[None], ia)
    cb, rb = counts64(Xb[None], Nb[None], ia)
    bad |= (ca != cb).any(-1)[0] | (ra != rb)[0]
    fa, fb = fpfh64(Xa[None], ia, None, ca, ra)[0], fpfh64(Xb[None], ia, None, cb, rb)[0]
    dist = np.linalg.norm(fa[:, None, :] - fb[None, :, :], axis=-1)
    for d in (dist, dist.T):
        order = np.sort(d, axis=1)
        bad |= (np.argmin(d, axis=1) != np.arange(len(d))) | (order[:, 1] - order[:, 0] <= MOVED_GAP)
    return bad


def generate(seed=32):
    """G32's arrays: per case the float32 points and normals, the index rows as int16 (INT32_MIN stored as -32768), the lengths where
    ragged, and the float64 counts as uint8.  Asserts the margin condition and every family's premise."""
    rng = np.random.default_rng(seed)
    out, names = {}, []

    def add(name, family, X, Nr, idx, lengths=None):
        X, Nr, idx = np.asarray(X, np.float32), np.asarray(Nr, np.float32), np.asarray(idx, np.int64)
        f = features64(X, Nr, idx, lengths)
        spfh_rows, _ = clean_rows(X, Nr, idx, lengths)
        assert not (violations(f).any(-1) & spfh_rows).any(), name
        counts, r = counts_of(f["pair"], f["g"])
        assert counts.max() <= 64 and (counts.reshape(counts.shape[:2] + (3, BINS)).sum(-1) == r[..., None]).all(), name
        short = np.where(idx == INT32_MIN, -32768, idx)
        assert np.abs(short).max() <= 32768 and X.shape[1] < 32767
        out[name + "/X"], out[name + "/normals"], out[name + "/idx"], out[name + "/counts"] = X, Nr, short.astype(np.int16), counts.astype(np.uint8)
        if lengths is not None:
            out[name + "/lengths"] = np.asarray(lengths, np.int32)
        names.append("%s|%s|%d" % (name, family, idx.shape[2]))
        return counts, r

    for fam, draw in (("sphere", draw_sphere), ("blob", draw_blob)):
        for n, K in SURFACE_SHAPES:
            add("%s_%dx%d" % (fam, n, K), fam, *settle(rng, draw, 1, n, K))
    # an exact lattice plane with a constant normal: every feature is 0, all mass in the middle bins 5, 16, 27
    gx, gy = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    X = np.stack([gx.ravel() / 8.0, gy.ravel() / 8.0, np.zeros(64)], -1)[None].astype(np.float32)
    Nr = np.broadcast_to(np.array([0, 0, 1], np.float32), X.shape).copy()
    counts, r = add("lattice_plane", "lattice_plane", X, Nr, knn_rows(X, 9))
    assert (r == 8).all() and (counts[..., [5, 16, 27]] == 8).all()
    # lattice points straight above one another along the normal: dp is parallel to n, no pair
    gx, gy, gz = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    X = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], -1)[None].astype(np.float32) / 4
    column = (np.arange(64) // 4 * 4)[:, None] + np.arange(4)[None, :]                  # the four points of the own column
    counts, r = add("lattice_column", "lattice_column", X, np.broadcast_to(np.array([0, 0, 1], np.float32), X.shape).copy(), column[None])
    assert (r == 0).all()

    # coincident points: every point stands twice, with its own normal each time
    def twice(X, Nr):
        X[:, 32:] = X[:, :32]
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 8, post=twice)
    counts, r = add("coincident", "coincident", X, Nr, idx)
    assert ((idx[0] == (np.arange(64)[:, None] + 32) % 64).any(-1)).all() and (r <= 6).all() and (r > 0).any()

    def third_zero(X, Nr):
        Nr[:, ::3] = 0
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 8, post=third_zero)
    counts, r = add("zero_normals", "zero_normals", X, Nr, idx)
    assert (r[0, ::3] == 0).all() and (r[0, 1::3] > 0).all() and (r[0, 1::3] < 7).any()
    # rows with -1 / N / INT32_MIN interleaved with real indices; rows without the point itself; rows with a repeated index
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 8)
    mixed = idx.copy()
    mixed[:, :, [1, 4]], mixed[:, :, 2], mixed[:, :, 6] = -1, 64, INT32_MIN
    counts, r = add("mixed", "mixed", X, Nr, mixed)
    assert (r == 3).all()
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 8, rows=lambda X: knn_rows(X, 8, drop_self=True))
    counts, r = add("no_self", "no_self", X, Nr, idx)
    assert (idx[0] != np.arange(64)[:, None]).all() and (r == 8).all()
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 8)
    idx[:, :, 5] = idx[:, :, 2]
    counts, r = add("repeated", "repeated", X, Nr, idx)
    assert (r == 7).all() and (counts.max(-1) >= 2).all()
    # K = 1, 2, 3 (K = 1: the nearest other point), K > n_b
    X, Nr, idx = settle(rng, draw_blob, 1, 64, 3)
    for name, rows in (("k1", idx[:, :, 1:2]), ("k2", idx[:, :, :2]), ("k3", idx)):
        counts, r = add(name, "small_k", X, Nr, rows)
        assert (r == rows.shape[2] - (name != "k1")).all()
    X, Nr, idx = settle(rng, draw_blob, 1, 5, 8)
    counts, r = add("k_above_n", "k_above_n", X, Nr, idx)
    assert (idx[:, :, 5:] == -1).all() and (r == 4).all()
    # ragged lengths: n_b = 0, 1, 2, 1 < n_b < K, and a full cloud
    lengths = np.array([0, 1, 2, 5, 40], np.int32)
    X, Nr, idx = settle(rng, draw_blob, 5, 40, 8, lengths=lengths)
    counts, r = add("ragged", "ragged", X, Nr, idx, lengths)
    assert (r[:2] == 0).all() and (r[2, :2] == 1).all() and (r[3, :5] == 4).all() and (r[4] == 7).all() and all((r[b, lengths[b]:] == 0).all() for b in range(5))
    # a cloud with NaN and infinite points and normals between two clean ones; it keeps the clean copy's rows
    X, Nr, idx = settle(rng, draw_blob, 2, 128, 8)
    X, Nr, idx = X[[0, 0, 1]], Nr[[0, 0, 1]], idx[[0, 0, 1]]
    near = idx[0, 3, :4]                                                          # point 3 and its three nearest: what they reach overlaps
    X[1, near[0], 0], X[1, near[1], 1], Nr[1, near[2], 2], Nr[1, near[3], 0] = np.nan, np.inf, np.nan, -np.inf
    counts, r = add("nonfinite", "nonfinite", X, Nr, idx)
    first, second = clean_rows(X, Nr, idx)
    assert first[[0, 2]].all() and 8 <= second[1].sum() < first[1].sum() < 124 and (counts[1][first[1]] == counts[0][first[1]]).all()
    # the moved copy: the cloud under a random rotation and a translation; both poses keep the condition and the three premises
    n, K = MOVED_SHAPE
    for fam, draw in (("sphere", draw_sphere), ("blob", draw_blob)):
        R, t = random_rotation(rng), rng.uniform(-1, 1, 3)

        def both(X, Nr, idx):
            Xb, Nb = moved_pose(X[0], Nr[0], R, t)
            return (violations(features64(Xb[None], Nb[None], idx)).any(-1) | moved_premises(X[0], Nr[0], Xb, Nb, K)[None])
        X, Nr, idx = settle(rng, draw, 1, n, K, check=both)
        Xb, Nb = moved_pose(X[0], Nr[0], R, t)
        ca, _ = add("moved_%s" % fam, "moved", np.stack([X[0], Xb]), np.stack([Nr[0], Nb]), np.concatenate([idx, idx]))
        assert (ca[0] == ca[1]).all() and not moved_premises(X[0], Nr[0], Xb, Nb, K).any()
    out["names"] = np.array(names)
    return out


def g32():
    return np.load(GOLDEN, allow_pickle=False)


def _case(name, family, X, Nr, idx, lengths, counts):
    b, n, K = idx.shape
    r = counts[..., :BINS].sum(-1)
    spfh_rows, fpfh_rows = clean_rows(X, Nr, idx, lengths)
    return {"name": name, "family": family, "X": X, "normals": Nr, "idx": idx, "lengths": lengths, "K": K, "b": b, "n": n, "counts": counts,
            "pairs": r, "spfh": spfh32(counts, r), "fpfh64": fpfh64(X, idx, lengths, counts, r), "spfh_rows": spfh_rows, "fpfh_rows": fpfh_rows}


def cases(z):
    """The fixture as a list of dicts: name, family, X, normals (float32), idx (int32), lengths (int32 or None), K, b, n, and the
    expectations re-formed from the stored float64 counts: counts (int64), pairs, spfh (float32, exact), fpfh64, and the rows a
    non-finite value cannot reach (spfh_rows, fpfh_rows: all True elsewhere).  The blob at MOVED_SHAPE also comes scaled by 2^+-20."""
    out = []
    for entry in z["names"]:
        name, family, K = str(entry).split("|")
        idx = z[name + "/idx"].astype(np.int64)
        idx = np.where(idx == -32768, INT32_MIN, idx).astype(np.int32)
        lengths = z[name + "/lengths"] if name + "/lengths" in z.files else None
        assert idx.shape[2] == int(K)
        out.append(_case(name, family, z[name + "/X"], z[name + "/normals"], idx, lengths, z[name + "/counts"].astype(np.int64)))
        if name == "blob_%dx%d" % MOVED_SHAPE:
            base = out[-1]
            for tag, e in (("up", 20), ("down", -20)):
                c = dict(base)
                c.update(name="%s_%s" % (name, tag), family="scaled", X=c["X"] * np.float32(2.0 ** e))
                c["fpfh64"] = fpfh64(c["X"], idx, lengths, c["counts"], c["pairs"])
                out.append(c)
    return out


# ---- the branch cases: inputs that sit exactly ON the definition's branches --------------------------------------------------------
# G32 keeps away from every branch on purpose (the margin condition).  These generators go the other way: each builds inputs on which
# one branch rule of the header alone decides the counts, asserts in float64 on the stored float32 inputs that the branch is reached, and
# leaves every OTHER quantity far enough from an edge that float32 and float64 must agree.  Pure numpy, fixed seeds, no fixture file;
# judged under undecided() instead of violations().
EDGE_B, EDGE_N, EDGE_KS = 3, 257, (5, 16, 33)                                 # k_spfh<8>, k_spfh<16>, k_spfh<64>
EDGE_ROWS = (0, 63, 64, 255, 256)                                             # a wave's and a workgroup's first and last query, the tail
EDGE_LENGTHS = {"ties": (257, 257, 130), "outer": (257, 257, 200)}            # one ragged cloud each
LONG = 1.0 + 2.0 ** -18                                                       # a "unit" normal a few float32 ulp long
OFF = 2.0 ** -10                                                              # rad: how far a pair leans off the exact degenerate direction
OVERSHOOT = 1e-5                                                              # g past 11 or below 0 by more than this: > 10 float32 ulp of 11
# A pair built OFF rad from a degenerate direction has |dp x n1| / d (or |n2 x v|) = sin OFF ~ 1e-3, so float32's 1e-7 of rounding
# turns its two well-defined-but-ill-conditioned features by up to ~1e-4 rad: 6e-4 in bins' units, more than MARGIN.  Those features
# are therefore held WIDE from every integer, 80 x that.
WIDE = 0.05
TILTS = ((0.6, 0.0, 0.8), (0.0, -0.8, 0.6), (0.48, 0.64, 0.6))                # one tilted normal per cloud, the same bits on every point


def _branch_case(name, family, X, Nr, idx, lengths):
    X, Nr, idx = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Nr, np.float32), np.ascontiguousarray(idx, np.int32)
    lengths = np.asarray(lengths, np.int32)
    f = features64(X, Nr, idx, lengths)
    assert not undecided(f, Nr).any(), name
    counts, _ = counts_of(f["pair"], f["g"])
    c = _case(name, family, X, Nr, idx, lengths, counts)
    assert c["spfh_rows"].all() and c["fpfh_rows"].all() and (c["n"], c["b"]) == (EDGE_N, EDGE_B), name
    c["f"] = f
    return c


def tie_case(K):
    """EXACT SWAP TIES.  Every cloud is a flat patch (z = 0, random x and y) whose points all carry one tilted normal, bit for bit; a
    row is the point's K - 1 nearest (itself among them) and one -1.  a1 and a2 are dots of the SAME normal with the same u: equal in
    any arithmetic, and the header says |a1| < |a2| strictly, so no pair swaps.  Premises (asserted): every pair's normals are
    bit-identical; both role assignments keep MARGIN from the interior integers; on at least half of the pairs they give different
    bins, so swapping on the tie changes the histogram."""
    rng = np.random.default_rng(3300 + K)
    lengths = np.array(EDGE_LENGTHS["ties"], np.int32)
    X = np.zeros((EDGE_B, EDGE_N, 3), np.float32)
    X[..., :2] = rng.uniform(-1, 1, (EDGE_B, EDGE_N, 2))
    Nr = np.broadcast_to(np.array(TILTS, np.float32)[:, None, :], X.shape).copy()
    for _ in range(200):
        idx = np.concatenate([knn_rows(X, K - 1, lengths), np.full((EDGE_B, EDGE_N, 1), -1, np.int64)], -1)
        f = features64(X, Nr, idx, lengths)
        bad = (undecided(f, Nr) | (f["pair"] & _near_interior_edge(f["g_alt"]))).any(-1)
        if not bad.any():
            break
        X[bad, :2] = rng.uniform(-1, 1, (int(bad.sum()), 2))
    c = _branch_case("ties_%d" % K, "ties", X, Nr, idx, lengths)
    f, pair = c["f"], c["f"]["pair"]
    assert same_normals(f, Nr)[pair].all() and f["tie"][pair].all()
    assert (f["a1"][pair] == f["a2"][pair]).all() and not _near_interior_edge(f["g_alt"])[pair].any()
    nl = lengths_of(lengths, EDGE_B, EDGE_N)
    assert all((c["pairs"][b, :nl[b]] == K - 2).all() and (c["pairs"][b, nl[b]:] == 0).all() for b in range(EDGE_B))
    c["ties"] = int(pair.sum())
    c["ties_that_differ"] = int((bins_of(f["g"]) != bins_of(f["g_alt"])).any(-1)[pair].sum())
    assert c["ties"] >= (K - 2) * int(nl.sum()) and 2 * c["ties_that_differ"] >= c["ties"]
    return c


def _one_pair(pi, ni, pj, nj):
    """features64 of the single pair (i -> j), squeezed."""
    f = features64(np.array([[pi, pj]], np.float32), np.array([[ni, nj]], np.float32), np.array([[[1], [0]]]))
    return {k: v[0, 0, 0] for k, v in f.items()}


def _wide(g):
    return np.abs(g - np.round(g)) >= WIDE


def outer_case(K):
    """BEYOND THE OUTER EDGES.  The queries stand in EDGE_ROWS; each has its own neighbours elsewhere in the cloud, every other point is
    filler with an empty row.  All normals have length LONG (the queries' exactly, along an axis).
      g3 queries: the neighbours lie OFF rad off the normal's line, alternately in front and behind, at distances 0.5 .. 1.0, so
                  f3 = a1 = +-LONG cos OFF: g3 = 11.000018 or -0.000018.  The neighbour's normal is drawn with |a2| <= 0.8.
      g2 queries: the neighbour's normal leans OFF rad off +-v = +-(dp x n1) / |dp x n1|, so f2 = +-LONG cos OFF and a2 ~ 0; dp makes
                  an angle with the query's normal that puts g3 in the middle of a bin, the lean's direction puts g1 in one.
    A neighbour's own row names its query back: the same pair seen from the other side swaps the roles and must overshoot too.
    Premises (asserted): on at least two pairs each g3 > 11 + OVERSHOOT, g3 < -OVERSHOOT, g2 > 11 + OVERSHOOT, g2 < -OVERSHOOT; every
    pair has |dp x n1| > 0 and | |a1| - |a2| | >= 0.1 (no swap tie); every feature that does not overshoot keeps WIDE from every
    integer.  The float64 counts then hold bins 10 and 0."""
    rng = np.random.default_rng(3400 + K)
    lengths = np.array(EDGE_LENGTHS["outer"], np.int32)
    X = np.zeros((EDGE_B, EDGE_N, 3), np.float32)
    X[..., 0], X[..., 1], X[..., 2] = 16 + np.arange(EDGE_N) / 8.0, -16.0, 16.0           # the filler: far from every query
    Nr = np.broadcast_to(np.array([0, 0, 1], np.float32), X.shape).copy()
    idx = np.full((EDGE_B, EDGE_N, K), -1, np.int32)
    mids = [(m + 0.5) / 5.5 - 1 for m in (1, 2, 3, 7, 8, 9)]                              # a1 with g3 in the middle of bin m

    def unit(v):
        return v / np.linalg.norm(v)

    for b in range(EDGE_B):
        free = iter(i for i in range(EDGE_N) if i not in EDGE_ROWS)
        for qi, q in enumerate(EDGE_ROWS):
            kind = "g3" if (qi + b) % 2 == 0 else "g2"
            axis, sign = np.eye(3)[(qi + b) % 3], 1.0 if (qi // 3 + b) % 2 == 0 else -1.0
            p1, p2 = np.eye(3)[(qi + b + 1) % 3], np.eye(3)[(qi + b + 2) % 3]
            X[b, q], Nr[b, q] = (4.0 * qi - 8, 4.0 * b - 4, 2.0 * (qi % 2)), sign * LONG * axis
            k = max(2, K - 1 - qi % 2)
            for t in range(k):
                j = next(free)
                idx[b, q, t], idx[b, j, 0] = j, q
                side, dist, phi = (1.0 if t % 2 == 0 else -1.0), 0.5 + 0.5 * t / (k - 1), rng.uniform(0, 2 * np.pi)
                around = np.cos(phi) * p1 + np.sin(phi) * p2
                for _ in range(1000):
                    if kind == "g3":
                        u = side * np.cos(OFF) * sign * axis + np.sin(OFF) * around
                        X[b, j] = X[b, q].astype(np.float64) + dist * u
                        Nr[b, j] = LONG * unit(rng.standard_normal(3))
                    else:
                        a1 = mids[(t // 2) % len(mids)]
                        u = a1 * sign * axis + np.sqrt(1 - a1 * a1) * around
                        X[b, j] = X[b, q].astype(np.float64) + dist * u
                        n1 = Nr[b, q].astype(np.float64)
                        dp = X[b, j].astype(np.float64) - X[b, q].astype(np.float64)               # the stored, rounded points
                        v = unit(np.cross(dp, n1))
                        psi = ((t + qi) % BINS + 0.5) * 2 * np.pi / BINS - np.pi                    # f1: the middle of a bin
                        lean = np.cos(psi) * unit(n1) + np.sin(psi) * unit(np.cross(n1, v))
                        Nr[b, j] = LONG * (np.cos(OFF) * side * v + np.sin(OFF) * lean)
                    s = _one_pair(X[b, q], Nr[b, q], X[b, j], Nr[b, j])
                    over = (s["g"] > BINS + OVERSHOOT) | (s["g"] < -OVERSHOOT)
                    if s["pair"] and abs(abs(s["a1"]) - abs(s["a2"])) >= 0.1 and (over | _wide(s["g"])).all() and over[2 if kind == "g3" else 1]:
                        break
                    phi = rng.uniform(0, 2 * np.pi)
                    around = np.cos(phi) * p1 + np.sin(phi) * p2
                else:
                    raise AssertionError("no neighbour found")
    c = _branch_case("outer_%d" % K, "outer", X, Nr, idx, lengths)
    f, pair = c["f"], c["f"]["pair"]
    g = f["g"][pair]
    over, under = g > BINS + OVERSHOOT, g < -OVERSHOOT
    assert (f["cn"][pair] > 0).all() and (np.abs(np.abs(f["a1"]) - np.abs(f["a2"]))[pair] >= 0.1).all() and not f["tie"][pair].any()
    assert (over | under | _wide(g)).all() and not (over | under)[:, 0].any()
    c["beyond"] = {"g2>11": int(over[:, 1].sum()), "g2<0": int(under[:, 1].sum()), "g3>11": int(over[:, 2].sum()), "g3<0": int(under[:, 2].sum())}
    assert min(c["beyond"].values()) >= 2, c["beyond"]
    swapped = (np.abs(f["a1"]) < np.abs(f["a2"]))[pair]                                    # both role assignments reach the outer bins
    assert (over | under).any(-1)[swapped].sum() >= 4 and (over | under).any(-1)[~swapped].sum() >= 4
    for s, col in ((BINS, 1), (2 * BINS, 2)):                                              # the float64 counts hold bins 10 and 0
        assert c["counts"][..., s + BINS - 1].sum() >= over[:, col].sum() and c["counts"][..., s].sum() >= under[:, col].sum()
    return c


@functools.lru_cache(maxsize=None)
def branch_cases(K):
    """The tie case and the outer-edge case at one K of EDGE_KS; built once, shared by the host and the device tests, never changed."""
    return (tie_case(K), outer_case(K))


@functools.lru_cache(maxsize=None)
def weight_case():
    """THE WEIGHT RULE, for so3_fpfh_f32 alone: points, rows, and GIVEN spfh (small multiples of 25) and pairs, so every row used has a
    known, finite answer.  Points 0 and 1 are 2^-65 apart: d2 = 2^-130, which a device may keep (w = 1 / d2 = inf: "used when w < inf"
    skips the slot) or flush to 0 (d2 > 0 skips it) -- the same answer.  Points 0 and 2 are 2^-59 apart: w = 2^118, used, and it
    dominates the row.  Points 1 and 2 never meet in a row (their d2 = 2^-118 + 2^-130 would depend on the flush).  Point 5 has
    pairs = 0.  Premises (asserted, float32 numpy): a slot with d2 > 0 and 1 / d2 == inf, a used slot with w >= 2^100, and a finite
    fpfh32 everywhere."""
    rng = np.random.default_rng(3500)
    X = np.array([[[0, 0, 0], [2.0 ** -65, 0, 0], [0, 2.0 ** -59, 0], [0.5, 0.25, 0], [-0.25, 0.5, 0.125], [0.125, -0.5, 0.75]]], np.float32)
    idx = np.array([[[1, 2, 3, 4, -1], [0, 3, 4, 5, -1], [0, 3, -1, 4, 5], [0, 1, 2, 4, 5], [5, 3, 2, 1, 0], [-1, 0, 1, 3, 6]]], np.int32)
    spfh = (25 * rng.integers(0, 5, (1, 6, SLOTS))).astype(np.float32)
    pairs = np.array([[3, 2, 4, 1, 3, 0]], np.int32)
    want = fpfh32(X, idx, None, spfh, pairs)
    with np.errstate(all="ignore"):
        valid, at, pi, _, pj, _ = _gather(X, X, idx, None, np.float32)
        dp = pj - pi
        d2 = pair_dist2_32(dp[..., 0], dp[..., 1], dp[..., 2]).astype(np.float32)
        w = (np.float32(1) / d2).astype(np.float32)
        used = valid & (d2 > 0) & (w < np.inf) & (pairs[0][at] > 0)
    assert (valid & (d2 > 0) & np.isinf(w)).sum() == 2 and (used & (w >= 2.0 ** 100)).sum() == 2 and np.isfinite(want).all()
    assert (valid & (pairs[0][at] == 0)).any() and (want != spfh).any()
    normals = np.broadcast_to(np.array([0, 0, 1], np.float32), X.shape).copy()                       # unused by the second launch
    return {"name": "weights", "X": X, "normals": normals, "idx": idx, "lengths": None, "spfh": spfh, "pairs": pairs, "fpfh32": want, "b": 1, "n": 6, "K": 5}
