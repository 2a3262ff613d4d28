"""Shared by tests/test_knn_host.py, tests/test_gpu_knn.py and tools/gen_golden.py (G28): knn_points restated in numpy from its
DEFINITION (include/so3proj.h), and the fixture's layout.  No reference code exists for this operation; the header is the contract.

    lengths:    cloud b uses its first n_b = clip(x_len[b], 0, N) points of X and m_b = clip(y_len[b], 0, M) points of Y
    d(i, j)   = ((dx * dx) + (dy * dy)) + (dz * dz) from coordinate differences (three_nn_ref.dist2: float32 arrays, so numpy rounds
                every operation on its own)
    row i < n_b: the r = min(K, m_b) smallest candidates j < m_b, among equal d the lower j first = the first r of a STABLE argsort
    padding:    dist2 0, idx -1 in the slots k >= r, the rows i >= n_b, the clouds with m_b == 0, and a slot without a candidate
                (a NaN or +inf d fails every <, so it never enters a list)
    backward:   per coordinate one chain from +0 (tests/f32_exact.fma32), the difference one rounded subtraction, the doubling exact:
                dX[b, i] over k ascending      acc = fma(g_ik, 2 (x_i - y_j), acc),   j = idx[b, i, k]
                dY[b, j] over (i, k) ascending acc = fma(g_ik, 2 (y_j - x_i), acc)    for the entries with idx[b, i, k] == j
knn32 and grad32 are exact: the kernels and the host model must reproduce them bit for bit.  knn64 and grad64 are the same in float64
(from the float32 inputs): the check that the defined order is an accurate one.

    excess:  the float64 d at knn32's k-th neighbour exceeds the float64 k-th smallest by at most EXCESS = 64 * 2^-24 on clouds of unit
             radius (a float32 d carries at most 8 * 2^-24 relative error, two candidates can change places when they are closer than
             both their errors: 16 * 2^-24 d, d <= 4).  Index equality against float64 is never asserted.
    grad:    a chain of h terms is within (h + 4) * 2^-24 * sum |g| 2 |v| of float64: one rounded difference per term (2^-24 relative
             of the term) plus one rounding per fma (2^-24 of a partial sum no larger than the sum of magnitudes); counted, not measured."""
import os

import numpy as np

from f32_exact import fma32
from support import lengths_of
import three_nn_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_knn.npz")
U = 2.0 ** -24
EXCESS = 64 * U
MAX_K = 64
SHAPES = [(1, 1, 1), (3, 7, 4), (5, 3, 8), (64, 65, 64), (255, 1023, 16), (257, 1025, 20), (300, 77, 8)]       # (N, M, K)
B_FULL, B_RAGGED = 2, 5              # ragged: cloud 0 n_b = 0, cloud 1 m_b = 0, cloud 2 m_b = 1, cloud 3 1 < m_b < K (where K, M allow)
FAMILIES = ("random", "subset", "all_equal", "lattice", "many_to_one")


def _targets(Y, b):
    Y = np.asarray(Y, np.float32)
    return np.broadcast_to(Y, (b,) + Y.shape) if Y.ndim == 2 else Y          # one shared (M, 3) target


def _knn(X, Y, K, x_lengths, y_lengths, dtype, rows_per_pass=1 << 22):
    X = np.asarray(X, np.float32)
    b, n = X.shape[:2]
    Y = _targets(Y, b)
    m = Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    d2, idx = np.zeros((b, n, K), dtype), np.full((b, n, K), -1, np.int64)
    for k in range(b):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        r, step = min(K, mb), max(1, rows_per_pass // mb)
        for n0 in range(0, nb, step):
            with np.errstate(invalid="ignore", over="ignore"):
                d = three_nn_ref.dist2(X[k:k + 1, n0:min(nb, n0 + step)], Y[k:k + 1, :mb], dtype)[0]
                d = np.where(d < np.inf, d, np.inf).astype(dtype)            # a NaN or +inf d never enters a list
            order = np.argsort(d, axis=-1, kind="stable")[:, :r]
            dd = np.take_along_axis(d, order, -1)
            got = dd < np.inf
            d2[k, n0:n0 + dd.shape[0], :r] = np.where(got, dd, 0)
            idx[k, n0:n0 + dd.shape[0], :r] = np.where(got, order, -1)
    return d2, idx


def knn32(X, Y, K, x_lengths=None, y_lengths=None):
    """-> dist2 (B, N, K) float32, idx (B, N, K) int64: the DEFINED bits."""
    return _knn(X, Y, K, x_lengths, y_lengths, np.float32)


def knn64(X, Y, K, x_lengths=None, y_lengths=None):
    return _knn(X, Y, K, x_lengths, y_lengths, np.float64)


def _live(idx, x_lengths, y_lengths, m):
    """(valid (B, N, K): the entries that contribute, the clamped index, n_b, m_b)."""
    idx = np.asarray(idx, np.int64)
    b, n, K = idx.shape
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    nl = np.where(ml > 0, nl, 0)
    r = np.minimum(K, ml)
    valid = (idx >= 0) & (np.arange(n)[None, :, None] < nl[:, None, None]) & (np.arange(K)[None, None, :] < r[:, None, None])
    at = np.clip(idx, 0, np.maximum(ml, 1)[:, None, None] - 1)
    return valid, at, nl, ml


def grad32(X, Y, x_lengths, y_lengths, idx, g):
    """-> (dX (B, N, 3), dY (B, M, 3)) float32: the DEFINED bits, one fma per entry in the defined order."""
    X, Y, g = np.asarray(X, np.float32), np.asarray(Y, np.float32), np.asarray(g, np.float32)
    b, n, K = np.asarray(idx).shape
    m = Y.shape[1]
    valid, at, nl, ml = _live(idx, x_lengths, y_lengths, m)
    dX, dY, rows, two = np.zeros((b, n, 3), np.float32), np.zeros((b, m, 3), np.float32), np.arange(b), np.float32(2)
    for k in range(K):                                           # dX: every query at once, k ascending
        y = np.stack([Y[c][at[c, :, k]] for c in range(b)])
        dX = np.where(valid[:, :, k, None], fma32(g[:, :, k, None], two * (X - y), dX), dX)
    for i in range(int(nl.max()) if b else 0):                   # dY: the entries in ascending (i, k), every cloud at once
        for k in range(K):
            j, ok = at[:, i, k], valid[:, i, k]
            if not ok.any():
                continue
            new = fma32(g[:, i, k, None], two * (Y[rows, j] - X[:, i]), dY[rows, j])
            dY[rows, j] = np.where(ok[:, None], new, dY[rows, j])
    return dX, dY


def grad64(X, Y, x_lengths, y_lengths, idx, g):
    """-> (dX, dY, bound_X, bound_Y) float64: the gradients in any order and the counted bound (h + 4) * 2^-24 * sum |g| 2 |v| of a
    chain of h terms, per coordinate."""
    X, Y, g = np.asarray(X, np.float64), np.asarray(Y, np.float64), np.asarray(g, np.float64)
    b, n, K = np.asarray(idx).shape
    m = Y.shape[1]
    valid, at, _, _ = _live(idx, x_lengths, y_lengths, m)
    dX, dY, aX, aY = np.zeros((b, n, 3)), np.zeros((b, m, 3)), np.zeros((b, n, 3)), np.zeros((b, m, 3))
    hX, hY = valid.sum(-1), np.zeros((b, m), np.int64)
    for c in range(b):
        v = 2 * (X[c][:, None, :] - Y[c][at[c]]) * valid[c][..., None]          # (N, K, 3)
        t = g[c][..., None] * v
        dX[c], aX[c] = t.sum(1), np.abs(t).sum(1)
        np.add.at(dY[c], at[c][valid[c]], -t[valid[c]])
        np.add.at(aY[c], at[c][valid[c]], np.abs(t[valid[c]]))
        np.add.at(hY[c], at[c][valid[c]], 1)
    return dX, dY, (hX[..., None] + 4) * U * aX, (hY[..., None] + 4) * U * aY


def excess(X, Y, K, x_lengths, y_lengths, idx32):
    """The largest amount by which the float64 d at knn32's k-th neighbour exceeds the float64 k-th smallest d, over every real slot."""
    X = np.asarray(X, np.float32)
    b, n = X.shape[:2]
    Y = _targets(Y, b)
    d64, _ = knn64(X, Y, K, x_lengths, y_lengths)
    worst = 0.0
    for c in range(b):
        real = idx32[c] >= 0
        v = X[c].astype(np.float64)[:, None, :] - Y[c].astype(np.float64)[np.clip(idx32[c], 0, None)]
        at32 = (v * v).sum(-1)
        if real.any():
            worst = max(worst, float((at32 - d64[c])[real].max()))
    return worst


def upstream(b, n, K, seed=2801):
    """The upstream gradient of dist2 the tests use: (B, N, K) float32, both signs."""
    return np.random.default_rng(seed + 7 * b + 3 * n + K).uniform(-1, 1, (b, n, K)).astype(np.float32)


def _ball(rng, *shape):
    d = rng.standard_normal(shape + (3,))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0, 1, shape + (1,)) ** (1 / 3)).astype(np.float32)


def ragged_lengths(rng, n, m, K):
    """(x_lengths, y_lengths) of a B_RAGGED batch: cloud 0 n_b = 0, cloud 1 m_b = 0, cloud 2 m_b = 1, cloud 3 1 < m_b < K where K and M
    allow it (else m_b = min(M, 2)), cloud 4 anything in the upper half."""
    xl = np.array([0, rng.integers(1, n + 1), rng.integers(1, n + 1), rng.integers(1, n + 1), rng.integers((n + 1) // 2, n + 1)], np.int32)
    few = int(rng.integers(2, min(K, m + 1))) if min(K, m + 1) > 2 else min(m, 2)
    yl = np.array([rng.integers(1, m + 1), 0, 1, few, rng.integers((m + 1) // 2, m + 1)], np.int32)
    return xl, yl


def small_last_hit_case(seed=2850, n=200, m=9, K=4):
    """The many-to-one chain with a copy whose LAST hit is far below the any-order bound: every x lies within 1e-2 of y_0 and the other
    targets lie on the far side of the unit ball, so slot 0 of every row names y_0 and dY[0]'s chain has N hits; in the copy the last entry's g is 1e-4 of the
    others'.  Dropping that hit, or taking it twice, stays inside (h + 4) * 2^-24 * sum |g| 2 |v| and changes the bits.
    -> (X, Y, g, g_small), one cloud each."""
    rng = np.random.default_rng(seed)
    Y = np.zeros((1, m, 3), np.float32)
    Y[0, 0] = (0.1, -0.2, 0.3)
    Y[0, 1:] = -Y[0, 0] / np.linalg.norm(Y[0, 0]) * 0.9 + rng.uniform(-0.05, 0.05, (m - 1, 3))      # the far side of the unit ball
    X = (Y[0, 0] + rng.uniform(-5e-3, 5e-3, (1, n, 3))).astype(np.float32)
    g = rng.uniform(0.25, 1, (1, n, K)).astype(np.float32)
    g_small = g.copy()
    g_small[0, -1, 0] *= np.float32(1e-4)
    return X, Y, g, g_small


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def generate(seed=28):
    """G28's arrays: per geometry the inputs of B_RAGGED clouds of unit radius, the lengths of the ragged flavour, and knn32's outputs of
    both flavours (full: the first B_FULL clouds, no lengths); the exact families.  Asserts the float64 excess bound on every case."""
    rng = np.random.default_rng(seed)
    out, names = {}, []

    def add(name, family, X, Y, K, xl=None, yl=None):
        d2, idx = knn32(X, Y, K, xl, yl)
        assert excess(X, Y, K, xl, yl, idx) <= EXCESS, name
        assert idx.max() < 32768
        out.update({name + "/dist2": d2, name + "/idx": idx.astype(np.int16)})
        names.append("%s|%s|%d" % (name, family, K))

    for n, m, K in SHAPES:
        geo = "random_%dx%dx%d" % (n, m, K)
        X, Y = _ball(rng, B_RAGGED, n), _ball(rng, B_RAGGED, m)
        xl, yl = ragged_lengths(rng, n, m, K)
        out.update({geo + "/X": X, geo + "/Y": Y, geo + "/x_lengths": xl, geo + "/y_lengths": yl})
        add(geo + "/full", "random", X[:B_FULL], Y[:B_FULL], K)
        add(geo + "/ragged", "random", X, Y, K, xl, yl)
    # X inside Y, every point of it twice in Y: distance exactly 0, the duplicate pair in index order
    base = _ball(rng, 2, 40)
    Y = np.concatenate([base, _ball(rng, 2, 17), base], 1)                          # point p of base at p and at 57 + p
    pick = np.stack([rng.permutation(40)[:30] for _ in range(2)])
    X = np.stack([base[c][pick[c]] for c in range(2)])
    out.update({"subset/X": X, "subset/Y": Y, "subset/pick": pick.astype(np.int16)})
    add("subset/full", "subset", X, Y, 4)
    # an all-equal target: the row is 0 .. r-1
    X, Y = _ball(rng, 2, 10), np.full((2, 30, 3), 0.25, np.float32)
    out.update({"all_equal/X": X, "all_equal/Y": Y})
    add("all_equal/full", "all_equal", X, Y, 8)
    # points on the lattice 2^-6 Z^3: many exact ties, decided by index
    X = (rng.integers(-8, 9, (2, 50, 3)) / 64.0).astype(np.float32)
    Y = (rng.integers(-8, 9, (2, 200, 3)) / 64.0).astype(np.float32)
    out.update({"lattice/X": X, "lattice/Y": Y})
    add("lattice/full", "lattice", X, Y, 16)
    # many-to-one: every x within 1e-2 of y_0, the other targets far away: dY[0]'s chain has N hits
    X, Y, _, _ = small_last_hit_case()
    out.update({"many_to_one/X": X, "many_to_one/Y": Y})
    add("many_to_one/full", "many_to_one", X, Y, 4)
    out["names"] = np.array(names)
    return out


def g28():
    return np.load(GOLDEN, allow_pickle=False)


def cases(z):
    """The fixture as a list of dicts: name, family, geometry, lengths ("full" / "ragged"), X, Y, K, x_lengths, y_lengths (None when
    full), dist2 float32, idx int64, b, n, m; pick for the subset family."""
    out = []
    for entry in z["names"]:
        name, family, K = str(entry).split("|")
        geo, flavour = name.split("/")
        c = {"name": name, "family": family, "geometry": geo, "lengths": flavour, "K": int(K), "x_lengths": None, "y_lengths": None}
        X, Y = z[geo + "/X"], z[geo + "/Y"]
        if family == "random" and flavour == "full":
            X, Y = X[:B_FULL], Y[:B_FULL]
        if flavour == "ragged":
            c["x_lengths"], c["y_lengths"] = z[geo + "/x_lengths"], z[geo + "/y_lengths"]
        if family == "subset":
            c["pick"] = z["subset/pick"].astype(np.int64)
        c.update(X=X, Y=Y, dist2=z[name + "/dist2"], idx=z[name + "/idx"].astype(np.int64), b=X.shape[0], n=X.shape[1], m=Y.shape[1])
        out.append(c)
    return out
