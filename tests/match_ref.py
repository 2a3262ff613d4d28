"""match_features restated as its docstring defines it, in float64 and without torch: for every row of fx the nearest LIVE row of fy
by the sum of squared differences, the lowest index among exactly equal candidates; -1 past x_lengths, for a query row that holds a
non-finite value, when no row of fy is live, and, with mutual, where the match does not point back.  A row of fy is live when it lies
inside y_lengths and all its values are finite.

Beside the answer stands a JUDGED mask: the rows on which an implementation that evaluates sum (a - b)^2 directly in the inputs' own
precision (relative error about (D + 2) eps, and a square root that can merge neighbours) has no freedom.  A search is judged when

  (a) the runner-up's d2 exceeds the nearest d2 by more than BAND(D, eps) * d2_runner-up, BAND = 4 (D + 3) eps, or
  (b) every candidate inside that band is a bit-identical copy of the nearest row (equal operands give equal results in any fixed
      order of evaluation: the lowest index is then required exactly), or
  (c) the case is EXACT -- integers, every d2 an integer below 2^24, so that float32 computes each d2 without rounding in any order
      and equal d2 give equal roots -- and every candidate inside the band has exactly the nearest d2: the lowest index is required
      (a candidate outside the band is further than the root's rounding, 2^-23 relative, can bridge).

With mutual, row i is judged when its forward search is and the back search from the row it found is -- or row i lies outside that
back search's band, so that the search cannot name it and -1 is required whichever row it does name.  expected() asserts on the
reference alone that at most CAP of a case's live rows are unjudged.  The case builders are below; every one is seeded."""
import numpy as np

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
CAP = 0.01
SHAPES = [(1, 1), (13, 9), (25, 25), (26, 9), (9, 26), (64, 64), (257, 300), (1025, 1300)]     # cdist's GEMM route starts above 25 rows
FAMILIES = ["fpfh_like", "decoys", "offset", "duplicates", "small_integer", "non_finite"]
CLOUDS = 3                                                                                     # every case holds 3 clouds; B = 1 is cloud 0
OFFSET = 4096.0
SMALL_INTEGER_D = 5                                                                            # tests/test_fpfh_host.py's family: short rows, many exact ties
ATTEMPTS = 40                                                                                  # redraws of a case whose unjudged share exceeds CAP
QUANTUM = 2.0 ** -11                                                                           # float32's step in [4096, 8192)


class CapExceeded(AssertionError):
    """More than CAP of a case's live rows are unjudged: the one condition for which build() draws again."""


def lengths_of(lengths, b, full):
    return np.full(b, full, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, full)


def band(d, eps):
    return 4.0 * (d + 3) * eps


# ---- the definition ---------------------------------------------------------------------------------------------------------
def sq_dists(fx, fy):
    """(B, N, M) float64 sums of squared differences (rows holding a non-finite value are read as zeros: the caller masks them)."""
    fx, fy = (np.where(np.isfinite(f).all(-1, keepdims=True), f, 0.0).astype(np.float64) for f in (fx, fy))
    b, n, m = fx.shape[0], fx.shape[1], fy.shape[1]
    out = np.empty((b, n, m), np.float64)
    step = max(1, (1 << 22) // max(1, m * fx.shape[2]))
    for c in range(b):
        for i in range(0, n, step):
            diff = fx[c, i:i + step, None, :] - fy[c, None, :, :]
            out[c, i:i + step] = np.einsum("nmd,nmd->nm", diff, diff)
    return out


def _search(d2, rows, live, tol, exact):
    """Along the last axis of d2 (Q, C) among the candidates `live` (C,): (nearest (Q,), judged (Q,), inside (Q, C): the candidates
    within the band of the nearest, itself included); rows (C, D) are the candidates."""
    q = d2.shape[0]
    if not live.any():
        return np.full(q, -1, np.int64), np.ones(q, bool), np.zeros(d2.shape, bool)
    masked = np.where(live[None, :], d2, np.inf)
    near = masked.argmin(1)                                                        # numpy's argmin is the first of equal values
    best = masked[np.arange(q), near]
    inside = live[None, :] & (masked * (1.0 - tol) <= best[:, None])               # NOT (d2 - best > tol * d2)
    group = np.unique(np.where(live[:, None], rows, 0.0), axis=0, return_inverse=True)[1].reshape(-1)   # equal rows, equal number
    free = inside & (group[None, :] != group[near][:, None])                      # in the band and not a copy of the nearest row
    if exact:
        free &= masked != best[:, None]
    judged = ~free.any(1)
    return near.astype(np.int64), judged, inside


def match_ref(fx, fy, x_lengths=None, y_lengths=None, mutual=True, eps=EPS32, exact=False, d2=None):
    """-> (match (B, N) int64, judged (B, N) bool).  d2: sq_dists(fx, fy), where the caller keeps it for several calls."""
    fx, fy = np.asarray(fx), np.asarray(fy)
    b, n, d = fx.shape
    m = fy.shape[1]
    out, judged = np.full((b, n), -1, np.int64), np.ones((b, n), bool)
    if n == 0 or m == 0:
        return out, judged
    d2 = sq_dists(fx, fy) if d2 is None else d2
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    tol = band(d, eps)
    for c in range(b):
        live_x = (np.arange(n) < nl[c]) & np.isfinite(fx[c]).all(-1)
        live_y = (np.arange(m) < ml[c]) & np.isfinite(fy[c]).all(-1)
        fwd, fj, _ = _search(d2[c], fy[c], live_y, tol, exact)
        keep = live_x & (fwd >= 0)
        ok = fj.copy()
        if mutual and keep.any():
            back, bj, within = _search(d2[c].T, fx[c], live_x, tol, exact)
            at = np.maximum(fwd, 0)
            ok &= bj[at] | ~within[at, np.arange(n)]                              # outside the back search's band: -1 whichever row it names
            keep &= back[at] == np.arange(n)
        out[c] = np.where(keep, fwd, -1)
        judged[c] = ok | ~live_x                                                   # a dead query row is -1 whatever the distances are
    return out, judged


def expected(case, b, label, mutual):
    """match_ref on the first b clouds of a case under the length variant `label`, with the cap asserted on the reference alone
    -> (match, judged, x_lengths, y_lengths, integer dtype).  Computed once per case: the tests share it."""
    key = (b, label, mutual)
    if key not in case["memo"]:
        n, m = case["fx"].shape[1], case["fy"].shape[1]
        _, xl, yl, itype = next(v for v in length_variants(n, m, b) if v[0] == label)
        fx, fy = case["fx"][:b], case["fy"][:b]
        want, judged = match_ref(fx, fy, xl, yl, mutual, eps=case["eps"], exact=case["exact"], d2=case["d2"][:b])
        live = (np.arange(n)[None, :] < lengths_of(xl, b, n)[:, None]) & np.isfinite(fx).all(-1)
        if (~judged).sum() > CAP * live.sum():
            raise CapExceeded((case["name"], key, int((~judged).sum()), int(live.sum())))
        want.setflags(write=False)
        judged.setflags(write=False)
        case["memo"][key] = (want, judged, xl, yl, itype)
    return case["memo"][key]


def variants_of(case):
    """Every (b, label, mutual) a case is run at."""
    n, m = case["fx"].shape[1], case["fy"].shape[1]
    return [(b, v[0], mutual) for b in (1, CLOUDS) for v in length_variants(n, m, b) for mutual in (True, False)]


def length_variants(n, m, b):
    """[(label, x_lengths, y_lengths, integer dtype)]: full, and ragged sets that hold 0, 1, a prefix, a value above the extent and a
    negative one, each of them in int32 and in int64, at B = 1 (one cloud per set) as at B = 3."""
    half_n, part_m = max(1, n // 2), max(1, (2 * m) // 3)
    if b == 1:
        return [("full", None, None, None), ("ragged32", [half_n], [m + 7], np.int32), ("ragged64", [n + 5], [part_m], np.int64),
                ("one32", [1], [1], np.int32), ("one64", [n], [1], np.int64), ("zero32", [0], [m], np.int32), ("zero64", [n], [0], np.int64),
                ("negative32", [n], [-1], np.int32), ("negative64", [-2], [m], np.int64)]
    assert b == 3
    return [("full", None, None, None), ("ragged32", [n + 5, half_n, 1], [part_m, m + 7, 1], np.int32),
            ("ragged32_empty", [0, n, -4], [m, -1, 0], np.int32), ("ragged64", [-2, n, n // 2 + 1], [m, 0, -1], np.int64),
            ("ragged64_mixed", [n + 9, 0, half_n], [-3, m + 2, 1], np.int64)]


# ---- the number formats -----------------------------------------------------------------------------------------------------
def round_to(a, fmt):
    """float64 -> the nearest value of `fmt`, returned as float32 (float16, bfloat16) or in its own dtype (float32, float64)."""
    if fmt == "float64":
        return np.asarray(a, np.float64)
    a32 = np.asarray(a, np.float64).astype(np.float32)
    if fmt == "float32":
        return a32
    if fmt == "float16":
        return a32.astype(np.float16).astype(np.float32)
    assert fmt == "bfloat16"
    u = a32.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000                                # round to nearest even on the upper 16 bits
    return u.astype(np.uint32).view(np.float32)


# ---- the families -------------------------------------------------------------------------------------------------------------
def histograms(rng, shape, d):
    """FPFH's magnitudes: ceil(d / 11) Dirichlet histograms of up to 11 bins, each summing to 200."""
    parts = [rng.dirichlet(np.ones(min(11, d - at)), shape) * 200.0 for at in range(0, d, 11)]
    return np.concatenate(parts, -1)


def queries(rng, fy, n, sigma, fresh):
    """fx (B, n, D): a permuted copy of fy's rows plus N(0, sigma) noise; where n exceeds M the further rows are fresh(count) draws."""
    b, m, d = fy.shape
    fx = np.empty((b, n, d))
    for c in range(b):
        take = rng.permutation(m)[:n]
        fx[c, :take.size] = fy[c, take] + sigma * rng.standard_normal((take.size, d))
        if n > take.size:
            fx[c, take.size:] = fresh(n - take.size)
    return fx


def quantise(a):
    return np.round(a / QUANTUM) * QUANTUM


def _fpfh_like(rng, n, m, d):
    fy = histograms(rng, (CLOUDS, m), d)
    return queries(rng, fy, n, 1e-3, lambda k: histograms(rng, (k,), d)), fy


def _decoys(rng, n, m, d):
    """Every odd row of fy is its even neighbour plus N(0, 0.02); all values are multiples of 2^-11 so that `offset` stays exact."""
    fy = histograms(rng, (CLOUDS, m), d)
    fy[:, 1::2] = fy[:, 0:2 * (m // 2):2] + 0.02 * rng.standard_normal((CLOUDS, m // 2, d))
    fy = quantise(fy)
    return quantise(queries(rng, fy, n, 1e-3, lambda k: histograms(rng, (k,), d))), fy


def _duplicates(rng, n, m, d):
    """Groups of three bit-identical rows in fy and in fx, and beside each group a decoy 0.05 away."""
    fy = histograms(rng, (CLOUDS, m), d)
    for c in range(CLOUDS):
        for g in range(m // 8):
            at = rng.permutation(m)[:4]
            step = rng.standard_normal(d)
            fy[c, at[1]] = fy[c, at[2]] = fy[c, at[0]]
            fy[c, at[3]] = fy[c, at[0]] + 0.05 * step / np.linalg.norm(step)
    fy = fy.astype(np.float32).astype(np.float64)
    fx = queries(rng, fy, n, 1e-3, lambda k: histograms(rng, (k,), d))
    for c in range(CLOUDS):
        for g in range(n // 8):
            at = rng.permutation(n)[:3]
            fx[c, at[1]] = fx[c, at[2]] = fx[c, at[0]]
    return fx, fy


def _small_integer(rng, n, m, d):
    """tests/test_fpfh_host.py's family: integers in [-3, 3], exact distances and many exact ties between different rows."""
    fx, fy = rng.integers(-3, 4, (CLOUDS, n, d)).astype(np.float64), rng.integers(-3, 4, (CLOUDS, m, d)).astype(np.float64)
    if m > 4:
        fy[:, 4] = fy[:, 1]
    if n > 7:
        fx[:, 7] = fx[:, 2]
    return fx, fy


def _non_finite(rng, n, m, d):
    """The decoys with one NaN row and one +inf row in fy and one NaN row in fx (M = 1: the NaN row is the whole cloud)."""
    fx, fy = _decoys(rng, n, m, d)
    fy[:, m // 3, rng.integers(0, d)] = np.nan
    if m > 1:
        fy[:, (2 * m) // 3 if (2 * m) // 3 != m // 3 else m - 1, rng.integers(0, d)] = np.inf
    fx[:, n // 2, :] = np.nan
    return fx, fy


def _half_exact(rng, n, m, d):
    """Integers in [0, 255] (exact in float16 and bfloat16): fy's odd rows are r, its even rows the decoy r + 2 e +- u_k, and the query is
    r + e with e in [-5, 5]^D: d2 = |e|^2 (about 10 D) to the odd row and |e|^2 + 2 |e_k| + 1 to the decoy BEFORE it, every sum exact
    in float32 and not in an 8- or 11-bit significand."""
    fy = rng.integers(12, 244, (CLOUDS, m, d)).astype(np.float64)
    fx = rng.integers(12, 244, (CLOUDS, n, d)).astype(np.float64)
    for c in range(CLOUDS):
        pairs = rng.permutation(m // 2)[:n]
        for i, p in enumerate(pairs):
            e, k = rng.integers(-5, 6, d).astype(np.float64), rng.integers(0, d)
            u = np.zeros(d)
            u[k] = 1.0 if e[k] >= 0 else -1.0
            fx[c, i] = fy[c, 2 * p + 1] + e
            fy[c, 2 * p] = fy[c, 2 * p + 1] + 2 * e + u
    return fx, fy


_BUILDERS = {"half_exact": _half_exact, "fpfh_like": _fpfh_like, "decoys": _decoys, "offset": _decoys, "duplicates": _duplicates, "small_integer": _small_integer,
             "non_finite": _non_finite}
_CACHE = {}


def make_case(name, fx, fy, eps, exact=False):
    c = {"name": name, "fx": fx, "fy": fy, "eps": eps, "exact": exact, "d2": sq_dists(fx, fy), "memo": {}}
    if exact:
        assert (fx == np.round(fx)).all() and (fy == np.round(fy)).all() and c["d2"].max() < 2 ** 24, name
    return c


def build(family, n, m, d=None, fmt="float32", fmt_y=None):
    """The case (family, N, M, D) -- D = 33 unless given, and SMALL_INTEGER_D = 5 for small_integer, the length at which integers in
    [-3, 3] tie often; the case's name carries the D it was built with -- with fx in `fmt` and fy in `fmt_y` (default: fmt), both stored as numpy arrays whose values the format
    holds exactly.  A draw whose unjudged share exceeds CAP at any (B, lengths, mutual) is drawn again with the next seed -- judged on
    the reference alone.  The arithmetic's eps is float64's when both sides promote to it, float32's otherwise (half inputs are computed in
    float32).  Built once per process: the tests share it and leave it unchanged."""
    fmt_y = fmt_y or fmt
    if d is None:
        d = SMALL_INTEGER_D if family == "small_integer" else 33
    key = (family, n, m, d, fmt, fmt_y)
    if key in _CACHE:
        return _CACHE[key]
    for attempt in range(ATTEMPTS):
        rng = np.random.default_rng([sorted(_BUILDERS).index(family), n, m, d, attempt])
        fx, fy = _BUILDERS[family](rng, n, m, d)
        if family == "offset":
            fx, fy = fx + OFFSET, fy + OFFSET
        fx, fy = round_to(fx, fmt), round_to(fy, fmt_y)
        if family in ("decoys", "offset", "non_finite") and not {"float16", "bfloat16"} & {fmt, fmt_y}:
            fin = np.isfinite(fx)
            assert (fx[fin] / QUANTUM == np.round(fx[fin] / QUANTUM)).all(), "the inputs are not exactly representable"
        eps = EPS64 if "float64" in (fmt, fmt_y) else EPS32
        case = make_case("%s %dx%d D=%d %s/%s" % (family, n, m, d, fmt, fmt_y), fx, fy, eps, exact=family in ("small_integer", "half_exact"))
        try:                                                                      # the cap is a condition of the case: draw again until it holds
            for v in variants_of(case):
                expected(case, *v)
        except CapExceeded:
            if attempt == ATTEMPTS - 1:
                raise
            continue
        for a in (case["fx"], case["fy"], case["d2"]):
            a.setflags(write=False)
        _CACHE[key] = case
        return case
