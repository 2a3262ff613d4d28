"""Families of (M, G) for the backward of the SVD -> SO(3) projection (K2 so3_project_bwd_*, K3's fused dM), their float64 answers and
the two figures every row is judged by.  No GPU: tests/test_project_bwd_host.py runs the float32 / float64 host model of the kernels'
templates on these rows and records what it reaches; tests/test_gpu_project_bwd.py holds the kernels to 4 x that on tilings of them.

Everything is built once from SEED.  M = U diag(s) V^T with Haar U, V in float64, ROUNDED TO FLOAT32; G is standard normal float32; the
answer `d64` is oracle.so3_oracle.projection_backward_np on exactly those float32 numbers, `r64`, `s`, `det` the float64 rotation,
singular values and sign of det(U V^T) of the same rows.

JUDGED families (the gap gamma = s2 + s3', s3' = det * s3, is well defined): a row with gamma / s1 > MIN_GAP is judged by

    J = max |dM - dM64| gamma^2 / (u s1 |G|_F)          u = 2^-24 (float32 kernels), 2^-53 (the float64 kernel)

the first-order bound of A y = b with lambda_min(A) = gamma: the error of b, the error of A and the rotation's own u s1 / gamma all enter
as u s1 |G| / gamma^2.  Every row; no quantile.  Rows at or below MIN_GAP are left out of J only, and are at most 1 % of each judged
family (asserted in data()).

UNJUDGED families (no defined gradient: exact ties, rank one, zero, reflections, NaN, Inf) must be finite (NaN / Inf rows: NaN, in
that row only), bit-stable across routes and, like every finite row, skew: both backward forms give dM = R [y]x, so sym(R^T dM) = 0,

    K = | R^T dM + (R^T dM)^T |_max / (u |dM|_max)       R: the same kernel's forward rotation of the row.

TILING: tile_index / tile_period of tests/heads_ref.py -- a prime period above the fixture's length, a stride coprime to it.  Inputs are
tiled with that index and answers GATHERED with it, never recomputed."""
import functools

import numpy as np

from heads_ref import tile_index, tile_period  # noqa: F401  (re-exported: the GPU test tiles with them)
from oracle import so3_oracle as so

U32 = 2.0**-24
U64 = 2.0**-53
SEED = 41
ROWS_JUDGED = 2048
ROWS_UNJUDGED = 512
ROWS_NONFINITE = 16
MIN_GAP = 1e-5                              # gamma / s1 at or below it: not judged by J
MAX_LEFT_OUT = 0.01                         # share of a judged family's rows that may be so
SMALL_E = (1e-1, 1e-2, 1e-3, 1e-4)
REFLECT_E = (1e-1, 1e-2, 1e-3)
SCALES = (("1e-5", 1e-5), ("1e5", 1e5), ("2^-40", 2.0**-40), ("2^40", 2.0**40), ("1e-18", 1e-18), ("1e18", 1e18))


def haar(rng, n):
    """Haar rotations: QR of a Gaussian with the signs of R's diagonal fixed, then det +1."""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def with_singular_values(rng, s):
    u, v = haar(rng, len(s)), haar(rng, len(s))
    return (u * s[:, None, :]) @ v.transpose(0, 2, 1)


def _judged(rng):
    n = ROWS_JUDGED
    one = np.ones(n)
    fams = {"gaussian": rng.standard_normal((n, 3, 3))}
    for e in SMALL_E:                                                     # settled rows with a small gap: backward_from_rotation
        fams["s=(1,e,-eU) e=%.0e" % e] = with_singular_values(rng, np.stack([one, e * one, -e * rng.uniform(0, 0.9, n)], 1))
    for e in SMALL_E:
        fams["s=(1,e,e) e=%.0e" % e] = with_singular_values(rng, np.stack([one, e * one, e * one], 1))
    for e in REFLECT_E:                                                   # two small gaps: s2 + s3' = e, s1 + s3' <= 2 e
        u = rng.random(n)
        fams["near-reflection e=%.0e" % e] = with_singular_values(rng, np.stack([one, 1 - e * u, -(1 - e * (1 + u))], 1))
    fams["graded (1,1e-2,1e-4)"] = with_singular_values(rng, np.stack([one, 1e-2 * one, 1e-4 * one], 1))
    fams["s=(1,10^U(-4,0),0)"] = with_singular_values(rng, np.stack([one, 10.0 ** rng.uniform(-4, 0, n), 0 * one], 1))
    fams["haar + 1e-3 gaussian"] = haar(rng, n) + 1e-3 * rng.standard_normal((n, 3, 3))
    fams["bf16 gaussian"] = _bf16(rng.standard_normal((n, 3, 3)))
    fams["entries in -3..3"] = rng.integers(-3, 4, (n, 3, 3)).astype(np.float64)
    for label, sc in SCALES:                                              # both sides of the prescale window |M|^2 in [2^-28, 2^34]
        fams["gaussian x " + label] = sc * rng.standard_normal((n, 3, 3))
    return fams


def _unjudged(rng):
    n = ROWS_UNJUDGED
    s = rng.random((n, 3)) + 0.5                                          # tools/k1_hard_rows.py: "generic ties"
    s[:, 0] += 1.0
    s[:, 2] = -s[:, 1] * (1 - 1e-6)
    fams = {"generic ties": with_singular_values(rng, s),
            "rank one": rng.standard_normal((n, 3, 1)) @ rng.standard_normal((n, 1, 3)),
            "entries in {-1,0,1}": rng.integers(-1, 2, (n, 3, 3)).astype(np.float64),
            "all zero": np.zeros((n, 3, 3)),
            "exact reflections": haar(rng, n).astype(np.float32).astype(np.float64) * np.array([1.0, 1.0, -1.0]),
            "nan rows": np.full((ROWS_NONFINITE, 3, 3), np.nan)}
    inf = np.where(rng.random((ROWS_NONFINITE, 3, 3)) < 0.5, -np.inf, np.inf)
    inf[0] = np.inf
    fams["inf rows"] = inf
    return fams


def _bf16(a):
    """Round to nearest even to the values a bfloat16 holds (finite input)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64).reshape(np.shape(a))


@functools.lru_cache(maxsize=None)
def data():
    """dict: m (n,9) float32, g (n,9) float32, d64 (n,9), r64 (n,9), s1, gamma (n,), fam (n,) family number, names, judged (per
    family), jrow (n,) rows judged by J, finite (n,) rows with finite input.  Read-only."""
    rng = np.random.default_rng(SEED)
    judged, unjudged = _judged(rng), _unjudged(rng)
    names = list(judged) + list(unjudged)
    m = np.concatenate([judged[k] for k in judged] + [unjudged[k] for k in unjudged]).reshape(-1, 9)
    with np.errstate(over="ignore"):
        m = m.astype(np.float32)
    fam = np.concatenate([np.full(len(v), i) for i, v in enumerate(list(judged.values()) + list(unjudged.values()))])
    n = len(m)
    g = rng.standard_normal((n, 9)).astype(np.float32)
    finite = np.isfinite(m).all(1)
    m64 = np.where(finite[:, None], m.astype(np.float64), 0.0)
    r64, s, det = so.symmetric_orthogonalization_np(m64, return_parts=True)
    with np.errstate(invalid="ignore"):                                    # 0 / 0 on the rows without a gradient
        d64 = so.projection_backward_np(m64, g).reshape(n, 9)
    gamma = s[:, 1] + det * s[:, 2]
    is_judged = np.arange(len(names)) < len(judged)
    with np.errstate(divide="ignore", invalid="ignore"):
        jrow = is_judged[fam] & finite & (gamma / s[:, 0] > MIN_GAP)
    for i, name in enumerate(names):
        if is_judged[i]:
            left_out = 1.0 - jrow[fam == i].mean()
            assert left_out <= MAX_LEFT_OUT, (name, left_out)
    t = haar(rng, n).reshape(n, 9).astype(np.float32)                      # K3's targets
    out = dict(m=m, g=g, t=t, d64=d64, r64=r64.reshape(n, 9), s1=s[:, 0], gamma=gamma, fam=fam, names=names, judged=is_judged, jrow=jrow,
               finite=finite, gnorm=np.linalg.norm(g.astype(np.float64), axis=1))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def j_figure(dm, idx=None, u=U32, d64=None, gnorm=None):
    """J per row (NaN where the row is not judged).  idx: the fixture rows the rows of dm were tiled from (None: the fixture itself).
    d64 / gnorm: another upstream's answers and norms for the same M (K3's G is formed from its own R)."""
    d = data()
    idx = np.arange(len(d["m"])) if idx is None else idx
    ref = d["d64"][idx] if d64 is None else d64
    gn = d["gnorm"][idx] if gnorm is None else gnorm
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        err = np.abs(np.asarray(dm, np.float64).reshape(len(idx), 9) - ref).max(1)
        fig = err * d["gamma"][idx] ** 2 / (u * d["s1"][idx] * gn)
    fig = np.where(d["jrow"][idx], fig, np.nan)
    return np.where(d["jrow"][idx] & np.isnan(fig), np.inf, fig)          # a judged row that came back NaN misses every bound


def answers(m, g):
    """The float64 answer and the judge's quantities for rows that are not the fixture's own (its rows rounded to bfloat16, scaled by a
    power of two, or K3's upstream, which is formed from the call's own R): d64, s1, gamma, gnorm, jrow."""
    m64 = np.asarray(m, np.float64).reshape(-1, 9)
    g64 = np.asarray(g, np.float64).reshape(-1, 9)
    _, s, det = so.symmetric_orthogonalization_np(m64, return_parts=True)
    gamma = s[:, 1] + det * s[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        d64 = so.projection_backward_np(m64, g64).reshape(-1, 9)
        jrow = gamma / s[:, 0] > MIN_GAP
    return dict(d64=d64, s1=s[:, 0], gamma=gamma, gnorm=np.linalg.norm(g64, axis=1), jrow=jrow)


def j_of(dm, ans, u=U32, extra=0.0):
    """J per row against answers() (NaN where gamma / s1 <= MIN_GAP); `extra`: an allowance subtracted from the error first (one
    bfloat16 ulp of the answer, where the kernel stores bfloat16)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        err = np.maximum(np.abs(np.asarray(dm, np.float64).reshape(-1, 9) - ans["d64"]) - extra, 0.0).max(1)
        fig = err * ans["gamma"] ** 2 / (u * ans["s1"] * ans["gnorm"])
    fig = np.where(ans["jrow"], fig, np.nan)
    return np.where(ans["jrow"] & np.isnan(fig), np.inf, fig)


@functools.lru_cache(maxsize=None)
def bf16_small_gap():
    """1 025 rows of the small-gap families (every twelfth row of s = (1, e, -eU) and s = (1, e, e), e <= 1e-2, and one more) ROUNDED TO
    BFLOAT16, with their own answers: the rounding (2^-9 relative) moves s2 and s3 by more than e, so these rows are no family of
    data() any more -- small gaps of every size down to the judge's limit.  m, g float32; `ans` as answers() gives it."""
    d = data()
    names = ["s=(1,e,-eU) e=%.0e" % e for e in SMALL_E[1:]] + ["s=(1,e,e) e=%.0e" % e for e in SMALL_E[1:]]
    rows = np.concatenate([np.flatnonzero(d["fam"] == d["names"].index(k)) for k in names])
    rows = np.concatenate((rows[::12], rows[5:6]))                         # 6 x 2 048 / 12 + 1
    assert len(rows) == 1025
    m = _bf16(d["m"][rows]).astype(np.float32)
    return dict(m=m, g=d["g"][rows], ans=answers(m, d["g"][rows]), rows=rows)


RANK_DEFICIENT = ("small integers", "outer products", "integer outer products", "nine equal entries", "rank two", "rank two + 1e-7", "outer + 1e-7",
                  "entries in -1..1", "reflections", "scaled 1e-5", "scaled 1e+5")


def rank_deficient(n, seed=123):
    """The families of tests/test_gpu_parity.py's test_numerically_rank_deficient_input_still_gives_rotations, drawn on the host: (name,
    float32 rows (n, 9)) one after the other.  No row has a defined gradient worth judging; every one is judged by K."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3, 3)).astype(np.float32)
    two = np.concatenate((a[:, :2], a[:, :1] + a[:, 1:2]), 1)
    outer = lambda: (rng.standard_normal((n, 3, 1)).astype(np.float32) @ rng.standard_normal((n, 1, 3)).astype(np.float32))
    fams = {"small integers": rng.integers(-3, 4, (n, 3, 3)), "outer products": outer(),
            "integer outer products": rng.integers(-3, 4, (n, 3, 1)) @ rng.integers(-3, 4, (n, 1, 3)),
            "nine equal entries": np.broadcast_to(rng.standard_normal((n, 1, 1)), (n, 3, 3)), "rank two": two,
            "rank two + 1e-7": two + np.float32(1e-7) * rng.standard_normal((n, 3, 3)).astype(np.float32),
            "outer + 1e-7": outer() + np.float32(1e-7) * a, "entries in -1..1": rng.integers(-1, 2, (n, 3, 3)),
            "reflections": so.symmetric_orthogonalization_np(rng.standard_normal((n, 9))).astype(np.float32) * np.array([1.0, 1.0, -1.0], np.float32),
            "scaled 1e-5": np.float32(1e-5) * a, "scaled 1e+5": np.float32(1e5) * a}
    assert tuple(fams) == RANK_DEFICIENT
    for name, m in fams.items():
        yield name, np.ascontiguousarray(m, np.float32).reshape(n, 9)


def k_figure(dm, r, u=U32):
    """K per row: NaN where dM is not finite; 0 where dM = 0."""
    dm = np.asarray(dm, np.float64).reshape(-1, 3, 3)
    r = np.asarray(r, np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = r.transpose(0, 2, 1) @ dm
        top = np.abs(w + w.transpose(0, 2, 1)).reshape(len(dm), -1).max(1)
        size = np.abs(dm).reshape(len(dm), -1).max(1)
        fig = np.where(size > 0, top / (u * size), 0.0)
    return np.where(np.isfinite(dm).all((1, 2)), fig, np.nan)


def per_family(fig, idx=None):
    """{family: largest figure} over the rows that have one (families without any: absent)."""
    d = data()
    fam = d["fam"] if idx is None else d["fam"][idx]
    out = {}
    for i, name in enumerate(d["names"]):
        v = fig[fam == i]
        v = v[~np.isnan(v)]
        if len(v):
            out[name] = float(v.max())
    return out


def over_bound(fig, bound, idx=None, factor=4.0):
    """Rows whose figure exceeds factor x its family's recorded figure: (row numbers, their figures, their bounds)."""
    d = data()
    fam = d["fam"] if idx is None else d["fam"][idx]
    limit = np.array([factor * bound.get(name, np.inf) for name in d["names"]])[fam]
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(fig > limit)
    return bad, fig[bad], limit[bad]
