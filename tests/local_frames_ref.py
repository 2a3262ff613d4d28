"""Shared by tests/test_local_frames_host.py, tests/test_gpu_local_frames.py and tools/gen_golden.py (G29): local_frames restated in
numpy from its DEFINITION (include/so3proj.h), the judges of its eigen stage, and the fixture's layout.  No reference code exists for
this operation; the header is the contract.

    lengths:  cloud b's rows i < n_b = clip(x_len[b], 0, N) are live, its points j < m_b = clip(y_len[b], 0, M) exist
    valid:    a slot of row (b, i) is valid when 0 <= idx < m_b; r = the number of valid slots, j_0 the first one (the pivot)
    cov32:    d_k = y_jk - y_j0 (one rounded subtraction), s = the chain of rounded additions from +0 in ascending k, m = s / (float)r,
              e_k = d_k - m, S_ab = the chain from +0 of fma(e_ka, e_kb, S_ab) (tests/f32_exact.fma32), C_ab = S_ab / (float)r for
              (xx, xy, xz, yy, yz, zz).  EXACT: the kernel and the host model must reproduce it bit for bit.
    frames64: the float64 covariance of the same float32 inputs through the same idx and numpy.linalg.eigh of it.

The eigen stage is an approximation; its judges, with u = 2^-24 and t = tr C64, over EVERY row (no quantiles):
    cov      |cov - C64|_max <= C_COV u t
    orth     |E^T E - I|_max <= C_ORTH u,  det E > 0,  normals == frames[..., 0] bitwise
    eig      ascending, >= 0,  |lambda_k - lambda64_k| <= C_EIG u t
    res      |C64 e_k - lambda_k e_k|_2 <= C_RES u t          (gap-free: the whole judgement of isotropic, collinear and tied rows)
    nrm      sin angle(e0, e64_0) <= min(1, C_NRM u t / (lambda64_1 - lambda64_0)), up to sign
    signs    the largest-magnitude component of e0 (without a viewpoint) and of e2 is positive, the lowest index among equal
             magnitudes; with a viewpoint v the float64 e0 . (v - y_j0) >= -8 u |v - y_j0|
    zero     C64 == 0 (r = 1, all neighbours equal): eigenvalues 0, the identity frame, whatever the viewpoint; r = 0 and dead rows: zeros everywhere
Each constant is 4 x what the float32 host model of the kernel's own device functions (tests/host_model/local_frames.cpp, libm's
sqrt and 1 / sqrt) reaches over G29 -- the rule of the head-edge tests: the device rounds v_rsq_f32 and v_sqrt_f32 differently (1 ulp),
and 4 x has covered that there.  MEASURED holds the host model's figures; tests/test_local_frames_host.py holds the model to them."""
import functools
import os

import numpy as np

from f32_exact import fma32
import knn_ref
from support import bits, lengths_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g29_local_frames.npz")
U = 2.0 ** -24
MAX_K = 64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                      # (xx, xy, xz, yy, yz, zz)
SURFACE_SHAPES = [(64, 64, 8), (257, 300, 16), (300, 1025, 64)]              # (N, M, K): the first N points of the cloud are the queries
SMALL_GAP, SMALL_GAP_SHARE = 1e-2, 0.10                                       # rows with gap < SMALL_GAP t: at most this share of a surface family
INT32_MIN = -2 ** 31
# what the host model reaches over G29 (the figures of MEASURED, rounded up) ...
MEASURED = {"cov": 2.5, "orth": 24.0, "eig": 3.6, "res": 3.7, "nrm": 1.6}
# ... and the judges' constants: 4 x
C_COV, C_ORTH, C_EIG, C_RES, C_NRM = (4 * MEASURED[k] for k in ("cov", "orth", "eig", "res", "nrm"))
CONSTANTS = {"cov": C_COV, "orth": C_ORTH, "eig": C_EIG, "res": C_RES, "nrm": C_NRM}
C_VIEW = 8.0


def _setup(Y, idx, x_lengths, y_lengths, dtype):
    """-> the gathered points (B, N, K, 3) in dtype, valid (B, N, K), r (B, N), the pivot's point (B, N, 3) in dtype, its index (B, N)."""
    idx = np.asarray(idx, np.int64)
    b, n, K = idx.shape
    Y = np.asarray(Y, np.float32)
    Y = np.broadcast_to(Y, (b,) + Y.shape) if Y.ndim == 2 else Y                  # one shared (M, 3) cloud
    m = Y.shape[1]
    nl, ml = lengths_of(x_lengths, b, n), lengths_of(y_lengths, b, m)
    valid = (idx >= 0) & (idx < ml[:, None, None]) & (np.arange(n)[None, :, None] < nl[:, None, None])
    r = valid.sum(-1)
    first = np.argmax(valid, -1)
    j0 = np.where(r > 0, np.take_along_axis(idx, first[..., None], -1)[..., 0], 0)
    batch = np.arange(b)[:, None, None]
    pts = Y.astype(dtype)[batch, np.where(valid, idx, 0)]
    piv = Y.astype(dtype)[batch[..., 0], j0]
    return pts, valid, r, piv, j0


def cov32(Y, idx, x_lengths=None, y_lengths=None):
    """-> cov (B, N, 6) float32: the DEFINED bits; zeros where r == 0."""
    pts, valid, r, piv, _ = _setup(Y, idx, x_lengths, y_lengths, np.float32)
    K = valid.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = pts - piv[:, :, None, :]
        s = np.zeros(piv.shape, np.float32)
        for k in range(K):
            s = np.where(valid[:, :, k, None], s + d[:, :, k], s)
        rf = np.maximum(r, 1).astype(np.float32)[..., None]
        e = d - (s / rf)[:, :, None, :]
        S = np.zeros(r.shape + (6,), np.float32)
        for k in range(K):
            new = np.stack([fma32(e[:, :, k, a], e[:, :, k, c], S[..., p]) for p, (a, c) in enumerate(PAIRS)], -1)
            S = np.where(valid[:, :, k, None], new, S)
        C = (S / rf).astype(np.float32)
    return np.where(r[..., None] > 0, C, np.float32(0))


def frames64(Y, idx, x_lengths=None, y_lengths=None, eigen=True):
    """-> C64 (B, N, 3, 3), lam64 (B, N, 3) ascending, E64 (B, N, 3, 3) with the eigenvectors as columns, r (B, N), pivot (B, N, 3);
    eigen=False: the covariance alone (None, None in place of lam64 and E64)."""
    pts, valid, r, piv, _ = _setup(Y, idx, x_lengths, y_lengths, np.float64)
    w = valid[..., None].astype(np.float64)
    rr = np.maximum(r, 1)[..., None]
    mean = (pts * w).sum(2) / rr
    e = (pts - mean[:, :, None, :]) * w
    C = np.einsum("bnka,bnkc->bnac", e, e) / rr[..., None]
    lam, E = np.linalg.eigh(C) if eigen else (None, None)
    return C, lam, E, r, piv


def expand6(cov):
    """(…, 6) -> the symmetric (…, 3, 3)."""
    cov = np.asarray(cov)
    return cov[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(cov.shape[:-1] + (3, 3))


def _lead(e):
    """The component the sign rule looks at: the largest magnitude, the lowest index among equal ones."""
    return np.take_along_axis(e, np.argmax(np.abs(e), -1)[..., None], -1)[..., 0]


def judge(name, Y, idx, x_lengths, y_lengths, viewpoint, cov=None, eigenvalues=None, normals=None, frames=None, want_cov=None, scale=1.0,
          constants=CONSTANTS, ref64=None):
    """Every row of every output that is given, under the judges with `constants`.  -> the measured figure of each judge (the smallest
    constant it would pass with).  want_cov: cov32's bits, compared exactly.  scale: the factor the eigenvalues and the covariance were
    multiplied by (the power-of-two property: the inputs here are the UNscaled ones).  ref64: frames64's result when it is at hand."""
    C64, lam64, E64, r, piv = frames64(Y, idx, x_lengths, y_lengths) if ref64 is None else ref64
    C64, lam64 = C64 * scale, lam64 * scale
    t = np.trace(C64, axis1=-2, axis2=-1)
    live, flat = r > 0, t == 0
    ut = U * np.where(t > 0, t, 1.0)
    got = {}
    if cov is not None:
        cov = np.asarray(cov)
        assert cov.dtype == np.float32 and cov.shape == r.shape + (6,), (name, cov.shape)
        if want_cov is not None:
            assert np.array_equal(bits(cov), bits(want_cov)), (name, "cov bits", int((bits(cov) != bits(want_cov)).sum()), np.argwhere(bits(cov) != bits(want_cov))[:4])
        err = np.abs(expand6(cov).astype(np.float64) - C64).max((-2, -1))
        assert (err[flat] == 0).all(), (name, "cov of a flat or dead row")
        got["cov"] = float((err / ut)[~flat].max()) if (~flat).any() else 0.0
    E = None
    if frames is not None:
        frames = np.asarray(frames)
        assert frames.dtype == np.float32, name
        E = frames.reshape(r.shape + (3, 3)).astype(np.float64)
        assert (E[~live] == 0).all(), (name, "frames of a dead row")
        assert (E[live & flat] == np.eye(3)).all(), (name, "C == 0 gives the identity frame")
        gram = np.abs(np.swapaxes(E, -1, -2) @ E - np.eye(3)).max((-2, -1))
        got["orth"] = float((gram[live] / U).max()) if live.any() else 0.0
        assert (np.linalg.det(E[live]) > 0).all(), (name, "det")
        e0, e2 = E[..., :, 0], E[..., :, 2]
        assert (_lead(e2[live]) > 0).all(), (name, "e2's sign")
        if viewpoint is None:
            assert (_lead(e0[live]) > 0).all(), (name, "e0's sign")
        else:
            w = np.asarray(viewpoint, np.float64)[:, None, :] - piv
            toward = (e0 * w).sum(-1)
            assert (toward[live & ~flat] >= -C_VIEW * U * np.linalg.norm(w, axis=-1)[live & ~flat]).all(), (name, "e0 faces the viewpoint")
        sin = np.linalg.norm(np.cross(e0, E64[..., :, 0]), axis=-1)
        gap = lam64[..., 1] - lam64[..., 0]
        got["nrm"] = float((sin * gap / ut)[live & ~flat].max()) if (live & ~flat).any() else 0.0
    if normals is not None:
        normals = np.asarray(normals)
        assert normals.dtype == np.float32 and normals.shape == r.shape + (3,), (name, normals.shape)
        assert (normals[~live] == 0).all(), (name, "normals of a dead row")
        if frames is not None:
            assert np.array_equal(bits(normals), bits(frames.reshape(r.shape + (3, 3))[..., :, 0])), (name, "normals == frames[..., 0]")
    if eigenvalues is not None:
        lam = np.asarray(eigenvalues)
        assert lam.dtype == np.float32 and lam.shape == r.shape + (3,), (name, lam.shape)
        assert (lam[~live | flat] == 0).all(), (name, "eigenvalues of a flat or dead row")
        lam = lam.astype(np.float64)
        assert (lam >= 0).all() and (np.diff(lam, axis=-1) >= 0).all(), (name, "eigenvalues ascending and >= 0")
        got["eig"] = float((np.abs(lam - lam64).max(-1) / ut)[live & ~flat].max()) if (live & ~flat).any() else 0.0
        if E is not None:
            res = np.linalg.norm(C64 @ E - E * lam[..., None, :], axis=-2).max(-1)
            got["res"] = float((res / ut)[live & ~flat].max()) if (live & ~flat).any() else 0.0
    for k, v in got.items():
        assert v <= constants[k], (name, k, v, constants[k])
    return got


def small_gap_share(lam64, r):
    t = lam64.sum(-1)
    live = r > 0
    return float(((lam64[..., 1] - lam64[..., 0])[live] < SMALL_GAP * t[live]).mean())


def facing_side(Y, viewpoint):
    """The points y of a unit sphere whose side faces the viewpoint v beyond doubt: y . v >= 2.  The viewpoint is above y's tangent
    plane when y . v > 1; an estimated normal n = +-(y cos a + t sin a) that leans by a from the radial direction still satisfies
    "n . (v - y) >= 0 picks the outward sign" when y . v - 1 > tan(a) |t . v|, and with |v| = 3 and y . v >= 2 that allows
    tan(a) up to 1 / sqrt(5): a lean of 24 degrees, where the patches of G29's sphere (12 of 150 points) lean by less than 20
    (asserted in generate())."""
    return (np.asarray(Y, np.float64) * np.asarray(viewpoint, np.float64)[:, None, :]).sum(-1) >= 2.0


# ---- the clouds --------------------------------------------------------------------------------------------------------------
def sphere(rng, *shape):
    d = rng.standard_normal(shape + (3,))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def blob(rng, *shape):
    """A Gaussian blob cut to the unit ball."""
    d = rng.standard_normal(shape + (3,)) / 3
    return (d / np.maximum(1.0, np.linalg.norm(d, axis=-1, keepdims=True))).astype(np.float32)


def plane(rng, *shape, sigma=0.01):
    """A tilted unit disc with Gaussian noise along its normal."""
    rad, phi = np.sqrt(rng.uniform(0, 1, shape)) * 0.98, rng.uniform(0, 2 * np.pi, shape)
    a, b_, nrm = np.array([0.6, 0.0, 0.8]), np.array([0.0, 1.0, 0.0]), np.array([-0.8, 0.0, 0.6])
    p = (rad * np.cos(phi))[..., None] * a + (rad * np.sin(phi))[..., None] * b_ + (sigma * rng.standard_normal(shape))[..., None] * nrm
    return p.astype(np.float32)


SURFACES = {"sphere": sphere, "blob": blob, "plane": plane}


def self_knn(Y, n, K, lengths=None):
    """idx (B, n, K) int32: the K nearest points of the cloud for its first n points (knn_ref.knn32: the point itself is slot 0)."""
    return knn_ref.knn32(Y[:, :n], Y, K, None if lengths is None else np.minimum(lengths, n), lengths)[1].astype(np.int32)


def mixed_rows(rng, b, n, m, K):
    """Rows whose valid slots are not a prefix: -1, M and INT32_MIN interleaved with real indices; row 0 has no valid slot, row 1 has
    exactly one, row 2 exactly two."""
    idx = rng.integers(0, m, (b, n, K)).astype(np.int64)
    junk = rng.choice([-1, m, INT32_MIN], (b, n, K))
    idx = np.where(rng.uniform(size=(b, n, K)) < 0.4, junk, idx)
    idx[:, :, 0] = junk[:, :, 0]                                              # the pivot is never slot 0
    idx[:, 0] = junk[:, 0]
    idx[:, 1], idx[:, 2] = junk[:, 1], junk[:, 2]
    idx[:, 1, K // 2] = 3
    idx[:, 2, 1], idx[:, 2, K - 1] = 5, 2
    return idx.astype(np.int32)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def generate(seed=29):
    """G29's arrays: per case the inputs (Y, idx, the lengths and the viewpoint where the case has them), cov32's output and frames64's
    (lam64, E64; C64 is formed again from the inputs).  Asserts on the restatement itself: cov32 within C_COV u t of float64, and at most SMALL_GAP_SHARE
    rows of a surface family (K >= 8) with a gap below SMALL_GAP t."""
    rng = np.random.default_rng(seed)
    out, names = {}, []

    def add(name, family, Y, idx, xl=None, yl=None, view=None):
        Y, idx = np.ascontiguousarray(Y, np.float32), np.ascontiguousarray(idx, np.int32)
        c32 = cov32(Y, idx, xl, yl)
        ref64 = frames64(Y, idx, xl, yl)
        judge(name, Y, idx, xl, yl, view, cov=c32, ref64=ref64)
        if family in SURFACES and idx.shape[-1] >= 8:
            assert small_gap_share(ref64[1], ref64[3]) <= SMALL_GAP_SHARE, (name, small_gap_share(ref64[1], ref64[3]))
        out.update({name + "/Y": Y, name + "/idx": idx.astype(np.int16) if np.abs(idx.astype(np.int64)).max() < 32768 else idx,
                    name + "/cov32": c32, name + "/lam64": ref64[1], name + "/E64": ref64[2]})
        for key, v in (("x_lengths", xl), ("y_lengths", yl), ("viewpoint", view)):
            if v is not None:
                out[name + "/" + key] = np.asarray(v, np.float32 if key == "viewpoint" else np.int32)
        names.append("%s|%s" % (name, family))

    for fam, make in SURFACES.items():
        for n, m, K in SURFACE_SHAPES:
            Y = make(rng, 1, m)
            add("%s_%dx%dx%d" % (fam, n, m, K), fam, Y, self_knn(Y, n, K))
    for fam in ("sphere", "plane"):                                            # K = 3: the residual judges
        Y = SURFACES[fam](rng, 1, 64)
        add("%s_64x64x3" % fam, fam, Y, self_knn(Y, 64, 3))
    Y = sphere(rng, 1, 150) + np.float32(100)                                 # far from the origin: the pivot keeps the digits
    add("shifted_100x150x12", "shifted", Y, self_knn(Y, 100, 12))
    g = np.arange(12) / 16.0 - 0.375                                          # an exact lattice plane z = 0.25: lambda_0 == 0, normal = +z
    Y = np.stack(np.meshgrid(g, g, [0.25], indexing="ij"), -1).reshape(1, 144, 3).astype(np.float32)
    add("lattice_plane", "lattice_plane", Y, self_knn(Y, 144, 9))
    Y = (rng.uniform(-1, 1, (1, 50, 1)) * (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))).astype(np.float32)
    add("collinear", "collinear", Y, self_knn(Y, 50, 8))
    octa = np.concatenate([np.eye(3), -np.eye(3)])[None].astype(np.float32)   # all eigenvalues tied
    add("octahedron", "tied", octa, self_knn(octa, 6, 6))
    cube = (np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) / np.sqrt(3.0))[None].astype(np.float32)
    add("cube", "tied", cube, self_knn(cube, 8, 8))
    Y = np.broadcast_to(np.array([0.25, -0.5, 0.125], np.float32), (1, 30, 3)).copy()
    add("all_equal", "flat", Y, self_knn(Y, 10, 5))                            # C == 0: the identity frame
    Y = sphere(rng, 1, 40)
    one = np.full((1, 12, 6), -1, np.int32)
    one[0, :, 0] = np.arange(12)
    add("r1", "flat", Y, one)                                                  # r = 1
    two = one.copy()
    two[0, :, 1] = np.arange(12) + 20
    add("r2", "r2", Y, two)                                                    # r = 2: rank one
    Y = blob(rng, 2, 90)
    add("mixed", "mixed", Y, mixed_rows(rng, 2, 33, 90, 12))
    n, m, K = 70, 80, 16                                                       # ragged: n_b = 0, m_b = 0, m_b = 1, 1 < m_b < K, anything
    Y = blob(rng, 5, m)
    xl, yl = np.array([0, 31, 70, 64, 65], np.int32), np.array([80, 0, 1, 9, 63], np.int32)
    idx = knn_ref.knn32(Y[:, :n], Y, K, xl, yl)[1].astype(np.int32)
    add("ragged", "ragged", Y, idx, xl, yl)
    Y = sphere(rng, 1, 150)
    idx = self_knn(Y, 100, 12)
    lean = np.abs((frames64(Y, idx)[2][..., :, 0] * Y[:, :100]).sum(-1))              # |cos| of the float64 normal's lean from the radial direction
    assert lean.min() > np.cos(np.radians(20.0)) and facing_side(Y[:, :100], [[3.0, 0.0, 0.0]]).sum() >= 5, lean.min()
    add("view_inside", "view", Y, idx, view=np.zeros((1, 3), np.float32))
    add("view_outside", "view", Y, idx, view=np.array([[3.0, 0.0, 0.0]], np.float32))
    out["names"] = np.array(names)
    return out


def g29():
    return np.load(GOLDEN, allow_pickle=False)


def cases(z):
    """The fixture as a list of dicts: name, family, Y (B, M, 3), idx (B, N, K) int32, x_lengths, y_lengths, viewpoint (None where the
    case has none), cov32 (B, N, 6), ref64 = (C64 formed here, the fixture's lam64 and E64, r, pivot) as frames64 returns it, b, n, m, K."""
    out = []
    for entry in z["names"]:
        name, family = str(entry).split("|")
        c = {"name": name, "family": family, "Y": z[name + "/Y"], "idx": z[name + "/idx"].astype(np.int32), "cov32": z[name + "/cov32"]}
        for key in ("x_lengths", "y_lengths", "viewpoint"):
            c[key] = z[name + "/" + key] if name + "/" + key in z.files else None
        C64, _, _, r, piv = frames64(c["Y"], c["idx"], c["x_lengths"], c["y_lengths"], eigen=False)
        c["ref64"] = (C64, z[name + "/lam64"], z[name + "/E64"], r, piv)
        c["b"], c["n"], c["K"] = c["idx"].shape
        c["m"] = c["Y"].shape[1]
        out.append(c)
    return out


# ---- the branch cases: inputs that sit exactly ON the sign rules ----------------------------------------------------------------------
# G29 is drawn at random, so no two components of a vector are ever bit-equal and no viewpoint ever lies exactly in a patch's plane.
# These patches are integer lattices on the planes x_p = +-x_q and along the lines e_p - e_q, shifted by (5, 5, 5): every step of the
# covariance is exact, the tied axes get bit-equal diagonal entries and exactly zero couplings to the third axis, and in sym_rotate
# d == 0 makes (c, s) = (|g|, g) / |(g, g)|, so the eigenvector's two tied components have the same magnitude bit for bit whatever rsq
# returns.  "The lowest index decides" and "exactly 0 keeps the sign" then decide alone.  Pure numpy, no fixture file.
EDGE_B, EDGE_N, EDGE_K, EDGE_VALID = 3, 257, 16, 9
EDGE_ROWS = (0, 63, 64, 255, 256)                                             # a wave's and a workgroup's first and last query, the tail
TIED_AXES = ((1, 2), (0, 1), (0, 2))                                          # (p, q), p < q: the planes y = +-z, x = +-y, x = +-z
SHIFT = 5.0


def lattice_plane(p, q, sigma):
    """The 9 points x_r in {-2, 0, 2}, x_p in {-1, 0, 1}, x_q = sigma x_p, shifted: the normal is (e_p - sigma e_q) / sqrt 2."""
    r = 3 - p - q
    pts = np.zeros((9, 3))
    a, c = np.meshgrid([-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0], indexing="ij")
    pts[:, r], pts[:, p], pts[:, q] = a.ravel(), c.ravel(), sigma * c.ravel()
    return (pts + SHIFT).astype(np.float32)


def lattice_line(p, q):
    """The 9 points t (e_p - e_q), t = -4 .. 4, shifted: e2 is (e_p - e_q) / sqrt 2, the other two eigenvalues are 0."""
    pts = np.zeros((9, 3))
    pts[:, p], pts[:, q] = np.arange(-4.0, 5.0), -np.arange(-4.0, 5.0)
    return (pts + SHIFT).astype(np.float32)


def _padded_row(points, i, m, keep_pivot=False):
    """The 9 indices `points` as a row of EDGE_K slots: their order rolled by i (keep_pivot: all but the first), between -1, the
    out-of-range indices m and INT32_MIN, in one of three layouts."""
    v = list(points[:1]) + list(np.roll(points[1:], i)) if keep_pivot else list(np.roll(points, i))
    row = (v, [-1, v[0], m] + v[1:], [INT32_MIN, -1] + v[:4] + [m] + v[4:])[i % 3]
    return row + [-1] * (EDGE_K - len(row) - 1) + [m if i % 3 == 0 else -1]


def _branch_case(name, Y, idx, view=None, **more):
    Y, idx = np.ascontiguousarray(Y, np.float32), np.ascontiguousarray(idx, np.int32)
    c = {"name": name, "family": "branch", "Y": Y, "idx": idx, "x_lengths": None, "y_lengths": None,
         "viewpoint": None if view is None else np.ascontiguousarray(view, np.float32), "cov32": cov32(Y, idx), "ref64": frames64(Y, idx), "m": Y.shape[1]}
    c["b"], c["n"], c["K"] = idx.shape
    c.update(more)
    assert (c["b"], c["n"], c["K"]) == (EDGE_B, EDGE_N, EDGE_K) and (c["ref64"][3] == EDGE_VALID).all(), name
    p, q = c["tied"][..., 0], c["tied"][..., 1]
    cov = bits(c["cov32"]).reshape(EDGE_B, EDGE_N, 6)
    diag, pair = np.array([0, 3, 5]), {(0, 1): 1, (0, 2): 2, (1, 2): 4}
    coupling = np.array([[pair[tuple(sorted((a, 3 - t[0] - t[1])))] for a in t] for t in TIED_AXES])      # (tied axes) -> C_pr, C_qr
    which = np.array([TIED_AXES.index((int(a), int(b_))) for a, b_ in zip(p.ravel(), q.ravel())]).reshape(p.shape)
    take = lambda cols: np.take_along_axis(cov, cols[..., None], -1)[..., 0]                               # noqa: E731
    assert (take(diag[p]) == take(diag[q])).all() and (c["cov32"] != 0).any(-1).all(), name               # the tied diagonal entries: bit-equal
    assert (take(coupling[which, 0]) << 1 == 0).all() and (take(coupling[which, 1]) << 1 == 0).all(), name  # their couplings to the third axis: 0
    return c


@functools.lru_cache(maxsize=None)
def sign_tie_case():
    """SIGN TIES.  One cloud of nine patches, shared by the three batch entries: the planes x_p = x_q (normal (e_p - e_q) / sqrt 2: the
    tie rule alone picks its sign), their mirrors x_p = -x_q, and the lines along e_p - e_q (e2 ties).  Row (b, i) names patch
    (4 i + b) mod 9 -- EDGE_ROWS reach all nine -- through 9 valid slots among 16.  No viewpoint.
    -> the case, with per row: tied (p, q), line (the tied vector is e2, else e0), opposite (the tied components' signs differ)."""
    patches = [lattice_plane(p, q, 1.0) for p, q in TIED_AXES] + [lattice_plane(p, q, -1.0) for p, q in TIED_AXES] + [lattice_line(p, q) for p, q in TIED_AXES]
    Y = np.concatenate(patches)
    m = len(Y)
    which = (4 * np.arange(EDGE_N)[None, :] + np.arange(EDGE_B)[:, None]) % 9
    assert {int(w) for w in which[:, EDGE_ROWS].ravel()} == set(range(9))
    idx = np.array([[_padded_row(np.arange(9) + 9 * which[b, i], i, m) for i in range(EDGE_N)] for b in range(EDGE_B)], np.int64)
    return _branch_case("sign_ties", np.broadcast_to(Y, (EDGE_B, m, 3)), idx, tied=np.array(TIED_AXES)[which % 3], line=which >= 6,
                        opposite=(which < 3) | (which >= 6))


@functools.lru_cache(maxsize=None)
def viewpoint_cases(mirror):
    """A VIEWPOINT EXACTLY IN THE PLANE.  Cloud b is the plane patch of TIED_AXES[b] (mirror: x_p = -x_q); every row keeps the patch's
    first point as its pivot.  -> four cases over the same rows: "none" (no viewpoint), "in" (v = pivot + 2 e_r + 4 t, t the in-plane
    lattice direction e_p + sigma e_q: the tied products are s * 4 and -s * 4, exact, so e0 . (v - pivot) is 0 in any order), and
    "above" / "below" (one lattice step e_p - sigma e_q off the plane on either side)."""
    sigma = -1.0 if mirror else 1.0
    Y = np.stack([lattice_plane(p, q, sigma) for p, q in TIED_AXES])
    idx = np.array([[_padded_row(np.arange(9), i, 9, keep_pivot=True) for i in range(EDGE_N)] for b in range(EDGE_B)], np.int64)
    inside, off = np.zeros((EDGE_B, 3)), np.zeros((EDGE_B, 3))
    for b, (p, q) in enumerate(TIED_AXES):
        inside[b, 3 - p - q], inside[b, p], inside[b, q] = 2, 4, 4 * sigma
        off[b, p], off[b, q] = 1, -sigma
    pivot = Y[:, 0].astype(np.float64)
    views = {"none": None, "in": pivot + inside, "above": pivot + inside + off, "below": pivot + inside - off}
    tied = np.broadcast_to(np.array(TIED_AXES)[:, None, :], (EDGE_B, EDGE_N, 2))
    flags = dict(tied=tied, line=np.zeros((EDGE_B, EDGE_N), bool), opposite=np.full((EDGE_B, EDGE_N), not mirror))
    out = {k: _branch_case("viewpoint %s%s" % (k, ", mirrored" if mirror else ""), Y, idx, v, **flags) for k, v in views.items()}
    assert all((c["ref64"][4] == pivot[:, None, :]).all() for c in out.values())
    return out
