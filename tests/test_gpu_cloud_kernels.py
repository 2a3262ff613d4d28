"""The cloud kernels (k_kabsch, k_kabsch_synth, k_rotate_clouds, k_pc_normalize, k_add_l1) through the raw C ABI, against float64, on every
launch geometry and at their edges.  They share one skeleton -- one wave per cloud at a time, a per-cloud buffer descriptor whose range
check stands in for the tail, lane j keeping the result of the wave's j-th cloud -- so one file drives them all:

  1. every samples-per-wave value the launchers' clamp(B / (CUs 16), 1, 64) takes, with a ragged last wave, at N in {1, 3, 7};
  2. both sides of every points-per-cloud switch (the loops' 64 x unroll trips, the templates chosen by N), outputs inside canaries;
  3. a cloud's answer does not depend on the lane slot and the wave it lands in, bit for bit;
  4. data nothing else feeds them: off-centre clouds, a translation far larger than the cloud, constant clouds, NaN and inf points.

Every cloud is compared, not a quantile.  The bounds (u = 2^-24):
  * H:  |dH_ab| <= 2 N u sum_i |q_ia| |p_ib|, the dot product's bound for any summation order, per cloud and entry;
  * R:  |dR| <= 2.5e-6 s1 / gap + 2 |dH|_F / gap with gap = s2 + s3 sign(det H) from the float64 SVD of the reference H -- the projection's
    own asserted bound (tests/test_gpu_certificate_search.py) plus the polar factor's perturbation bound; a cloud with gap / s1 < 1e-3
    is judged on orthogonality and determinant alone (1e-5 each), and no cloud of 64 points or more may fall under that exclusion;
  * rotated points 2e-6, normalised points and scale 2e-6, centroid 1e-6 (test_g12_cloud_pairing_and_normalisation's numbers), ADD-L1 3e-6
    on the loss and 3e-6 + 8 / (N B) on the batch mean's gradient (test_add_l1_ragged_sizes_against_oracle's), each times max(1, |reference|);
  * the ADD sums before the division: the same dot-product bound over the 3 N summed terms, 6 N u sum_ic S_ic, where
    S_ic = sum_k |dR_ck| |p_ik| + |dt_c| is the sum of the absolute values of the products behind d_ic; for the L2 distance (2 N + 8) u sum_i |S_i|_2
    (N additions; 8 u for the four roundings of d, the input differences' own, and the square root's);
  * the per-sample ADD gradients, which the batch mean's allowance cannot judge at 3e5 samples: the dot-product bound of their sums plus, for
    L1, the sign flips of exactly those coordinates whose |d_ic| lies within 8 u S_ic of the kink (2 |p_ij| / (3 N) each); for L2 the unit
    vector's conditioning, |du_i| <= 16 u |S_i|_2 / |d_i| + 8 u.
"""
import ctypes

import numpy as np
import pytest
import torch

from support import dev, ptr, to_device  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = 0x7FC5A5A5          # a NaN whose payload no arithmetic produces: an output slot that still holds it was not written
PAD = 67                     # floats in front of and behind a guarded output: 268 bytes, so the output is 4-byte and not 16-byte aligned


@pytest.fixture(scope="module")
def wave_slots(dev):
    """W = 16 CUs: the batch at which the launchers go from one cloud per wave to two."""
    return 16 * torch.cuda.get_device_properties(dev).multi_processor_count


def per_wave(b, w):
    return min(max(b // w, 1), 64)


def _so():
    from oracle import so3_oracle as so
    return so


class Out:
    """An output tensor pre-filled with CANARY; `guarded`: inside a larger buffer at a 4-byte-aligned offset, canaries on both sides."""

    def __init__(self, dev, shape, guarded):
        self.n = int(np.prod(shape))
        self.lead = PAD if guarded else 0
        self.buf = torch.full((self.n + 2 * self.lead,), CANARY, dtype=torch.int32, device=dev)
        self.t = self.buf.view(torch.float32)[self.lead:self.lead + self.n].view(shape)
        if guarded:
            assert self.t.data_ptr() % 4 == 0 and self.t.data_ptr() % 16 != 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def untouched(self):
        return bool((self.buf == CANARY).all().item())

    def get(self, index=None):
        """The output on the host (rows `index` only when given), after checking that every slot was written and no canary was."""
        lo, hi = self.lead, self.lead + self.n
        assert bool((self.buf[:lo] == CANARY).all().item()) and bool((self.buf[hi:] == CANARY).all().item()), "a canary was overwritten"
        assert not bool((self.buf[lo:hi] == CANARY).any().item()), "an output slot was not written"
        return (self.t if index is None else self.t[index]).cpu().numpy()


class Abi:
    """The seven entry points over device tensors; every output is an Out."""

    def __init__(self, dev, guarded=False):
        from poseestimation_amd import _lib
        self._lib, self.lib, self.dev, self.guarded = _lib, _lib.load(), dev, guarded

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _out(self, *shape):
        return Out(self.dev, shape, self.guarded)

    def kabsch(self, P, Q):
        b, n = P.shape[:2]
        R, H = self._out(b, 3, 3), self._out(b, 3, 3)
        self._lib.check(self.lib.so3_kabsch_f32(ptr(P), ptr(Q), R.ptr, H.ptr, b, n, self._st()), "so3_kabsch_f32")
        return R, H

    def synth(self, P, Rgt, sigma, seed):
        b, n = P.shape[:2]
        R, H = self._out(b, 3, 3), self._out(b, 3, 3)
        self._lib.check(self.lib.so3_kabsch_synth_f32(ptr(P), ptr(Rgt), sigma, seed, R.ptr, H.ptr, b, n, self._st()), "so3_kabsch_synth_f32")
        return R, H

    def rotate(self, P, R, transposed):
        b, n = P.shape[:2]
        out = self._out(b, 3, n) if transposed else self._out(b, n, 3)
        self._lib.check(self.lib.so3_rotate_clouds_f32(ptr(P), ptr(R), out.ptr, int(transposed), b, n, self._st()), "so3_rotate_clouds_f32")
        return out

    def normalize(self, P):
        b, n = P.shape[:2]
        out, cen, scl = self._out(b, n, 3), self._out(b, 3), self._out(b)
        self._lib.check(self.lib.so3_pc_normalize_f32(ptr(P), out.ptr, cen.ptr, scl.ptr, b, n, self._st()), "so3_pc_normalize_f32")
        return out, cen, scl

    def add(self, kind, Tgt, Tpred, pts, grad_scale=1.0):
        """kind: "l1", "dis" or "l2" -> (dists or None, loss_sum as float64 numpy, dTpred)."""
        b, n = pts.shape[:2]
        loss = torch.full((3,), float("nan"), dtype=torch.float64, device=self.dev)
        dT = self._out(b, 4, 4)
        if kind == "dis":
            dists = None
            code = self.lib.so3_add_l1_disentangled_f32(ptr(Tpred), ptr(Tgt), ptr(pts), ptr(loss), dT.ptr, grad_scale, b, n, self._st())
        else:
            dists = self._out(b)
            fn = self.lib.so3_add_l1_f32 if kind == "l1" else self.lib.so3_add_l2_f32
            code = fn(ptr(Tgt), ptr(Tpred), ptr(pts), dists.ptr, ptr(loss), dT.ptr, grad_scale, b, n, self._st())
        self._lib.check(code, "so3_add_%s_f32" % kind)
        return dists, loss.cpu().numpy(), dT


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def _rotations(rng, b):
    """Haar rotations from unit quaternions, float64 (B,3,3)."""
    q = rng.standard_normal((b, 4))
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(b, 3, 3)


def make_batch(b, n, seed, offset=0.0, extent=1.0, dt_shift=0.0):
    """float32 numpy: P uniform in a cube of side `extent` about `offset`, rotations Rgt, Q = Rgt (P - offset) + 0.01 noise + offset, and two
    poses (Tgt, Tpred) whose translations differ by N(0, 1) + dt_shift per axis."""
    rng = np.random.default_rng(seed)
    P0 = extent * (rng.random((b, n, 3)) - 0.5)
    Rgt = _rotations(rng, b)
    Q = np.einsum("bac,bic->bia", Rgt, P0) + 0.01 * extent * rng.standard_normal((b, n, 3)) + offset
    Tgt, Tpred = np.tile(np.eye(4), (b, 1, 1)), np.tile(np.eye(4), (b, 1, 1))
    Tgt[:, :3, :3], Tpred[:, :3, :3] = Rgt, np.roll(Rgt, 1, axis=0) if b > 1 else Rgt.transpose(0, 2, 1)
    Tgt[:, :3, 3] = rng.standard_normal((b, 3)) + dt_shift
    Tpred[:, :3, 3] = rng.standard_normal((b, 3))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in dict(P=P0 + offset, Q=Q, Rgt=Rgt, Tgt=Tgt, Tpred=Tpred).items()}


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def h_bound(P, Q):
    n = P.shape[1]
    return 2.0 * n * U * np.einsum("bia,bic->bac", np.abs(np.asarray(Q, np.float64)), np.abs(np.asarray(P, np.float64)))


def r_reference(h_ref, bound):
    """(R_ref, the bound on |dR| per cloud, which clouds it judges) from the float64 SVD of the reference H."""
    r_ref, s, d = _so().symmetric_orthogonalization_np(h_ref, return_parts=True)
    gap = s[:, 1] + s[:, 2] * np.sign(d)
    judged = gap >= 1e-3 * s[:, 0]
    judged &= s[:, 0] > 0
    safe = np.where(judged, gap, 1.0)
    return r_ref, 2.5e-6 * s[:, 0] / safe + 2.0 * np.linalg.norm(bound, axis=(1, 2)) / safe, judged


def check_rotation(R, label):
    R = np.asarray(R, np.float64)
    orth = np.linalg.norm(np.einsum("bji,bjk->bik", R, R) - np.eye(3), axis=(1, 2))
    det = np.linalg.det(R)
    assert orth.max() < 1e-5 and np.abs(det - 1).max() < 1e-5, (label, orth.max(), np.abs(det - 1).max())


def check_h_and_r(H, R, P, Q64, label, synth=None):
    """Every cloud's H and R against float64 (module docstring).  synth = (Rgt, sigma) for the synthesiser, whose q = Rgt p + sigma n is
    itself rounded: H is then also held to the same bound with |q_ia| replaced by the products behind it, sum_k |g_ak| |p_ik| + sigma |n_ia|
    (asserted without noise; with it the hardware's logarithm, sine and cosine come on top, and the figure is printed).  The bound on
    |q| itself is asserted last, after everything else has been judged.

    At N = 1, 2, 3 that last bound has no slack for the roundings of q's own products where they cancel: plain float32 numpy in place of
    the kernel misses it (N = 1: 23 x, N = 3: 105 x the bound), and so did k_kabsch_synth (N = 1: up to 1.3e5 x over 258 049 clouds,
    N = 2: 2.4 x, N = 3: up to 30 x; N = 7 and every N >= 63: below 0.6).  Clouds of at most eight points therefore go through
    k_kabsch_synth_few, which forms q in float64, noise included, and rounds it once."""
    n = P.shape[1]
    h_ref = _so().cross_covariance_np(P, Q64)
    bound = h_bound(P, Q64)
    err = np.abs(H - h_ref)
    worst = np.max(err / np.maximum(bound, 1e-300))
    r_ref, rb, judged = r_reference(h_ref, bound)
    r_err = np.abs(R - r_ref).max(axis=(1, 2))
    print("%-44s B %6d N %4d  H err/bound %.3f  R err/bound %.3f  judged %d" % (label, len(P), n, worst,
          np.max(r_err[judged] / rb[judged]) if judged.any() else 0.0, judged.sum()))
    check_rotation(R, label)
    assert (r_err[judged] <= rb[judged]).all(), (label, "R", np.nonzero(judged)[0][r_err[judged] > rb[judged]][:4])
    if n >= 64:
        assert judged.all(), (label, "a cloud of 64 points or more is too ill-conditioned to judge R: change the seed")
    if synth is not None:
        g, p = np.abs(np.asarray(synth[0], np.float64)).reshape(-1, 3, 3), np.asarray(P, np.float64)
        products = np.einsum("bac,bic->bia", g, np.abs(p)) + np.abs(Q64 - np.einsum("bac,bic->bia", np.asarray(synth[0], np.float64), p))
        worst2 = np.max(err / np.maximum(h_bound(P, products) * max(2 * n, n + 3) / (2 * n), 1e-300))     # N additions + q's three roundings
        print("%-44s                     H err/bound over the products behind q %.3f" % (label, worst2))
        assert synth[1] != 0.0 or worst2 <= 1.0, (label, "H, products", worst2)
    assert (err <= bound).all(), (label, "H", worst, np.argwhere(err > bound)[:4])


def check_rotated(out, outT, P, R, label):
    ref = _so().rotate_clouds_np(P, R)
    # |reference| = the cloud's largest coordinate, as the suite scales everywhere: the three roundings of q = R p are relative to the products
    # (1e3 for a cloud 1e3 off centre), whatever is left of them in one coordinate of q.
    tol = np.broadcast_to(2e-6 * np.maximum(1.0, np.abs(ref).max(axis=(1, 2), keepdims=True)), ref.shape)
    e, eT = np.abs(out - ref), np.abs(outT - ref.transpose(0, 2, 1))
    assert (e <= tol).all() and (eT <= tol.transpose(0, 2, 1)).all(), (label, e.max(), eT.max())


def check_normalized(out, cen, scl, P, label, centre_rounding=False):
    """centre_rounding (off-centre clouds): the float32 centre (mx + mn) / 2 is u |c| away from the float64 one, which the division by the
    scale magnifies -- 2 u |c| / scale more on the points."""
    with np.errstate(invalid="ignore", divide="ignore"):
        rn, rc, rs = _so().pc_normalize_np(P)
    assert np.array_equal(np.isnan(out), np.isnan(rn)) and np.array_equal(np.isnan(scl), np.isnan(rs)), label
    ok = ~np.isnan(rn)
    tol = np.full(rn.shape, 2e-6)
    if centre_rounding:
        tol += (2 * U * np.abs(rc).max(axis=-1) / np.maximum(rs, 1e-300))[:, None, None]
    assert (np.abs(out - rn)[ok] <= tol[ok]).all(), (label, "points", np.abs(out - rn)[ok].max())
    assert (np.abs(scl - rs) <= 2e-6 * np.maximum(1.0, rs)).all(), (label, "scale", np.abs(scl - rs).max())
    assert (np.abs(cen - rc) <= 1e-6 * np.maximum(1.0, np.abs(rc))).all(), (label, "centroid", np.abs(cen - rc).max())


def add_terms(Tgt, Tpred, pts, dis):
    """float64: d_ic = (dR p_i + dt)_c and S_ic = sum_k |dR_ck| |p_ik| + |dt_c|  (dt = 0 for the disentangled rotation term)."""
    tg, tp, p = (np.asarray(v, np.float64) for v in (Tgt, Tpred, pts))
    dr = tg[:, :3, :3] - tp[:, :3, :3]
    dt = (tg[:, :3, 3] - tp[:, :3, 3]) * (0.0 if dis else 1.0)
    d = np.einsum("bck,bik->bic", dr, p) + dt[:, None, :]
    return d, np.einsum("bck,bik->bic", np.abs(dr), np.abs(p)) + np.abs(dt)[:, None, :], p


def check_add(kind, dists, loss, dT, Tgt, Tpred, pts, label):
    """One ADD entry run with grad_scale = 1 (dT rows are the per-sample gradients of dist_b) against float64, every sample."""
    so = _so()
    b, n = pts.shape[:2]
    assert (dT[:, 3, :] == 0).all(), (label, "the pose's last row has no gradient")
    d, S, p = add_terms(Tgt, Tpred, pts, kind == "dis")
    absp = np.abs(p)
    if kind in ("l1", "dis"):
        ref_loss, ref_grad, extra = so.add_l1_np(Tgt, Tpred, pts, disentangled=(kind == "dis"))
        if kind == "l1":
            sums = np.abs(dists.astype(np.float64) * (3 * n) - extra * (3 * n))
            bound = 6.0 * n * U * S.sum((1, 2))
            assert (sums <= bound).all(), (label, "dists", np.max(sums / bound))
            assert abs(loss[0] / b - ref_loss) < 3e-6 * max(1.0, abs(ref_loss)), (label, loss[0] / b, ref_loss)
        else:
            assert (np.abs(loss / b - extra) < 3e-6 * np.maximum(1.0, np.abs(extra))).all(), (label, loss / b, extra)
            assert abs(loss.sum() / b - ref_loss) < 3e-6 * max(1.0, abs(ref_loss)), (label, loss.sum() / b, ref_loss)
        mean_err = np.abs(dT.astype(np.float64) / b - ref_grad)
        assert mean_err.max() < 3e-6 * max(1.0, np.abs(ref_grad).max()) + 8.0 / (n * b), (label, "mean gradient", mean_err.max())
        ref_ps = ref_grad * b
        kink = (np.abs(d) <= 8 * U * S).astype(np.float64)
        tol = np.zeros((b, 4, 4))
        tol[:, :3, :3] = (2.0 * n * U * absp.sum(1)[:, None, :] + 2.0 * np.einsum("bic,bij->bcj", kink, absp)) / (3 * n)
        if kind == "l1":
            tol[:, :3, 3] = 2.0 * kink.sum(1) / (3 * n)
    else:
        T, nd = np.sqrt((S ** 2).sum(-1)), np.linalg.norm(d, axis=-1)
        sums = np.abs(dists.astype(np.float64) * n - nd.sum(1))
        bound = (2.0 * n + 8.0) * U * T.sum(1)
        assert (sums <= bound).all(), (label, "dists", np.max(sums / bound))
        ref_loss = nd.mean()
        assert abs(loss[0] / b - ref_loss) < 3e-6 * max(1.0, abs(ref_loss)), (label, loss[0] / b, ref_loss)
        unit = d / np.where(nd > 0, nd, 1.0)[..., None]
        ref_ps = np.zeros((b, 4, 4))
        ref_ps[:, :3, :3] = -np.einsum("bic,bij->bcj", unit, p) / n
        ref_ps[:, :3, 3] = -unit.sum(1) / n
        w = (16.0 * T / np.where(nd > 0, nd, 1e-300) + 8.0 + 2.0 * n) * U
        tol = np.zeros((b, 4, 4))
        tol[:, :3, :3] = (np.einsum("bi,bij->bj", w, absp) / n)[:, None, :]
        tol[:, :3, 3] = (w.sum(1) / n)[:, None]
    tol += 4 * U * np.abs(ref_ps) + 1e-12          # (1e-12: the float64 reference's own sums -- signs that cancel exactly come back as 1e-15)
    err = np.abs(dT - ref_ps)
    assert (err <= tol).all(), (label, "per-sample gradient", np.argwhere(err > tol)[:4], np.max(err / tol))
    return float(np.max(err / tol))


PARTS = ("kabsch", "synth0", "synth1", "clouds", "l1", "dis", "l2")


def run_part(abi, dev, data, part, label, sigma=0.01, seed=1234):
    """One kernel of the family (PARTS; "clouds" = rotate in both layouts and normalise) on one batch, every output of every cloud against
    float64."""
    so = _so()
    label = "%s %s" % (label, part)
    P = to_device(data["P"], dev)
    if part == "kabsch":
        R, H = abi.kabsch(P, to_device(data["Q"], dev))
        check_h_and_r(H.get(), R.get(), data["P"], data["Q"], label)
    elif part in ("synth0", "synth1"):
        sg = float(np.float32(sigma)) if part == "synth1" else 0.0           # the ABI takes sigma as a float32: the reference gets that value
        R, H = abi.synth(P, to_device(data["Rgt"], dev), sg, seed)
        check_h_and_r(H.get(), R.get(), data["P"], so.synth_pairs_np(data["P"], data["Rgt"], sg, seed), label, synth=(data["Rgt"], sg))
    elif part == "clouds":
        Rgt = to_device(data["Rgt"], dev)
        check_rotated(abi.rotate(P, Rgt, False).get(), abi.rotate(P, Rgt, True).get(), data["P"], data["Rgt"], label)
        out, cen, scl = abi.normalize(P)
        check_normalized(out.get(), cen.get(), scl.get(), data["P"], label)
    else:
        dists, loss, dT = abi.add(part, to_device(data["Tgt"], dev), to_device(data["Tpred"], dev), P)
        worst = check_add(part, None if dists is None else dists.get(), loss, dT.get(), data["Tgt"], data["Tpred"], data["P"], label)
        print("%-44s B %6d N %4d  per-sample gradient err/bound %.3f" % (label, len(data["P"]), data["P"].shape[1], worst))
    torch.cuda.synchronize()


# ---- 1. every samples-per-wave geometry -------------------------------------------------------------------------------------------------
# (k, clouds in the last wave, N): the last wave holds 1, k - 1 and an in-between number of clouds across the cases; 70 W + 1 is capped at 64.
GEOMETRIES = [(2, 1, 7), (3, 2, 3), (5, 3, 1), (15, 14, 7), (17, 9, 3), (63, 1, 1), (64, 63, 1), (64, 31, 7), (70, 1, 3)]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("k,last,n", GEOMETRIES, ids=lambda v: str(v))
def test_every_samples_per_wave_geometry(dev, wave_slots, k, last, n, part):
    """B = k W + r clouds: k clouds per wave (64 at most) and a last wave of `last` clouds, every kernel, every cloud against float64.
    Fails if a keep-loop writes lane j + 1 instead of lane j, or if a wave's cloud count or first cloud is computed wrongly."""
    w = wave_slots
    pw = min(k, 64)
    b = 70 * w + 1 if k == 70 else k * w + last                               # k W is a multiple of k: the last wave holds r = last
    assert per_wave(b, w) == pw and (k == 70 or (b - 1) % pw + 1 == last)
    run_part(Abi(dev), dev, make_batch(b, n, 1000 * k + last), part, "per_wave %d last %d" % (pw, last))


# ---- 2. both sides of every points-per-cloud switch ---------------------------------------------------------------------------------------
POINTS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537, 2049, 3001]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("n", POINTS)
def test_both_sides_of_every_points_per_cloud_switch(dev, n, part):
    """B in {1, 5, 67} at every N around the loops' trip lengths (64 x 2, 4, 8, 16) and the templates' thresholds (k_pc_normalize <4> / <16> /
    two-pass at 256 / 1024, k_add_l1 unroll 2 / 8 / 16 at 128 / 512), and beyond 1024 where the Kabsch kernels take a second trip (the
    synthesiser's pair index (i0 >> 7) + (u >> 1) with i0 > 0).  Outputs sit between canaries at a 4-byte-aligned address."""
    abi = Abi(dev, guarded=True)
    for b in (1, 5, 67):
        run_part(abi, dev, make_batch(b, n, 7 * n + b), part, "switch B %d" % b)


def test_zero_points_are_refused_with_nothing_written(dev):
    abi = Abi(dev, guarded=True)
    lib, st = abi.lib, abi._st()
    P, T = torch.zeros(4, 1, 3, device=dev), torch.eye(4, device=dev).repeat(4, 1, 1).contiguous()
    out, cen, scl, dists, dT = Out(dev, (4, 1, 3), True), Out(dev, (4, 3), True), Out(dev, (4,), True), Out(dev, (4,), True), Out(dev, (4, 4, 4), True)
    loss = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    assert lib.so3_pc_normalize_f32(ptr(P), out.ptr, cen.ptr, scl.ptr, 4, 0, st) != 0
    assert lib.so3_add_l1_f32(ptr(T), ptr(T), ptr(P), dists.ptr, ptr(loss), dT.ptr, 1.0, 4, 0, st) != 0
    assert lib.so3_add_l2_f32(ptr(T), ptr(T), ptr(P), dists.ptr, ptr(loss), dT.ptr, 1.0, 4, 0, st) != 0
    assert lib.so3_add_l1_disentangled_f32(ptr(T), ptr(T), ptr(P), ptr(loss), dT.ptr, 1.0, 4, 0, st) != 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (out, cen, scl, dists, dT)) and bool(torch.isnan(loss).all().item())


# ---- 3. a cloud does not depend on where it sits ---------------------------------------------------------------------------------------------
def _embed(dev, small, b, pos, seed):
    """Device batches of b clouds / poses: random filler (every seventh cloud scaled by 1e6, another seventh by 1e-6) with the 40 clouds of
    `small` at the positions `pos`."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    n = small["P"].shape[1]
    idx = torch.arange(b, device=dev)
    scale = torch.where(idx % 7 == 3, 1e6, torch.where(idx % 7 == 5, 1e-6, 1.0)).to(torch.float32)
    big = {}
    for k in ("P", "Q"):
        big[k] = (torch.rand(b, n, 3, device=dev, generator=gen) - 0.5) * scale[:, None, None]
    big["Rgt"] = torch.randn(b, 3, 3, device=dev, generator=gen)
    for k in ("Tgt", "Tpred"):
        big[k] = torch.randn(b, 4, 4, device=dev, generator=gen) * scale[:, None, None]
    for k in big:
        big[k][pos] = small[k]
    return big


def _family_outputs(abi, t, index=None):
    """Every output of the family whose sum order depends on (N, lane) alone, as host arrays (rows `index` of the batch)."""
    got = {}
    R, H = abi.kabsch(t["P"], t["Q"])
    got["kabsch R"], got["kabsch H"] = R.get(index), H.get(index)
    R, H = abi.synth(t["P"], t["Rgt"], 0.0, 99)
    got["synth R"], got["synth H"] = R.get(index), H.get(index)
    got["rotated"], got["rotated T"] = abi.rotate(t["P"], t["Rgt"], False).get(index), abi.rotate(t["P"], t["Rgt"], True).get(index)
    out, cen, scl = abi.normalize(t["P"])
    got["normalised"], got["centroid"], got["scale"] = out.get(index), cen.get(index), scl.get(index)
    for kind in ("l1", "dis", "l2"):
        dists, _, dT = abi.add(kind, t["Tgt"], t["Tpred"], t["P"])
        if dists is not None:
            got[kind + " dists"] = dists.get(index)
        got[kind + " dT"] = dT.get(index)
    return got


@pytest.mark.parametrize("n", [65, 513])
def test_a_cloud_does_not_depend_on_where_it_sits(dev, wave_slots, n):
    """40 clouds alone (one per wave), scattered through a batch with five clouds per wave, and through one capped at 64 per wave, among
    neighbours 1e6 times larger and smaller: H, the rotated and the normalised points, centroid, scale and the ADD rows come back with the
    same bits, because a cloud's sum order depends on (N, lane) alone.
    R is held to the bound of the module docstring instead, against float64 and between the runs: so3::project_rotation takes wave-level
    decisions -- the prescale of rows outside the scale window, the refinement loop and the Jacobi path each run under a wave-uniform
    branch that any row of the wave can ask for (the 1e6 neighbours' H, ~1e12 N, is outside the window) -- and although each is written to
    leave the other rows' bits alone, that is its own property, which test_a_row_does_not_depend_on_its_neighbours pins for K1."""
    w = wave_slots
    data = make_batch(40, n, 31 + n)
    small = {k: to_device(v, dev) for k, v in data.items()}
    abi = Abi(dev)
    alone = _family_outputs(abi, small)
    h_ref = _so().cross_covariance_np(data["P"], data["Q"])
    r_ref, rb, judged = r_reference(h_ref, h_bound(data["P"], data["Q"]))
    assert judged.all()
    assert (np.abs(alone["kabsch R"] - r_ref).max(axis=(1, 2)) <= rb).all()
    for b in (5 * w + 3, 64 * w + 37):
        rng = np.random.default_rng(b)
        pos = np.sort(rng.choice(b, 40, replace=False))
        pos[0], pos[-1] = 0, b - 1                                           # the first wave's first slot and the ragged last wave's last
        assert len(set(pos % per_wave(b, w))) > 3
        pos_t = torch.from_numpy(pos).to(dev)
        big = _embed(dev, small, b, pos_t, b)
        there = _family_outputs(abi, big, pos_t)
        del big
        for key, v in alone.items():
            if key.endswith(" R"):
                same = np.array_equal(v, there[key])
                print("N %d B %d %s bit-identical: %s" % (n, b, key, same))
                if key == "kabsch R":
                    assert (np.abs(there[key] - r_ref).max(axis=(1, 2)) <= rb).all(), (b, key)
                assert (np.abs(there[key] - v).max(axis=(1, 2)) <= rb).all(), (b, key)
            else:
                assert np.array_equal(v.view(np.int32), there[key].view(np.int32)), (b, key)
    torch.cuda.synchronize()


# ---- 4. data the suite never fed these kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [10.0, 1000.0])
def test_off_centre_clouds(dev, offset):
    """P and Q both `offset` away from the origin on every axis: nothing is centred (nor is the reference), so H is N c c^T plus a
    small part -- within the dot product's bound all the same, and R a rotation.  The rotated points stay within 2e-6 max(1, |reference|);
    the normalised ones carry the float32 centre's rounding on top of theirs (check_normalized)."""
    abi = Abi(dev, guarded=True)
    for b, n in ((5, 65), (67, 513), (3, 1025)):
        data = make_batch(b, n, int(offset) + n, offset=offset)
        P, Q, Rgt = (to_device(data[k], dev) for k in ("P", "Q", "Rgt"))
        R, H = abi.kabsch(P, Q)
        h, r = H.get(), R.get()
        bound = h_bound(data["P"], data["Q"])
        err = np.abs(h - _so().cross_covariance_np(data["P"], data["Q"]))
        print("offset %g B %d N %d H err/bound %.3f" % (offset, b, n, np.max(err / bound)))
        assert (err <= bound).all(), (offset, b, n, np.max(err / bound))
        check_rotation(r, "offset %g" % offset)
        check_rotated(abi.rotate(P, Rgt, False).get(), abi.rotate(P, Rgt, True).get(), data["P"], data["Rgt"], "offset %g rotate" % offset)
        out, cen, scl = abi.normalize(P)
        check_normalized(out.get(), cen.get(), scl.get(), data["P"], "offset %g normalize" % offset, centre_rounding=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 65, 129, 513, 1025])
def test_add_with_a_translation_far_larger_than_the_cloud(dev, n):
    """Translations 1e3 apart per axis, clouds of extent 0.05: every zero-filled slot of ADD-L1 adds |dt| ~ 3e3 and a sign, which npad takes
    back out in float32 -- at these N every lane carries such slots under each unroll.  Fails if npad counts anything but slots - valid."""
    abi = Abi(dev, guarded=True)
    for b in (5, 67):
        data = make_batch(b, n, 5 * n + b, extent=0.05, dt_shift=1e3)
        Tgt, Tpred, P = (to_device(data[k], dev) for k in ("Tgt", "Tpred", "P"))
        for kind in ("l1", "dis", "l2"):
            dists, loss, dT = abi.add(kind, Tgt, Tpred, P)
            worst = check_add(kind, None if dists is None else dists.get(), loss, dT.get(), data["Tgt"], data["Tpred"], data["P"], "far %s N %d B %d" % (kind, n, b))
            print("far translation %s N %d B %d per-sample gradient err/bound %.3f" % (kind, n, b, worst))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 2, 300, 2000])
def test_constant_clouds_normalise_as_numpy_does(dev, n):
    """All points equal: the centroid is the point exactly, the scale exactly 0, the normalised points NaN (numpy's 0 / 0).  Fails if a
    zero-filled slot enters the box (the `in ?` masks): none of these points is the origin."""
    pts = np.array([[0.25, -3.0, 7.5], [1000.0, 1000.0, 1000.0], [-1e-3, 2e10, -5.0], [1.0, 1.0, 1.0], [-0.7, 0.3, 123.456]], np.float32)
    P = np.ascontiguousarray(np.broadcast_to(pts[:, None, :], (5, n, 3)))
    with np.errstate(invalid="ignore", divide="ignore"):
        rn, rc, rs = _so().pc_normalize_np(P)
    assert np.isnan(rn).all() and (rs == 0).all() and np.array_equal(rc, pts.astype(np.float64))
    out, cen, scl = Abi(dev, guarded=True).normalize(to_device(P, dev))
    assert np.array_equal(cen.get(), pts) and (scl.get() == 0).all() and np.isnan(out.get()).all()


def test_non_finite_points_stay_in_their_cloud_and_propagate_as_in_numpy(dev, wave_slots):
    """Five clouds per wave; one cloud has a NaN point, one a point whose x alone is NaN, one a +inf point (all in P).  Every other cloud
    comes back with the bits of the same batch without them.  The three give what the float64 formula gives: H is NaN (inf) in the
    columns the point's coordinates make so, the rotated point alone is non-finite, ADD's distance is non-finite, and pc_normalize
    returns what numpy's max / min make of it -- a NaN reaches the box, so the NaN point's cloud, centroid and scale are all NaN (before
    this test fmaxf / fminf dropped it and the cloud came back finite apart from that point).  R of a non-finite H is NaN (DESIGN.md,
    "Documented divergences": the reference's LAPACK raises)."""
    so, w, n = _so(), wave_slots, 65
    b = 5 * w + 3
    assert per_wave(b, w) == 5
    data = make_batch(b, n, 77)
    bad = {"nan": 5 * 1000 + 2, "nan x": 5 * 2000 + 4, "inf": 5 * 3000 + 0}
    dirty = data["P"].copy()
    dirty[bad["nan"], 17, :] = np.nan
    dirty[bad["nan x"], 64, 0] = np.nan
    dirty[bad["inf"], 3, :] = np.inf
    rows = np.array(sorted(bad.values()))
    others = np.ones(b, bool)
    others[rows] = False
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):          # the reference semantics first, on the host alone
        rn, rc, rs = so.pc_normalize_np(dirty[rows].astype(np.float64))
        order = {k: int(np.searchsorted(rows, v)) for k, v in bad.items()}
        assert np.isnan(rn[order["nan"]]).all() and np.isnan(rc[order["nan"]]).all() and np.isnan(rs[order["nan"]])
        assert np.isnan(rn).all() and np.isnan(rs).all()
        h_ref = so.cross_covariance_np(dirty[rows], data["Q"][rows])
        rot_ref = so.rotate_clouds_np(dirty[rows], data["Rgt"][rows])
        d, _, _ = add_terms(data["Tgt"][rows], data["Tpred"][rows], dirty[rows], False)
        l1_ref, l2_ref = np.abs(d).mean((1, 2)), np.linalg.norm(d, axis=-1).mean(1)
    abi = Abi(dev)
    dev_in = {k: to_device(v, dev) for k, v in data.items()}
    clean = _family_outputs(abi, dev_in)
    dev_in["P"] = to_device(dirty, dev)
    got = _family_outputs(abi, dev_in)
    for key, v in clean.items():
        if key.startswith("synth"):
            continue                                             # (sigma = 0: nothing of it is specific to a non-finite point)
        assert np.array_equal(v[others].view(np.int32), got[key][others].view(np.int32)), key

    def same_kind(x, ref, what, tol):
        assert np.array_equal(np.isnan(x), np.isnan(ref)), what
        assert np.array_equal(np.isposinf(x), np.isposinf(ref)) and np.array_equal(np.isneginf(x), np.isneginf(ref)), what
        ok = np.isfinite(ref)
        assert (np.abs(x - ref)[ok] <= tol[ok]).all(), what

    clean_bound = h_bound(data["P"][rows], data["Q"][rows])
    same_kind(got["kabsch H"][rows], h_ref, "H", clean_bound)
    assert np.isnan(h_ref[order["nan"]]).all() and np.isnan(h_ref[order["nan x"]][:, 0]).all() and np.isfinite(h_ref[order["nan x"]][:, 1:]).all()
    assert np.isnan(got["kabsch R"][rows]).all()
    same_kind(got["rotated"][rows], rot_ref, "rotated", np.full(rot_ref.shape, 2e-6))
    same_kind(got["rotated T"][rows], rot_ref.transpose(0, 2, 1), "rotated T", np.full((3, 3, n), 2e-6))
    same_kind(got["normalised"][rows], rn, "normalised", np.zeros(rn.shape))
    same_kind(got["scale"][rows], rs, "scale", np.zeros(rs.shape))
    same_kind(got["centroid"][rows], rc, "centroid", 1e-6 * np.maximum(1.0, np.abs(np.nan_to_num(rc, posinf=0.0))))
    same_kind(got["l1 dists"][rows], l1_ref, "ADD-L1 dists", np.zeros(3))
    same_kind(got["l2 dists"][rows], l2_ref, "ADD dists", np.zeros(3))
    assert not np.isfinite(l1_ref).any() and not np.isfinite(l2_ref).any()
