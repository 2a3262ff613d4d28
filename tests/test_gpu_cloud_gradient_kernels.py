"""The cloud gradient kernels and rigid_align through the raw C ABI, against float64, on every launch geometry and at their edges:
    so3_kabsch_bwd_f32         k_kabsch_bwd<DP, DQ>                3 instantiations
    so3_rotate_clouds_bwd_f32  k_rotate_clouds_bwd<T, DP, DR>      6
    so3_rigid_align_f32        k_rigid_align<WEIGHTED>             2
    so3_rigid_align_bwd_f32    k_rigid_align_bwd<DP, DQ, DW>       7
They share k_kabsch's skeleton (tests/test_gpu_cloud_kernels.py, whose helpers this file imports): clamp(B / (16 CUs), 1, 64) clouds
per wave, lane j keeping the wave's j-th cloud, a per-cloud buffer descriptor standing in for the point tail, 64 x 8 points per trip.
The backward kernels also STORE through those descriptors (dP, dQ as b96, dw as b32) and broadcast a cloud's constants with
readlane(j).  so3_last_kernel() does not name the instantiation for these launchers, so nothing here relies on it: an instantiation
is reached through the null pattern of the output pointers, the weights and the layout flag.

  1. every clouds-per-wave value with a ragged last wave, at N in {1, 3, 7};
  2. both sides of every points-per-cloud boundary, every instantiation, inputs and outputs at 4-byte (not 16-byte) aligned
     addresses, every output between canaries;
  3. impulses: one non-zero point pins the tail and the second trip without a tolerance;
  4. a cloud's answer does not depend on the lane slot and the wave it lands in;
  5. B = 0 and N = 0, a masked head, NaN and inf, clouds 1000 off centre.

Every point of every cloud is judged: no quantile, no sample.  The inputs, the float64 references, the figures and their bounds are
tests/cloud_gradients_ref.py's (its docstring states each bound); the limits are tests/test_cloud_gradient_kernels_host.py's, where
the float32 restatements pass the same checkers on the CPU and the measured ones are 4 x what those reach.

WHAT THESE TESTS CATCH.  Each of these mistakes, applied to the float32 restatement's output, exceeds its bound in the checker
(tests/test_cloud_gradient_kernels_host.py::test_seeded_wrong_answers_fail; the worst figure over the bound at N = 3 / 65 / 513, the
least sensitive of the outputs it reaches):
    cloud j takes cloud j + 1's dH (kabsch)                  4.9e7 / 6.2e7 / 4.3e7
    cloud j takes cloud j + 1's constants (rigid)            4.0e7 / 6.9e7 / 4.0e7
    the last point is left out of dR                         2.4e5 at N = 65, 1.3e4 at 513, 539 at 3001
    dP is computed with dH instead of dH^T                   3.5e5 / 4.5e5 / 5.1e5 (kabsch), 2.8e5 / 4.4e5 / 5.0e5 (rigid)
    the transposed G is read as (B, N, 3)                    6.7e7 / 3.5e8 / 4.4e8
    the (w_i / W) g_t term is dropped from dQ                2.5e5 / 7.8e4 / 4.5e4
    u = R g_t is used instead of R^T g_t                     2.6e5 / 5.2e4 / 3.9e4
    the -g_t pbar^T term is dropped from gR'                 6.0e4 / 1.7e4 / 7.5e3
    the 1 / W terms are dropped from dw                      2.1e4 / 6.8e3 / 3.1e4
    the centroid of the previous cloud is used               1.4e6 / 4.5e5 / 2.0e5
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import cloud_gradients_ref as cg
from support import dev, ptr  # noqa: F401
import test_cloud_gradient_kernels_host as hostk
import test_rigid_align_host as host
from test_gpu_cloud_kernels import CANARY, GEOMETRIES, PAD, Out, _rotations, h_bound, make_batch, per_wave, r_reference, wave_slots      # noqa: F401

pytestmark = pytest.mark.gpu

ROT_SIDES = (("dP", "dR"), ("dP",), ("dR",))
KABSCH_SIDES = (("dP", "dQ"), ("dP",), ("dQ",))
LARGE = 100000
RIGID_SIDES = tuple(s for r in (3, 2, 1) for s in itertools.combinations(("dP", "dQ", "dw"), r))


def _optr(o):
    return None if o is None else o.ptr


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class GradAbi:
    """The four entry points over device tensors.  Every output is an Out; `want` names the outputs that get a pointer, the others
    are passed as null; an upstream gradient or the weights given as None are passed as null.  guarded: outputs between canaries
    and inputs (put) one float past an allocation's start, so that both sit at 4-byte, not 16-byte aligned addresses."""

    def __init__(self, dev, guarded=False):
        from poseestimation_amd import _lib
        self._lib, self.lib, self.dev, self.guarded = _lib, _lib.load(), dev, guarded

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _out(self, *shape):
        return Out(self.dev, shape, self.guarded)

    def put(self, a):
        if a is None:
            return None
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        if not self.guarded:
            return a.to(self.dev)
        buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=self.dev)
        t = buf[1:].view(a.shape)
        t.copy_(a)
        assert t.data_ptr() % 16 == 4
        return t

    def put_all(self, d):
        return {k: self.put(v) for k, v in d.items()}

    def rotate_bwd(self, P, R, G, transposed, want=("dP", "dR")):
        b, n = P.shape[:2]
        o = {"dP": self._out(b, n, 3) if "dP" in want else None, "dR": self._out(b, 3, 3) if "dR" in want else None}
        self._lib.check(self.lib.so3_rotate_clouds_bwd_f32(ptr(P), ptr(R), ptr(G), _optr(o["dP"]), _optr(o["dR"]), int(transposed), b, n,
                                                           self._st()), "so3_rotate_clouds_bwd_f32")
        return o

    def kabsch_bwd(self, P, Q, H, gR, gH, want=("dP", "dQ")):
        b, n = P.shape[:2]
        o = {k: self._out(b, n, 3) if k in want else None for k in ("dP", "dQ")}
        self._lib.check(self.lib.so3_kabsch_bwd_f32(ptr(P), ptr(Q), ptr(H), ptr(gR), ptr(gH), _optr(o["dP"]), _optr(o["dQ"]), b, n, self._st()),
                        "so3_kabsch_bwd_f32")
        return o

    def rigid(self, P, Q, w, want=("H", "stats")):
        b, n = P.shape[:2]
        o = {"R": self._out(b, 3, 3), "t": self._out(b, 3), "H": self._out(b, 3, 3) if "H" in want else None,
             "stats": self._out(b, 7) if "stats" in want else None}
        self._lib.check(self.lib.so3_rigid_align_f32(ptr(P), ptr(Q), ptr(w), o["R"].ptr, o["t"].ptr, _optr(o["H"]), _optr(o["stats"]), b, n, self._st()),
                        "so3_rigid_align_f32")
        return o

    def rigid_bwd(self, P, Q, w, H, R, stats, gR, gt, gH, want=("dP", "dQ", "dw")):
        b, n = P.shape[:2]
        o = {"dP": self._out(b, n, 3) if "dP" in want else None, "dQ": self._out(b, n, 3) if "dQ" in want else None,
             "dw": self._out(b, n) if "dw" in want else None}
        self._lib.check(self.lib.so3_rigid_align_bwd_f32(ptr(P), ptr(Q), ptr(w), ptr(H), ptr(R), ptr(stats), ptr(gR), ptr(gt), ptr(gH),
                                                         _optr(o["dP"]), _optr(o["dQ"]), _optr(o["dw"]), b, n, self._st()), "so3_rigid_align_bwd_f32")
        return o


def fetch(outs, index=None):
    """The outputs that were asked for, on the host, after Out.get's check that every slot was written and no canary was."""
    return {k: o.get(index) for k, o in outs.items() if o is not None}


@functools.lru_cache(maxsize=2)
def inputs(b, n, seed, offset=0.0):
    """cloud_gradients_ref.bwd_inputs, kept for the entry points that share a batch.  Never changed by a test."""
    return cg.bwd_inputs(b, n, seed, offset)


def one_sided_equal_full(run, sides, full, label):
    """Every instantiation but the full one: what it writes has the bits of the full one's output."""
    for want in sides[1:]:
        got = fetch(run(want))
        assert set(got) == set(want), (label, want)
        for k in want:
            assert same_bits(got[k], full[k]), (label, "one-sided", want, k)


# ---- one entry point on one batch ---------------------------------------------------------------------------------------------------
def run_rotate(abi, d, label, sides=False):
    lim = hostk.limits()
    D = abi.put_all({k: d[k] for k in ("P", "R", "G", "GT")})
    r = cg.rotate_bwd_ref(d["P"], d["R"], d["G"])
    for transposed, g in ((False, D["G"]), (True, D["GT"])):
        full = fetch(abi.rotate_bwd(D["P"], D["R"], g, transposed))
        hostk.hold(cg.check_rotate_bwd(full, r), lim, "%s rotate_bwd transposed %d" % (label, transposed))
        if sides:
            one_sided_equal_full(lambda want: abi.rotate_bwd(D["P"], D["R"], g, transposed, want), ROT_SIDES, full, label)
    torch.cuda.synchronize()


def run_kabsch(abi, d, label, sides=False, upstreams=False):
    """sides: every one-sided instantiation; upstreams: every single-null upstream (gR null is held to the derived bound, a null one
    equals a zero one as values) and both null (every output zero)."""
    lim = hostk.limits()
    D = abi.put_all({k: d[k] for k in ("P", "Q", "H", "gR", "gH")})
    r = cg.kabsch_bwd_ref(d["P"], d["Q"], d["H"], d["gR"], d["gH"])
    full = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], D["gR"], D["gH"]))
    hostk.hold(cg.check_kabsch_bwd(full, r), lim, label + " kabsch_bwd")
    if sides:
        one_sided_equal_full(lambda want: abi.kabsch_bwd(D["P"], D["Q"], D["H"], D["gR"], D["gH"], want), KABSCH_SIDES, full, label)
    if upstreams:
        zero = abi.put(np.zeros_like(d["gR"]))
        for g_r, g_h, names in ((None, D["gH"], (None, "gH")), (D["gR"], None, ("gR", None))):
            null = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], g_r, g_h))
            as_zero = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], zero if g_r is None else g_r, zero if g_h is None else g_h))
            rr = cg.kabsch_bwd_ref(d["P"], d["Q"], d["H"], *(None if k is None else d[k] for k in names))
            hostk.hold(cg.check_kabsch_bwd(null, rr), lim, "%s kabsch_bwd upstreams %s" % (label, names))
            assert all(np.array_equal(null[k], as_zero[k]) for k in null), (label, names)          # (K2 of a zero gR is a zero)
            if sides:
                one_sided_equal_full(lambda want: abi.kabsch_bwd(D["P"], D["Q"], D["H"], g_r, g_h, want), KABSCH_SIDES, null, label)
        none = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], None, None))
        assert all((v == 0).all() for v in none.values()), (label, "both upstreams null")
    torch.cuda.synchronize()


def run_rigid_bwd(abi, d, label, sides=False, upstreams=False, weights=(False, True)):
    """A batch too large for a handful of float64 K2 references (LARGE) holds a run with a null upstream to the run with a zero one
    alone, which is held to float64 as the full run is: the same instantiation on the same path."""
    lim = hostk.limits()
    D = abi.put_all({k: d[k] for k in ("P", "Q", "w", "H", "R", "stats", "stats_w", "gR", "gt", "gH")})
    for weighted in weights:
        w, st, dw_, dst = (d["w"], d["stats_w"], D["w"], D["stats_w"]) if weighted else (None, d["stats"], None, D["stats"])
        tag = "%s rigid_align_bwd %s" % (label, "weighted" if weighted else "unweighted")
        r = cg.rigid_bwd_ref(d["P"], d["Q"], w, d["H"], d["R"], st, d["gR"], d["gt"], d["gH"])
        call = lambda g3, want=("dP", "dQ", "dw"): abi.rigid_bwd(D["P"], D["Q"], dw_, D["H"], D["R"], dst, *g3, want)          # noqa: E731
        full = fetch(call((D["gR"], D["gt"], D["gH"])))
        hostk.hold(cg.check_rigid_bwd(full, r), lim, tag)
        if sides:
            one_sided_equal_full(lambda want: call((D["gR"], D["gt"], D["gH"]), want), RIGID_SIDES, full, tag)
        if upstreams and weighted:
            for drop in range(3):
                names = [None if i == drop else k for i, k in enumerate(("gR", "gt", "gH"))]
                null = fetch(call([None if k is None else D[k] for k in names]))
                zeros = [abi.put(np.zeros_like(d[k])) if names[i] is None else D[k] for i, k in enumerate(("gR", "gt", "gH"))]
                as_zero = fetch(call(zeros))
                if len(d["P"]) <= LARGE:
                    rr = cg.rigid_bwd_ref(d["P"], d["Q"], w, d["H"], d["R"], st, *(None if k is None else d[k] for k in names))
                    hostk.hold(cg.check_rigid_bwd(null, rr), lim, "%s upstreams %s" % (tag, names))
                assert all(np.array_equal(null[k], as_zero[k]) for k in null), (tag, names)
            only_h = fetch(call((None, None, D["gH"])))                                  # the path without K2
            hostk.hold(cg.check_rigid_bwd(only_h, cg.rigid_bwd_ref(d["P"], d["Q"], w, d["H"], d["R"], st, None, None, d["gH"])), lim, tag + " gH alone")
            if sides:
                one_sided_equal_full(lambda want: call((None, None, D["gH"]), want), RIGID_SIDES, only_h, tag)
            none = fetch(call((None, None, None)))
            assert all((v == 0).all() for v in none.values()), (tag, "every upstream null")
    torch.cuda.synchronize()


def run_rigid_fwd(abi, b, n, seed, label, offsets=(0.0,)):
    """Real clouds, weights null and U[0.05, 1]: every cloud's H, centroids, W, pose identity and R (cloud_gradients_ref.check_rigid_fwd);
    the share of clouds whose R is left to the properties is capped (forward_limits)."""
    for offset in offsets:
        f = make_batch(b, n, seed, offset=offset)
        w = np.ascontiguousarray(np.random.default_rng(seed + 1).uniform(0.05, 1.0, (b, n)), dtype=np.float32)
        P, Q = abi.put(f["P"]), abi.put(f["Q"])
        for ww in (None, w):
            got = fetch(abi.rigid(P, Q, abi.put(ww)))
            bare = fetch(abi.rigid(P, Q, abi.put(ww), want=()))                          # H and stats are optional outputs
            assert set(bare) == {"R", "t"} and all(same_bits(bare[k], got[k]) for k in bare), (label, "without H and stats")
            fig = cg.check_rigid_fwd(got, f["P"], f["Q"], ww, hostk.FWD_TOL)
            hostk.hold(fig, hostk.forward_limits(n, b), "%s rigid_align offset %g %s" % (label, offset, "weighted" if ww is not None else "unweighted"))
    torch.cuda.synchronize()


ENTRIES = ("rotate_bwd", "kabsch_bwd", "rigid_align", "rigid_align_bwd")


def run_entry(entry, abi, b, n, seed, label, every=False):
    """One entry point on the batch (b, n, seed); every: each instantiation and each null pattern of the upstream gradients too."""
    label = "%s B %d N %d" % (label, b, n)
    if entry == "rigid_align":
        return run_rigid_fwd(abi, b, n, seed, label, offsets=(0.0, 10.0) if every else (0.0,))
    d = inputs(b, n, seed)
    if entry == "rotate_bwd":
        run_rotate(abi, d, label, sides=every)
    elif entry == "kabsch_bwd":
        run_kabsch(abi, d, label, sides=every, upstreams=every)
    else:
        run_rigid_bwd(abi, d, label, sides=every, upstreams=every, weights=(False, True) if every or b <= LARGE else (True,))


# ---- 1. every clouds-per-wave geometry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("k,last,n", GEOMETRIES, ids=lambda v: str(v))
def test_every_clouds_per_wave_geometry(dev, wave_slots, k, last, n, entry):          # noqa: F811
    """B = k W + r clouds: k clouds per wave (64 at most) and a last wave of `last` clouds; all gradients, all upstreams, every point
    of every cloud against float64.  Two geometries also run every one-sided instantiation and every null upstream.
    Fails on a readlane(j + 1), a wrong first cloud in interior waves, a wrong lane slot, a cloud count off by one in the last wave."""
    w = wave_slots
    pw = min(k, 64)
    b = 70 * w + 1 if k == 70 else k * w + last
    assert per_wave(b, w) == pw and (k == 70 or (b - 1) % pw + 1 == last)
    run_entry(entry, GradAbi(dev), b, n, 1000 * k + last, "per_wave %d last %d" % (pw, last), every=(k, last, n) in ((3, 2, 3), (64, 31, 7)))


# ---- 2. both sides of every points-per-cloud boundary -----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", cg.POINTS)
def test_both_sides_of_every_points_per_cloud_boundary(dev, n, entry):
    """B in {1, 5, 67} around the trip length 64 x 8 = 512 and its lane rows of 64, and beyond where the loops take a second, third
    and sixth trip.  Every instantiation; inputs and outputs at 4-byte, not 16-byte aligned addresses; every output between canaries,
    every slot written, no canary touched (Out.get).  Fails on an unwritten last row of dQ or a dropped 513th point of dR."""
    abi = GradAbi(dev, guarded=True)
    for b in (1, 5, 67):
        run_entry(entry, abi, b, n, 7 * n + b, "boundary", every=True)


# ---- 3. impulses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 513, 3001])
def test_impulses(dev, n):
    """Eight clouds whose G (or gH's factors P and Q) are zero except at one point, i in {0, 63, 64, N - 1}, two clouds each: dR is
    fl(g_i p_i^T) exactly, since every other addend is an exact zero, and every other point's row of dP, dQ and dw is exactly zero (a
    figure's bound is zero there, so the checkers demand it; it is asserted on its own as well)."""
    abi, lim = GradAbi(dev, guarded=True), hostk.limits()
    b = 8
    where = np.array([0, 63, 64, n - 1] * 2)
    hot = np.zeros((b, n, 1), np.float32)
    hot[np.arange(b), where] = 1.0
    src = inputs(b, n, 900 + n)
    d = dict(src, G=src["G"] * hot, P0=src["P"] * hot, Q0=src["Q"] * hot)
    d["GT"] = np.ascontiguousarray(d["G"].transpose(0, 2, 1))
    d["stats0"] = np.concatenate([np.zeros((b, 6), np.float32), np.full((b, 1), n, np.float32)], 1)          # pbar = qbar = 0: a_i = p_i
    D = abi.put_all({k: d[k] for k in ("P", "R", "G", "GT", "P0", "Q0", "H", "gH", "stats0")})
    cold = hot[..., 0] == 0
    want_dr = d["G"][np.arange(b), where][:, :, None] * d["P"][np.arange(b), where][:, None, :]              # one float32 product per entry
    r = cg.rotate_bwd_ref(d["P"], d["R"], d["G"])
    for transposed, g in ((False, D["G"]), (True, D["GT"])):
        got = fetch(abi.rotate_bwd(D["P"], D["R"], g, transposed))
        hostk.hold(cg.check_rotate_bwd(got, r), lim, "impulse N %d rotate_bwd transposed %d" % (n, transposed))
        assert np.array_equal(got["dR"], want_dr), (n, transposed, "dR is not the one product")
        assert (got["dP"][cold] == 0).all() and (got["dP"][~cold] != 0).any()
    got = fetch(abi.kabsch_bwd(D["P0"], D["Q0"], D["H"], None, D["gH"]))
    hostk.hold(cg.check_kabsch_bwd(got, cg.kabsch_bwd_ref(d["P0"], d["Q0"], d["H"], None, d["gH"])), lim, "impulse N %d kabsch_bwd" % n)
    assert all((got[k][cold] == 0).all() and (got[k][~cold] != 0).all() for k in ("dP", "dQ"))
    got = fetch(abi.rigid_bwd(D["P0"], D["Q0"], None, D["H"], D["R"], D["stats0"], None, None, D["gH"]))
    rr = cg.rigid_bwd_ref(d["P0"], d["Q0"], None, d["H"], d["R"], d["stats0"], None, None, d["gH"])
    hostk.hold(cg.check_rigid_bwd(got, rr), lim, "impulse N %d rigid_align_bwd" % n)
    assert all((got[k][cold] == 0).all() and (got[k][~cold] != 0).any() for k in ("dP", "dQ", "dw"))
    torch.cuda.synchronize()


# ---- 4. a cloud does not depend on where it sits ---------------------------------------------------------------------------------------------
PER_POINT = ("P", "Q", "G")


def _embed(dev, small, b, pos, seed):
    """Device batches of b clouds: random filler (every seventh cloud scaled by 1e6, another seventh by 1e-6; weights in [0.05, 1], W > 0)
    with the 40 clouds of `small` at the positions `pos`."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.arange(b, device=dev)
    scale = torch.where(idx % 7 == 3, 1e6, torch.where(idx % 7 == 5, 1e-6, 1.0)).to(torch.float32)
    big = {}
    for k, v in small.items():
        shape = (b,) + tuple(v.shape[1:])
        if k == "w":
            big[k] = torch.rand(shape, device=dev, generator=gen) * 0.95 + 0.05
        else:
            big[k] = torch.randn(shape, device=dev, generator=gen) * scale.view((b,) + (1,) * (len(shape) - 1))
        if k.startswith("stats"):
            big[k][:, 6] = torch.rand(b, device=dev, generator=gen) * v.shape[1] + 0.5
        big[k][pos] = v
    return big


def _family_outputs(abi, t, index=None):
    """Every output of the four entry points, as host arrays (rows `index` of the batch).  Keys ending in "~" have K2 on their path."""
    got = {}
    for transposed, g in ((False, t["G"]), (True, t["GT"])):
        for k, v in fetch(abi.rotate_bwd(t["P"], t["R"], g, transposed), index).items():
            got["rotate%d %s" % (transposed, k)] = v
    for k, v in fetch(abi.kabsch_bwd(t["P"], t["Q"], t["H"], None, t["gH"]), index).items():
        got["kabsch gH " + k] = v
    for k, v in fetch(abi.kabsch_bwd(t["P"], t["Q"], t["H"], t["gR"], t["gH"]), index).items():
        got["kabsch %s~" % k] = v
    for name, w, st in (("unweighted", None, t["stats"]), ("weighted", t["w"], t["stats_w"])):
        for k, v in fetch(abi.rigid(t["P"], t["Q"], w), index).items():
            got["forward %s %s%s" % (name, k, "~" if k in ("R", "t") else "")] = v
        for k, v in fetch(abi.rigid_bwd(t["P"], t["Q"], w, t["H"], t["R"], st, None, None, t["gH"]), index).items():
            got["rigid %s gH %s" % (name, k)] = v
        for k, v in fetch(abi.rigid_bwd(t["P"], t["Q"], w, t["H"], t["R"], st, t["gR"], t["gt"], t["gH"]), index).items():
            got["rigid %s %s~" % (name, k)] = v
    return got


def _k2_judges(d):
    """For every "~" key of _family_outputs: (float64 answer, per-row denominator or None, limit)."""
    lim, out = hostk.limits(), {}
    r = cg.kabsch_bwd_ref(d["P"], d["Q"], d["H"], d["gR"], d["gH"])
    for k in ("dP", "dQ"):
        out["kabsch %s~" % k] = (r[k], r[k + "_D"], lim["kb_" + k])
    for name, w, st in (("unweighted", None, d["stats"]), ("weighted", d["w"], d["stats_w"])):
        r = cg.rigid_bwd_ref(d["P"], d["Q"], w, d["H"], d["R"], st, d["gR"], d["gt"], d["gH"])
        for k in ("dP", "dQ", "dw"):
            out["rigid %s %s~" % (name, k)] = (r[k], r[k + "_D"], lim["ra_" + k])
    return out


@pytest.mark.parametrize("n,k,last", [(65, 5, 3), (513, 5, 3), (65, 64, 37)])
def test_a_cloud_does_not_depend_on_where_it_sits(dev, wave_slots, n, k, last):          # noqa: F811
    """40 clouds alone (one per wave) and the same clouds scattered, first slot and last slot included, through a batch of k W + last
    clouds whose other clouds are 1e6 times larger and smaller.  dR, the forward's H and stats and every per-point gradient on the path
    without K2 (gR and g_t null) come back with the same bits, because a cloud's sum order depends on (N, lane) alone.  With K2 on the
    path (and for the forward's R and t, behind the projection) the results are held to their bounds against float64 and between the
    two runs, and whether they were bit-identical is printed: the projection and its backward take wave-level decisions that any row
    of the wave can ask for."""
    w = wave_slots
    b = k * w + last
    assert per_wave(b, w) == k
    d = inputs(40, n, 31 + n)
    abi = GradAbi(dev)
    small = abi.put_all(d)
    alone = _family_outputs(abi, small)
    judges = _k2_judges(d)
    fwd = {name: cg.ref.answers(d["P"], d["Q"], ww) for name, ww in (("unweighted", None), ("weighted", d["w"]))}
    rb = {}
    for name, want in fwd.items():
        hden = np.maximum(np.abs(want["H"]).reshape(40, -1).max(1), 1e-3 * want["stats"][:, 6])
        r_ref, bound, judged = r_reference(want["H"], host.H_TOL * hden[:, None, None] * np.ones((1, 3, 3)))
        assert judged.all()
        rb[name] = (r_ref, bound)
    rng = np.random.default_rng(b)
    pos = np.sort(rng.choice(b, 40, replace=False))
    pos[0], pos[-1] = 0, b - 1                                           # the first wave's first slot and the ragged last wave's last
    assert len(set(pos % k)) > 3
    pos_t = torch.from_numpy(pos).to(dev)
    big = _embed(dev, small, b, pos_t, b)
    there = _family_outputs(abi, big, pos_t)
    del big
    for key, v in alone.items():
        if not key.endswith("~"):
            assert same_bits(v, there[key]), (b, key)
            continue
        print("N %d B %d %-28s bit-identical: %s" % (n, b, key, same_bits(v, there[key])))
        if key in judges:
            want, D, limit = judges[key]
            for what, got, base in (("alone", v, want), ("scattered", there[key], want), ("between the runs", there[key], v.astype(np.float64))):
                fig = cg.row_figure(got, base, D)
                assert fig <= limit, (b, key, what, fig, limit)
        else:
            name = key.split()[1]
            if key.endswith("R~"):
                r_ref, bound = rb[name]
                for got, base in ((v, r_ref), (there[key], r_ref), (there[key], v)):
                    assert (np.abs(got - base).max(axis=(1, 2)) <= bound).all(), (b, key)
            else:                                                        # t, through the pose identity with the run's own R and stats
                for run in (alone, there):
                    R, st = run["forward %s R~" % name].astype(np.float64), run["forward %s stats" % name].astype(np.float64)
                    miss = np.abs(np.einsum("bij,bj->bi", R, st[:, :3]) + run[key] - st[:, 3:6]).max(1)
                    assert (miss <= host.T_TOL * np.maximum(1.0, np.abs(st[:, :6]).max(1))).all(), (b, key)
    torch.cuda.synchronize()


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------
def test_no_clouds_and_no_points(dev):
    """B = 0 and N = 0 return 0 and write nothing.  Two documented exceptions at N = 0: so3_rotate_clouds_bwd_f32 writes dR = 0 (an
    empty sum), and so3_rigid_align_f32 writes the empty cloud's pose, R = I, t = 0, H = 0, stats = 0."""
    abi = GradAbi(dev, guarded=True)
    lib, st = abi.lib, abi._st()
    b = 5
    x = {k: torch.ones(b, 8, device=dev) for k in "abcdefghi"}
    p = [ptr(v) for v in x.values()]
    for bb, nn in ((0, 4), (b, 0)):
        o = {k: Out(dev, (b, 4, 3), True) for k in ("dP", "dQ", "dw", "R", "t", "H", "stats", "dR")}
        assert lib.so3_kabsch_bwd_f32(p[0], p[1], p[2], p[3], p[4], o["dP"].ptr, o["dQ"].ptr, bb, nn, st) == 0
        assert lib.so3_rigid_align_bwd_f32(*p, o["dP"].ptr, o["dQ"].ptr, o["dw"].ptr, bb, nn, st) == 0
        for transposed in (0, 1):
            assert lib.so3_rotate_clouds_bwd_f32(p[0], p[1], p[2], o["dP"].ptr, o["dR"].ptr, transposed, bb, nn, st) == 0
        assert lib.so3_rigid_align_f32(p[0], p[1], p[2], o["R"].ptr, o["t"].ptr, o["H"].ptr, o["stats"].ptr, bb, nn, st) == 0
        torch.cuda.synchronize()
        assert all(o[k].untouched() for k in ("dP", "dQ", "dw")), (bb, nn)
        assert all(bool((v.buf[:PAD] == CANARY).all().item()) and bool((v.buf[PAD + v.n:] == CANARY).all().item()) for v in o.values())
        if bb == 0:
            assert all(v.untouched() for v in o.values())
        else:
            flat = {k: o[k].buf.view(torch.float32)[PAD:PAD + b * 12].cpu().numpy() for k in ("dR", "R", "t", "H", "stats")}
            assert (flat["dR"][:b * 9] == 0).all() and same_bits(flat["dR"][b * 9:], np.full(b * 3, CANARY, np.int32).view(np.float32))
            assert np.array_equal(flat["R"][:b * 9].reshape(b, 3, 3), np.tile(np.eye(3, dtype=np.float32), (b, 1, 1)))
            assert (flat["t"][:b * 3] == 0).all() and (flat["H"][:b * 9] == 0).all() and (flat["stats"][:b * 7] == 0).all()
            assert same_bits(flat["t"][b * 3:], np.full(b * 9, CANARY, np.int32).view(np.float32))


def test_a_masked_head_equals_the_truncated_cloud(dev):
    """Weight 0 on the first 37 of 200 points, the pivot included, at ordinary coordinates: the forward equals the call on the other
    163 points within 2 x the forward tolerances (each is within one of float64), the masked points' dP and dQ are exactly zero (their
    D_i is zero, so the checker demands it), dw is finite and every gradient is within its bound of float64."""
    abi, lim = GradAbi(dev, guarded=True), hostk.limits()
    b, n, cut = 67, 200, 37
    d = inputs(b, n, 4242)
    w = d["w"].copy()
    w[:, :cut] = 0.0
    P, Q, W = abi.put(d["P"]), abi.put(d["Q"]), abi.put(w)
    masked = abi.rigid(P, Q, W)
    m = fetch(masked)
    t = fetch(abi.rigid(abi.put(d["P"][:, cut:]), abi.put(d["Q"][:, cut:]), abi.put(w[:, cut:])))
    hostk.hold(cg.check_rigid_fwd(m, d["P"], d["Q"], w, hostk.FWD_TOL), hostk.forward_limits(n, b), "masked head, forward")
    scale = np.maximum(1.0, np.abs(t["stats"][:, :6]).max(1))
    hden = np.maximum(np.abs(t["H"]).reshape(b, -1).max(1), 1e-3 * t["stats"][:, 6])
    assert np.abs(m["R"] - t["R"]).max() <= 2 * host.R_TOL
    assert (np.abs(m["t"] - t["t"]).max(1) <= 2 * host.T_TOL * scale).all() and (np.abs(m["stats"][:, :6] - t["stats"][:, :6]).max(1) <= 2 * host.T_TOL * scale).all()
    assert (np.abs(m["H"] - t["H"]).reshape(b, -1).max(1) <= 2 * host.H_TOL * hden).all()
    assert (np.abs(m["stats"][:, 6] - t["stats"][:, 6]) <= 2 * host.W_TOL * np.maximum(1.0, t["stats"][:, 6])).all()
    g = abi.put_all({k: d[k] for k in ("gR", "gt", "gH")})
    got = fetch(abi.rigid_bwd(P, Q, W, masked["H"].t, masked["R"].t, masked["stats"].t, g["gR"], g["gt"], g["gH"]))
    assert (got["dP"][:, :cut] == 0).all() and (got["dQ"][:, :cut] == 0).all() and np.isfinite(got["dw"]).all()
    r = cg.rigid_bwd_ref(d["P"], d["Q"], w, m["H"], m["R"], m["stats"], d["gR"], d["gt"], d["gH"])
    hostk.hold(cg.check_rigid_bwd(got, r), lim, "masked head, backward")


def _rows_differ_only(clean, dirty, allowed, key):
    """Rows (clouds, or points of clouds) outside the boolean mask `allowed` have the clean run's bits."""
    assert same_bits(clean[~allowed], dirty[~allowed]), key


def test_non_finite_values_stay_where_they_are(dev, wave_slots):          # noqa: F811
    """Five clouds per wave.  One cloud has a NaN coordinate in one point of P and an inf in another, and a NaN in one point of Q.
    so3_kabsch_bwd_f32: only those points' dQ (dP) rows are non-finite; so3_rotate_clouds_bwd_f32: only that cloud's dR;
    so3_rigid_align_f32: only that cloud's H, R, t and stats; so3_rigid_align_bwd_f32 with given H, R, stats: only those points'
    rows.  Every other row has the bits of the clean run.  Then one NaN in one cloud's H: only that cloud's rows are non-finite, the
    others stay within their bounds, and whether they kept their bits is printed (K2 takes wave-level decisions)."""
    w, n = wave_slots, 65
    b = 5 * w + 3
    assert per_wave(b, w) == 5
    d = inputs(b, n, 77)
    c = 5 * 1000 + 2
    dirty_p, dirty_q = d["P"].copy(), d["Q"].copy()
    dirty_p[c, 17, 0], dirty_p[c, 64, 1], dirty_q[c, 5, 2] = np.nan, np.inf, np.nan
    abi, lim = GradAbi(dev), hostk.limits()
    D = abi.put_all(d)
    DP, DQ = abi.put(dirty_p), abi.put(dirty_q)
    cloud = np.zeros(b, bool)
    cloud[c] = True
    p_pts, q_pts = np.zeros((b, n), bool), np.zeros((b, n), bool)
    p_pts[c, [17, 64]], q_pts[c, 5] = True, True

    clean, dirty = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], D["gR"], D["gH"])), fetch(abi.kabsch_bwd(DP, DQ, D["H"], D["gR"], D["gH"]))
    _rows_differ_only(clean["dQ"], dirty["dQ"], p_pts, "kabsch dQ")
    _rows_differ_only(clean["dP"], dirty["dP"], q_pts, "kabsch dP")
    assert not np.isfinite(dirty["dQ"][p_pts]).all(1).any() and not np.isfinite(dirty["dP"][q_pts]).all(1).any()

    for transposed, g in ((False, D["G"]), (True, D["GT"])):
        clean, dirty = fetch(abi.rotate_bwd(D["P"], D["R"], g, transposed)), fetch(abi.rotate_bwd(DP, D["R"], g, transposed))
        assert same_bits(clean["dP"], dirty["dP"])
        _rows_differ_only(clean["dR"], dirty["dR"], cloud, "rotate dR")
        assert not np.isfinite(dirty["dR"][c]).all()

    for ww in (None, D["w"]):
        clean, dirty = fetch(abi.rigid(D["P"], D["Q"], ww)), fetch(abi.rigid(DP, DQ, ww))
        for k in clean:
            _rows_differ_only(clean[k], dirty[k], cloud, "forward " + k)
        assert not np.isfinite(dirty["H"][c]).all() and not np.isfinite(dirty["R"][c]).all() and not np.isfinite(dirty["t"][c]).all()
        st = D["stats"] if ww is None else D["stats_w"]
        args = (ww, D["H"], D["R"], st, D["gR"], D["gt"], D["gH"])
        clean, dirty = fetch(abi.rigid_bwd(D["P"], D["Q"], *args)), fetch(abi.rigid_bwd(DP, DQ, *args))
        _rows_differ_only(clean["dQ"], dirty["dQ"], p_pts, "rigid dQ")
        _rows_differ_only(clean["dP"], dirty["dP"], q_pts, "rigid dP")
        _rows_differ_only(clean["dw"], dirty["dw"], p_pts | q_pts, "rigid dw")
        assert not np.isfinite(dirty["dQ"][p_pts]).all(1).any() and not np.isfinite(dirty["dP"][q_pts]).all(1).any()
        assert not np.isfinite(dirty["dw"][p_pts | q_pts]).any()

    bad_h = d["H"].copy()
    bad_h[c, 1, 2] = np.nan
    BH = abi.put(bad_h)
    others = ~cloud
    clean, dirty = fetch(abi.kabsch_bwd(D["P"], D["Q"], D["H"], D["gR"], D["gH"])), fetch(abi.kabsch_bwd(D["P"], D["Q"], BH, D["gR"], D["gH"]))
    r = cg.kabsch_bwd_ref(d["P"][others], d["Q"][others], d["H"][others], d["gR"][others], d["gH"][others])
    hostk.hold(cg.check_kabsch_bwd({k: v[others] for k, v in dirty.items()}, r), lim, "NaN in a neighbour's H, kabsch_bwd")
    for k in dirty:
        print("NaN in one H: kabsch %s of the other clouds bit-identical: %s" % (k, same_bits(clean[k][others], dirty[k][others])))
        assert not np.isfinite(dirty[k][c]).all(), k
    args = (D["R"], D["stats_w"], D["gR"], D["gt"], D["gH"])
    clean, dirty = fetch(abi.rigid_bwd(D["P"], D["Q"], D["w"], D["H"], *args)), fetch(abi.rigid_bwd(D["P"], D["Q"], D["w"], BH, *args))
    r = cg.rigid_bwd_ref(d["P"][others], d["Q"][others], d["w"][others], d["H"][others], d["R"][others], d["stats_w"][others], d["gR"][others],
                         d["gt"][others], d["gH"][others])
    hostk.hold(cg.check_rigid_bwd({k: v[others] for k, v in dirty.items()}, r), lim, "NaN in a neighbour's H, rigid_align_bwd")
    for k in dirty:
        print("NaN in one H: rigid %s of the other clouds bit-identical: %s" % (k, same_bits(clean[k][others], dirty[k][others])))
        assert not np.isfinite(dirty[k][c]).all(), k


def test_clouds_far_off_centre(dev):
    """P and Q 1000 away from the origin on every axis, so3_kabsch_bwd_f32 and so3_rotate_clouds_bwd_f32: the bounds are unchanged,
    since every one of them scales with the products (|p_i| is ~1700 in D_i and in the sums of absolute values)."""
    abi = GradAbi(dev, guarded=True)
    for b, n in ((5, 65), (67, 513), (3, 1025)):
        d = inputs(b, n, 1000 + n, 1000.0)
        run_rotate(abi, d, "offset 1000 B %d N %d" % (b, n), sides=True)
        run_kabsch(abi, d, "offset 1000 B %d N %d" % (b, n), sides=True, upstreams=True)
