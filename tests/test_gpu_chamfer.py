"""chamfer_distance on the GPU: G27 through the Python surface and through the raw C ABI with the checks and bounds of
tests/test_chamfer_host.py (4 x the float32 host model's figures; see its docstring), batch shapes that force each work-item size of
k_chamfer_fwd against the float64 restatement on the same random input and, in the squared flavour through the C ABI, BIT FOR BIT
against the float32 restatement of the defined order (chamfer_ref.search32, grad32: indices, d^2 and both gradients; G27's cases get
the same equality inside check_against_g27, the 2500-hit chain of the many-to-one family among them), every reduction, the boundary cases, repeatability, replay
from a graph, and the speed condition against the torch spelling."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import chamfer_ref as ref
from support import bits, dev, guarded, guards_intact, lengths_of, ptr, to_device  # noqa: F401
import test_chamfer_host as host

pytestmark = pytest.mark.gpu
KERNELS = []                        # abi_run: the k_chamfer_fwd instantiation of every forward call, in call order
F32_PAIRS = 1 << 25                 # pairs the float32 restatement forms per test case


@pytest.fixture(scope="module")
def g27_cases():
    return ref.cases(ref.g27())


def _ball(rng, *shape):
    d = rng.standard_normal(shape + (3,))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0, 1, shape + (1,)) ** (1 / 3)).astype(np.float32)


def want64(X, Y, xl, yl, squared, dev):
    """chamfer_ref.chamfer64 with the float64 brute force on the GPU, a cloud at a time (small clouds: the whole batch at once)."""
    b, n, m = X.shape[0], X.shape[1], Y.shape[1]
    nl, ml = lengths_of(xl, b, n), lengths_of(yl, b, m)
    x, y = to_device(X, dev).double(), to_device(Y, dev).double()
    out = {"dist_x": np.zeros((b, n)), "nearest_x": np.full((b, n), -1, np.int64), "dist_y": np.zeros((b, m)),
           "nearest_y": np.full((b, m), -1, np.int64)}
    if n * m <= 4096:                                     # small clouds: the whole batch at once, lengths as masks
        nlt, mlt = torch.from_numpy(nl).to(dev), torch.from_numpy(ml).to(dev)
        in_x = torch.arange(n, device=dev)[None, :] < torch.where(mlt > 0, nlt, torch.zeros_like(nlt))[:, None]
        in_y = torch.arange(m, device=dev)[None, :] < torch.where(nlt > 0, mlt, torch.zeros_like(mlt))[:, None]
        d2 = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
        d2 = torch.where(in_x[:, :, None] & in_y[:, None, :], d2, torch.full_like(d2, float("inf")))
        for side, dim, keep in (("x", 2, in_x), ("y", 1, in_y)):
            v, i = d2.min(dim)
            v, i, keep = v.cpu().numpy(), i.cpu().numpy(), keep.cpu().numpy()
            out["dist_" + side] = np.where(keep, ref.term(np.where(keep, v, 0.0), squared), 0.0)
            out["nearest_" + side] = np.where(keep, i, -1)
    else:
        for k in range(b):
            nb, mb = int(nl[k]), int(ml[k])
            if nb == 0 or mb == 0:
                continue
            d2 = ((x[k, :nb, None, :] - y[k, None, :mb, :]) ** 2).sum(-1)
            v, i = d2.min(1)
            out["dist_x"][k, :nb], out["nearest_x"][k, :nb] = ref.term(v.cpu().numpy(), squared), i.cpu().numpy()
            v, i = d2.min(0)
            out["dist_y"][k, :mb], out["nearest_y"][k, :mb] = ref.term(v.cpu().numpy(), squared), i.cpu().numpy()
    live = (nl > 0) & (ml > 0)
    out["sums"] = np.stack([out["dist_x"].sum(1), out["dist_y"].sum(1)], 1) * live[:, None]
    out["rows"] = out["sums"] / np.maximum(np.stack([nl, ml], 1), 1)
    return out


def surface_run(c, dev, single=False, long_lengths=False):
    """Forward and backward through chamfer_distance: per-cloud rows (batch_reduction=None), the upstream gradient ref.scales' first
    vector; the scales the backward folds are rebuilt here in float32 the way the library forms them."""
    import poseestimation_amd as pa
    b, n, m = c["b"], c["n"], c["m"]
    X, Y = to_device(c["X"], dev).requires_grad_(), to_device(c["Y"], dev).requires_grad_()
    ltype = np.int64 if long_lengths else np.int32
    xl, yl = to_device(c["x_lengths"], dev, ltype), to_device(c["y_lengths"], dev, ltype)
    loss, info = pa.chamfer_distance(X, Y, xl, yl, squared=c["squared"], batch_reduction=None, single_directional=single, return_nearest=True)
    assert loss.shape == (b,) and loss.dtype == torch.float32 and info["nearest_x"].dtype == torch.int64 and info["dist_x"].shape == (b, n)
    assert set(info) == ({"nearest_x", "dist_x"} if single else {"nearest_x", "dist_x", "nearest_y", "dist_y"})
    g = ref.scales(b)[0]
    loss.backward(to_device(g, dev))
    got = {k: v.cpu().numpy() for k, v in info.items()}
    got["loss"] = loss.detach().cpu().numpy()
    nl, ml = lengths_of(c["x_lengths"], b, n), lengths_of(c["y_lengths"], b, m)
    got["scale_x"] = g * np.float32(1.0 / n) if c["x_lengths"] is None else g / np.maximum(nl, 1).astype(np.float32)
    got["scale_y"] = g * np.float32(1.0 / m) if c["y_lengths"] is None else g / np.maximum(ml, 1).astype(np.float32)
    got["dX"] = X.grad.cpu().numpy()
    got["dY"] = Y.grad.cpu().numpy()
    return got


def abi_run(c, dev, single=False):
    """One case through the raw C ABI into NaN / -2 pre-filled, guarded device buffers and a NaN workspace (nothing needs a zero-fill),
    then again with every optional output NULL."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, m = c["b"], c["n"], c["m"]
    X, Y = to_device(c["X"], dev), to_device(c["Y"], dev)
    xl, yl = to_device(c["x_lengths"], dev, np.int32), to_device(c["y_lengths"], dev, np.int32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flags = (0 if c["squared"] else host.UNSQUARED) | (host.SINGLE if single else 0)
    spec = {"dist_x": ((b, n), np.nan, torch.float32), "nearest_x": ((b, n), -2, torch.int32), "rows": ((b, 2), np.nan, torch.float32),
            "dX": ((b, n, 3), np.nan, torch.float32), "dY": ((b, m, 3), np.nan, torch.float32)}
    if not single:
        spec.update(dist_y=((b, m), np.nan, torch.float32), nearest_y=((b, m), -2, torch.int32))
    whole, out = {}, {}
    for k, (shape, fill, dtype) in spec.items():
        whole[k], out[k] = guarded(shape, fill, dtype, dev)
    words = lib.so3_chamfer_workspace_bytes(b, n, m) // 4
    work_whole, work = guarded((words,), np.nan, torch.float32, dev)
    sx, sy = ref.scales(b)
    sxd, syd = to_device(sx, dev), (None if single else to_device(sy, dev))
    _lib.check(lib.so3_chamfer_fwd_f32(ptr(X), ptr(Y), ptr(xl), ptr(yl), ptr(out["dist_x"]), ptr(out["nearest_x"]), ptr(out.get("dist_y")),
                                       ptr(out.get("nearest_y")), ptr(out["rows"]), ptr(work), flags, b, n, m, st), "so3_chamfer_fwd_f32")
    KERNELS.append(lib.so3_last_kernel().decode())                                          # the forward's instantiation, for the caller
    _lib.check(lib.so3_chamfer_bwd_f32(ptr(X), ptr(Y), ptr(xl), ptr(yl), ptr(out["nearest_x"]), ptr(out.get("nearest_y")), ptr(sxd), ptr(syd),
                                       ptr(out["dX"]), ptr(out["dY"]), flags, b, n, m, st), "so3_chamfer_bwd_f32")
    assert lib.so3_last_kernel().decode() == "k_chamfer_bwd<%s>" % ("true" if c["squared"] else "false")
    rows2 = torch.full((b, 2), np.nan, device=dev)                                          # every optional output left out
    _lib.check(lib.so3_chamfer_fwd_f32(ptr(X), ptr(Y), ptr(xl), ptr(yl), None, None, None, None, ptr(rows2), ptr(work), flags, b, n, m, st),
               "so3_chamfer_fwd_f32")
    assert torch.equal(rows2, out["rows"])
    for only in ("dX", "dY"):                                                              # each gradient alone
        alone = torch.full(spec[only][0], np.nan, device=dev)
        _lib.check(lib.so3_chamfer_bwd_f32(ptr(X), ptr(Y), ptr(xl), ptr(yl), ptr(out["nearest_x"]), ptr(out.get("nearest_y")), ptr(sxd), ptr(syd),
                                           ptr(alone) if only == "dX" else None, ptr(alone) if only == "dY" else None, flags, b, n, m, st),
                   "so3_chamfer_bwd_f32")
        assert torch.equal(alone, out[only])
    torch.cuda.synchronize()
    for k, (shape, fill, dtype) in spec.items():
        assert guards_intact(whole[k], fill), k
    assert guards_intact(work_whole, np.nan)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- G27 ------------------------------------------------------------------------------------------------------------------------
def test_g27_through_the_python_surface(dev, g27_cases):
    host.check_against_g27(g27_cases, lambda c: surface_run(c, dev), "surface")


def test_g27_through_the_c_abi(dev, g27_cases):
    host.check_against_g27(g27_cases, lambda c: abi_run(c, dev), "abi")


def test_g27_single_direction(dev, g27_cases):
    picked = [c for c in g27_cases if c["geometry"] in ("random_257x1025", "subset_300x700")]
    host.check_against_g27(picked, lambda c: abi_run(c, dev, single=True), "abi single", single=True)
    host.check_against_g27(picked, lambda c: surface_run(c, dev, single=True), "surface single", single=True)


# ---- every work split -----------------------------------------------------------------------------------------------------------
def _rule(b, n, m, cus):
    u = 4
    while u > 1 and b * ((n + 256 * u - 1) // (256 * u) + (m + 256 * u - 1) // (256 * u)) < 2 * cus:
        u >>= 1
    return u


SPLIT_SIZES = ref.SIZES + [(1025, 1023), (2049, 2047)]
SPLITS = [(b, n, m) for b in (1, 3, 65) for n, m in SPLIT_SIZES]


def _split_case(b, n, m, ragged, squared):
    rng = np.random.default_rng(27000 + 97 * b + n + m)
    c = {"name": "split", "family": "random", "X": _ball(rng, b, n), "Y": _ball(rng, b, m), "x_lengths": None, "y_lengths": None,
         "squared": squared, "b": b, "n": n, "m": m}
    if ragged:
        c["x_lengths"], c["y_lengths"] = rng.integers(0, n + 1, b), rng.integers(0, m + 1, b)
    return c


def _split_check(c, dev, long_lengths, label):
    from poseestimation_amd import _lib
    got = surface_run(c, dev, long_lengths=long_lengths)
    kernel = _lib.load().so3_last_kernel().decode()
    want = want64(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["squared"], dev)
    f = ref.forward_figures(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["squared"], got, want=want)
    assert f["exact"] == 0.0, (label, f)
    f.update(ref.gradient_figures(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["squared"], got["nearest_x"], got["nearest_y"],
                                  got["scale_x"], got["scale_y"], got["dX"], got["dY"]))
    print(label, "  ".join("%s %.2e" % kv for kv in f.items()))
    bnd = dict(host.bounds(), search=host.SEARCH_REASONED)
    for k, v in f.items():
        assert v <= bnd[k], (label, k, v, bnd[k])
    return kernel


@pytest.mark.parametrize("b,n,m", SPLITS, ids=lambda v: str(v))
def test_work_splits_against_float64(dev, b, n, m):
    """Fresh random clouds of unit radius, ragged with int32 or int64 lengths or full, squared or not (alternating over the cases):
    every figure against float64 on the same input, and the instantiation the launcher's rule names."""
    k = SPLITS.index((b, n, m))
    c = _split_case(b, n, m, ragged=k % 3 != 0, squared=k % 2 == 0)
    # so3_last_kernel is per thread and autograd runs the backward on its own: this thread's last launch is the forward
    kernel = _split_check(c, dev, long_lengths=k % 3 == 2, label="split B=%d N=%d M=%d" % (b, n, m))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    u = _rule(b, n, m, cus)
    assert kernel == "k_chamfer_fwd<%s, %d>" % ("true" if c["squared"] else "false", u)


def test_batch_above_the_grid_cap(dev):
    """More work items than the grid holds (64 workgroups per compute unit): workgroups take several items, at U = 4."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    b, n, m = cus * 32 + 1, 12, 12
    c = _split_case(b, n, m, ragged=True, squared=True)
    assert _split_check(c, dev, long_lengths=False, label="above the cap B=%d" % b) == "k_chamfer_fwd<true, 4>"
    if cus == 256:                      # an MI355X in SPX mode: with this one the shapes of the work splits reach every instantiation
        assert {_rule(*s, cus) for s in SPLITS} | {4} == {1, 2, 4}


# ---- every work split, bit for bit ----------------------------------------------------------------------------------------------
def _exact_case(b, n, m):
    """Fresh clouds of unit radius, squared, ragged: the first and the last cloud keep every point (the sizes are tile and chunk edges),
    the others random lengths >= 1, and from three clouds on cloud 1 has an empty x side."""
    c = _split_case(b, n, m, ragged=True, squared=True)
    rng = np.random.default_rng(27500 + 97 * b + n + m)
    c["x_lengths"], c["y_lengths"] = rng.integers(1, n + 1, b), rng.integers(1, m + 1, b)
    for k in (0, b - 1):
        c["x_lengths"][k], c["y_lengths"][k] = n, m
    if b >= 3:
        c["x_lengths"][1] = 0
    return c


def _restated_clouds(b, n, m):
    """The clouds the float32 restatement covers within F32_PAIRS pairs (both directions: 2 N M per cloud): the first, the last and
    every k-th between, k the smallest power of two that fits.  -> (indices, k)."""
    k = 1
    while True:
        keep = np.union1d(np.arange(0, b, k), [b - 1])
        if len(keep) * 2 * n * m <= F32_PAIRS:
            return keep, k
        k *= 2


def _exact_check(c, dev, label, single=False):
    """so3_chamfer_fwd_f32 / so3_chamfer_bwd_f32 through the raw C ABI (NaN / -2 pre-filled, guarded buffers; each gradient alone gives
    the bits of both: abi_run) against chamfer_ref.search32 and, through the device's OWN indices and ref.scales' float32 scales,
    grad32.  Equality of indices and of bit patterns, every slot of every restated cloud."""
    b, n, m = c["b"], c["n"], c["m"]
    got = abi_run(c, dev, single)
    kernel = KERNELS[-1]                                                                     # abi_run's forward into the checked buffers
    keep, k = _restated_clouds(b, n, m)
    print("%s: %s, %d of %d clouds restated (every %d%s)" % (label, kernel, len(keep), b, k, "" if k == 1 else ", the first and the last"))
    sub = lambda a: None if a is None else np.asarray(a)[keep]
    want = ref.search32(c["X"][keep], c["Y"][keep], sub(c["x_lengths"]), sub(c["y_lengths"]), single)
    for key, w in want.items():
        g = got[key][keep]
        wrong = np.argwhere(g != w) if key.startswith("nearest") else np.argwhere(bits(g) != bits(w))
        assert len(wrong) == 0, (label, key, len(wrong), keep[wrong[:4, 0]], wrong[:4, 1], g[tuple(wrong[:4].T)], w[tuple(wrong[:4].T)])
    if not single:                                  # the unsquared flavour takes the root of the same minimum: its indices are the same
        l2 = abi_run(dict(c, squared=False), dev)
        assert KERNELS[-1] == kernel.replace("<true", "<false")
        for key in ("nearest_x", "nearest_y"):
            assert np.array_equal(l2[key][keep], want[key]), (label, "unsquared", key)
    sx, sy = ref.scales(b)
    dX, dY = ref.grad32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], got["nearest_x"], None if single else got["nearest_y"], sx, None if single else sy,
                        clouds=keep)
    for key, w in (("dX", dX), ("dY", dY)):
        wrong = np.argwhere(bits(got[key][keep]) != bits(w[keep]))
        assert len(wrong) == 0, (label, key, len(wrong), keep[wrong[:4, 0]], wrong[:4, 1:], got[key][keep][tuple(wrong[:4].T)], w[keep][tuple(wrong[:4].T)])
    return kernel, keep


@pytest.mark.parametrize("b,n,m", SPLITS, ids=lambda v: str(v))
def test_work_splits_bit_for_bit(dev, b, n, m):
    """The squared flavour on every size of the work-split test: nearest_x / nearest_y equal search32's indices, dist_x / dist_y its
    d^2 and dX / dY grad32, bit for bit; the instantiation is the one the launcher's rule names.  SO3_CHAMFER_SINGLE on every third."""
    c = _exact_case(b, n, m)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    kernel, _ = _exact_check(c, dev, "exact B=%d N=%d M=%d" % (b, n, m))
    assert kernel == "k_chamfer_fwd<true, %d>" % _rule(b, n, m, cus)
    if SPLITS.index((b, n, m)) % 3 == 0:
        _exact_check(c, dev, "exact single B=%d N=%d M=%d" % (b, n, m), single=True)


def test_four_points_per_lane_on_multi_tile_clouds_bit_for_bit(dev):
    """The sizes above reach U = 4 only on clouds of 12 points: the smallest batch whose rule gives U = 4 at (1025, 1023) -- two tiles, the
    second of one point and seven pads, and x's second work item holding one real point."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    b = next(b for b in range(1, 4 * cus) if _rule(b, 1025, 1023, cus) == 4)
    kernel, _ = _exact_check(_exact_case(b, 1025, 1023), dev, "exact U = 4 B=%d N=1025 M=1023" % b)
    assert kernel == "k_chamfer_fwd<true, 4>"


def test_a_small_last_hit_of_a_long_chain_bit_for_bit(dev):
    """2500 hits on one owner, the last of them a tenth of what the float64 figure's bound lets pass and tens of ulps of the running sum
    (tests/test_f32_exact_host.py holds the premise): in the last, partial block of k_chamfer_bwd's scan."""
    c = ref.small_last_hit_case()
    _exact_check(c, dev, "exact " + c["name"])


def test_batch_above_the_grid_cap_bit_for_bit(dev):
    """More work items than the grid holds: two items per cloud at U = 4, so the last cloud's items are served on the grid's second
    trip, and every cloud is restated (k = 1).  With it the exact comparison has run under U = 1, 2 and 4 on an MI355X."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    b, n, m = cus * 32 + 1, 12, 12
    kernel, keep = _exact_check(_exact_case(b, n, m), dev, "exact above the cap B=%d" % b)
    assert kernel == "k_chamfer_fwd<true, 4>"
    grid, per = cus * 64, 2                                     # chamfer_grid; chunks_x + chunks_y
    assert b * per > grid and (keep * per + per - 1 >= grid).any() and len(keep) == b       # a second-trip cloud is among the restated ones
    if cus == 256:                      # every case above asserts the instantiation its rule names: on an MI355X in SPX mode they are all three
        assert {_rule(*s, cus) for s in SPLITS} | {4} == {1, 2, 4}


# ---- reductions and arguments ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(dev):
    rng = np.random.default_rng(2727)
    b, n, m = 3, 257, 130
    c = {"X": _ball(rng, b, n), "Y": _ball(rng, b, m), "x_lengths": np.array([257, 100, 31]), "y_lengths": np.array([64, 130, 1]), "b": b, "n": n, "m": m}
    assert ref.min_nonzero_distance(c["X"], c["Y"], c["x_lengths"], c["y_lengths"]) >= ref.MIN_DISTANCE
    return c


def test_every_reduction_against_float64(dev, small):
    import poseestimation_amd as pa
    c, b, n, m = small, small["b"], small["n"], small["m"]
    xl, yl = to_device(c["x_lengths"], dev, np.int64), to_device(c["y_lengths"], dev, np.int64)
    gvec = np.array([0.5, -2.0, 1.25])
    for pr, br, single, squared, ragged in itertools.product(("mean", "sum"), ("mean", "sum", None), (False, True), (True, False), (True, False)):
        lx, ly = (c["x_lengths"], c["y_lengths"]) if ragged else (None, None)
        X, Y = to_device(c["X"], dev).requires_grad_(), to_device(c["Y"], dev).requires_grad_()
        loss, info = pa.chamfer_distance(X, Y, xl if ragged else None, yl if ragged else None, squared=squared, point_reduction=pr, batch_reduction=br,
                                         single_directional=single, return_nearest=True)
        g = gvec if br is None else 0.75
        loss.backward(to_device(g, dev) if br is None else torch.tensor(g, device=dev))
        fwd = ref.chamfer64(c["X"], c["Y"], lx, ly, squared)
        want = ref.loss64(fwd, lx, ly, n, m, pr, br, single)
        rel = ref._relative(np.atleast_1d(loss.detach().cpu().numpy()), np.atleast_1d(want), np.abs(np.atleast_1d(want)))
        a, cc = ref.fold_scales(g, b, n, m, lx, ly, pr, br)
        f = ref.gradient_figures(c["X"], c["Y"], lx, ly, squared, info["nearest_x"].cpu().numpy(), None if single else info["nearest_y"].cpu().numpy(),
                                 a, None if single else cc, X.grad.cpu().numpy(), Y.grad.cpu().numpy())
        print("reduction %-4s %-4s single=%d squared=%d ragged=%d  loss %.2e  grad %.2e" % (pr, br, single, squared, ragged, rel, f["grad"]))
        assert loss.shape == (() if br is not None else (b,))
        assert rel <= host.REDUCTION_TOL and f["grad"] <= host.FOLDED_GRAD_TOL, (pr, br, single, squared, ragged, rel, f)


def test_padded_slots_and_empty_clouds(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(5)
    X, Y = to_device(_ball(rng, 4, 70), dev).requires_grad_(), to_device(_ball(rng, 4, 300), dev).requires_grad_()
    xl, yl = torch.tensor([0, 70, 33, 99], device=dev), torch.tensor([300, 0, 257, -4], device=dev)      # clipped: 99 -> 70, -4 -> 0
    loss, info = pa.chamfer_distance(X, Y, xl, yl, batch_reduction=None, return_nearest=True)
    loss.sum().backward()
    assert loss[[0, 1, 3]].eq(0).all() and loss[2] > 0
    for k in (0, 1, 3):
        assert info["dist_x"][k].eq(0).all() and info["nearest_x"][k].eq(-1).all() and info["dist_y"][k].eq(0).all() and info["nearest_y"][k].eq(-1).all()
        assert X.grad[k].eq(0).all() and Y.grad[k].eq(0).all()
    assert info["nearest_x"][2, 33:].eq(-1).all() and info["dist_x"][2, 33:].eq(0).all() and X.grad[2, 33:].eq(0).all()
    assert info["nearest_y"][2, 257:].eq(-1).all() and info["dist_y"][2, 257:].eq(0).all() and Y.grad[2, 257:].eq(0).all()
    assert info["nearest_x"][2, :33].ge(0).all() and info["nearest_x"][2, :33].lt(257).all() and info["nearest_y"][2, :257].lt(33).all()
    assert X.grad[2, :33].abs().sum() > 0 and torch.isfinite(X.grad).all() and torch.isfinite(Y.grad).all()


def test_autograd_surface(dev, small):
    import poseestimation_amd as pa
    c = small
    X0, Y0 = to_device(c["X"], dev), to_device(c["Y"], dev)
    # a strided per-cloud upstream gradient equals its contiguous copy, and a scalar upstream gradient scales the result
    g = torch.arange(1, 7, device=dev, dtype=torch.float32)[::2]
    grads = []
    for up in (g, g.contiguous()):
        X, Y = X0.clone().requires_grad_(), Y0.clone().requires_grad_()
        pa.chamfer_distance(X, Y, batch_reduction=None).backward(up)
        grads.append((X.grad, Y.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # a scalar upstream gradient: 3 / B folded into the scales
    X, Y = X0.clone().requires_grad_(), Y0.clone().requires_grad_()
    loss, info = pa.chamfer_distance(X, Y, return_nearest=True)
    (loss * 3.0).backward()
    a, cc = ref.fold_scales(3.0, c["b"], c["n"], c["m"], None, None, "mean", "mean")
    f = ref.gradient_figures(c["X"], c["Y"], None, None, True, info["nearest_x"].cpu().numpy(), info["nearest_y"].cpu().numpy(), a, cc,
                             X.grad.cpu().numpy(), Y.grad.cpu().numpy())
    assert f["grad"] <= host.FOLDED_GRAD_TOL, f
    X2, Y2 = X0.clone().requires_grad_(), Y0.clone().requires_grad_()
    pa.chamfer_distance(X2, Y2).backward()
    # Y alone requires grad; X alone; neither
    Y = Y0.clone().requires_grad_()
    pa.chamfer_distance(X0, Y).backward()
    assert torch.equal(Y.grad, Y2.grad)
    X = X0.clone().requires_grad_()
    pa.chamfer_distance(X, Y0).backward()
    assert torch.equal(X.grad, X2.grad)
    assert not pa.chamfer_distance(X0, Y0).requires_grad
    # float64 clouds get float64 gradients
    Xd = X0.double().requires_grad_()
    pa.chamfer_distance(Xd, Y0).backward()
    assert Xd.grad.dtype == torch.float64 and torch.equal(Xd.grad.float(), X2.grad)
    # double backward is refused
    X = X0.clone().requires_grad_()
    (gx,) = torch.autograd.grad(pa.chamfer_distance(X, Y0), X, create_graph=True)
    assert not gx.requires_grad
    w = torch.ones((), device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(pa.chamfer_distance(X, Y0) * w, X, create_graph=True)[0].sum().backward()
    # bad shapes
    for bad in ((X0[0], Y0), (X0, Y0[0]), (X0, Y0[:2]), (X0[..., :2], Y0), (X0[:, :0], Y0)):
        with pytest.raises(RuntimeError, match=r"expected a source \(B, N, 3\) and a target \(B, M, 3\)"):
            pa.chamfer_distance(*bad)
    with pytest.raises(RuntimeError, match="x_lengths"):
        pa.chamfer_distance(X0, Y0, torch.ones(2, device=dev, dtype=torch.int64))


# ---- repeatability --------------------------------------------------------------------------------------------------------------
def _run(pa, X0, Y0, xl, yl, squared):
    X, Y = X0.clone().requires_grad_(), Y0.clone().requires_grad_()
    loss = pa.chamfer_distance(X, Y, xl, yl, squared=squared, batch_reduction=None)
    loss.backward(torch.linspace(0.5, 2.0, len(X0), device=X0.device))
    return loss.detach(), X.grad, Y.grad


@pytest.mark.parametrize("squared", (True, False))
def test_same_bits_from_call_to_call_and_in_any_batch_order(dev, squared):
    import poseestimation_amd as pa
    rng = np.random.default_rng(9)
    b, n, m = 5, 700, 1300
    X0, Y0 = to_device(_ball(rng, b, n), dev), to_device(_ball(rng, b, m), dev)
    Y0[:, :40] = X0[:, 5:6]                                       # forty points of Y share their nearest x: a long chain
    xl, yl = torch.tensor([700, 650, 1, 700, 333], device=dev), torch.tensor([1300, 64, 1300, 1025, 777], device=dev)
    up = torch.linspace(0.5, 2.0, b, device=dev)
    first = _run(pa, X0, Y0, xl, yl, squared)
    again = _run(pa, X0, Y0, xl, yl, squared)
    assert all(torch.equal(a, c) for a, c in zip(first, again))
    # the batch reversed: the same bits per cloud (the upstream gradient is reversed with it)
    X, Y = X0.flip(0).clone().requires_grad_(), Y0.flip(0).clone().requires_grad_()
    loss = pa.chamfer_distance(X, Y, xl.flip(0), yl.flip(0), squared=squared, batch_reduction=None)
    loss.backward(up.flip(0))
    assert torch.equal(loss.detach().flip(0), first[0]) and torch.equal(X.grad.flip(0), first[1]) and torch.equal(Y.grad.flip(0), first[2])
    # a NaN cloud changes no other cloud
    Xn, Yn = X0.clone(), Y0.clone()
    Xn[1] = float("nan")
    Yn[1, 3] = float("nan")
    poisoned = _run(pa, Xn, Yn, xl, yl, squared)
    keep = [0, 2, 3, 4]
    assert all(torch.equal(a[keep], c[keep]) for a, c in zip(first, poisoned))


def test_replay_from_a_captured_graph(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(10)
    b, n, m = 3, 300, 520
    X0, Y0 = to_device(_ball(rng, b, n), dev), to_device(_ball(rng, b, m), dev)
    xl, yl = torch.tensor([300, 17, 256], device=dev, dtype=torch.int32), torch.tensor([520, 500, 3], device=dev, dtype=torch.int32)
    X, Y = X0.clone().requires_grad_(), Y0.clone().requires_grad_()

    def step():
        loss = pa.chamfer_distance(X, Y, xl, yl, squared=False, point_reduction="sum")
        gx, gy = torch.autograd.grad(loss, (X, Y))
        return loss.detach(), gx, gy

    eager = step()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                       # warm up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(eager, captured))
    with torch.no_grad():                                            # new inputs in place: the replay follows them
        X.copy_(X0.flip(1))
    graph.replay()
    torch.cuda.synchronize()
    fresh = step()
    assert all(torch.equal(a, c) for a, c in zip(fresh, captured))


# ---- speed ----------------------------------------------------------------------------------------------------------------------
def test_chamfer_is_not_slower_than_the_torch_spelling(dev):
    """B = 16, N = M = 2048, forward plus backward, HIP events, 5 warm-ups, median of 20: chamfer_distance against the torch spelling on
    the same device in the same process -- the pairwise (B,N,M) differences, min both ways, gather and mean, with autograd."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    rng = np.random.default_rng(16)
    b, n, m = 16, 2048, 2048
    X, Y = to_device(_ball(rng, b, n), dev).requires_grad_(), to_device(_ball(rng, b, m), dev).requires_grad_()

    def torch_spelling(X, Y):
        with torch.no_grad():
            d2 = ((X[:, :, None, :] - Y[:, None, :, :]) ** 2).sum(-1)
            j, i = d2.argmin(2), d2.argmin(1)
        ex = ((X - Y.gather(1, j[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
        ey = ((Y - X.gather(1, i[..., None].expand(-1, -1, 3))) ** 2).sum(-1).mean(1)
        return (ex + ey).mean()

    def both(fn):
        X.grad = Y.grad = None
        fn(X, Y).backward()

    def median_ms(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    ours = median_ms(lambda: both(pa.chamfer_distance))
    theirs = median_ms(lambda: both(torch_spelling))
    with torch.no_grad():
        got = pa.chamfer_distance(X, Y).item()
        want = torch_spelling(X.detach().double(), Y.detach().double()).item()
    line = "chamfer B=16 N=M=2048 fwd+bwd: chamfer_distance %.4f ms, torch pairwise/min/gather/mean %.4f ms (x%.1f)" % (ours, theirs, theirs / ours)
    print(line)
    REPORT_LINES.append(line)
    # the rows' bound, one rounding for the sum of the two directions and at most B - 1 = 15 for the batch mean (test_chamfer_host.py)
    assert abs(got - want) <= (host.ROWS_TOL + 16 * 2.0 ** -24) * want, (got, want)
    assert theirs / ours >= 1.0, line
