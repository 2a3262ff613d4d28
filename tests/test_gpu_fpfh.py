"""fpfh_features on the GPU: pairs and counts EXACTLY the float64 ones under the margin condition, spfh bit for bit (100 c) / r, fpfh
bit for bit the restatement of its defined order and within 4 x the host model's figure of float64 (tests/fpfh_ref.py), through the
Python surface and through the raw C ABI into pre-filled, guarded buffers -- G32, spfh alone and pairs alone, every group width and N
around a wave's and a workgroup's queries, B, a batch above the grid cap, int32 and int64 indices and lengths, indices straight from
knn_points and query_ball_point, idx=None, estimate_normals' normals end to end, the power-of-two property, repeatability, the
reversed batch, the non-finite cloud, exact swap ties, features past the outer edges and the weight rule, replay from a graph, the
moved copy matched by match_features, the warning, the surface's errors, and the speed condition against the torch spelling."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import fpfh_ref as ref
from support import bits, dev, guarded, guards_intact, last_kernel, median_ms, ptr, to_device  # noqa: F401
import test_fpfh_host as host

pytestmark = pytest.mark.gpu
SENTINEL = -7                        # what the pairs buffer holds before the call


@pytest.fixture(scope="module")
def g32_cases():
    return ref.cases(ref.g32())


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


def make_case(name, X, Nr, idx, lengths=None, strict=True):
    """A fresh case in the fixture's layout, its float64 counts computed here, once.  strict: every row keeps the margin condition
    (cut from G32's families it does: dropping slots drops pairs); otherwise the rows that break it are left out of the judgement."""
    X, Nr, idx = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Nr, np.float32), np.ascontiguousarray(idx, np.int32)
    f = ref.features64(X, Nr, idx, lengths)
    counts, _ = ref.counts_of(f["pair"], f["g"])
    c = ref._case(name, "fresh", X, Nr, idx, lengths, counts)
    broken = ref.violations(f).any(-1)
    assert not (strict and (broken & c["spfh_rows"]).any()), name
    c["spfh_rows"] = c["spfh_rows"] & ~broken
    batch, valid = np.arange(c["b"])[:, None, None], f["valid"]
    c["fpfh_rows"] = c["fpfh_rows"] & c["spfh_rows"] & ~(valid & ~c["spfh_rows"][batch, f["at"]]).any(-1)
    return c


def cut(c, n, K, clouds=1):
    """The first n points and the first K slots of a G32 case (an index past n becomes -1), `clouds` times: the second cloud keeps the
    LAST K slots instead, the third every other point's row shifted by one slot -- three different clouds from one family."""
    X, Nr, rows = c["X"][0, :n], c["normals"][0, :n], c["idx"][0, :n]
    variants = [rows[:, :K], rows[:, rows.shape[1] - K:], np.roll(rows, 1, axis=1)[:, :K]][:clouds]
    idx = np.stack([np.where(v < n, v, -1) for v in variants])
    return make_case("%s cut to %d x %d x %d" % (c["name"], clouds, n, K), np.stack([X] * clouds), np.stack([Nr] * clouds), idx)


def abi_run(c, dev, want=(True, True), kernel=None):
    """The raw C ABI into pre-filled buffers (NaN, SENTINEL) with GUARD elements in front of and behind each output.  -> (spfh, pairs,
    fpfh) as numpy arrays; None where not wanted, and no fpfh unless both are."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, K = c["b"], c["n"], c["K"]
    Xd, Nd, id_, ld = to_device(c["X"], dev), to_device(c["normals"], dev), to_device(c["idx"], dev, np.int32), to_device(c["lengths"], dev, np.int32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    s_whole, s = guarded((b, n, ref.SLOTS), float("nan"), torch.float32, dev) if want[0] else (None, None)
    p_whole, p = guarded((b, n), SENTINEL, torch.int32, dev) if want[1] else (None, None)
    _lib.check(lib.so3_spfh_f32(ptr(Xd), ptr(Nd), ptr(id_), ptr(ld), ptr(s), ptr(p), K, b, n, st), "so3_spfh_f32")
    width = 1 << max(0, math.ceil(math.log2(K)))
    assert last_kernel() == "k_spfh<%d>" % width == (kernel or last_kernel())
    f_whole, f = None, None
    if all(want):
        f_whole, f = guarded((b, n, ref.SLOTS), float("nan"), torch.float32, dev)
        _lib.check(lib.so3_fpfh_f32(ptr(Xd), ptr(id_), ptr(ld), ptr(s), ptr(p), ptr(f), K, b, n, st), "so3_fpfh_f32")
        assert last_kernel() == "k_fpfh"
    torch.cuda.synchronize()
    for whole, fill in ((s_whole, float("nan")), (p_whole, SENTINEL), (f_whole, float("nan"))):
        assert whole is None or guards_intact(whole, fill), "a guard was written"
    return tuple(None if t is None else t.cpu().numpy() for t in (s, p, f))


def surface_run(c, dev, long=False, dtype=np.float32):
    import poseestimation_amd as pa
    itype = np.int64 if long else np.int32
    fpfh, spfh, pairs = pa.fpfh_features(to_device(c["X"], dev, dtype), to_device(c["normals"], dev, dtype), to_device(c["idx"], dev, itype),
                                         lengths=to_device(c["lengths"], dev, itype), return_spfh=True)
    b, n = c["b"], c["n"]
    assert fpfh.shape == spfh.shape == (b, n, ref.SLOTS) and pairs.shape == (b, n) and fpfh.dtype == spfh.dtype == torch.float32 and pairs.dtype == torch.int64
    assert not (fpfh.requires_grad or spfh.requires_grad)
    return spfh.cpu().numpy(), pairs.cpu().numpy().astype(np.int32), fpfh.cpu().numpy()


def same_bits(a, b_):
    return all((u is None and v is None) or np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b_))


# ---- G32 --------------------------------------------------------------------------------------------------------------------
def test_g32_through_the_c_abi(dev, g32_cases):
    worst = host.check_against_g32(g32_cases, lambda c: abi_run(c, dev), "abi")
    print("device over G32: fpfh's largest relative deviation from float64 %.3g (the host model: %.3g, the bound: %.3g)"
          % (worst, ref.MEASURED["fpfh"], ref.FPFH_BOUND))


def test_g32_through_the_python_surface(dev, g32_cases):
    host.check_against_g32(g32_cases, lambda c: surface_run(c, dev), "surface")
    some = [c for c in g32_cases if c["family"] in ("mixed", "ragged", "k_above_n", "nonfinite")]    # int64 indices and lengths
    host.check_against_g32(some, lambda c: surface_run(c, dev, long=True), "surface int64")
    c = by_name(g32_cases, "blob_257x16")                                                            # any float dtype; the arithmetic is float32
    assert same_bits(surface_run(c, dev, dtype=np.float64), surface_run(c, dev))


def test_spfh_alone_and_pairs_alone(dev, g32_cases):
    for name in ("blob_257x16", "ragged", "mixed"):
        c = by_name(g32_cases, name)
        spfh, pairs, _ = abi_run(c, dev)
        only_s, only_p = abi_run(c, dev, (True, False)), abi_run(c, dev, (False, True))
        assert only_s[1] is None and only_p[0] is None and same_bits((only_s[0], only_p[1]), (spfh, pairs)), name
        host.check_case("spfh alone", c, spfh=only_s[0])
        host.check_case("pairs alone", c, pairs=only_p[1])


# ---- every launch geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_every_group_width_and_n(dev, g32_cases, b):
    """K: every group width 1 .. 64 at and just past a power of two.  N: partial waves, a partial last group, N * 33 no multiple
    of 64, around a workgroup's queries.  Cut from the sphere and the blob at 300 x 64, whose rows keep the margin condition."""
    for fam in ("sphere_300x64", "blob_300x64")[:1 if b == 3 else 2]:
        c0 = by_name(g32_cases, fam)
        for K in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64):
            for n in ((1, 2, 63, 64, 65, 255, 256, 257) if K in (5, 16, 33) else (2, 65)):
                c = cut(c0, n, K, b)
                host.check_case("abi", c, *abi_run(c, dev))
                if (K + n) % 3 == 0:
                    host.check_case("surface", c, *surface_run(c, dev, long=bool(n % 2)))


def test_a_batch_above_the_grid_cap(dev):
    """N = 12: more work items than the grid holds in both kernels.  A handful of settled clouds (full, ragged, one point, empty),
    tiled, their answers gathered by the same index."""
    rng = np.random.default_rng(3210)
    n, K, few = 12, 8, np.array([12, 12, 12, 12, 7, 3, 1, 0], np.int32)
    X, Nr, idx = ref.settle(rng, ref.draw_blob, len(few), n, K, lengths=few)
    base = make_case("settled", X, Nr, idx, few)
    b = host.GRID_CAP + 3
    assert -(-n // (host.BLOCK // 8)) * b > host.GRID_CAP and -(-n * ref.SLOTS // host.BLOCK) * b > host.GRID_CAP
    sel = rng.integers(0, len(few), b)
    c = {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    c.update(name="beyond the grid", b=b)
    host.check_case("abi", c, *abi_run(c, dev, kernel="k_spfh<8>"))                                  # abi_run asserts so3_last_kernel of both


# ---- where the definition branches exactly (tests/fpfh_ref.py: the branch cases) ------------------------------------------------------
@pytest.mark.parametrize("K", ref.EDGE_KS)
def test_swap_ties_and_outer_edges(dev, K):
    """Exact swap ties (no swap) and features past the outer edges (bins 10 and 0), N = 257, B = 3, one ragged cloud, rows padded with
    -1, in k_spfh<8>, <16> and <64>: exact counts, spfh and fpfh bit for bit, and the same bits at 2^+-20."""
    for c in ref.branch_cases(K):
        base = abi_run(c, dev, kernel="k_spfh<%d>" % {5: 8, 16: 16, 33: 64}[K])
        host.check_branch_case("abi", c, *base)
        host.check_branch_case("surface", c, *surface_run(c, dev, long=K == 16))
        host.check_power_of_two("abi", c, base, lambda d: abi_run(d, dev))


def test_the_weight_rule_through_the_second_launch_alone(dev):
    """so3_fpfh_f32 from GIVEN spfh and pairs: a slot with 1 / d2 = inf is skipped, one with w = 2^118 is used; the answer is the same
    whether the device keeps or flushes the subnormal d2."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    c = ref.weight_case()
    b, n, K = c["b"], c["n"], c["K"]
    Xd, id_, sd, pd = to_device(c["X"], dev), to_device(c["idx"], dev, np.int32), to_device(c["spfh"], dev), to_device(c["pairs"], dev, np.int32)
    whole, f = guarded((b, n, ref.SLOTS), float("nan"), torch.float32, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.so3_fpfh_f32(ptr(Xd), ptr(id_), None, ptr(sd), ptr(pd), ptr(f), K, b, n, st), "so3_fpfh_f32")
    assert last_kernel() == "k_fpfh"
    torch.cuda.synchronize()
    assert guards_intact(whole, float("nan")), "a guard was written"
    host.check_weight_case("abi", c, f.cpu().numpy())


# ---- indices from the library's own searches -------------------------------------------------------------------------------------
def test_indices_straight_from_the_searches(dev):
    """No margin condition here: the rows that break it are left out, every other row is exact."""
    import poseestimation_amd as pa
    rng = np.random.default_rng(3220)
    b, n = 2, 200
    Xn, Nn = (np.stack(a) for a in zip(*(ref.draw_sphere(rng, n) for _ in range(b))))
    X, Nr = to_device(Xn, dev), to_device(Nn, dev)
    lengths = to_device(np.array([200, 150]), dev, np.int64)
    _, idx = pa.knn_points(X, X, 12, lengths, lengths)                                               # int64, -1 rows past the length
    fpfh, spfh, pairs = pa.fpfh_features(X, Nr, idx, lengths=lengths, return_spfh=True)
    c = make_case("knn_points", Xn, Nn, idx.cpu().numpy(), np.array([200, 150], np.int32), strict=False)
    assert c["fpfh_rows"].mean() > 0.5
    host.check_case("knn_points", c, spfh.cpu().numpy(), pairs.cpu().numpy().astype(np.int32), fpfh.cpu().numpy())
    assert (fpfh[1, 150:] == 0).all() and (pairs[1, :150] == 11).all() and (pairs[0] == 11).all()
    auto = pa.fpfh_features(X, Nr, K=12, lengths=lengths, return_spfh=True)                          # idx=None: the same search, the same bits
    assert all(torch.equal(u, v) for u, v in zip(auto, (fpfh, spfh, pairs)))
    assert torch.equal(pa.fpfh_features(X, Nr), pa.fpfh_features(X, Nr, pa.knn_points(X, X, 16)[1]))       # the default K
    far = X.clone()
    far[:, 0] = 5.0                                                                                  # point 0 stands alone: its ball holds only itself
    ball = pa.query_ball_point(0.4, 16, far, far)
    centres = far.clone()
    centres[:, 1] = -5.0                                                                             # ... and centre 1 sees nothing: its slots hold N
    empty = pa.query_ball_point(0.4, 16, far, centres)
    assert (empty[:, 1] == n).all() and (ball[:, 0] == 0).all()
    for name, rows in (("query_ball_point", ball), ("an empty ball", empty)):
        fpfh, spfh, pairs = pa.fpfh_features(far, Nr, rows, return_spfh=True)
        c = make_case(name, far.cpu().numpy(), Nn, rows.cpu().numpy(), strict=False)
        assert c["fpfh_rows"].mean() > 0.3
        host.check_case(name, c, spfh.cpu().numpy(), pairs.cpu().numpy().astype(np.int32), fpfh.cpu().numpy())
    assert (pairs[:, 1] == 0).all() and (fpfh[:, 1] == 0).all()
    padded = ball.clone()                                                                            # the padding repeats the first hit: a multiset counts it
    as_set = torch.where((padded == padded[..., :1]) & (torch.arange(16, device=dev) > 0), torch.full_like(padded, -1), padded)
    assert (pa.fpfh_features(far, Nr, as_set, return_spfh=True)[2] <= pa.fpfh_features(far, Nr, padded, return_spfh=True)[2]).all()


def test_normals_from_estimate_normals_end_to_end(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(3230)
    X = to_device(np.stack([ref.draw_sphere(rng, 300)[0] for _ in range(2)]), dev)
    lengths = to_device(np.array([300, 120]), dev, np.int32)
    normals = pa.estimate_normals(X, 16, lengths)
    fpfh, spfh, pairs = pa.fpfh_features(X, normals, K=16, lengths=lengths, return_spfh=True)
    assert torch.isfinite(fpfh).all() and torch.isfinite(spfh).all() and (fpfh >= 0).all()
    live = (pairs > 0).double()[..., None]
    assert (host.sums_of(spfh.cpu().numpy()) - 100.0 * live.cpu().numpy()).__abs__().max() <= 1e-3
    total = host.sums_of(fpfh.cpu().numpy())
    assert np.abs(total[..., None] - [0.0, 100.0, 200.0]).min(-1).max() <= 1e-2 and (total[0] > 199).all() and (total[1, 120:] == 0).all()


# ---- properties ---------------------------------------------------------------------------------------------------------------
def test_power_of_two_on_the_device(dev, g32_cases):
    for name in ("sphere_257x16", "blob_257x16", "blob_300x64", "lattice_plane", "coincident", "mixed", "ragged", "moved_blob"):
        c = by_name(g32_cases, name)
        host.check_power_of_two("abi", c, abi_run(c, dev), lambda d: abi_run(d, dev))
    up, down, base = (by_name(g32_cases, "blob_257x16" + tag) for tag in ("_up", "_down", ""))
    assert same_bits(abi_run(up, dev), abi_run(base, dev)) and same_bits(abi_run(down, dev), abi_run(base, dev))


def test_repeatable_and_reversed(dev, g32_cases):
    c = cut(by_name(g32_cases, "blob_300x64"), 257, 20, 3)
    c["lengths"] = np.array([257, 100, 31], np.int32)
    c = make_case("three clouds", c["X"], c["normals"], c["idx"], c["lengths"])
    one = abi_run(c, dev)
    host.check_case("abi", c, *one)
    assert same_bits(one, abi_run(c, dev))                                                           # two calls, the same bits
    rev = dict(c, X=c["X"][::-1], normals=c["normals"][::-1], idx=c["idx"][::-1], lengths=c["lengths"][::-1])
    assert same_bits(one, tuple(o[::-1] for o in abi_run(rev, dev)))                                 # the reversed batch, per cloud


def test_the_nonfinite_cloud_is_contained(dev, g32_cases):
    c = by_name(g32_cases, "nonfinite")
    host.check_nonfinite_is_contained("abi", c, lambda d: abi_run(d, dev))
    host.check_nonfinite_is_contained("surface", c, lambda d: surface_run(d, dev))


def test_replay_from_a_captured_graph(dev, g32_cases):
    import poseestimation_amd as pa
    first, second = by_name(g32_cases, "sphere_257x16"), by_name(g32_cases, "blob_257x16")
    X, Nr, idx = to_device(first["X"], dev), to_device(first["normals"], dev), to_device(first["idx"], dev, np.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            pa.fpfh_features(X, Nr, idx, return_spfh=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fpfh, spfh, pairs = pa.fpfh_features(X, Nr, idx, return_spfh=True)
    X.copy_(to_device(second["X"], dev))
    Nr.copy_(to_device(second["normals"], dev))
    idx.copy_(to_device(second["idx"], dev, np.int32))
    graph.replay()
    torch.cuda.synchronize()
    host.check_case("replay", second, spfh.cpu().numpy(), pairs.cpu().numpy().astype(np.int32), fpfh.cpu().numpy())


def test_the_moved_copy_is_matched_to_itself(dev, g32_cases):
    """The descriptor's purpose: both poses give the same counts, and every point's nearest descriptor in the other pose is its own."""
    import poseestimation_amd as pa
    for fam in ("sphere", "blob"):
        c = by_name(g32_cases, "moved_" + fam)
        spfh, pairs, fpfh = surface_run(c, dev)
        host.check_case("surface", c, spfh, pairs, fpfh)
        assert np.array_equal(bits(spfh[0]), bits(spfh[1])) and np.array_equal(pairs[0], pairs[1]), fam
        f = to_device(fpfh, dev)
        match = pa.match_features(f[:1], f[1:], mutual=True)
        assert torch.equal(match, torch.arange(c["n"], device=dev)[None]), fam
        assert torch.equal(pa.match_features(f[1:], f[:1], mutual=False), match)


def test_the_requires_grad_warning_appears_once(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    rr._WARNED.discard("fpfh_features")
    X = torch.rand(1, 30, 3, device=dev, requires_grad=True)
    Nr = torch.nn.functional.normalize(torch.rand(1, 30, 3, device=dev), dim=-1)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a = pa.fpfh_features(X, Nr, K=4)
        b = pa.fpfh_features(X.detach(), Nr.requires_grad_(True), K=4)
    mine = [w for w in seen if "forward-only" in str(w.message)]
    assert len(mine) == 1 and issubclass(mine[0].category, RuntimeWarning) and not (a.requires_grad or b.requires_grad) and torch.equal(a, b)


def test_the_surface_refuses_bad_arguments_on_the_device(dev):
    import poseestimation_amd as pa
    X, Nr, idx = torch.zeros(2, 7, 3, device=dev), torch.zeros(2, 7, 3, device=dev), torch.zeros(2, 7, 4, dtype=torch.long, device=dev)
    shapes = r"fpfh_features: expected points and normals as \(B, N, 3\) floating-point tensors with 1 <= N <= 1048576, got"
    for bad_x, bad_n in ((X[..., :2], Nr[..., :2]), (X[0], Nr[0]), (X, Nr[:1]), (X, Nr[:, :5]), (X.long(), Nr), (X, Nr.int()), (X[:, :0], Nr[:, :0])):
        with pytest.raises(ValueError, match=shapes):
            pa.fpfh_features(bad_x, bad_n, idx)
    rows = r"fpfh_features: expected idx \(B, N, K\) \(int32 or int64\) on .* with B = 2, N = 7 and 1 <= K <= 64, got"
    for bad_i in (idx[0], idx[:1], idx[:, :5], idx.float(), idx.short(), idx[:, :, :0], torch.zeros(2, 7, 65, dtype=torch.long, device=dev)):
        with pytest.raises(ValueError, match=rows):
            pa.fpfh_features(X, Nr, bad_i)
    for k in (0, -1, 65, 3.0, True):
        with pytest.raises(ValueError, match="fpfh_features: expected an int 1 <= K <= 64, got"):
            pa.fpfh_features(X, Nr, K=k)
    for bad_l in (torch.tensor([1.0, 2.0], device=dev), torch.tensor([1, 2, 3], device=dev), torch.tensor([1, 2], dtype=torch.int16, device=dev)):
        with pytest.raises(ValueError, match=r"fpfh_features: expected lengths as a \(B,\) int32 or int64 tensor on .* for B = 2, got"):
            pa.fpfh_features(X, Nr, idx, lengths=bad_l)
    with pytest.raises(RuntimeError, match="HIP device only"):                                       # the indices, the lengths on the host
        pa.fpfh_features(X, Nr, idx.cpu())
    with pytest.raises(RuntimeError, match="HIP device only"):
        pa.fpfh_features(X, Nr, idx, lengths=torch.tensor([1, 2]))
    out = pa.fpfh_features(X, Nr, torch.zeros(2, 7, 64, dtype=torch.int32, device=dev))             # the limit itself is legal; coincident points: no pair
    assert out.shape == (2, 7, 33) and (out == 0).all()


# ---- the speed condition ----------------------------------------------------------------------------------------------------------
def torch_spelling(X, Nr, idx):
    """fpfh_features in torch: two (B,N,K,3) gathers, the Darboux frame, three bucketisations, a scatter_add into (B,N,33), a second
    (B,N,K,33) gather and the weighted mean.  idx holds valid indices only (knn_points on a full cloud), slot 0 the point itself."""
    import poseestimation_amd as pa
    b, n, K = idx.shape
    pj, nj = pa.knn_gather(X, idx), pa.knn_gather(Nr, idx)
    pi, ni = X[:, :, None, :], Nr[:, :, None, :].expand(b, n, K, 3)
    dp = pj - pi
    d2 = (dp * dp).sum(-1)
    pair = d2 > 0
    u = dp / d2.clamp_min(1e-38).sqrt()[..., None]
    a1, a2 = (ni * u).sum(-1), (nj * u).sum(-1)
    swap = (a1.abs() < a2.abs())[..., None]
    n1, n2, u = torch.where(swap, nj, ni), torch.where(swap, ni, nj), torch.where(swap, -u, u)
    f3 = torch.where(swap[..., 0], -a2, a1)
    v = torch.nn.functional.normalize(torch.cross(u, n1, dim=-1), dim=-1)
    w = torch.cross(n1, v, dim=-1)
    f2 = (v * n2).sum(-1)
    f1 = torch.atan2((w * n2).sum(-1), (n1 * n2).sum(-1))
    g = torch.stack([11 * (f1 + math.pi) / (2 * math.pi), 11 * (f2 + 1) / 2, 11 * (f3 + 1) / 2], -1)
    slot = g.floor().clamp(0, 10).long() + torch.arange(3, device=X.device) * 11                     # (B, N, K, 3)
    hist = torch.zeros(b, n, 33, device=X.device).scatter_add_(2, slot.reshape(b, n, K * 3), pair[..., None].expand(b, n, K, 3).reshape(b, n, K * 3).float())
    r = pair.sum(-1, keepdim=True).float()
    spfh = torch.where(r > 0, 100 * hist / r.clamp_min(1), torch.zeros_like(hist))
    wgt = torch.where(pair, 1 / d2.clamp_min(1e-38), torch.zeros_like(d2))
    mean = (wgt[..., None] * pa.knn_gather(spfh, idx)).sum(2) / wgt.sum(-1, keepdim=True).clamp_min(1e-38)
    return spfh + mean


def test_fpfh_is_not_slower_than_the_torch_spelling(dev):
    """32 x 1024, K = 16, idx given, HIP events, 5 warm-ups, the median of 20, in this process (support.median_ms): fpfh_features
    must not be slower than the gather / cross / atan2 / scatter_add spelling on the same device.  Measured on an MI355X: see
    profiles/fpfh_bench.txt."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    rng = np.random.default_rng(3299)
    b, n, K = 32, 1024, 16
    Xn, Nn = (np.stack(a) for a in zip(*(ref.draw_sphere(rng, n) for _ in range(b))))
    X, Nr = to_device(Xn, dev), to_device(Nn, dev)
    _, idx = pa.knn_points(X, X, K)
    ours, theirs = pa.fpfh_features(X, Nr, idx), torch_spelling(X, Nr, idx)
    assert (ours - theirs).abs().max(-1).values.median() <= 1e-3                                     # the spelling is the same descriptor (bins' edges apart)
    t_ours, t_torch = median_ms(lambda: pa.fpfh_features(X, Nr, idx)), median_ms(lambda: torch_spelling(X, Nr, idx))
    ratio = t_torch / t_ours
    REPORT_LINES.append("fpfh_features 32 x 1024, K = 16, idx given: %.3f ms, torch spelling (gathers, cross, atan2, scatter_add) %.3f ms, ratio %.2f"
                        % (t_ours, t_torch, ratio))
    print(REPORT_LINES[-1])
    assert ratio >= 1.0, (t_ours, t_torch)
