"""knn_points on the GPU: everything bit for bit against tests/knn_ref.py's knn32 / grad32, through the Python surface and through the
raw C ABI into NaN- and -2-pre-filled, guarded buffers -- G28, every launch geometry (K, M around the 64-candidate block, N around the
queries of one wave and of one work item for every shipped Q, a batch above the grid cap), the optional outputs, ragged lengths as
int32 and int64, K = 3 against so3_three_nn_f32, a shared target, autograd, the many-to-one chain, repeatability, a NaN cloud, replay
from a graph, knn_gather / knn_group, and the speed condition against the torch spelling."""
import ctypes

import numpy as np
import pytest
import torch

import knn_ref as ref
from support import bits, dev, guarded, guards_intact, ptr, to_device  # noqa: F401
import test_knn_host as host

pytestmark = pytest.mark.gpu
KERNELS = set()                     # the k_knn instantiations the raw calls ran


@pytest.fixture(scope="module")
def g28_cases():
    return ref.cases(ref.g28())


def abi_run(X, Y, K, xl, yl, g, dev, shared=False):
    """The raw C ABI into guarded buffers, then again with each optional output left out.  -> (dist2, idx, dX, dY) numpy."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n, m = X.shape[0], X.shape[1], Y.shape[-2]
    Xd, Yd, xld, yld, gd = to_device(X, dev), to_device(Y, dev), to_device(xl, dev, np.int32), to_device(yl, dev, np.int32), to_device(g, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spec = {"dist2": ((b, n, K), np.nan, torch.float32), "idx": ((b, n, K), -2, torch.int32), "dX": ((b, n, 3), np.nan, torch.float32),
            "dY": ((b, m, 3), np.nan, torch.float32)}
    whole, out = {}, {}
    for k, (shape, fill, dtype) in spec.items():
        whole[k], out[k] = guarded(shape, fill, dtype, dev)
    stride = 0 if shared else 3 * m
    _lib.check(lib.so3_knn_f32(ptr(Xd), ptr(Yd), stride, ptr(xld), ptr(yld), ptr(out["dist2"]), ptr(out["idx"]), K, b, n, m, st), "so3_knn_f32")
    kernel = lib.so3_last_kernel().decode()
    assert kernel == "k_knn<%d>" % host.queries_per_wave(b, n, m), kernel
    KERNELS.add(kernel)
    alone = torch.full((b, n, K), -2, dtype=torch.int32, device=dev)                        # dist2 left out
    _lib.check(lib.so3_knn_f32(ptr(Xd), ptr(Yd), stride, ptr(xld), ptr(yld), None, ptr(alone), K, b, n, m, st), "so3_knn_f32")
    assert torch.equal(alone, out["idx"])
    if shared:
        Yd = Yd.expand(b, m, 3).contiguous()
    if g is not None:
        args = (ptr(Xd), ptr(Yd), ptr(xld), ptr(yld), ptr(out["idx"]), ptr(gd))
        _lib.check(lib.so3_knn_bwd_f32(*args, ptr(out["dX"]), ptr(out["dY"]), K, b, n, m, st), "so3_knn_bwd_f32")
        assert lib.so3_last_kernel().decode() == "k_knn_bwd"
        for only in ("dX", "dY"):                                                           # each gradient alone
            one = torch.full(spec[only][0], np.nan, device=dev)
            _lib.check(lib.so3_knn_bwd_f32(*args, ptr(one) if only == "dX" else None, ptr(one) if only == "dY" else None, K, b, n, m, st),
                       "so3_knn_bwd_f32")
            assert torch.equal(one, out[only]), only
    torch.cuda.synchronize()
    for k, (shape, fill, dtype) in spec.items():
        assert guards_intact(whole[k], fill), k
    res = {k: v.cpu().numpy() for k, v in out.items()}
    return res["dist2"], res["idx"], (res["dX"] if g is not None else None), (res["dY"] if g is not None else None)


def surface_run(X, Y, K, xl, yl, g, dev, long_lengths=False):
    import poseestimation_amd as pa
    ltype = np.int64 if long_lengths else np.int32
    Xd, Yd = to_device(X, dev).requires_grad_(), to_device(Y, dev).requires_grad_()
    dist2, idx = pa.knn_points(Xd, Yd, K, to_device(xl, dev, ltype), to_device(yl, dev, ltype))
    assert dist2.dtype == torch.float32 and idx.dtype == torch.int64 and dist2.shape == idx.shape == (X.shape[0], X.shape[1], K)
    assert not idx.requires_grad and dist2.requires_grad
    dist2.backward(to_device(g, dev))
    return dist2.detach().cpu().numpy(), idx.cpu().numpy(), Xd.grad.cpu().numpy(), Yd.grad.cpu().numpy()


def check_case(name, X, Y, K, xl, yl, dev, surface=False, long_lengths=False):
    """A fresh case through one route against knn32 and grad32 (computed here, once)."""
    want_d, want_i = ref.knn32(X, Y, K, xl, yl)
    g = ref.upstream(X.shape[0], X.shape[1], K)
    run = (lambda: surface_run(X, Y, K, xl, yl, g, dev, long_lengths)) if surface else (lambda: abi_run(X, Y, K, xl, yl, g, dev))
    d2, idx, dX, dY = run()
    host.check_forward(name, d2, idx, want_d, want_i)
    host.check_gradients(name, X, Y, xl, yl, want_i, g, dX, dY)
    return d2, idx, dX, dY


# ---- G28 --------------------------------------------------------------------------------------------------------------------
def test_g28_through_the_c_abi(dev, g28_cases):
    host.check_against_g28(g28_cases, lambda c, g: abi_run(c["X"], c["Y"], c["K"], c["x_lengths"], c["y_lengths"], g, dev), "abi")


def test_g28_through_the_python_surface(dev, g28_cases):
    host.check_against_g28(g28_cases, lambda c, g: surface_run(c["X"], c["Y"], c["K"], c["x_lengths"], c["y_lengths"], g, dev), "surface")
    ragged = [c for c in g28_cases if c["lengths"] == "ragged"]
    host.check_against_g28(ragged, lambda c, g: surface_run(c["X"], c["Y"], c["K"], c["x_lengths"], c["y_lengths"], g, dev, True), "surface int64")


# ---- every launch geometry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_every_k_and_every_candidate_block(dev, b):
    rng = np.random.default_rng(2810 + b)
    for K in (1, 2, 3, 4, 16, 63, 64):
        for m in (1, 63, 64, 65, 127, 128, 129):
            X, Y = ref._ball(rng, b, 9), ref._ball(rng, b, m)
            check_case("B=%d K=%d M=%d" % (b, K, m), X, Y, K, None, None, dev, surface=(K + m) % 2 == 0)


def test_n_around_a_wave_and_a_work_item_for_every_shipped_q(dev):
    """N one below, at and one above the queries of one wave (Q) and of one work item (4 Q), with B chosen so that the dispatch rule
    picks each shipped Q; ragged lengths on the way.  Every instantiation must have run."""
    rng = np.random.default_rng(2820)
    KERNELS.clear()
    for q in host.SHIPPED_Q:
        for n in sorted({max(1, q - 1), q, q + 1, 4 * q - 1, 4 * q, 4 * q + 1}):
            wide = q == host.WIDE_Q                              # the wide rule needs a long target: one shared by the batch
            b, m = (-(-host.WIDE_QUERIES // n), host.WIDE_TARGETS) if wide else (2, 70)
            assert host.queries_per_wave(b, n, m) == q
            X, Y = ref._ball(rng, b, n), (ref._ball(rng, m) if wide else ref._ball(rng, b, m))
            xl, yl = rng.integers(0, n + 1, b).astype(np.int32), rng.integers(0, m + 1, b).astype(np.int32)
            want_d, want_i = ref.knn32(X, Y, 5, xl, yl)
            d2, idx, _, _ = abi_run(X, Y, 5, xl, yl, None, dev, shared=wide)
            host.check_forward("Q=%d N=%d B=%d" % (q, n, b), d2, idx, want_d, want_i)
    b, n, m = 410, 40, host.WIDE_TARGETS + 1                     # three wide work items per cloud
    assert host.queries_per_wave(b, n, m) == host.WIDE_Q
    X, Y, yl = ref._ball(rng, b, n), ref._ball(rng, m), rng.integers(0, m + 1, b).astype(np.int32)
    host.check_forward("wide, N=40", *abi_run(X, Y, 7, None, yl, None, dev, shared=True)[:2], *ref.knn32(X, Y, 7, None, yl))
    assert KERNELS == {"k_knn<%d>" % q for q in host.SHIPPED_Q}, KERNELS
    for n, b in ((257, 3), (600, 28)):                           # several work items per cloud on both sides of the rule, with gradients
        X, Y = ref._ball(rng, b, n), ref._ball(rng, b, 130)
        check_case("N=%d B=%d" % (n, b), X, Y, 7, rng.integers(0, n + 1, b).astype(np.int32), rng.integers(0, 131, b).astype(np.int32), dev)


def test_a_batch_above_the_grid_cap(dev):
    rng = np.random.default_rng(2830)
    b = host.GRID_CAP + 3
    X, Y = ref._ball(rng, b, 5), ref._ball(rng, b, 12)
    xl, yl = rng.integers(0, 6, b).astype(np.int32), rng.integers(0, 13, b).astype(np.int32)
    assert -(-5 // (4 * host.queries_per_wave(b, 5, 12))) * b > host.GRID_CAP
    check_case("beyond the grid", X, Y, 4, xl, yl, dev)


def test_padding_and_k_above_m(dev):
    rng = np.random.default_rng(2840)
    X, Y = ref._ball(rng, 3, 20), ref._ball(rng, 3, 5)
    d2, idx, dX, dY = check_case("K > M", X, Y, 9, np.array([20, 0, 7], np.int32), np.array([5, 3, 0], np.int32), dev)
    assert (idx[0, :, 5:] == -1).all() and (idx[0, :, :5] >= 0).all() and (idx[1:] == -1).all() and (d2[1:] == 0).all()
    assert (dX[1:] == 0).all() and (dY[1:] == 0).all()


def test_the_backward_scan_around_its_in_flight_group(dev):
    """k_knn_bwd's dY scan reads a cloud's n_b * K index entries in groups of 64 * kChamferScanBlocks = 512: one below, at and one above a
    group, and the same around two groups through a ragged n_b."""
    rng = np.random.default_rng(2845)
    for n, K in ((73, 7), (8, 64), (171, 3)):
        assert n * K in (511, 512, 513)
        X, Y = ref._ball(rng, 2, n), ref._ball(rng, 2, 70)
        check_case("n_b * K = %d" % (n * K), X, Y, K, None, None, dev)
    X, Y = ref._ball(rng, 3, 260), ref._ball(rng, 3, 90)
    xl = np.array([255, 256, 257], np.int32)                     # n_b * 4 = 1020, 1024, 1028 in a (3, 260, 4) index tensor
    check_case("n_b * K around two groups", X, Y, 4, xl, None, dev)


def test_the_surface_refuses_bad_shapes_lengths_and_k_on_the_device(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import _lib
    X, Y = torch.zeros(2, 5, 3, device=dev), torch.zeros(2, 7, 3, device=dev)
    limit = "1 <= N, M <= %d" % _lib.ADD_S_MAX_N
    for bad_x, bad_y in ((X[..., :2], Y), (X, Y[..., :2]), (X[None], Y), (X[0], Y), (X, Y[:1]), (X, torch.zeros(3, 7, 3, device=dev)),
                         (X[:, :0], Y), (X, Y[:, :0]), (X, Y[0, :0]), (X, Y[None])):
        with pytest.raises(ValueError, match=r"knn_points: expected a source \(B, N, 3\) and a target \(B, M, 3\) or \(M, 3\) with " + limit) as info:
            pa.knn_points(bad_x, bad_y, 3)
        assert str(tuple(bad_x.shape)) in str(info.value) and str(tuple(bad_y.shape)) in str(info.value)
    for name, xl, yl in (("x_lengths", torch.tensor([1.0, 2.0], device=dev), None), ("x_lengths", torch.tensor([1, 2, 3], device=dev), None),
                         ("y_lengths", None, torch.tensor([[1, 2]], device=dev)), ("y_lengths", None, torch.tensor([1, 2], dtype=torch.int16, device=dev)),
                         ("y_lengths", torch.tensor([1, 2], device=dev), torch.tensor(3, device=dev))):
        with pytest.raises(ValueError, match=r"knn_points: expected %s as a \(B,\) int32 or int64 tensor on .* for B = 2, got" % name):
            pa.knn_points(X, Y, 3, xl, yl)
    with pytest.raises(RuntimeError, match="HIP device only"):                # lengths on the host
        pa.knn_points(X, Y, 3, torch.tensor([1, 2]))
    for k in (0, -1, 65, 3.0, None):
        with pytest.raises(ValueError, match="knn_points: expected an int 1 <= K <= 64, got"):
            pa.knn_points(X, Y, k)
        with pytest.raises(ValueError, match="1 <= K <= 64"):
            pa.knn_group(k, Y, X, None)
    for bad in ((torch.zeros(2, 7, device=dev), torch.zeros(2, 5, 3, dtype=torch.long, device=dev)),
                (torch.zeros(2, 7, 4, device=dev), torch.zeros(2, 5, 3, device=dev)), (torch.zeros(3, 7, 4, device=dev), torch.zeros(2, 5, 3, dtype=torch.long, device=dev))):
        with pytest.raises(ValueError, match=r"knn_gather: expected points \(B, M, C\) and idx \(B, N, K\)"):
            pa.knn_gather(*bad)
    d2, idx = pa.knn_points(X, Y, 64)                             # the limits themselves are legal: K = 64 > M
    assert d2.shape == idx.shape == (2, 5, 64) and (idx[..., 7:] == -1).all() and (idx[..., :7] >= 0).all()


def test_k3_is_three_nn_and_a_shared_target_is_the_expanded_one(dev):
    from poseestimation_amd import _lib
    import poseestimation_amd as pa
    lib = _lib.load()
    rng = np.random.default_rng(2850)
    b, n, m = 3, 300, 77
    X, Y = to_device(ref._ball(rng, b, n), dev), to_device(ref._ball(rng, b, m), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d3, i3 = torch.empty(b, n, 3, device=dev), torch.empty(b, n, 3, dtype=torch.int32, device=dev)
    _lib.check(lib.so3_three_nn_f32(ptr(X), ptr(Y), ptr(d3), ptr(i3), None, b, n, m, st), "so3_three_nn_f32")
    d2, idx = pa.knn_points(X, Y, 3)
    assert torch.equal(idx, i3.long()) and torch.equal(d2.view(torch.int32), d3.view(torch.int32))
    ds, is_ = pa.knn_points(X, Y[0], 6)                                                  # one shared target
    de, ie = pa.knn_points(X, Y[:1].expand(b, m, 3), 6)
    assert torch.equal(is_, ie) and torch.equal(ds.view(torch.int32), de.view(torch.int32))
    want_d, want_i = ref.knn32(X.cpu().numpy(), Y[0].cpu().numpy(), 6)
    host.check_forward("shared", ds.cpu().numpy(), is_.cpu().numpy(), want_d, want_i)
    Xg = X.clone().requires_grad_()                                                      # the source's gradient through a shared target
    pa.knn_points(Xg, Y[0], 6)[0].sum().backward()
    Xe = X.clone().requires_grad_()
    pa.knn_points(Xe, Y[:1].expand(b, m, 3).contiguous(), 6)[0].sum().backward()
    assert torch.equal(Xg.grad, Xe.grad)
    with pytest.raises(ValueError, match="expand"):
        pa.knn_points(X, Y[0].clone().requires_grad_(), 6)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def test_autograd(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2860)
    b, n, m, K = 2, 70, 90, 5
    Xn, Yn = ref._ball(rng, b, n), ref._ball(rng, b, m)
    g = ref.upstream(b, n, K)
    _, want_i = ref.knn32(Xn, Yn, K)
    want_dX, want_dY = ref.grad32(Xn, Yn, None, None, want_i, g)
    _, _, abi_dX, abi_dY = abi_run(Xn, Yn, K, None, None, g, dev)
    X, Y = to_device(Xn, dev).requires_grad_(), to_device(Yn, dev).requires_grad_()
    wide = torch.zeros(b, n, 2 * K, device=dev)
    wide[..., ::2] = to_device(g, dev)
    d2, idx = pa.knn_points(X, Y, K)
    gX, gY = torch.autograd.grad(d2, (X, Y), wide[..., ::2])                              # a strided upstream gradient; the C ABI's bits
    assert np.array_equal(bits(gX.cpu().numpy()), bits(abi_dX)) and np.array_equal(bits(gY.cpu().numpy()), bits(abi_dY))
    assert np.array_equal(bits(abi_dX), bits(want_dX)) and np.array_equal(bits(abi_dY), bits(want_dY))
    Yo = to_device(Yn, dev).requires_grad_()                                                     # only Y requires grad
    d2o, _ = pa.knn_points(to_device(Xn, dev), Yo, K)
    d2o.backward(to_device(g, dev))
    assert torch.equal(Yo.grad, gY)
    X64, Y64 = to_device(Xn, dev).double().requires_grad_(), to_device(Yn, dev).double().requires_grad_()      # float64 clouds: results in their dtype
    d64, i64 = pa.knn_points(X64, Y64, K)
    d64.backward(to_device(g, dev).double())
    assert d64.dtype == X64.grad.dtype == Y64.grad.dtype == torch.float64 and torch.equal(i64, idx)
    assert torch.equal(X64.grad, gX.double()) and torch.equal(Y64.grad, gY.double()) and torch.equal(d64, d2.detach().double())
    Xd = to_device(Xn, dev).requires_grad_()
    d2d, _ = pa.knn_points(Xd, Y, K)
    (first,) = torch.autograd.grad(d2d.sum(), Xd, create_graph=True)
    assert not first.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        up = torch.ones_like(d2d).requires_grad_()
        torch.autograd.grad(pa.knn_points(Xd, Y, K)[0], Xd, up, create_graph=True)


def test_the_many_to_one_chain_and_its_small_last_hit(dev):
    X, Y, g, g_small = ref.small_last_hit_case()
    K = g.shape[-1]
    _, want_i = ref.knn32(X, Y, K)
    for name, up in (("many-to-one", g), ("many-to-one, a small last hit", g_small)):
        d2, idx, dX, dY = abi_run(X, Y, K, None, None, up, dev)
        assert np.array_equal(idx, want_i) and (idx[0, :, 0] == 0).all()
        host.check_gradients(name, X, Y, None, None, want_i, up, dX, dY)


def test_repeatable_reversed_and_isolated(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2870)
    b, n, m, K = 5, 130, 200, 20
    Xn, Yn = ref._ball(rng, b, n), ref._ball(rng, b, m)
    xl, yl = to_device(rng.integers(1, n + 1, b), dev, np.int32), to_device(rng.integers(1, m + 1, b), dev, np.int32)
    g = to_device(ref.upstream(b, n, K), dev)

    def run(X, Y, xl, yl, g):
        X, Y = X.clone().requires_grad_(), Y.clone().requires_grad_()
        d2, idx = pa.knn_points(X, Y, K, xl, yl)
        d2.backward(g)
        return d2.detach(), idx, X.grad, Y.grad

    X, Y = to_device(Xn, dev), to_device(Yn, dev)
    one, two = run(X, Y, xl, yl, g), run(X, Y, xl, yl, g)
    assert all(torch.equal(u, v) for u, v in zip(one, two))                               # two calls, the same bits
    rev = run(X.flip(0), Y.flip(0), xl.flip(0), yl.flip(0), g.flip(0))
    assert all(torch.equal(u, v.flip(0)) for u, v in zip(one, rev))                       # the reversed batch, per cloud
    Xb, Yb = X.clone(), Y.clone()
    Xb[2], Yb[2, 5] = float("nan"), float("nan")
    bad = run(Xb, Yb, xl, yl, g)
    keep = [0, 1, 3, 4]
    assert all(torch.equal(u[keep], v[keep]) for u, v in zip(one, bad))                   # a NaN cloud changes no other cloud
    assert (bad[1][2] == -1).all() and (bad[0][2] == 0).all()


def test_replay_from_a_captured_graph(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2880)
    b, n, m, K = 2, 100, 150, 8
    X, Y = to_device(ref._ball(rng, b, n), dev).requires_grad_(), to_device(ref._ball(rng, b, m), dev).requires_grad_()
    g = to_device(ref.upstream(b, n, K), dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(pa.knn_points(X, Y, K)[0], (X, Y), g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d2, idx = pa.knn_points(X, Y, K)
        gX, gY = torch.autograd.grad(d2, (X, Y), g)
    Xn, Yn = ref._ball(rng, b, n), ref._ball(rng, b, m)
    with torch.no_grad():
        X.copy_(to_device(Xn, dev))
        Y.copy_(to_device(Yn, dev))
    graph.replay()
    torch.cuda.synchronize()
    want_d, want_i = ref.knn32(Xn, Yn, K)
    host.check_forward("replay", d2.detach().cpu().numpy(), idx.cpu().numpy(), want_d, want_i)
    host.check_gradients("replay", Xn, Yn, None, None, want_i, g.cpu().numpy(), gX.cpu().numpy(), gY.cpu().numpy())


def test_knn_gather_and_knn_group(dev):
    import poseestimation_amd as pa
    rng = np.random.default_rng(2890)
    b, n, s, K, d = 2, 120, 30, 6, 5
    xyz, new_xyz, pts = to_device(ref._ball(rng, b, n), dev), to_device(ref._ball(rng, b, s), dev), to_device(rng.standard_normal((b, n, d)), dev)
    d2, idx = pa.knn_points(new_xyz, xyz, K, None, to_device(np.array([n, 3]), dev, np.int64))          # cloud 1: three real slots, three of -1
    got = pa.knn_gather(pts, idx)
    want = pts[torch.arange(b, device=dev)[:, None, None], idx.clamp(min=0)] * (idx >= 0)[..., None]
    assert got.shape == (b, s, K, d) and torch.equal(got, want) and (got[1, :, 3:] == 0).all() and (idx[1, :, 3:] == -1).all()
    _, full = pa.knn_points(new_xyz, xyz, K)
    assert torch.equal(pa.knn_group(K, xyz, new_xyz, pts), pa.group_points(xyz, new_xyz, pts, full))
    cf = pa.knn_group(K, xyz, new_xyz, pts.transpose(1, 2).contiguous(), channels_first=True)
    assert cf.shape == (b, 3 + d, K, s) and torch.equal(cf, pa.group_points(xyz, new_xyz, pts.transpose(1, 2).contiguous(), full, channels_first=True))
    assert torch.equal(pa.group_points(xyz, new_xyz, pts, idx)[1, :, 3:], torch.zeros(s, K - 3, 3 + d, device=dev))      # -1 is an empty slot


# ---- the speed condition ----------------------------------------------------------------------------------------------------------
def test_faster_than_the_torch_spelling(dev):
    """32 x 1024 <- 1024, K = 16, forward plus backward, HIP events, 5 warm-ups, the median of 20, in this process: knn_points must not
    be slower than (x[:, :, None] - y[:, None]).square().sum(-1).topk(K, largest=False).  Measured on an MI355X: see
    profiles/knn_bench.txt."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    rng = np.random.default_rng(2899)
    b, n, m, K = 32, 1024, 1024, 16
    X, Y = to_device(ref._ball(rng, b, n), dev).requires_grad_(), to_device(ref._ball(rng, b, m), dev).requires_grad_()
    g = torch.rand(b, n, K, device=dev)

    def ours():
        return torch.autograd.grad(pa.knn_points(X, Y, K)[0], (X, Y), g)

    def spelling():
        d = (X[:, :, None] - Y[:, None]).square().sum(-1).topk(K, largest=False)[0]
        return torch.autograd.grad(d, (X, Y), g)

    def median_ms(fn):
        times = []
        for rep in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    t_ours, t_torch = median_ms(ours), median_ms(spelling)
    ratio = t_torch / t_ours
    REPORT_LINES.append("knn_points 32 x 1024 <- 1024, K = 16, forward + backward: %.3f ms, torch spelling %.3f ms, ratio %.2f" % (t_ours, t_torch, ratio))
    print(REPORT_LINES[-1])
    assert ratio >= 1.0, (t_ours, t_torch)
