"""knn_points, knn_gather and knn_group (so3_knn_f32, so3_knn_bwd_f32) without a GPU: the boundary (header, binding table, exports,
argument validation, the Python names), the G28 fixture's own consistency, and the kernels' device functions compiled for the host
(tests/host_model/knn.cpp with SO3_HOST_MODEL) on G28.

The operation's arithmetic is a definition (include/so3proj.h), so everything is compared EXACTLY with the numpy restatement
(tests/knn_ref.py): dist2, idx and both gradients bit for bit, however the queries are dealt to the waves (Q = 1 and the shipped
values).  Beside the equality stand the two reasoned bounds against float64 that show the defined order to be an accurate one (the
excess of a neighbour's distance, 64 * 2^-24 on unit clouds, and (h + 4) * 2^-24 * sum |g| 2 |v| for a gradient chain of h terms; see
tests/knn_ref.py).  tests/test_gpu_knn.py imports the checks and runs them on the device."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import knn_ref as ref
from support import bits, boundary, build_host_model, lengths_of, np_ptr, on_own_thread
import three_nn_ref

NEW_SYMBOLS = {"so3_knn_f32": 12, "so3_knn_bwd_f32": 13}
SRC = os.path.join(ROOT, "tests", "host_model", "knn.cpp")
GRID_CAP = 8192                      # so3proj.hip: kThreeMaxGrid
WIDE_Q, NARROW_Q, WIDE_QUERIES, WIDE_TARGETS = 4, 1, 16384, 2048       # so3_device.h: kKnnWideQ, kKnnNarrowQ, kKnnWideQueries, kKnnWideTargets
SHIPPED_Q = sorted({WIDE_Q, NARROW_Q})


def queries_per_wave(b, n, m):
    return WIDE_Q if m >= WIDE_TARGETS and b * n >= WIDE_QUERIES else NARROW_Q


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_KNN_MAX_K (\d+)", raw).group(1)) == _lib.KNN_MAX_K == ref.MAX_K == 64


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error

    def fwd(b, n, m, k=4, X=p, Y=p, stride=None, dist2=p, idx=p):
        return lib.so3_knn_f32(X, Y, 3 * max(m, 0) if stride is None else stride, None, None, dist2, idx, k, b, n, m, None)

    def bwd(b, n, m, k=4, X=p, Y=p, idx=p, g=p, dX=p, dY=p):
        return lib.so3_knn_bwd_f32(X, Y, None, None, idx, g, dX, dY, k, b, n, m, None)

    assert fwd(0, 8, 8, X=None, Y=None, dist2=None, idx=None) == 0                            # B == 0: a no-op, whatever the pointers
    assert bwd(0, 8, 8, X=None, Y=None, idx=None, g=None, dX=None, dY=None) == 0
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert fwd(b, n, m) != 0 and err() == b"so3_knn_f32: B/N/M: invalid argument", (b, n, m, err())
        assert bwd(b, n, m) != 0 and err() == b"so3_knn_bwd_f32: B/N/M: invalid argument", (b, n, m, err())
    for k in (0, -1, 65, 2**31 - 1):
        assert fwd(4, 8, 8, k) != 0 and err() == b"so3_knn_f32: K: invalid argument", (k, err())
        assert bwd(4, 8, 8, k) != 0 and err() == b"so3_knn_bwd_f32: K: invalid argument", (k, err())
        assert fwd(0, 8, 8, k) != 0 and bwd(0, 8, 8, k) != 0                                  # K is checked before the no-op
    for stride in (1, 23, -24):
        assert fwd(4, 8, 8, stride=stride) != 0 and err() == b"so3_knn_f32: y_stride: invalid argument", (stride, err())
    for kw in ({"X": None}, {"Y": None}, {"idx": None}):                                      # dist2 alone may be null
        assert fwd(4, 8, 8, **kw) != 0 and err() == b"so3_knn_f32: null pointer: invalid argument", (kw, err())
    for kw in ({"X": None}, {"Y": None}, {"idx": None}, {"g": None}, {"dX": None, "dY": None}):      # dX or dY alone may be null
        assert bwd(4, 8, 8, **kw) != 0 and err() == b"so3_knn_bwd_f32: null pointer: invalid argument", (kw, err())


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("knn_points", "knn_gather", "knn_group"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    X, Y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for fn in (lambda: pa.knn_points(X, Y, 3), lambda: pa.knn_points(X, Y[0], 64), lambda: pa.knn_points(X.clone().requires_grad_(), Y, 1),
               lambda: pa.knn_points(X, Y, 2, torch.tensor([1, 2]), torch.tensor([3, 4])), lambda: pa.knn_group(2, Y, X, None)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    for k in (0, -1, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="1 <= K <= 64"):
            pa.knn_points(X, Y, k)
    with pytest.raises(ValueError, match="knn_gather: expected points"):
        pa.knn_gather(torch.zeros(2, 7), torch.zeros(2, 5, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="knn_gather: expected points"):
        pa.knn_gather(torch.zeros(2, 7, 4), torch.zeros(2, 5, 3))
    # knn_gather is plain torch: a -1 slot gives a row of zeros and takes no gradient
    pts = torch.arange(2 * 7 * 2, dtype=torch.float64).reshape(2, 7, 2).requires_grad_()
    idx = torch.tensor([[[0, 6, -1]], [[3, -1, -1]]])
    out = pa.knn_gather(pts, idx)
    assert out.shape == (2, 1, 3, 2) and torch.equal(out[0, 0, 1], pts[0, 6].detach()) and (out[0, 0, 2] == 0).all() and (out[1, 0, 1:] == 0).all()
    out.sum().backward()
    want = torch.zeros(2, 7, 2, dtype=torch.float64)
    want[0, 0] = want[0, 6] = want[1, 3] = 1
    assert torch.equal(pts.grad, want)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g28_cases():
    return ref.cases(ref.g28())


def gather_gradients(c, g):
    """Float64 torch autograd of the gather spelling  sum g_ik |x_i - y_idx[i,k]|^2  on the fixture's own indices, over the real slots."""
    X = torch.tensor(c["X"], dtype=torch.float64, requires_grad=True)
    Y = torch.tensor(c["Y"], dtype=torch.float64, requires_grad=True)
    idx = torch.as_tensor(c["idx"])
    batch = torch.arange(c["b"])[:, None, None]
    v = X[:, :, None, :] - Y[batch, idx.clamp(min=0)]
    d2 = (v * v).sum(-1)
    (torch.where(idx >= 0, d2, torch.zeros_like(d2)) * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return X.grad.numpy(), Y.grad.numpy()


def test_g28_is_self_consistent(g28_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    shapes = [(c["n"], c["m"], c["K"]) for c in g28_cases if c["family"] == "random" and c["lengths"] == "full"]
    assert shapes == ref.SHAPES and shapes == [(c["n"], c["m"], c["K"]) for c in g28_cases if c["lengths"] == "ragged"]
    assert {c["family"] for c in g28_cases} == set(ref.FAMILIES)
    for c in g28_cases:
        X, Y, xl, yl, K = c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["K"]
        both = np.concatenate([X, Y], 1)
        assert X.dtype == Y.dtype == np.float32 and np.isfinite(both).all() and np.linalg.norm(both, axis=-1).max() <= 1 + 1e-6, c["name"]
        d2, idx = ref.knn32(X, Y, K, xl, yl)
        assert np.array_equal(idx, c["idx"]) and np.array_equal(d2.view(np.uint32), c["dist2"].view(np.uint32)), c["name"]
        nl, ml = lengths_of(xl, c["b"], c["n"]), lengths_of(yl, c["b"], c["m"])
        if c["lengths"] == "ragged":
            assert c["b"] == ref.B_RAGGED and nl[0] == 0 and ml[1] == 0 and ml[2] == 1 and nl[1:].min() >= 1, c["name"]
            assert 1 < ml[3] < K or min(K, c["m"] + 1) <= 2, c["name"]
        for k in range(c["b"]):                                                      # the padding, slot by slot
            nb, r = (int(nl[k]), min(K, int(ml[k]))) if ml[k] > 0 else (0, 0)
            real = np.zeros((c["n"], K), bool)
            real[:nb, :r] = True
            assert (idx[k][~real] == -1).all() and (d2[k][~real] == 0).all() and (idx[k][real] >= 0).all() and (idx[k][real] < ml[k]).all(), c["name"]
            assert (np.diff(d2[k][:nb, :r], axis=-1) >= 0).all(), c["name"]
        assert ref.excess(X, Y, K, xl, yl, idx) <= ref.EXCESS, c["name"]                  # the defined d is an accurate one
        g = ref.upstream(c["b"], c["n"], K)
        dX, dY, bX, bY = ref.grad64(X, Y, xl, yl, idx, g)
        gX, gY = gather_gradients(c, g)
        assert np.abs(dX - gX).max() <= 1e-12 and np.abs(dY - gY).max() <= 1e-12 * max(1.0, np.abs(gY).max()), c["name"]
        if c["family"] == "subset":                      # X inside Y, every point of it twice in Y: the duplicate pair in index order
            assert (d2[..., :2] == 0).all() and np.array_equal(idx[..., 0], c["pick"]) and np.array_equal(idx[..., 1], c["pick"] + 57)
            assert (d2[..., 2] > 0).all()
        if c["family"] == "all_equal":
            assert np.array_equal(idx, np.broadcast_to(np.arange(K), idx.shape)) and (d2 == d2[..., :1]).all()
        if c["family"] == "lattice":                     # many exact ties, decided by index
            assert np.array_equal(X * 64, np.round(X * 64)) and np.array_equal(Y * 64, np.round(Y * 64))
            ties = d2[..., 1:] == d2[..., :-1]
            assert ties.mean() > 0.3 and (np.diff(idx, axis=-1)[ties] > 0).all()
        if c["family"] == "many_to_one":
            assert np.linalg.norm(X[0].astype(np.float64) - Y[0, 0], axis=1).max() <= 1e-2 and (idx[0, :, 0] == 0).all()
            assert (idx[0, :, 1:] > 0).all()                                           # dY[0]'s chain has exactly N hits


def test_the_small_last_hit_is_what_only_the_equality_sees():
    X, Y, g, g_small = ref.small_last_hit_case()
    _, idx = ref.knn32(X, Y, g.shape[-1])
    assert (idx[0, :, 0] == 0).all() and (idx[0, :, 1:] > 0).all()
    dX, dY, _, bY = ref.grad64(X, Y, None, None, idx, g_small)
    last = np.abs(np.float64(g_small[0, -1, 0]) * 2 * (Y[0, 0].astype(np.float64) - X[0, -1]))
    moved = last > 4 * np.spacing(np.abs(dY[0, 0]).astype(np.float32))
    assert (last < bY[0, 0] / 10).all() and moved.any()                          # far inside the bound, above the sum's ulp
    with_it = ref.grad32(X, Y, None, None, idx, g_small)[1]
    dropped = g_small.copy()
    dropped[0, -1, 0] = 0
    without = ref.grad32(X, Y, None, None, idx, dropped)[1]
    assert (np.abs(without[0, 0] - dY[0, 0]) <= bY[0, 0]).all()                       # a dropped hit stays inside the any-order bound ...
    assert (with_it[0, 0].view(np.uint32) != without[0, 0].view(np.uint32))[moved].all()      # ... and changes the bits


def test_knn32_at_k3_is_three_nn_on_g24():
    for c in three_nn_ref.cases(three_nn_ref.g24()):
        if c["kind"] != "disjoint":
            continue
        d3, i3, _ = three_nn_ref.three_nn(c["xyz1"], c["xyz2"])
        d2, idx = ref.knn32(c["xyz1"], c["xyz2"], 3)
        assert np.array_equal(idx, i3) and np.array_equal(d2.view(np.uint32), d3.view(np.uint32)), c["name"]


# ---- the checks, shared with tests/test_gpu_knn.py -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g28_expected():
    out = {}
    for c in ref.cases(ref.g28()):
        g = ref.upstream(c["b"], c["n"], c["K"])
        out[c["name"]] = (g,) + ref.grad32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["idx"], g)
    return out


def expected32(c):
    """(g, dX, dY) of a fixture case: ref.upstream and ref.grad32 through the fixture's own indices, computed once and shared."""
    return _g28_expected()[c["name"]]


def check_forward(name, got_d, got_i, want_d, want_i):
    got_i = np.asarray(got_i, np.int64)
    assert got_i.shape == want_i.shape and np.array_equal(got_i, want_i), (name, "idx", int((got_i != want_i).sum()), np.argwhere(got_i != want_i)[:4])
    if got_d is not None:
        got_d = np.asarray(got_d)
        assert got_d.dtype == np.float32 and np.array_equal(bits(got_d), bits(want_d)), (name, "dist2", int((bits(got_d) != bits(want_d)).sum()))


def check_gradients(name, X, Y, xl, yl, idx, g, got_dX, got_dY, want=None):
    """Both gradients bit for bit with grad32 through `idx`, and within the counted bound of float64."""
    want_dX, want_dY = ref.grad32(X, Y, xl, yl, idx, g) if want is None else want
    dX64, dY64, bX, bY = ref.grad64(X, Y, xl, yl, idx, g)
    for what, got, want32, want64, bound in (("dX", got_dX, want_dX, dX64, bX), ("dY", got_dY, want_dY, dY64, bY)):
        if got is None:
            continue
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == want32.shape, (name, what)
        assert (np.abs(got - want64) <= bound).all(), (name, what, np.abs(got - want64).max(), (np.abs(got - want64) - bound).max())
        assert np.array_equal(bits(got), bits(want32)), (name, what, int((bits(got) != bits(want32)).sum()), np.argwhere(bits(got) != bits(want32))[:4])


def check_against_g28(cases, run, label):
    """`run(case, g)` -> (dist2, idx, dX, dY) as numpy arrays, the gradients through the RETURNED indices with upstream gradient g."""
    for c in cases:
        g, dX, dY = expected32(c)
        got_d, got_i, got_dX, got_dY = run(c, g)
        check_forward(label + " " + c["name"], got_d, got_i, c["dist2"], c["idx"])
        check_gradients(label + " " + c["name"], c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["idx"], g, got_dX, got_dY, (dX, dY))


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "knn", SRC)
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.model_knn.argtypes = [P, P, I64, P, P, P, P, I32, I64, I32, I32, I32]
    lib.model_knn_bwd.argtypes = [P] * 8 + [I32, I64, I32, I32]
    lib.model_knn_queries_per_wave.argtypes = [I64, I32, I32]
    lib.model_knn.restype = lib.model_knn_bwd.restype = None
    return lib


def host_run(model, c, g, q):
    b, n, m, K = c["b"], c["n"], c["m"], c["K"]
    X, Y = np.ascontiguousarray(c["X"]), np.ascontiguousarray(c["Y"])
    xl = None if c["x_lengths"] is None else np.ascontiguousarray(c["x_lengths"], np.int32)
    yl = None if c["y_lengths"] is None else np.ascontiguousarray(c["y_lengths"], np.int32)
    d2, idx = np.full((b, n, K), np.nan, np.float32), np.full((b, n, K), -2, np.int32)
    dX, dY = np.full((b, n, 3), np.nan, np.float32), np.full((b, m, 3), np.nan, np.float32)
    model.model_knn(np_ptr(X), np_ptr(Y), 3 * m, np_ptr(xl), np_ptr(yl), np_ptr(d2), np_ptr(idx), K, b, n, m, q)
    model.model_knn_bwd(np_ptr(X), np_ptr(Y), np_ptr(xl), np_ptr(yl), np_ptr(idx), np_ptr(np.ascontiguousarray(g)), np_ptr(dX), np_ptr(dY), K, b, n, m)
    return d2, idx, dX, dY


def test_host_model_against_g28(model, g28_cases):
    assert {model.model_knn_queries_per_wave(b, n, m) for b, n, m in ((32, 1024, 1024), (32, 512, 128), (8, 4096, 4096))} == set(SHIPPED_Q)
    for b, n in ((1, 1), (1, WIDE_QUERIES - 1), (1, WIDE_QUERIES), (WIDE_QUERIES, 1), (3, 5461), (3, 5462)):
        for m in (1, WIDE_TARGETS - 1, WIDE_TARGETS, 1 << 20):
            assert model.model_knn_queries_per_wave(b, n, m) == queries_per_wave(b, n, m)
    for q in sorted({1} | set(SHIPPED_Q)):
        check_against_g28(g28_cases, lambda c, g: host_run(model, c, g, q), "host Q=%d" % q)
    c = next(c for c in g28_cases if c["name"] == "random_257x1025x20/ragged")
    g = expected32(c)[0]
    a, b_ = host_run(model, c, g, WIDE_Q), host_run(model, c, g, WIDE_Q)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b_))


def test_host_model_pads_what_never_received_a_candidate(model):
    """Non-finite coordinates: a NaN or +inf d fails every <, the slot reads (0, -1) and takes no gradient; the other rows are untouched."""
    rng = np.random.default_rng(2860)
    X, Y = ref._ball(rng, 1, 6), ref._ball(rng, 1, 9)
    Y[0, 2, 1], Y[0, 5, 0], X[0, 3, 2] = np.nan, np.inf, np.nan
    c = {"b": 1, "n": 6, "m": 9, "K": 8, "X": X, "Y": Y, "x_lengths": None, "y_lengths": None}
    want_d, want_i = ref.knn32(X, Y, 8)
    assert (want_i[0, 3] == -1).all() and (want_i[0, :3, 7] == -1).all() and (want_i[0, :3, :7] >= 0).all() and not np.isin(want_i, (2, 5)).any()
    g = ref.upstream(1, 6, 8)
    d2, idx, dX, dY = host_run(model, c, g, 1)
    check_forward("non-finite", d2, idx, want_d, want_i)
    want_dX, want_dY = ref.grad32(X, Y, None, None, want_i, g)
    assert np.array_equal(bits(dX), bits(want_dX)) and np.array_equal(bits(dY), bits(want_dY)) and (dX[0, 3] == 0).all() and (dY[0, [2, 5]] == 0).all()
