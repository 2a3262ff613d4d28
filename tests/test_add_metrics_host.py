"""ADD, ADD-S, the ADD-S gradient and the cloud diameter (so3_add_l2_f32, so3_add_s_fwd_f32, so3_add_s_bwd_f32, so3_cloud_diameter_f32)
without a GPU: the boundary (header, binding table, exports, argument validation), the G19 fixture's own consistency, and the kernels'
device functions compiled for the host (tests/host_model/add_metrics.cpp with SO3_HOST_MODEL) on G19.

TOLERANCES.  HOST_* are the largest absolute errors of the float32 host model against G19's float64 answers over every case of the
fixture (clouds on the unit sphere, poses about two units from the origin), measured here; the bound of each check, on the host and on
the GPU alike, is 4 x that value (the device's v_sqrt / v_rcp are 1-ulp approximations and it contracts a * b + c).  Gradients are the
largest |difference| of a dT entry; the reference gradient of ADD-S is float64 autograd of (1/N) sum |x_i - y_idx(i)| with the indices
the code under test returned, so ties cannot enter.  The ADD-S gradient's figure is set by the pose errors of 1e-3: e = x - y is formed
from two posed points of magnitude ~2.5, each within 1.5e-7, so its direction u = e / |e| carries a relative error of ~1e-4 per point
-- that is the price of the definition (a distance from coordinate differences of clouds posed by the same code), not of a kernel.
Indices are not compared for equality: for every point the float64 distance to the returned neighbour may exceed the float64 minimum by
at most the per-point bound.  tests/test_gpu_add_metrics.py imports the bounds from here; DESIGN.md section 7b quotes them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import add_metrics_ref as ref
from support import boundary, build_host_model, np_ptr

#                                 measured on the host       bound (4 x)
HOST_ADD = 1.24e-7;               ADD_TOL = 4 * HOST_ADD                 # noqa: E702
HOST_ADDS = 8.94e-8;              ADDS_TOL = 4 * HOST_ADDS               # noqa: E702
HOST_POINT = 4.73e-7;             POINT_TOL = 4 * HOST_POINT             # noqa: E702
HOST_DIAM = 1.37e-7;              DIAM_TOL = 4 * HOST_DIAM               # noqa: E702
HOST_ADD_GRAD = 4.93e-8;          ADD_GRAD_TOL = 4 * HOST_ADD_GRAD       # noqa: E702
HOST_ADDS_GRAD = 1.17e-5;         ADDS_GRAD_TOL = 4 * HOST_ADDS_GRAD     # noqa: E702

NEW_SYMBOLS = ["so3_add_l2_f32", "so3_add_s_fwd_f32", "so3_add_s_bwd_f32", "so3_cloud_diameter_f32"]
NEW_NAMES = ["compute_ADD_loss", "compute_ADD_S_loss", "cloud_diameter"]
SRC = os.path.join(ROOT, "tests", "host_model", "add_metrics.cpp")


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert len(_lib.SYMBOLS["so3_add_l2_f32"][1]) == len(_lib.SYMBOLS["so3_add_l1_f32"][1])           # "arguments as so3_add_l1_f32"
    assert _lib.SYMBOLS["so3_add_l2_f32"] == _lib.SYMBOLS["so3_add_l1_f32"]
    assert int(re.search(r"#define\s+SO3_ADD_S_MAX_N\s+(\d+)", raw).group(1)) == _lib.ADD_S_MAX_N      # the stated upper bound on N


def test_argument_validation_without_gpu(built_library):
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    # (leading pointers, the arguments between them and (B, N, stream))
    shapes = {"so3_add_l2_f32": (3, [None, None, None, 1.0]), "so3_add_s_fwd_f32": (4, [None, None, None]),
              "so3_add_s_bwd_f32": (4, [None, 1.0, p]), "so3_cloud_diameter_f32": (3, [])}
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        nptr, rest = shapes[name]
        nulls = [None if a is p else a for a in rest]
        assert fn(*([None] * nptr), *nulls, 0, 8, None) == 0, name                       # B == 0: a no-op, whatever the pointers
        assert fn(*([None] * nptr), *nulls, 4, 8, None) != 0 and b"null pointer" in err(), (name, err())
        for b, n in ((-1, 8), (2**62, 8), (4, 0), (4, -3), (4, 2**31 - 1)):
            assert fn(*([p] * nptr), *rest, b, n, None) != 0 and b": B/N" in err(), (name, b, n, err())
    assert lib.so3_add_s_fwd_f32(p, p, p, p, None, None, None, 4, _lib.ADD_S_MAX_N + 1, None) != 0 and b": B/N" in err()
    assert lib.so3_add_s_fwd_f32(p, p, p, None, None, None, None, 4, 8, None) != 0 and b"null pointer" in err()      # point_dist is required
    assert lib.so3_add_s_bwd_f32(p, p, p, None, None, 1.0, p, 4, 8, None) != 0 and b"null pointer" in err()          # so are the indices
    assert lib.so3_cloud_diameter_f32(p, None, p, 4, 8, None) != 0 and b"null pointer" in err()


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    for name in NEW_NAMES:
        assert name in pa.__all__ and hasattr(pa, name), name
    t, pts = torch.eye(4)[None].repeat(2, 1, 1), torch.zeros(2, 5, 3)
    for fn in (lambda: pa.compute_ADD_loss(t, t, pts), lambda: pa.compute_ADD_S_loss(t, t, pts), lambda: pa.compute_ADD_S_loss(t, t, pts[0]),
               lambda: pa.compute_ADD_loss(t, t, pts[0], use_batch_mean=False), lambda: pa.cloud_diameter(pts), lambda: pa.cloud_diameter(pts[0])):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g19():
    return ref.g19()


@pytest.fixture(scope="module")
def g19_cases(g19):
    return ref.cases(g19)


def test_g19_is_self_consistent(g19, g19_cases):
    assert os.path.getsize(ref.GOLDEN) <= 200 * 1024
    assert g19["pts"].dtype == np.float32 and g19["tgt"].dtype == np.float32 and g19["add"].dtype == np.float64 and g19["nearest"].dtype == np.int32
    assert {c["n"] for c in g19_cases} == set(ref.SIZES)
    assert {c["family"] for c in g19_cases} == set(ref.FAMILIES)
    assert {c["n"] for c in g19_cases if c["family"] == "haar"} == set(ref.SIZES)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    for c in g19_cases:
        tag = (c["family"], c["n"])
        assert np.linalg.norm(c["pts"].astype(np.float64), axis=-1).max() <= 1 + 1e-6, tag              # the unit sphere
        again = ref.answers(c["tgt"], c["tpred"], c["pts"])                                            # the stored answers are the restatement's
        for k, v in again.items():
            assert np.array_equal(v, c[k]) if k == "nearest" else np.allclose(v, c[k], rtol=0, atol=1e-14), (tag, k)
        assert (c["adds"] <= c["add"] * (1 + 2.0**-50)).all() and (c["adds"] <= c["diam"]).all(), tag      # (float64 rounding of two equal sums)
        # the closed-form gradients against float64 autograd: ADD through the definition, ADD-S through a cdist formulation
        tg, tp, p = T(c["tgt"]), T(c["tpred"]), T(c["pts"])
        assert np.allclose(ref.autograd_wrt_pred(ref.add64, tg, tp, p).numpy(), c["grad_add"], rtol=0, atol=1e-12), tag
        if c["family"] not in ("identical", "twofold", "duplicated"):      # (exact zeros and exact ties: cdist's subgradient is a convention there)
            assert np.allclose(ref.autograd_wrt_pred(ref.adds_cdist64, tg, tp, p).numpy(), c["grad_adds"], rtol=0, atol=1e-9), tag
        assert np.allclose(ref.autograd_wrt_pred(ref.adds_through_indices64, tg, tp, p, c["nearest"]).numpy(), c["grad_adds"], rtol=0, atol=1e-12), tag
        assert (c["grad_add"][:, 3] == 0).all() and (c["grad_adds"][:, 3] == 0).all()
        if c["family"] == "identical":
            assert (c["add"] == 0).all() and (c["adds"] == 0).all() and (c["nearest"] == np.arange(c["n"])).all(), tag
        if c["family"] == "twofold":
            assert (c["adds"] <= 1e-15).all() and (c["add"] > 0.1).all(), tag                          # ADD-S about 0 while ADD is large
        if c["family"] == "small_error":
            assert (np.abs(c["add"] - 1e-3) < 2e-4).all(), tag
        if c["family"] == "collinear":
            p64 = c["pts"][0].astype(np.float64)
            assert np.linalg.matrix_rank(p64 - p64[0], tol=1e-6) == 1, tag
        if c["family"] == "duplicated":
            assert len(np.unique(c["pts"][0], axis=0)) < c["n"], tag


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_host_model(tmp_path_factory, "add_metrics", SRC)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_run(model, c):
    """The host model on one case: dict of float32 / int32 results named as the fixture's answers."""
    b, n = c["b"], c["n"]
    tg, tp, pts = _c(c["tgt"]), _c(c["tpred"]), _c(c["pts"])
    B, N = ctypes.c_int64(b), ctypes.c_int32(n)
    out = {"point_dist": np.full((b, n), np.nan, np.float32), "nearest": np.full((b, n), -1, np.int32), "adds": np.full(b, np.nan, np.float32),
           "add": np.full(b, np.nan, np.float32), "diam": np.full(b, np.nan, np.float32), "grad_add": np.full((b, 4, 4), np.nan, np.float32),
           "grad_adds": np.full((b, 4, 4), np.nan, np.float32)}
    work = np.empty((b, n), np.float32)
    model.model_add_s_fwd(np_ptr(tg), np_ptr(tp), np_ptr(pts), np_ptr(out["point_dist"]), np_ptr(out["nearest"]), np_ptr(out["adds"]), B, N)
    model.model_cloud_diameter(np_ptr(pts), np_ptr(work), np_ptr(out["diam"]), B, N)
    model.model_add_s_bwd(np_ptr(tg), np_ptr(tp), np_ptr(pts), np_ptr(out["nearest"]), None, ctypes.c_float(1.0), np_ptr(out["grad_adds"]), B, N)
    model.model_add_l2(np_ptr(tg), np_ptr(tp), np_ptr(pts), np_ptr(out["add"]), np_ptr(out["grad_add"]), ctypes.c_float(1.0), B, N)
    return out


def figures(c, got):
    """Largest absolute errors of one case's results `got` (as host_run returns them) against the fixture: the quantities both test files bound."""
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    idx = got["nearest"]
    assert idx.min() >= 0 and idx.max() < c["n"]
    want_grad_s = ref.autograd_wrt_pred(ref.adds_through_indices64, T(c["tgt"]), T(c["tpred"]), T(c["pts"]), idx).numpy()
    return {"add": np.abs(got["add"] - c["add"]).max(), "adds": np.abs(got["adds"] - c["adds"]).max(),
            "point": np.abs(got["point_dist"] - c["point_dist"]).max(), "diam": np.abs(got["diam"] - c["diam"]).max(),
            "add_grad": np.abs(got["grad_add"] - c["grad_add"]).max(), "adds_grad": np.abs(got["grad_adds"] - want_grad_s).max(),
            "index_excess": ref.index_excess(c, idx).max()}


BOUNDS = {"add": ADD_TOL, "adds": ADDS_TOL, "point": POINT_TOL, "diam": DIAM_TOL, "add_grad": ADD_GRAD_TOL, "adds_grad": ADDS_GRAD_TOL,
          "index_excess": POINT_TOL}


def check_against_g19(cases, run, label):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as host_run does."""
    worst = {k: 0.0 for k in BOUNDS}
    rows = []
    for c in cases:
        f = figures(c, run(c))
        rows.append((c, f))
        print("%s %-12s N=%4d  " % (label, c["family"], c["n"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst[k], float(v))
    print(label, "worst:", "  ".join("%s %.3e (bound %.3e)" % (k, v, BOUNDS[k]) for k, v in worst.items()))
    for c, f in rows:
        for k, v in f.items():
            assert v <= BOUNDS[k], (label, c["family"], c["n"], k, v, BOUNDS[k])
    return worst


def test_host_model_against_g19(model, g19_cases):
    worst = check_against_g19(g19_cases, lambda c: host_run(model, c), "host")
    # the recorded HOST_* constants are this measurement (to the three digits they are written with)
    for k, host in (("add", HOST_ADD), ("adds", HOST_ADDS), ("point", HOST_POINT), ("diam", HOST_DIAM), ("add_grad", HOST_ADD_GRAD),
                    ("adds_grad", HOST_ADDS_GRAD)):
        assert worst[k] <= host * 1.005, (k, worst[k], host)


def test_host_model_exact_cases(model, g19_cases):
    """T_pred == T_gt: exact zeros and the identity index; the 2-fold cloud under a half turn: ADD-S exactly 0 in float32 too."""
    for c in g19_cases:
        got = host_run(model, c)
        if c["family"] == "identical":
            assert (got["add"] == 0).all() and (got["adds"] == 0).all() and (got["point_dist"] == 0).all(), c["n"]
            assert (got["nearest"] == np.arange(c["n"])).all(), c["n"]
            assert (got["grad_add"] == 0).all() and (got["grad_adds"] == 0).all()
        if c["family"] == "twofold":
            assert (got["adds"] == 0).all() and (got["add"] > 0.1).all(), c["n"]
        assert (got["grad_add"][:, 3] == 0).all() and (got["grad_adds"][:, 3] == 0).all()
