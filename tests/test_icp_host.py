"""nearest_neighbors and icp_align (so3_nearest_f32, so3_icp_workspace_bytes, so3_icp_f32) without a GPU: the boundary (header, binding
table, exports, argument validation, the Python names), the G21 fixture's own consistency, and the kernels' device functions compiled
for the host (tests/host_model/icp.cpp with SO3_HOST_MODEL) on G21.

The search is discontinuous, so nothing compares indices or whole trajectories for equality, except where the answer is far from a tie
(a point that is IN the target; the converged exact cases, whose runner-up is 0.12 away).  Clouds are of unit radius.
  search   for every point, (float64 distance to the returned neighbour) - (float64 minimum), and |dist - float64 minimum|
  step     the returned `nearest` and the float64 distances to those neighbours give the trimmed weights (no such distance lies within
           icp_ref.MARGIN of max_distance: re-asserted here); rigid_align_ref on those pairs gives the pose to compare with:
           R  max |dR|,   T  max |dt| / max(1, |pbar|_inf, |qbar|_inf)   (test_rigid_align_host.py's norms),   rmse  |d rmse|;
           inliers are compared exactly.  Cases whose rotation is not unique (fewer than three inliers, two sources on one target)
           are held to properties: finite, R a rotation.  An empty inlier set keeps the pose bit for bit, rmse 0, inliers 0.
  converge after 20 iterations  conv_R max |R - R_gt|,  conv_T max |t - t_gt|,  conv_rmse the last rmse,  nearest == the permutation
  noise    rmse never rises by more than RMSE_TOL (untrimmed), one more float64 step from the returned pose moves it by less than
           R_TOL / T_TOL, R is a rotation.

TOLERANCES.  HOST_* are the largest errors of the float32 host model (at 256 compute units) over G21, measured here; the bound of
each check, on the host and on the GPU alike, is 4 x that value (the device's v_rcp / v_sqrt are 1-ulp approximations and it
contracts a * b + c).  ROT_TOL = 6 * R_TOL as in test_rigid_align_host.py.  CONDITION, not a measurement: on the offset families
4 x the measured R error must stay below 1e-5 -- above that the pivot is wrong.  tests/test_gpu_icp.py imports the bounds and the
checks; DESIGN.md section 7d quotes them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import icp_ref as ref
import rigid_align_ref as ra
from support import boundary, build_host_model, np_ptr, on_own_thread

#                                 measured on the host       bound (4 x)
HOST_SEARCH = 9.795e-8;           SEARCH_TOL = 4 * HOST_SEARCH           # noqa: E702
HOST_R = 2.181e-6;                R_TOL = 4 * HOST_R                     # noqa: E702
HOST_T = 1.115e-6;                T_TOL = 4 * HOST_T                     # noqa: E702
HOST_RMSE = 9.355e-6;             RMSE_TOL = 4 * HOST_RMSE               # noqa: E702
HOST_CONV_R = 1.645e-7;           CONV_R_TOL = 4 * HOST_CONV_R           # noqa: E702
HOST_CONV_T = 5.960e-8;           CONV_T_TOL = 4 * HOST_CONV_T           # noqa: E702
HOST_CONV_RMSE = 1.625e-7;        CONV_RMSE_TOL = 4 * HOST_CONV_RMSE     # noqa: E702
ROT_TOL = 6 * R_TOL
# The host model on the geometry case G4 of tests/search_geometry_ref.py (64 CUs + 37 clouds of 12 points, weighted, trimmed, two
# iterations), measured in tests/test_search_geometry_host.py: among 16 421 small clouds the worst conditioned that still counts as
# unique ((s2 + s3) / s1 = 0.16, s3 / s1 = 0.003) is beyond G21's figures, so for that shape R and T are bounded by 4 x these.
HOST_R_G4 = 9.868e-6;             R_TOL_G4 = 4 * HOST_R_G4               # noqa: E702
HOST_T_G4 = 5.085e-6;             T_TOL_G4 = 4 * HOST_T_G4               # noqa: E702
MEASURED = {"search": HOST_SEARCH, "R": HOST_R, "T": HOST_T, "rmse": HOST_RMSE, "conv_R": HOST_CONV_R, "conv_T": HOST_CONV_T,
            "conv_rmse": HOST_CONV_RMSE}

NEW_SYMBOLS = {"so3_nearest_f32": 9, "so3_icp_workspace_bytes": 2, "so3_icp_f32": 18}
SRC = os.path.join(ROOT, "tests", "host_model", "icp.cpp")
CUS = 256                           # the device the host model stands in for


def bounds():
    return {"search": SEARCH_TOL, "dist": SEARCH_TOL, "R": R_TOL, "T": T_TOL, "rmse": RMSE_TOL, "conv_R": CONV_R_TOL, "conv_T": CONV_T_TOL,
            "conv_rmse": CONV_RMSE_TOL, "rotation": ROT_TOL, "move_R": R_TOL, "move_T": T_TOL, "rise": RMSE_TOL, "exact": 0.0}


def bounds_g4():
    return dict(bounds(), R=R_TOL_G4, T=T_TOL_G4)


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_ADD_S_MAX_N (\d+)", raw).group(1)) == _lib.ADD_S_MAX_N


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    near = lambda X, Y, stride, dist, nn, b, n, m: lib.so3_nearest_f32(X, Y, stride, dist, nn, b, n, m, None)
    icp = lambda b, n, m, P=p, Q=p, stride=0, R=p, t=p, ws=p, it=3: lib.so3_icp_f32(P, Q, stride, None, None, -1.0, it, R, t, None, None, None, None, ws, b, n, m, None)
    assert near(None, None, 0, None, None, 0, 8, 8) == 0 and icp(0, 8, 8, None, None, 0, None, None, None) == 0          # B == 0: a no-op, whatever the pointers
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert near(p, p, 0, p, p, b, n, m) != 0 and b"so3_nearest_f32: B/N" in err(), (b, n, m, err())
        assert icp(b, n, m) != 0 and b"so3_icp_f32: B/N" in err(), (b, n, m, err())
    for args in ((None, p, 0, p, p), (p, None, 0, p, p), (p, p, 0, None, p)):                                             # nearest alone is optional
        assert near(*args, 4, 8, 8) != 0 and b"so3_nearest_f32: null pointer" in err(), args
    assert near(p, p, 23, p, None, 4, 8, 8) != 0 and b"y_stride" in err()                                                 # clouds would overlap
    for kw in ({"P": None}, {"Q": None}, {"R": None}, {"t": None}, {"ws": None}):
        assert icp(4, 8, 8, **kw) != 0 and b"so3_icp_f32: null pointer" in err(), kw
    assert icp(4, 8, 8, stride=5) != 0 and b"q_stride" in err()
    for it in (-1, 1001):
        assert icp(4, 8, 8, it=it) != 0 and b"iterations" in err()
    wb = lib.so3_icp_workspace_bytes
    assert wb(0, 8) == 0 and wb(-1, 8) == 0 and wb(4, 0) == 0 and wb(4, big) == 0
    assert wb(1, 1) == (24 + 20) * 4 and wb(3, 257) == 3 * (24 + 2 * 20) * 4 and wb(2, 256) == 2 * (24 + 20) * 4


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("icp_align", "nearest_neighbors"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    P, Q, w = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.ones(2, 5)
    for fn in (lambda: pa.nearest_neighbors(P, Q), lambda: pa.nearest_neighbors(P, Q[0]), lambda: pa.icp_align(P, Q),
               lambda: pa.icp_align(P, Q[0], torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), iterations=0, max_distance=0.5, weights=w, return_info=True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g21_cases():
    return ref.cases(ref.g21())


def initial_pose(c):
    """Float64 (R0, t0) of a case: the stored float32 pose, or the identity where the call is made without one."""
    if c["R0"] is None:
        return np.broadcast_to(np.eye(3), (c["b"], 3, 3)).copy(), np.zeros((c["b"], 3))
    return c["R0"].astype(np.float64), c["t0"].astype(np.float64)


def test_g21_is_self_consistent(g21_cases):
    assert os.path.getsize(ref.GOLDEN) <= 1024 * 1024
    by = {k: [c for c in g21_cases if c["kind"] == k] for k in ref.KINDS}
    assert {(c["n"], c["m"], c["shared"]) for c in by["search"]} >= {(n, m, s) for n, m in ref.SIZES for s in (False, True)}
    for n, m in ref.SIZES:
        mine = [c for c in by["step"] if (c["n"], c["m"]) == (n, m)]
        assert {c["weights"] for c in mine} == set(ref.WEIGHTS) and {c["max_distance"] is None for c in mine} == {True, False}, (n, m)
        assert {c["offset"] for c in mine} == set(ref.OFFSETS), (n, m)
    assert any(c["shared"] for c in by["step"]) and any(c["R0"] is None for c in by["step"])
    for c in g21_cases:
        assert c["P"].dtype == np.float32 and c["Q"].dtype == np.float32 and np.isfinite(c["P"]).all() and np.isfinite(c["Q"]).all(), c["name"]
        R0, t0 = initial_pose(c)
        if c["kind"] == "search":
            d, idx = ref.nearest64(c["P"], c["Q"])
            assert np.array_equal(d, c["dist"]) and np.array_equal(idx, c["nearest"]), c["name"]
            assert np.abs(c["P"]).max() <= 1 and np.abs(c["Q"]).max() <= 1
        elif c["kind"] == "step":
            d, idx = ref.nearest64(ref.pose_points(c["P"], R0, t0), c["Q"])
            if c["max_distance"] is not None:                                            # the margin that makes the mask unambiguous
                assert np.abs(d - c["max_distance"]).min() > ref.MARGIN, c["name"]
            s = ref.step_from(c["P"], c["Q"], idx, d, R0, t0, c["w"], c["max_distance"])
            assert np.allclose(s["R"], c["R"], rtol=0, atol=1e-12) and np.allclose(s["rmse"], c["rmse"][0], rtol=0, atol=1e-12), c["name"]
            assert np.array_equal(s["inliers"], c["inliers"][0]), c["name"]
        else:
            assert c["iterations"] == 20 and c["rmse"].shape == (20, c["b"])
            if c["kind"] == "converge":                                                  # Q = T_gt (P permuted) exactly; reached within 10 iterations
                image = ref.pose_points(c["P"], c["Rgt"], c["tgt"])
                assert np.abs(image - ref.gather(c["Q"], c["perm"].astype(np.int64), c["b"])).max() < 1e-14, c["name"]
                assert (c["rmse"][9:] < 1e-12).all() and np.array_equal(c["nearest"], c["perm"]), c["name"]
                assert np.abs(c["R"] - c["Rgt"]).max() < 1e-12 and np.abs(c["t"] - c["tgt"]).max() < 1e-12
                ang = np.degrees(np.arccos(np.clip((np.einsum("bij,bij->b", R0, c["Rgt"]) - 1) / 2, -1, 1)))
                assert ang.max() <= 2.0 + 1e-3 and np.linalg.norm(t0 - c["tgt"], axis=1).max() <= 0.02 + 1e-6, c["name"]
            else:
                assert ref.runner_up_gap(c["P"], c["Q"], c["R"], c["t"]) > 1e-3, c["name"]
            if c["m"] > c["n"]:                                                          # the extra target points are never inliers
                assert c["max_distance"] is not None and (c["inliers"] == c["n"]).all(), c["name"]
    assert any(c["kind"] == "step" and (c["inliers"] == 0).all() for c in g21_cases)      # an empty inlier set


# ---- the checks, shared with tests/test_gpu_icp.py -----------------------------------------------------------------------------
def search_figures(X, Y, dist, nearest, dmin=None, device="cpu"):
    """Check 1 for a search's results against the float64 brute force (dmin: its distances, when they are at hand)."""
    if dmin is None:
        dmin, _ = ref.nearest64(X, Y, device)
    eye, zero = np.broadcast_to(np.eye(3), (len(X), 3, 3)), np.zeros((len(X), 3))
    nearest = np.asarray(nearest, np.int64)
    assert nearest.min() >= 0 and nearest.max() < np.shape(Y)[-2]
    return {"search": float((ref.dist_to(X, Y, nearest, eye, zero) - dmin).max()), "dist": float(np.abs(np.asarray(dist, np.float64) - dmin).max())}


def step_figures(P, Q, w, R0, t0, max_distance, got, check=ref.FULL, it=0):
    """Check 2 for iteration `it` of a call's results, which started from the float64 pose (R0, t0) and whose search is got["nearest"]."""
    nearest = np.asarray(got["nearest"], np.int64)
    assert nearest.min() >= 0 and nearest.max() < np.shape(Q)[-2]
    d = ref.dist_to(P, Q, nearest, R0, t0)
    if max_distance is not None:
        assert np.abs(d - max_distance).min() > ref.MARGIN
    s = ref.step_from(P, Q, nearest, d, R0, t0, w, max_distance)
    f = {"rmse": float(np.abs(got["rmse"][it] - s["rmse"]).max()), "exact": 0.0 if np.array_equal(got["inliers"][it], s["inliers"]) else np.inf}
    f["rotation"] = max(ra.rotation_defect(got["R"]))
    if not np.isfinite(got["R"]).all() or not np.isfinite(got["t"]).all():
        f["exact"] = np.inf
    live = s["inliers"] > 0
    keep = np.concatenate([np.asarray(R0, np.float32).reshape(-1, 9), np.asarray(t0, np.float32)], 1)
    mine = np.concatenate([got["R"].reshape(-1, 9), got["t"]], 1)
    if not np.array_equal(mine[~live], keep[~live]) or (got["rmse"][it][~live] != 0).any():      # an empty inlier set keeps the pose
        f["exact"] = np.inf
    if check == ref.FULL and live.any():
        scale = np.maximum(1.0, np.abs(s["stats"][:, :6]).max(1))
        f["R"] = float(np.abs(got["R"] - s["R"])[live].max())
        f["T"] = float((np.abs(got["t"] - s["t"]).max(1) / scale)[live].max())
    return f


def case_figures(c, got):
    """The figures of one fixture case for the results `got` of running it (dist, nearest; for ICP also R, t, rmse, inliers)."""
    R0, t0 = initial_pose(c)
    if c["kind"] == "search":
        f = search_figures(c["P"], c["Q"], got["dist"], got["nearest"], c["dist"])
        if (c["dist"] == 0).all():                                                       # X inside Y: exactly 0, the first duplicate
            f["exact"] = 0.0 if (got["dist"] == 0).all() and np.array_equal(got["nearest"], c["nearest"]) else np.inf
        return f
    if c["kind"] == "step":
        f = step_figures(c["P"], c["Q"], c["w"], R0, t0, c["max_distance"], got, c["check"])
        if c["offset"] == 0.0:
            f["dist"] = float(np.abs(got["dist"] - ref.dist_to(c["P"], c["Q"], np.asarray(got["nearest"], np.int64), R0, t0)).max())
        return f
    f = {"rotation": max(ra.rotation_defect(got["R"]))}
    if c["kind"] == "converge":
        f.update(conv_R=float(np.abs(got["R"] - c["Rgt"]).max()), conv_T=float(np.abs(got["t"] - c["tgt"]).max()), conv_rmse=float(got["rmse"][-1].max()),
                 exact=0.0 if np.array_equal(got["nearest"], c["perm"]) and (got["inliers"] == c["n"]).all() else np.inf)
        return f
    R, t = got["R"].astype(np.float64), got["t"].astype(np.float64)                        # noise: properties
    if c["max_distance"] is None:
        f["rise"] = float(max(0.0, (got["rmse"][1:] - got["rmse"][:-1]).max()))
    d, idx = ref.nearest64(ref.pose_points(c["P"], R, t), c["Q"])
    s = ref.step_from(c["P"], c["Q"], idx, d, R, t, c["w"], c["max_distance"])
    f["move_R"] = float(np.abs(s["R"] - R).max())
    f["move_T"] = float((np.abs(s["t"] - t).max(1) / np.maximum(1.0, np.abs(s["stats"][:, :6]).max(1))).max())
    return f


def check_against_g21(cases, run, label):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as numpy arrays."""
    bnd = bounds()
    worst, rows = {}, []
    for c in cases:
        f = case_figures(c, run(c))
        rows.append((c, f))
        print("%s %-40s " % (label, c["name"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
            if c["offset"] > 0:
                worst[k + "@offset"] = max(worst.get(k + "@offset", 0.0), float(v))
    print(label, "worst:", "  ".join("%s %.3e" % kv for kv in worst.items()))
    for c, f in rows:
        for k, v in f.items():
            assert v <= bnd[k], (label, c["name"], k, v, bnd[k])
    return worst


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "icp", SRC)
    lib.model_icp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int32] + \
        [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    lib.model_nearest.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    lib.model_icp_points_per_lane.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]
    return lib


def initial_rows(c):
    """The C ABI's T_init (B,12) of a case, or None."""
    return None if c["R0"] is None else np.ascontiguousarray(np.concatenate([c["R0"], c["t0"][:, :, None]], 2).reshape(-1, 12), dtype=np.float32)


def abi_run(near, icp, c, tail=(), iterations=None, workspace=None):
    """One case through functions with the C ABI's argument order (the host model here, the library's entries on numpy-like buffers)."""
    b, n, m = c["b"], c["n"], c["m"]
    stride = 0 if c["shared"] else 3 * m
    P, Q = np.ascontiguousarray(c["P"]), np.ascontiguousarray(c["Q"])
    out = {"dist": np.full((b, n), np.nan, np.float32), "nearest": np.full((b, n), -1, np.int32)}
    if c["kind"] == "search":
        near(np_ptr(P), np_ptr(Q), stride, np_ptr(out["dist"]), np_ptr(out["nearest"]), b, n, m, *tail)
        return out
    it = c["iterations"] if iterations is None else iterations
    out.update(R=np.full((b, 3, 3), np.nan, np.float32), t=np.full((b, 3), np.nan, np.float32), rmse=np.full((it, b), np.nan, np.float32),
               inliers=np.full((it, b), -1, np.int32))
    w, T0 = (None if c["w"] is None else np.ascontiguousarray(c["w"])), initial_rows(c)
    md = -1.0 if c["max_distance"] is None else c["max_distance"]
    icp(np_ptr(P), np_ptr(Q), stride, np_ptr(w), np_ptr(T0), md, it, np_ptr(out["R"]), np_ptr(out["t"]), np_ptr(out["rmse"]), np_ptr(out["inliers"]), np_ptr(out["nearest"]), np_ptr(out["dist"]),
        *(() if workspace is None else (workspace,)), b, n, m, *tail)
    return out


def host_run(model, c, cus=CUS, iterations=None):
    return abi_run(model.model_nearest, model.model_icp, c, (cus,) if c["kind"] != "search" else (), iterations)


def test_host_model_against_g21(model, g21_cases):
    worst = check_against_g21(g21_cases, lambda c: host_run(model, c), "host")
    # the recorded HOST_* constants are this measurement (to the three digits they are written with); search and dist share one
    worst["search"] = max(worst["search"], worst["dist"])
    for k, host in MEASURED.items():
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)
    # the condition on the algorithm: far from the origin the rotation is as good as at it
    assert 4 * worst["R@offset"] < 1e-5, worst["R@offset"]


def test_host_model_at_every_work_item_size(model, g21_cases):
    """The launcher's rule picks U = 1, 2, 4 as the device grows smaller: the sums are combined in another order, within the same bounds."""
    c = next(c for c in g21_cases if c["kind"] == "step" and (c["n"], c["m"]) == (1000, 2500) and c["weights"] == "random")
    seen = {}
    for cus in (256, 1, 0):
        u = model.model_icp_points_per_lane(c["b"], c["n"], cus)
        seen[u] = host_run(model, c, cus)
        f = case_figures(c, seen[u])
        print("host U=%d " % u + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            assert v <= bounds()[k], (u, k, v)
    assert sorted(seen) == [1, 2, 4]
    assert all(np.array_equal(seen[u]["nearest"], seen[1]["nearest"]) for u in seen)       # the search itself does not depend on U


def test_host_model_zero_iterations_and_repeatability(model, g21_cases):
    for c in g21_cases:
        if c["kind"] != "step" or c["n"] > 3:
            continue
        got = host_run(model, c, iterations=0)
        R0, t0 = initial_pose(c)
        assert np.array_equal(got["R"], R0.astype(np.float32)) and np.array_equal(got["t"], t0.astype(np.float32)), c["name"]
    c = next(c for c in g21_cases if c["kind"] == "noise")
    a, b = host_run(model, c), host_run(model, c)
    assert all(np.array_equal(a[k], b[k]) for k in a)
