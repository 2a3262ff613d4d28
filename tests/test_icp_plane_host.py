"""icp_align_plane (so3_icp_plane_workspace_bytes, so3_icp_plane_f32) without a GPU: the boundary (header, binding table, exports, argument
validation, the Python names), the G30 fixture's own consistency, and the kernels' device functions compiled for the host
(tests/host_model/icp_plane.cpp with SO3_HOST_MODEL) on G30.

Everything is measured against the float64 restatement (tests/icp_plane_ref.py) solved on the pairs the implementation RETURNED, so a
search tie cannot fail a step.  A cloud's step is compared as numbers only where it is unique (float64's equilibrated cond(A) <= 1e3 and
at least 6 inliers); there it must also come back solved.  Elsewhere it is held to properties: finite, R a rotation, the pose kept bit
for bit when it reports solved = 0, rmse 0 and solved 0 without inlier weight.  rmse, rmse_point and inliers are compared everywhere.
  search     at offset 0: (float64 distance to the returned neighbour) - (float64 minimum), and |dist - that distance|
  R, T       max |dR|,  max |dt| / max(1, |pbar|_inf, |qbar|_inf)  (pbar, qbar: the weighted centroids of the posed source and its targets)
  rmse, rmse_point   absolute differences
  rotation   R^T R - I and det R - 1 (rigid_align_ref.rotation_defect)
  conv_*     after 20 iterations of the exact case: max |R - R_gt|, max |t - t_gt|, the last rmse; nearest == the permutation
  compare    float64 point-to-plane rmse of the pose after k iterations / the float64 trajectory's plateau

TOLERANCES.  MEASURED holds the largest errors of the float32 host model (at 256 compute units) over G30, measured here; the bound
of each check, on the host and on the GPU alike, is 4 x that value (the device's v_rcp / v_sqrt are 1-ulp approximations and it
contracts a * b + c); the host model itself is held to the figures as written.  `compare` is not a measurement: the generator
asserts that float64 reaches 1.1 x the plateau in k iterations, and a float32 pose differs from it by 1e-6, which moves an rmse of
2e-3 by less than a percent: the bound is 1.1 x 1.01.  tests/test_gpu_icp_plane.py imports the bounds and the checks; DESIGN.md
section 7l quotes them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import icp_plane_ref as ref
import rigid_align_ref as ra
from support import boundary, build_host_model, np_ptr, on_own_thread

#            measured on the host (the bound is 4 x)
MEASURED = {"search": 1.078e-7, "R": 4.172e-6, "T": 1.501e-6, "rmse": 5.109e-6, "rmse_point": 4.515e-6, "rotation": 1.304e-7,
            "conv_R": 1.073e-7, "conv_T": 2.980e-8, "conv_rmse": 3.718e-8}
COMPARE_TOL = 1.1 * 1.01
PIVOT_EPS = 2.0 ** -7               # include/so3proj.h: SO3_ICP_PLANE_PIVOT_EPS

NEW_SYMBOLS = {"so3_icp_plane_workspace_bytes": 2, "so3_icp_plane_f32": 22}
SRC = os.path.join(ROOT, "tests", "host_model", "icp_plane.cpp")
CUS = 256                           # the device the host model stands in for


def bounds():
    return dict({k: 4 * v for k, v in MEASURED.items()}, dist=4 * MEASURED["search"], compare=COMPARE_TOL, exact=0.0)


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert float(re.search(r"#define SO3_ICP_PLANE_PIVOT_EPS ([0-9.]+)f", raw).group(1)) == PIVOT_EPS


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    icp = lambda b, n, m, P=p, Q=p, nrm=p, stride=0, R=p, t=p, ws=p, it=3, damping=0.0: lib.so3_icp_plane_f32(
        P, Q, nrm, stride, None, None, -1.0, damping, it, R, t, None, None, None, None, None, None, ws, b, n, m, None)
    assert icp(0, 8, 8, None, None, None, 0, None, None, None) == 0                    # B == 0: a no-op, whatever the pointers
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert icp(b, n, m) == -1 and err() == b"so3_icp_plane_f32: B/N: invalid argument", (b, n, m, err())
    for kw in ({"P": None}, {"Q": None}, {"nrm": None}, {"R": None}, {"t": None}, {"ws": None}):
        assert icp(4, 8, 8, **kw) == -1 and err() == b"so3_icp_plane_f32: null pointer: invalid argument", (kw, err())
    assert icp(4, 8, 8, stride=5) == -1 and err() == b"so3_icp_plane_f32: q_stride: invalid argument"
    for it in (-1, 1001):
        assert icp(4, 8, 8, it=it) == -1 and err() == b"so3_icp_plane_f32: iterations: invalid argument"
    for damping in (-0.5, float("nan"), -1e-30):
        assert icp(4, 8, 8, damping=damping) == -1 and err() == b"so3_icp_plane_f32: damping: invalid argument", damping
    assert icp(0, 8, 8, damping=-1.0) == -1                                           # the ranges are checked before B == 0 returns
    wb = lib.so3_icp_plane_workspace_bytes
    assert wb(0, 8) == 0 and wb(-1, 8) == 0 and wb(4, 0) == 0 and wb(4, big) == 0
    assert wb(1, 1) == (24 + 32) * 4 and wb(3, 257) == 3 * (24 + 2 * 32) * 4 and wb(2, 256) == 2 * (24 + 32) * 4


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    assert "icp_align_plane" in pa.__all__ and pa.icp_align_plane is rr.icp_align_plane
    P, Q, w = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.ones(2, 5)
    for fn in (lambda: pa.icp_align_plane(P, Q), lambda: pa.icp_align_plane(P, Q[0], Q[0]),
               lambda: pa.icp_align_plane(P, Q, Q, torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), iterations=0, max_distance=0.5, weights=w,
                                          damping=0.1, return_info=True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g30_cases():
    return ref.cases(ref.g30())


def initial_pose(c):
    """Float64 (R0, t0) of a case: the stored float32 pose, or the identity where the call is made without one."""
    if c["R0"] is None:
        return np.broadcast_to(np.eye(3), (c["b"], 3, 3)).copy(), np.zeros((c["b"], 3))
    return c["R0"].astype(np.float64), c["t0"].astype(np.float64)


def test_g30_is_self_consistent(g30_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    by = {k: [c for c in g30_cases if c["kind"] == k] for k in ref.KINDS}
    assert all(by[k] for k in ref.KINDS)
    for n, m in ref.SIZES:
        mine = [c for c in by["step"] if (c["n"], c["m"]) == (n, m)]
        assert {c["weights"] for c in mine} == set(ref.WEIGHTS) and {c["max_distance"] is None for c in mine} == {True, False}, (n, m)
        assert {c["offset"] for c in mine} == set(ref.OFFSETS) and {c["shared"] for c in mine} == {True, False}, (n, m)
    assert {c["surface"] for c in by["step"]} == {"ellipsoid", "blob"} and any(c["R0"] is None for c in by["step"])
    assert any(c["zero_every"] and (c["Nrm"][..., 1::3, :] == 0).all() and (c["Nrm"][..., 0::3, :] != 0).any() for c in by["step"])
    random_unique = []
    for c in g30_cases:
        assert c["P"].dtype == c["Q"].dtype == c["Nrm"].dtype == np.float32 and c["Nrm"].shape == c["Q"].shape, c["name"]
        assert all(np.isfinite(c[k]).all() for k in ("P", "Q", "Nrm")), c["name"]
        R0, t0 = initial_pose(c)
        if c["kind"] in ("step", "degenerate"):
            d, idx = ref.nearest64(ref.pose_points(c["P"], R0, t0), c["Q"])
            if c["max_distance"] is not None:                                            # the margin that makes the mask unambiguous
                assert np.abs(d - c["max_distance"]).min() > ref.MARGIN, c["name"]
            s = ref.step_from(c["P"], c["Q"], c["Nrm"], idx, d, R0, t0, c["w"], c["max_distance"], c["damping"])
            for k in ("R", "t", "rmse", "rmse_point"):
                assert np.allclose(s[k], c[k], rtol=0, atol=1e-11), (c["name"], k)
            assert np.array_equal(s["inliers"], c["inliers"]) and np.array_equal(s["unique"], c["unique"]), c["name"]
            fin = np.isfinite(c["cond"]) & (c["cond"] < 1e12)
            assert np.array_equal(fin, np.isfinite(s["cond"]) & (s["cond"] < 1e12)) and (np.abs(s["cond"][fin] / c["cond"][fin] - 1) < 1e-3).all(), c["name"]
            if c["kind"] == "step" and c["n"] >= ref.MIN_INLIERS and (s["inliers"] > 0).any():
                random_unique.extend(s["unique"].tolist())
            if c["expect_solved"] >= 0:
                assert (s["unique"] == bool(c["expect_solved"])).all(), c["name"]
        elif c["kind"] == "converge":                                                    # Q = T_gt P exactly, forty targets out of reach
            image = ref.pose_points(c["P"], c["Rgt"], c["tgt"])
            assert np.abs(image - ref.gather(c["Q"], c["perm"].astype(np.int64), c["b"])).max() < 1e-14 and c["m"] == c["n"] + 40
            assert c["iterations"] == 20 and (c["rmse"][9:] < 1e-12).all() and (c["inliers"] == c["n"]).all()
            assert np.abs(c["R"] - c["Rgt"]).max() < 1e-12 and np.abs(c["t"] - c["tgt"]).max() < 1e-12
        else:                                                                            # the property the generator asserted, once more
            import icp_ref
            k = c["iterations"]
            plane = ref.icp_plane64(c["P"], c["Q"], c["Nrm"], R0, t0, k)
            point = icp_ref.icp64(c["P"], c["Q"], R0, t0, 3 * k)
            assert (ref.plane_rmse64(c["P"], c["Q"], c["Nrm"], plane["R"], plane["t"]) <= 1.1 * c["plateau"]).all()
            assert (ref.plane_rmse64(c["P"], c["Q"], c["Nrm"], point["R"], point["t"]) > 2.0 * c["plateau"]).all()
            ang = np.arccos(np.clip((np.einsum("bii->b", R0) - 1) / 2, -1, 1))
            assert np.abs(ang - 0.15).max() < 2e-3 and np.abs(np.linalg.norm(t0, axis=1) - 0.1).max() < 1e-6
    assert random_unique and 1.0 - np.mean(random_unique) <= 0.05
    assert any(c["kind"] == "step" and (c["inliers"] == 0).all() for c in g30_cases)      # an empty inlier set


# ---- the checks, shared with tests/test_gpu_icp_plane.py ------------------------------------------------------------------------
def step_figures(c, got, it=0, R0=None, t0=None):
    """The figures of iteration `it` of a call's results, which started from the float64 pose (R0, t0) and whose search is got["nearest"]."""
    if R0 is None:
        R0, t0 = initial_pose(c)
    nearest = np.asarray(got["nearest"], np.int64)
    assert nearest.min() >= 0 and nearest.max() < c["m"]
    d = ref.dist_to(c["P"], c["Q"], nearest, R0, t0)
    if c["max_distance"] is not None:
        assert np.abs(d - c["max_distance"]).min() > ref.MARGIN
    s = ref.step_from(c["P"], c["Q"], c["Nrm"], nearest, d, R0, t0, c["w"], c["max_distance"], c["damping"])
    solved = np.asarray(got["solved"][it]).astype(bool)
    f = {"rmse": float(np.abs(got["rmse"][it] - s["rmse"]).max()), "rmse_point": float(np.abs(got["rmse_point"][it] - s["rmse_point"]).max()),
         "rotation": max(ra.rotation_defect(got["R"])), "exact": 0.0}
    live, unique = s["W"] > 0, s["unique"]
    keep = np.concatenate([np.asarray(R0, np.float32).reshape(-1, 9), np.asarray(t0, np.float32)], 1)
    mine = np.concatenate([got["R"].reshape(-1, 9), got["t"]], 1)
    ok = np.array_equal(got["inliers"][it], s["inliers"]) and np.isfinite(mine).all()
    ok = ok and np.array_equal(mine[~solved], keep[~solved])                             # an unsolved step keeps the pose bit for bit
    ok = ok and not solved[~live].any() and (got["rmse"][it][~live] == 0).all() and (got["rmse_point"][it][~live] == 0).all()
    ok = ok and solved[unique].all()                                                    # a unique step is solved
    if c["expect_solved"] >= 0:
        ok = ok and (solved == bool(c["expect_solved"])).all()
    if not ok:
        f["exact"] = np.inf
    if unique.any():
        scale = np.maximum(1.0, np.maximum(np.abs(s["pbar"]).max(1), np.abs(s["qbar"]).max(1)))
        f["R"] = float(np.abs(got["R"] - s["R"])[unique].max())
        f["T"] = float((np.abs(got["t"] - s["t"]).max(1) / scale)[unique].max())
    if c["offset"] == 0.0 and c["kind"] == "step":
        dmin, _ = ref.nearest64(ref.pose_points(c["P"], R0, t0), c["Q"])
        f["search"] = float((d - dmin).max())
        f["dist"] = float(np.abs(got["dist"] - d).max())
    return f


def case_figures(c, got):
    if c["kind"] in ("step", "degenerate"):
        return step_figures(c, got)
    f = {"rotation": max(ra.rotation_defect(got["R"]))}
    if c["kind"] == "converge":
        good = np.array_equal(got["nearest"], c["perm"]) and (got["inliers"] == c["n"]).all() and np.asarray(got["solved"]).all()
        f.update(conv_R=float(np.abs(got["R"] - c["Rgt"]).max()), conv_T=float(np.abs(got["t"] - c["tgt"]).max()), conv_rmse=float(got["rmse"][-1].max()),
                 exact=0.0 if good else np.inf)
        return f
    e = ref.plane_rmse64(c["P"], c["Q"], c["Nrm"], got["R"].astype(np.float64), got["t"].astype(np.float64))
    f.update(compare=float((e / c["plateau"]).max()), exact=0.0 if np.asarray(got["solved"]).all() else np.inf)
    return f


def check_against_g30(cases, run, label):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as numpy arrays."""
    bnd = bounds()
    worst, rows = {}, []
    for c in cases:
        f = case_figures(c, run(c))
        rows.append((c, f))
        print("%s %-58s " % (label, c["name"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
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
    lib = build_host_model(tmp_path_factory, "icp_plane", SRC)
    lib.model_icp_plane.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_int32] + \
        [ctypes.c_void_p] * 9 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    lib.model_plane_solve.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    lib.model_plane_retraction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.model_plane_pivot_eps.restype = ctypes.c_float
    return lib


def initial_rows(c):
    """The C ABI's T_init (B,12) of a case, or None."""
    return None if c["R0"] is None else np.ascontiguousarray(np.concatenate([c["R0"], c["t0"][:, :, None]], 2).reshape(-1, 12), dtype=np.float32)


def abi_run(icp, c, tail=(), iterations=None, workspace=(), normals=None):
    """One case through a function with the C ABI's argument order (the host model here: its `ratio` output goes where the workspace is)."""
    b, n, m = c["b"], c["n"], c["m"]
    it = c["iterations"] if iterations is None else iterations
    P, Q, N = np.ascontiguousarray(c["P"]), np.ascontiguousarray(c["Q"]), np.ascontiguousarray(c["Nrm"] if normals is None else normals)
    out = {"dist": np.full((b, n), np.nan, np.float32), "nearest": np.full((b, n), -1, np.int32), "R": np.full((b, 3, 3), np.nan, np.float32),
           "t": np.full((b, 3), np.nan, np.float32), "rmse": np.full((it, b), np.nan, np.float32), "rmse_point": np.full((it, b), np.nan, np.float32),
           "inliers": np.full((it, b), -1, np.int32), "solved": np.full((it, b), -1, np.int32)}
    w, T0 = (None if c["w"] is None else np.ascontiguousarray(c["w"])), initial_rows(c)
    md = -1.0 if c["max_distance"] is None else c["max_distance"]
    icp(np_ptr(P), np_ptr(Q), np_ptr(N), 0 if c["shared"] else 3 * m, np_ptr(w), np_ptr(T0), md, c["damping"], it, np_ptr(out["R"]), np_ptr(out["t"]), np_ptr(out["rmse"]),
        np_ptr(out["rmse_point"]), np_ptr(out["inliers"]), np_ptr(out["solved"]), np_ptr(out["nearest"]), np_ptr(out["dist"]), *workspace, b, n, m, *tail)
    return out


def host_run(model, c, cus=CUS, iterations=None, normals=None, want_ratio=False):
    it = c["iterations"] if iterations is None else iterations
    ratio = np.full((it, c["b"]), np.nan, np.float32)
    out = abi_run(model.model_icp_plane, c, (cus,), iterations, (np_ptr(ratio),), normals)
    if want_ratio:
        out["ratio"] = ratio
    return out


def test_host_model_against_g30(model, g30_cases):
    assert model.model_plane_pivot_eps() == PIVOT_EPS
    worst = check_against_g30(g30_cases, lambda c: host_run(model, c), "host")
    worst["search"] = max(worst["search"], worst["dist"])   # search and dist share one figure
    for k, host in MEASURED.items():                       # the recorded constants are this measurement, to the digits they are written with
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)
    # CONDITION on the pivot, not a measurement.  The definition forms a_i and e_i from the POSED float32 coordinates, which at offset
    # 100 are rounded to ulp(100) / 2 = 3.8e-6 each; a pose fitted to hundreds of such points stays within one point's rounding,
    # ulp(100) = 2^-17.  Moments about the origin instead of the pivot would lose 100^2 eps = 6e-4.
    assert worst["R@offset"] < 2.0 ** -17 and worst["T@offset"] < 2.0 ** -17, (worst["R@offset"], worst["T@offset"])


def test_pivot_eps_is_the_largest_power_of_two_that_solves_every_unique_step(model, g30_cases):
    """The rule of include/so3proj.h for SO3_ICP_PLANE_PIVOT_EPS, from the host model's smallest pivot ratios: every unique step passes
    at the constant and one of them fails at twice it; the exact plane and the exact sphere stay below it (unsolved at damping 0)."""
    lowest_unique, highest_degenerate = np.inf, 0.0
    for c in g30_cases:
        got = host_run(model, c, want_ratio=True)
        if c["kind"] in ("step", "degenerate"):
            unique = c["unique"]
            if unique.any():
                lowest_unique = min(lowest_unique, float(got["ratio"][0][unique].min()))
            if c["expect_solved"] == 0:
                highest_degenerate = max(highest_degenerate, float(got["ratio"][0].max()))
        else:
            lowest_unique = min(lowest_unique, float(got["ratio"].min()))
    print("pivot ratios: lowest unique %.3e (margin x%.2f above eps), highest plane / sphere %.3e (margin x%.3g below eps)"
          % (lowest_unique, lowest_unique / PIVOT_EPS, highest_degenerate, PIVOT_EPS / max(highest_degenerate, 1e-300)))
    assert PIVOT_EPS < lowest_unique <= 2 * PIVOT_EPS
    assert highest_degenerate < PIVOT_EPS


def test_host_model_at_every_work_item_size(model, g30_cases):
    """The launcher's rule picks U = 1, 2, 4 as the device grows smaller: the sums are combined in another order, within the same bounds."""
    c = next(c for c in g30_cases if c["kind"] == "step" and (c["n"], c["m"]) == (1000, 2500) and c["weights"] == "random")
    seen = {}
    for cus, u in ((256, 1), (1, 2), (0, 4)):
        seen[u] = host_run(model, c, cus)
        f = case_figures(c, seen[u])
        print("host U=%d " % u + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            assert v <= bounds()[k], (u, k, v)
    assert all(np.array_equal(seen[u]["nearest"], seen[1]["nearest"]) and np.array_equal(seen[u]["dist"], seen[1]["dist"]) for u in seen)
    assert any(not np.array_equal(seen[u]["t"], seen[1]["t"]) for u in (2, 4))            # the orders do differ: the three runs are three work splits


def test_host_model_zero_iterations_and_repeatability(model, g30_cases):
    for c in g30_cases:
        if c["kind"] != "step" or c["n"] > 3:
            continue
        got = host_run(model, c, iterations=0)
        R0, t0 = initial_pose(c)
        assert np.array_equal(got["R"], R0.astype(np.float32)) and np.array_equal(got["t"], t0.astype(np.float32)), c["name"]
        one = host_run(model, c)
        assert np.array_equal(got["nearest"], one["nearest"]) and np.array_equal(got["dist"], one["dist"]), c["name"]      # the first search
    c = next(c for c in g30_cases if c["kind"] == "converge")
    a, b = host_run(model, c), host_run(model, c)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_negated_normals_give_the_same_bits(model, g30_cases):
    rng = np.random.default_rng(7)
    for c in g30_cases:
        flip = np.where(rng.uniform(0, 1, c["Nrm"].shape[:-1] + (1,)) < 0.5, -1.0, 1.0).astype(np.float32)
        a, b = host_run(model, c), host_run(model, c, normals=c["Nrm"] * flip)
        assert all(np.array_equal(a[k], b[k]) for k in a), c["name"]


# ---- the 6x6 solve and the retraction alone -----------------------------------------------------------------------------------
def _solve(model, A, g, damping=0.0):
    A32, g32 = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(g, np.float32)
    delta, ratio = np.full(6, np.nan, np.float32), np.full(1, np.nan, np.float32)
    ok = model.model_plane_solve(np_ptr(A32), np_ptr(g32), damping, np_ptr(delta), np_ptr(ratio))
    return bool(ok), delta, float(ratio[0])


def test_the_solve_against_numpy_on_random_spd_systems(model):
    """Random SPD systems of equilibrated condition number <= 1e3 and any scaling.  The pivot rule decides which are solved: one whose
    float64 pivots all exceed 2 PIVOT_EPS of their diagonal must be, one with a pivot below PIVOT_EPS / 2 must not be.  Where solved,
    the error against float64's solve of the float32 system is bounded by 8 eps cond relative to the largest component, in the
    equilibrated unknowns (a Cholesky solve's first-order bound with room for the 6 x 6 constants; the worst ratio to it is printed)."""
    rng = np.random.default_rng(30)
    eps32, worst, count = 2.0 ** -24, 0.0, [0, 0]
    for trial in range(400):
        q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = 10.0 ** -rng.uniform(0, 3.0, 6)
        C = (q * lam) @ q.T
        s = 10.0 ** rng.uniform(-2, 2, 6)
        A = (C * np.outer(s, s)).astype(np.float32)
        A = np.triu(A) + np.triu(A, 1).T
        g = rng.standard_normal(6).astype(np.float32) * s.astype(np.float32)
        cond = ref.equilibrated_cond(A.astype(np.float64))
        if cond > ref.COND_MAX:
            continue
        ok, delta, ratio = _solve(model, A, g)
        want = -np.linalg.solve(A.astype(np.float64), g.astype(np.float64))
        L = np.linalg.cholesky(A.astype(np.float64))
        ratio64 = (np.diag(L) ** 2 / np.diag(A)).min()
        assert ok == (ratio > PIVOT_EPS) and abs(ratio / ratio64 - 1) < 1e-3, (trial, cond, ratio, ratio64)
        assert ok or ratio64 < 2 * PIVOT_EPS, (trial, ratio64)
        assert not ok or ratio64 > PIVOT_EPS / 2, (trial, ratio64)
        count[ok] += 1
        if not ok:
            assert (delta == 0).all()
            continue
        err = np.abs((delta - want) * s).max() / np.abs(want * s).max()                     # in the equilibrated unknowns
        worst = max(worst, err / (8 * eps32 * cond))
        assert err <= 8 * eps32 * cond, (trial, cond, err)
    print("6x6 solve: %d solved, %d refused by the pivot rule; worst error / (8 eps cond) = %.3f" % (count[1], count[0], worst))
    assert count[1] >= 100


def test_the_solve_on_the_plane_and_the_sphere(model, g30_cases):
    """From float64 sums rounded to float32: the exact plane (three zero columns) and the exact sphere are unsolved at damping 0 with
    delta = 0; the plane with damping 0.1 is solved: its zero columns come out 0 and the others as numpy solves them."""
    for c in g30_cases:
        if c["kind"] != "degenerate":
            continue
        R0, t0 = initial_pose(c)
        d, idx = ref.nearest64(ref.pose_points(c["P"], R0, t0), c["Q"])
        s = ref.step_from(c["P"], c["Q"], c["Nrm"], idx, d, R0, t0, None, None, 0.0)          # undamped sums: the model scales the diagonal
        for A, g in zip(s["A"], s["g"]):
            ok, delta, ratio = _solve(model, A, g, c["damping"])
            assert ok == bool(c["expect_solved"]), (c["name"], ratio)
            if not ok:
                assert (delta == 0).all() and ratio < PIVOT_EPS, (c["name"], delta, ratio)
                continue
            A32 = A.astype(np.float32).astype(np.float64)
            A32[np.diag_indices(6)] *= np.float64(np.float32(1.0) + np.float32(c["damping"]))
            keep = np.diag(A32) != 0
            assert keep.sum() == 3 and (delta[~keep] == 0).all()
            want = -np.linalg.solve(A32[np.ix_(keep, keep)], g.astype(np.float32).astype(np.float64)[keep])
            assert np.abs(delta[keep] - want).max() <= 1e-5 * np.abs(want).max(), (delta, want)


def test_the_retraction_is_orthogonal_and_the_cayley_formula(model):
    """dR against the float64 formula on steps from 1e-6 to 3 rad: the entries are at most 1 in magnitude and each is a handful of
    rounded operations on them, so 16 eps; orthogonality follows from that bound on a 3 x 3 product, 3 x 2 x 16 eps."""
    rng = np.random.default_rng(31)
    eps32, worst = 2.0 ** -24, (0.0, 0.0)
    for trial in range(300):
        axis = rng.standard_normal(3)
        omega = (axis / np.linalg.norm(axis) * 10.0 ** rng.uniform(-6, np.log10(3.0))).astype(np.float32)
        dr = np.full(9, np.nan, np.float32)
        model.model_plane_retraction(np_ptr(omega), np_ptr(dr))
        dr = dr.reshape(3, 3).astype(np.float64)
        want = ref.cayley64(omega.astype(np.float64))
        err, orth = np.abs(dr - want).max(), np.abs(dr.T @ dr - np.eye(3)).max()
        worst = (max(worst[0], err), max(worst[1], orth))
        assert err <= 16 * eps32 and orth <= 96 * eps32 and abs(np.linalg.det(dr) - 1) <= 96 * eps32, (omega, err, orth)
    assert np.abs(ref.cayley64([0.0, 0.0, 0.0]) - np.eye(3)).max() == 0
    w = np.array([0.3, -0.2, 0.5])
    th = 1e-3 * np.linalg.norm(w)
    K = ref.hat(w / np.linalg.norm(w))
    assert np.abs(ref.cayley64(1e-3 * w) - (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)).max() < 1e-9      # agrees with exp to second order
    print("retraction: worst |dR - cayley64| %.2e, worst |dR^T dR - I| %.2e" % worst)


def test_host_model_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing loaded into Python): tests/host_model/icp_plane.cpp with -fsanitize=address,undefined
    on one ragged-edge case in heap buffers of exactly the documented sizes."""
    from oracle import kernel_model
    cxx = kernel_model.clangxx()
    if cxx is None:
        pytest.skip("clang++ is not available (ext_vector_type)")
    exe = str(tmp_path / "icp_plane_san")
    build = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-DSO3_ICP_PLANE_MAIN", "-o", exe, SRC], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower():
        pytest.skip("the sanitizer runtime is not installed")
    assert build.returncode == 0, build.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.startswith("SANITIZE OK"), res.stdout + res.stderr
    print(res.stdout.strip())
