"""rigid_align (so3_rigid_align_f32, so3_rigid_align_bwd_f32) without a GPU: the boundary (header, binding table, exports, argument
validation, the Python names), the G20 fixture's own consistency, and the kernels' device functions compiled for the host
(tests/host_model/rigid_align.cpp with SO3_HOST_MODEL) on G20.

TOLERANCES.  HOST_* are the largest errors of the float32 host model against G20's float64 answers over every fully checked case of
the fixture (unit-radius clouds of 3 to 1000 points, centred or offset by 10 or 100 along every axis, with and without weights),
measured here; the bound of each check, on the host and on the GPU alike, is 4 x that value (the device's v_rcp / v_sqrt are 1-ulp
approximations and it contracts a * b + c).
  R      max |dR|
  H      max |dH| / max(max |H|, 1e-3 W)      (the floor: an H that is zero up to float64 rounding -- one point, coincident points --
                                               is not divided by itself; 1e-3 W is the H of a cloud of radius 0.03)
  T      max |dt| / max(1, |pbar|_inf, |qbar|_inf); the centroids in stats are held to the same bound
  DP, DQ, DW   max |d grad| / max(1, |reference grad|_inf of the cloud)
Two bounds are reasoned, not measured: W is a lane-strided float32 sum of at most 1000 non-negative terms, ceil(1000 / 64) = 16
additions per lane and 6 butterfly steps, each within 2^-24 relative: W_TOL = 22 * 2^-24.  A matrix within R_TOL of a rotation,
entry by entry, has |R^T R - I| <= 2 * 3 * R_TOL to first order, and its determinant is as close to 1: ROT_TOL = 6 * R_TOL.
CONDITION, not a measurement: on the offset families 4 x the measured R error must stay below 1e-5; above that the accumulation is
cancelling and the algorithm has to change, not the bound.
Cases whose rotation is not unique or badly conditioned (N < 3, collinear, coincident, the reflected pair) are held to properties only:
finite, R a rotation, R pbar + t = qbar, finite gradients; H and the centroids are compared in every case.  All-zero weights give
exactly R = I, t = 0, H = 0 and zero gradients.  tests/test_gpu_rigid_align.py imports the bounds; DESIGN.md section 7c quotes them."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import rigid_align_ref as ref
from support import boundary, build_host_model, np_ptr, on_own_thread

#                                 measured on the host       bound (4 x)
HOST_R = 4.94e-7;                 R_TOL = 4 * HOST_R                     # noqa: E702
HOST_H = 1.29e-6;                 H_TOL = 4 * HOST_H                     # noqa: E702
HOST_T = 5.24e-7;                 T_TOL = 4 * HOST_T                     # noqa: E702
HOST_DP = 2.07e-5;                DP_TOL = 4 * HOST_DP                   # noqa: E702
HOST_DQ = 1.45e-5;                DQ_TOL = 4 * HOST_DQ                   # noqa: E702
HOST_DW = 1.06e-3;                DW_TOL = 4 * HOST_DW                   # noqa: E702
W_TOL = 22 * 2.0**-24
ROT_TOL = 6 * R_TOL

NEW_SYMBOLS = ["so3_rigid_align_f32", "so3_rigid_align_bwd_f32"]
SRC = os.path.join(ROOT, "tests", "host_model", "rigid_align.cpp")
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("dP", "dQ", "dw"), r)]      # every instantiation of the backward


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    boundary(built_library, dict(zip(NEW_SYMBOLS, (10, 15))))


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    for name, nptr in (("so3_rigid_align_f32", 7), ("so3_rigid_align_bwd_f32", 12)):
        fn = getattr(lib, name)
        assert fn(*([None] * nptr), 0, 8, None) == 0, name                               # B == 0: a no-op, whatever the pointers
        assert fn(*([None] * nptr), 4, 8, None) != 0 and b"null pointer" in err(), (name, err())
        for b, n in ((-1, 8), (2**62, 8), (4, -3), (4, 2**31 - 1)):
            assert fn(*([p] * nptr), b, n, None) != 0 and (name.encode() + b": B/N") in err(), (name, b, n, err())
    assert lib.so3_rigid_align_f32(p, p, None, None, p, None, None, 4, 8, None) != 0 and b"null pointer" in err()      # R is required
    assert lib.so3_rigid_align_f32(p, p, None, p, None, None, None, 4, 8, None) != 0 and b"null pointer" in err()      # so is t
    assert lib.so3_rigid_align_f32(None, p, None, p, p, None, None, 4, 8, None) != 0 and b"null pointer" in err()      # and the clouds, N > 0
    for missing in (3, 4, 5):                                                            # the backward needs H, R and stats
        args = [p] * 12
        args[missing] = None
        assert lib.so3_rigid_align_bwd_f32(*args, 4, 8, None) != 0 and b"null pointer" in err(), missing
    assert lib.so3_rigid_align_bwd_f32(p, p, None, p, p, p, None, None, None, None, None, None, 4, 8, None) == 0       # nothing asked for: no launch
    assert lib.so3_rigid_align_bwd_f32(None, None, None, p, p, p, None, None, None, p, p, p, 4, 0, None) == 0          # N == 0: nothing to write


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    assert "rigid_align" in pa.__all__ and pa.rigid_align is rr.rigid_align
    P, w = torch.zeros(2, 5, 3), torch.ones(2, 5)
    for fn in (lambda: pa.rigid_align(P, P), lambda: pa.rigid_align(P, P, w), lambda: pa.rigid_align(P, P, w, return_h=True),
               lambda: pa.rigid_align(P.clone().requires_grad_(True), P), lambda: pa.rigid_align(P, P, w.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g20():
    return ref.g20()


@pytest.fixture(scope="module")
def g20_cases(g20):
    return ref.cases(g20)


@pytest.fixture(scope="module")
def g20_grads(g20_cases):
    """Float64 (dP, dQ, dw) of every case: computed once, shared, never changed."""
    return [ref.case_grads(c) for c in g20_cases]


def test_g20_is_self_consistent(g20, g20_cases, g20_grads):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    assert g20["P"].dtype == np.float32 and g20["Q"].dtype == np.float32 and g20["w"].dtype == np.float32 and g20["R"].dtype == np.float64
    haar = [c for c in g20_cases if c["family"] == "haar"]
    assert {c["family"] for c in g20_cases} == set(ref.FAMILIES)
    assert {c["n"] for c in haar} == set(ref.SIZES)
    for n in ref.SIZES:                                                                   # every kind of weights and every offset at every size
        assert {c["weights"] for c in haar if c["n"] == n} == set(ref.WEIGHTS), n
        assert {c["offset"] for c in haar if c["n"] == n} == set(ref.OFFSETS), n
    for n in ref.SMALL_SIZES:
        assert {(c["weights"], c["offset"]) for c in haar if c["n"] == n} == set(itertools.product(ref.WEIGHTS, ref.OFFSETS)), n
        assert all(tuple(c["sigma"]) == ref.SIGMAS for c in haar if c["n"] == n), n
    assert {float(s) for c in haar if c["n"] not in ref.SMALL_SIZES for s in c["sigma"]} == set(ref.SIGMAS)
    T = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64)
    for c, grads in zip(g20_cases, g20_grads):
        tag = (c["family"], c["weights"], c["n"], c["offset"])
        again = ref.answers(c["P"], c["Q"], c["w"])                                      # the stored answers are the restatement's
        for k, v in again.items():
            assert np.allclose(v, c[k], rtol=0, atol=1e-12 * max(1.0, c["offset"])), (tag, k)
        pbar, qbar, W = c["stats"][:, :3], c["stats"][:, 3:6], c["stats"][:, 6]
        orth, det = ref.rotation_defect(c["R"])
        assert orth < 1e-13 and det < 1e-13, tag                                         # a rotation, the reflected pair included
        assert np.abs(np.einsum("bij,bj->bi", c["R"], pbar) + c["t"] - qbar).max() < 1e-12 * max(1.0, c["offset"]), tag
        real = c["P"][c["w"] > 0] if c["weights"] == "mask" else c["P"]                   # unit radius about the offset (the masked tail is junk)
        assert np.abs(real.astype(np.float64) - c["offset"]).max() <= 1 + 1e-4 * max(1.0, c["offset"]), tag
        assert np.isfinite(c["P"]).all() and np.isfinite(c["Q"]).all()
        if c["weights"] == "zero":
            assert c["check"] == ref.ZERO and (W == 0).all() and (c["R"] == np.eye(3)).all() and (c["t"] == 0).all() and (c["H"] == 0).all(), tag
            assert all((g == 0).all() for g in grads), tag
        if c["weights"] == "mask" and c["n"] > 3:
            tail = c["w"][0] == 0
            assert tail.any() and not tail[0] and np.abs(c["P"][0][tail].astype(np.float64) - c["offset"]).max() > 5, tag      # junk, far outside
        if c["family"] == "reflected":
            assert np.abs(c["R"] - np.diag([1.0, 1.0, -1.0])).max() > 0.5, tag           # not the reflection
        if c["check"] == ref.FULL:                                                        # the closed form against float64 autograd
            auto = ref.autograd64(T(c["P"]), T(c["Q"]), T(c["w"]), T(c["gR"]), T(c["gt"]), T(c["gH"]))
            for name, g, a in zip(("dP", "dQ", "dw"), grads, auto):
                assert np.abs(g - a.numpy()).max() <= 1e-9 * max(1.0, np.abs(g).max()), (tag, name)


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_host_model(tmp_path_factory, "rigid_align", SRC)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def empty_results(c):
    b, n = c["b"], c["n"]
    return {"R": np.full((b, 3, 3), np.nan, np.float32), "t": np.full((b, 3), np.nan, np.float32), "H": np.full((b, 3, 3), np.nan, np.float32),
            "stats": np.full((b, 7), np.nan, np.float32), "dP": np.full((b, n, 3), np.nan, np.float32), "dQ": np.full((b, n, 3), np.nan, np.float32),
            "dw": np.full((b, n), np.nan, np.float32)}


def abi_run(fwd, bwd, c, tail=()):
    """One case through a pair of functions with the C ABI's argument order (the host model here, the library on the GPU): the
    forward, then the backward for all three gradients.  Returns float32 results named as the fixture's answers, plus dP, dQ, dw."""
    P, Q, w, gR, gt, gH = (_c(c[k]) for k in ("P", "Q", "w", "gR", "gt", "gH"))
    out = empty_results(c)
    B, N = ctypes.c_int64(c["b"]), ctypes.c_int32(c["n"])
    fwd(np_ptr(P), np_ptr(Q), np_ptr(w), np_ptr(out["R"]), np_ptr(out["t"]), np_ptr(out["H"]), np_ptr(out["stats"]), B, N, *tail)
    bwd(np_ptr(P), np_ptr(Q), np_ptr(w), np_ptr(out["H"]), np_ptr(out["R"]), np_ptr(out["stats"]), np_ptr(gR), np_ptr(gt), np_ptr(gH), np_ptr(out["dP"]), np_ptr(out["dQ"]), np_ptr(out["dw"]), B, N, *tail)
    return out


def figures(c, got, grads, which=("dP", "dQ", "dw")):
    """The quantities both test files bound, for one case's results `got` (as abi_run returns them) against the fixture and the
    float64 gradients `grads` = (dP, dQ, dw); `which` names the gradients that `got` holds."""
    f = {}
    st, W = c["stats"], c["stats"][:, 6]
    if "stats" not in got:                       # the Python surface does not return them: the fixture's stand in for the pose identity
        got = dict(got, stats=st.astype(np.float32))
    scale = np.maximum(1.0, np.abs(st[:, :6]).max(1))
    hden = np.maximum(np.abs(c["H"]).reshape(c["b"], -1).max(1), 1e-3 * W)
    herr = np.abs(got["H"] - c["H"]).reshape(c["b"], -1).max(1)
    f["H"] = float(np.where(hden > 0, herr / np.where(hden > 0, hden, 1.0), np.where(herr == 0, 0.0, np.inf)).max())
    f["centroid"] = float((np.abs(got["stats"][:, :6] - st[:, :6]).max(1) / scale).max())
    f["W"] = float((np.abs(got["stats"][:, 6] - W) / np.maximum(1.0, W)).max())
    orth, det = ref.rotation_defect(got["R"])
    f["rotation"] = max(orth, det)
    g64 = got["R"].astype(np.float64), got["t"].astype(np.float64), got["stats"].astype(np.float64)
    f["pose"] = float((np.abs(np.einsum("bij,bj->bi", g64[0], g64[2][:, :3]) + g64[1] - g64[2][:, 3:6]).max(1) / scale).max())   # R pbar + t = qbar
    if c["check"] == ref.FULL:
        f["R"] = float(np.abs(got["R"] - c["R"]).max())
        f["T"] = float((np.abs(got["t"] - c["t"]).max(1) / scale).max())
        for name, want in zip(("dP", "dQ", "dw"), grads):
            if name in which:
                err = np.abs(got[name] - want).reshape(c["b"], -1).max(1) if c["n"] else np.zeros(c["b"])
                f[name] = float((err / np.maximum(1.0, np.abs(want).reshape(c["b"], -1).max(1) if c["n"] else 1.0)).max())
    elif c["check"] == ref.ZERO:
        exact = (got["R"] == np.eye(3, dtype=np.float32)).all() and (got["t"] == 0).all() and (got["H"] == 0).all() and (got["stats"] == 0).all()
        f["zero"] = 0.0 if exact and all((got[k] == 0).all() for k in which) else np.inf
    else:
        f["finite"] = 0.0 if all(np.isfinite(got[k]).all() for k in ("R", "t", "H", "stats") + tuple(which)) else np.inf
    return f


def bounds():
    return {"R": R_TOL, "H": H_TOL, "T": T_TOL, "centroid": T_TOL, "W": W_TOL, "rotation": ROT_TOL, "pose": T_TOL, "dP": DP_TOL, "dQ": DQ_TOL,
            "dw": DW_TOL, "zero": 0.0, "finite": 0.0}


def check_against_g20(cases, grads, run, label, which=("dP", "dQ", "dw")):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as abi_run does."""
    bnd = bounds()
    worst, rows = {}, []
    for c, g in zip(cases, grads):
        f = figures(c, run(c), g, which)
        rows.append((c, f))
        print("%s %-10s %-6s N=%4d off %5.1f  " % (label, c["family"], c["weights"], c["n"], c["offset"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
            if c["offset"] > 0:
                worst[k + "@offset"] = max(worst.get(k + "@offset", 0.0), float(v))
    print(label, "worst:", "  ".join("%s %.3e" % kv for kv in worst.items()))
    for c, f in rows:
        for k, v in f.items():
            assert v <= bnd[k], (label, c["family"], c["weights"], c["n"], c["offset"], k, v, bnd[k])
    return worst


def host_run(model, c):
    return abi_run(model.model_rigid_align, model.model_rigid_align_bwd, c)


def test_host_model_against_g20(model, g20_cases, g20_grads):
    worst = check_against_g20(g20_cases, g20_grads, lambda c: host_run(model, c), "host")
    # the recorded HOST_* constants are this measurement (to the three digits they are written with)
    for k, host in (("R", HOST_R), ("H", HOST_H), ("T", HOST_T), ("dP", HOST_DP), ("dQ", HOST_DQ), ("dw", HOST_DW)):
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)
    # the condition on the algorithm: far from the origin the rotation is as good as at it
    assert 4 * worst["R@offset"] < 1e-5, worst["R@offset"]


def test_host_model_one_sided_backward_and_null_gradients(model, g20_cases):
    """Each gradient asked for alone equals the three asked for together; a null upstream gradient equals a zero one."""
    for c in g20_cases:
        if c["n"] not in (3, 65) or c["offset"] == 100.0:
            continue
        full = host_run(model, c)
        P, Q, w, gR, gt, gH = (_c(c[k]) for k in ("P", "Q", "w", "gR", "gt", "gH"))
        B, N = ctypes.c_int64(c["b"]), ctypes.c_int32(c["n"])
        for name in ("dP", "dQ", "dw"):
            out = empty_results(c)
            ptrs = {k: np_ptr(out[k]) if k == name else None for k in ("dP", "dQ", "dw")}
            model.model_rigid_align_bwd(np_ptr(P), np_ptr(Q), np_ptr(w), np_ptr(full["H"]), np_ptr(full["R"]), np_ptr(full["stats"]), np_ptr(gR), np_ptr(gt), np_ptr(gH),
                                        ptrs["dP"], ptrs["dQ"], ptrs["dw"], B, N)
            assert np.array_equal(out[name], full[name], equal_nan=True), (c["family"], c["n"], name)
        for drop in range(3):
            gs = [gR, gt, gH]
            zeros = [np.zeros_like(g) if i == drop else g for i, g in enumerate(gs)]
            gs[drop] = None
            a, b = empty_results(c), empty_results(c)
            for out, g3 in ((a, gs), (b, zeros)):
                model.model_rigid_align_bwd(np_ptr(P), np_ptr(Q), np_ptr(w), np_ptr(full["H"]), np_ptr(full["R"]), np_ptr(full["stats"]), np_ptr(g3[0]), np_ptr(g3[1]), np_ptr(g3[2]),
                                            np_ptr(out["dP"]), np_ptr(out["dQ"]), np_ptr(out["dw"]), B, N)
            for name in ("dP", "dQ", "dw"):
                assert np.array_equal(a[name], b[name], equal_nan=True), (c["family"], c["n"], drop, name)
