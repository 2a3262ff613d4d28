"""chamfer_distance (so3_chamfer_workspace_bytes, so3_chamfer_fwd_f32, so3_chamfer_bwd_f32) without a GPU: the boundary (header,
binding table, exports, argument validation, the Python names), the G27 fixture's own consistency, and the kernels' device functions
compiled for the host (tests/host_model/chamfer.cpp with SO3_HOST_MODEL) on G27.

The figures are tests/chamfer_ref.py's (search, dist, rows, grad, exact), all against float64, where indices are compared for equality
only in the exact families -- and `bits` (bit_figure), 0 or inf: the indices, the squared d^2 and the squared gradients EQUAL the float32
restatement of the defined order (chamfer_ref.search32 / grad32), on the host model and on the device.  Clouds are of unit radius, and no non-zero nearest distance of the fixture lies below chamfer_ref.MIN_DISTANCE (asserted by
the generator and again here: a condition on the inputs that keeps v / |v| away from its singularity).

TOLERANCES.  HOST_* are the largest figures of the float32 host model (at 256 compute units) over G27, measured here; the bound of
each check, on the host and on the GPU alike, is 4 x that value (the device's v_rcp / v_sqrt are 1-ulp approximations).
tests/test_gpu_chamfer.py imports the bounds and the checks; DESIGN.md section 7i quotes them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import chamfer_ref as ref
from support import bits, boundary, build_host_model, lengths_of, np_ptr, on_own_thread

#                                 measured on the host       bound (4 x)
HOST_SEARCH = 0.0;                SEARCH_TOL = 4 * HOST_SEARCH           # noqa: E702
HOST_DIST = 4.349e-7;             DIST_TOL = 4 * HOST_DIST               # noqa: E702
HOST_ROWS = 1.209e-7;             ROWS_TOL = 4 * HOST_ROWS               # noqa: E702
HOST_GRAD = 3.521e-7;             GRAD_TOL = 4 * HOST_GRAD               # noqa: E702
MEASURED = {"search": HOST_SEARCH, "dist": HOST_DIST, "rows": HOST_ROWS, "grad": HOST_GRAD}

NEW_SYMBOLS = {"so3_chamfer_workspace_bytes": 3, "so3_chamfer_fwd_f32": 15, "so3_chamfer_bwd_f32": 15}
SRC = os.path.join(ROOT, "tests", "host_model", "chamfer.cpp")
CUS = 256                           # the device the host model stands in for
UNSQUARED, SINGLE = 1, 2


# Reasoned, not measured: what the Python surface adds to the rows in float32.  The per-cloud loss is one more addition (one rounding,
# 2^-24 relative: both rows are >= 0); point_reduction="sum" multiplies a row back by its length, the batch reduction of B clouds adds
# at most B - 1 more roundings (B = 3 in the reductions test): four roundings cover every combination.  A folded scale carries at most
# two roundings of its own (g / B, then / n_b).
LOSS_TOL = ROWS_TOL + 2.0 ** -24
REDUCTION_TOL = ROWS_TOL + 4 * 2.0 ** -24
FOLDED_GRAD_TOL = GRAD_TOL + 2 * 2.0 ** -24
# Inputs that are not the fixture's (the work splits run fresh random clouds of unit radius): a float32 d^2 carries the roundings of
# three subtractions (each counted twice by the square), three products and two additions, at most 8 * 2^-24 relative; the float32
# and the float64 search can disagree when two candidates are closer than both their errors, 16 * 2^-24 d^2 <= 64 * 2^-24 for d <= 2
# (and less for the unsquared term, whose error is half as large relative to d <= 2).
SEARCH_REASONED = 64 * 2.0 ** -24


def bounds():
    return {"search": SEARCH_TOL, "dist": DIST_TOL, "rows": ROWS_TOL, "loss": LOSS_TOL, "grad": GRAD_TOL, "exact": 0.0, "bits": 0.0}


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    for name, value in (("SO3_CHAMFER_UNSQUARED", _lib.CHAMFER_UNSQUARED), ("SO3_CHAMFER_SINGLE", _lib.CHAMFER_SINGLE)):
        assert int(re.search(r"#define %s (\d+)u" % name, raw).group(1)) == value
    assert (_lib.CHAMFER_UNSQUARED, _lib.CHAMFER_SINGLE) == (UNSQUARED, SINGLE)


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error

    def fwd(b, n, m, X=p, Y=p, dist_x=None, near_x=None, dist_y=None, near_y=None, rows=p, work=p, flags=0):
        return lib.so3_chamfer_fwd_f32(X, Y, None, None, dist_x, near_x, dist_y, near_y, rows, work, flags, b, n, m, None)

    def bwd(b, n, m, X=p, Y=p, near_x=p, near_y=p, scale_x=p, scale_y=p, dX=p, dY=p, flags=0):
        return lib.so3_chamfer_bwd_f32(X, Y, None, None, near_x, near_y, scale_x, scale_y, dX, dY, flags, b, n, m, None)

    none = dict(X=None, Y=None)
    assert fwd(0, 8, 8, rows=None, work=None, **none) == 0                                   # B == 0: a no-op, whatever the pointers
    assert bwd(0, 8, 8, near_x=None, near_y=None, scale_x=None, scale_y=None, dX=None, dY=None, **none) == 0
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert fwd(b, n, m) != 0 and b"so3_chamfer_fwd_f32: B/N/M" in err(), (b, n, m, err())
        assert bwd(b, n, m) != 0 and b"so3_chamfer_bwd_f32: B/N/M" in err(), (b, n, m, err())
    for kw in ({"X": None}, {"Y": None}, {"rows": None}, {"work": None}):                    # every other output is optional
        assert fwd(4, 8, 8, **kw) != 0 and b"so3_chamfer_fwd_f32: null pointer" in err(), kw
    for kw in ({"dist_y": p}, {"near_y": p}):
        assert fwd(4, 8, 8, flags=SINGLE, **kw) != 0 and b"SO3_CHAMFER_SINGLE" in err(), kw
    for kw in ({"X": None}, {"Y": None}, {"near_x": None}, {"scale_x": None}, {"dX": None, "dY": None}):
        assert bwd(4, 8, 8, **kw) != 0 and b"so3_chamfer_bwd_f32: null pointer" in err(), kw
    for kw in ({"near_y": None}, {"scale_y": None}, {"flags": SINGLE}, {"flags": SINGLE, "near_y": None}, {"flags": SINGLE, "scale_y": None}):
        assert bwd(4, 8, 8, **kw) != 0 and b"SO3_CHAMFER_SINGLE" in err(), kw
    for flags in (4, 8, 1 << 31):
        assert fwd(4, 8, 8, flags=flags) != 0 and err() == b"so3_chamfer_fwd_f32: unknown flag: invalid argument", err()
        assert bwd(4, 8, 8, flags=flags) != 0 and err() == b"so3_chamfer_bwd_f32: unknown flag: invalid argument", err()
    wb = lib.so3_chamfer_workspace_bytes
    assert wb(-1, 8, 8) == 0 and wb(4, 0, 8) == 0 and wb(4, 8, 0) == 0 and wb(4, big, 8) == 0 and wb(4, 8, big) == 0 and wb(0, 8, 8) == 0
    assert wb(1, 1, 1) == 2 * 4 and wb(3, 257, 256) == 3 * (2 + 1) * 4 and wb(2, 1000, 2500) == 2 * (4 + 10) * 4


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    assert "chamfer_distance" in pa.__all__ and pa.chamfer_distance is rr.chamfer_distance
    X, Y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for fn in (lambda: pa.chamfer_distance(X, Y), lambda: pa.chamfer_distance(X.requires_grad_(), Y, squared=False, return_nearest=True),
               lambda: pa.chamfer_distance(X, Y, torch.tensor([1, 2]), torch.tensor([3, 4]), batch_reduction=None, single_directional=True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    for kw in ({"point_reduction": "max"}, {"batch_reduction": "none"}):
        with pytest.raises(ValueError, match="chamfer_distance"):
            pa.chamfer_distance(X, Y, **kw)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g27_cases():
    return ref.cases(ref.g27())


def gather_gradients(c, scale_x, scale_y):
    """Float64 torch autograd of the gather spelling  sum_b a_b sum_i e(x_i - y_j(i)) + c_b sum_j e(y_j - x_i(j))  on the fixture's own
    indices (e = |v|^2 or |v|), over the live points."""
    X = torch.tensor(c["X"], dtype=torch.float64, requires_grad=True)
    Y = torch.tensor(c["Y"], dtype=torch.float64, requires_grad=True)
    nl, ml = lengths_of(c["x_lengths"], c["b"], c["n"]), lengths_of(c["y_lengths"], c["b"], c["m"])
    total = torch.zeros((), dtype=torch.float64)
    for k in range(c["b"]):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        for P, Q, idx, s in ((X[k, :nb], Y[k], c["nearest_x"][k, :nb], scale_x[k]), (Y[k, :mb], X[k], c["nearest_y"][k, :mb], scale_y[k])):
            v = P - Q[torch.as_tensor(idx, dtype=torch.int64)]
            d2 = (v * v).sum(-1)
            e = d2 if c["squared"] else torch.sqrt(d2[d2 > 0])                        # |v| has no gradient at 0: phi(0) = 0 by definition
            total = total + float(s) * e.sum()
    total.backward()
    return X.grad.numpy(), Y.grad.numpy()


def test_g27_is_self_consistent(g27_cases):
    assert os.path.getsize(ref.GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g21_icp.npz"))
    sizes = {(c["n"], c["m"]) for c in g27_cases if c["family"] == "random"}
    assert sizes == set(ref.SIZES)
    for n, m in ref.SIZES:
        mine = [c for c in g27_cases if (c["n"], c["m"]) == (n, m) and c["family"] == "random"]
        assert {(c["lengths"], c["squared"]) for c in mine} == {(t, s) for t in ("full", "ragged") for s in (True, False)}
    assert {c["family"] for c in g27_cases} == set(ref.FAMILIES)
    for c in g27_cases:
        X, Y, xl, yl = c["X"], c["Y"], c["x_lengths"], c["y_lengths"]
        assert X.dtype == np.float32 and Y.dtype == np.float32 and np.abs(X).max() <= 1 and np.abs(Y).max() <= 1, c["name"]
        if c["lengths"] == "ragged":
            nl, ml = lengths_of(xl, c["b"], c["n"]), lengths_of(yl, c["b"], c["m"])
            assert nl[0] == 0 and ml[1] == 0 and ml[2] == 1 and nl[3] >= 1 and ml[3] >= 1, c["name"]
        assert ref.min_nonzero_distance(X, Y, xl, yl) >= ref.MIN_DISTANCE, c["name"]          # the unsquared gradient's condition
        f = ref.chamfer64(X, Y, xl, yl, c["squared"])
        assert np.array_equal(f["nearest_x"], c["nearest_x"]) and np.array_equal(f["nearest_y"], c["nearest_y"]), c["name"]
        assert np.array_equal(f["rows"], c["rows"]), c["name"]
        sx, sy = ref.scales(c["b"])
        dX, dY, aX, aY = ref.grad64(X, Y, xl, yl, c["nearest_x"], c["nearest_y"], sx, sy, c["squared"])
        gX, gY = gather_gradients(c, sx, sy)
        assert np.abs(dX - gX).max() <= 1e-12 * max(1.0, aX.max()) and np.abs(dY - gY).max() <= 1e-12 * max(1.0, aY.max()), c["name"]
        if c["family"] == "subset":                                                       # X inside Y, every point of it twice in Y
            assert (f["dist_x"] == 0).all() and np.array_equal(c["nearest_x"], c["pick"]) and (c["pick"] < c["m"] // 2).all()
        if c["family"] == "many_to_one":
            assert (c["nearest_y"] == 0).all() and np.linalg.norm(Y[0].astype(np.float64) - X[0, 0], axis=1).max() <= 1e-2
            assert np.abs(np.linalg.norm(X[0, 1:].astype(np.float64) - X[0, 0], axis=1) - 1).max() < 1e-6


# ---- the checks, shared with tests/test_gpu_chamfer.py -----------------------------------------------------------------------
SEARCH32 = {}


def expected_search32(c):
    """ref.search32 of a fixture case, computed once per (geometry, lengths): both flavours, the host model and the device share it."""
    key = (c["geometry"], c["lengths"])
    if key not in SEARCH32:
        SEARCH32[key] = ref.search32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"])
    return SEARCH32[key]


def bit_figure(c, got, single=False):
    """0 or inf: what the definition fixes down to the bits equals the float32 restatement (chamfer_ref.search32, grad32) -- the
    indices in both flavours; in the squared one d^2 and, where the gradients came from ref.scales through the C ABI's argument order
    (the Python surface folds its own scales), dX and dY through the RETURNED indices."""
    want, wrong = expected_search32(c), []
    for side in ("x",) if single else ("x", "y"):
        if not np.array_equal(got["nearest_" + side], want["nearest_" + side]):
            wrong.append(("nearest_" + side, int((np.asarray(got["nearest_" + side]) != want["nearest_" + side]).sum())))
        if c["squared"] and not np.array_equal(bits(got["dist_" + side]), bits(want["dist_" + side])):
            wrong.append(("dist_" + side, int((bits(got["dist_" + side]) != bits(want["dist_" + side])).sum())))
    if c["squared"] and "scale_x" not in got:
        sx, sy = ref.scales(c["b"])
        dX, dY = ref.grad32(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], got["nearest_x"], None if single else got["nearest_y"], sx, None if single else sy)
        wrong += [(k, int((bits(got[k]) != bits(w)).sum())) for k, w in (("dX", dX), ("dY", dY)) if not np.array_equal(bits(got[k]), bits(w))]
    if wrong:
        print("%s: elements whose bits differ from the float32 restatement: %s" % (c["name"], wrong))
    return np.inf if wrong else 0.0


def case_figures(c, got, single=False):
    """The figures of one fixture case for the results `got` of running it forward and backward with ref.scales as the gradient
    scales (or the scale_x, scale_y it carries): dist_x, nearest_x, (dist_y, nearest_y,) rows or loss, dX, dY."""
    f = ref.forward_figures(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["squared"], got, single)
    f["bits"] = bit_figure(c, got, single)
    sx, sy = got.get("scale_x", ref.scales(c["b"])[0]), got.get("scale_y", ref.scales(c["b"])[1])
    if f["exact"] == 0.0:
        f.update(ref.gradient_figures(c["X"], c["Y"], c["x_lengths"], c["y_lengths"], c["squared"], got["nearest_x"],
                                      None if single else got["nearest_y"], sx, None if single else sy, got["dX"], got["dY"]))
    nl, ml = lengths_of(c["x_lengths"], c["b"], c["n"]), lengths_of(c["y_lengths"], c["b"], c["m"])
    for k in range(c["b"]):                                                              # padded slots and empty clouds: rows of zeros
        nb, mb = (int(nl[k]), int(ml[k])) if nl[k] > 0 and ml[k] > 0 else (0, 0)
        if (got["dX"][k, nb:] != 0).any() or (got["dY"][k, mb:] != 0).any():
            f["exact"] = np.inf
    if c["family"] == "subset":              # the x direction exactly 0, the first duplicate, an own term of exactly 0
        own_only = ref.grad64(c["X"], c["Y"], None, None, got["nearest_x"], None, sx, None, c["squared"])[0]
        if not ((got["dist_x"] == 0).all() and np.array_equal(got["nearest_x"], c["pick"]) and ("rows" not in got or got["rows"][:, 0].max() == 0) and
                (own_only == 0).all()):
            f["exact"] = np.inf
    if c["family"] == "many_to_one" and not single:      # every y names x_0: dX[0] is the long chain, the others their own term alone
        own_only = ref.grad64(c["X"], c["Y"], None, None, got["nearest_x"], None, sx, None, c["squared"])
        if not (np.asarray(got["nearest_y"]) == 0).all():
            f["exact"] = np.inf
        f["grad"] = max(f.get("grad", np.inf), ref._relative(got["dX"][:, 1:], own_only[0][:, 1:], own_only[2][:, 1:]))
    return f


def check_against_g27(cases, run, label, single=False, bnd=None):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as numpy arrays."""
    bnd = bounds() if bnd is None else bnd
    worst, rows = {}, []
    for c in cases:
        f = case_figures(c, run(c), single)
        rows.append((c, f))
        print("%s %-34s " % (label, c["name"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    print(label, "worst:", "  ".join("%s %.3e" % kv for kv in worst.items()))
    for c, f in rows:
        for k, v in f.items():
            assert v <= bnd[k], (label, c["name"], k, v, bnd[k])
    return worst


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "chamfer", SRC)
    P, I64, I32, U32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    lib.model_chamfer_fwd.argtypes = [P] * 9 + [U32, I64, I32, I32, I64]
    lib.model_chamfer_bwd.argtypes = [P] * 10 + [U32, I64, I32, I32]
    lib.model_chamfer_points_per_lane.argtypes = [I64, I32, I32, I32, I64]
    lib.model_chamfer_fwd.restype = lib.model_chamfer_bwd.restype = None
    return lib


def abi_run(fwd, bwd, c, single=False, fwd_tail=(), bwd_tail=(), work=None):
    """One case through functions with the C ABI's argument order (the host model here, the library's entries on numpy-like
    buffers): forward into NaN / -2 pre-filled buffers, then backward through the returned indices with ref.scales."""
    b, n, m = c["b"], c["n"], c["m"]
    X, Y = np.ascontiguousarray(c["X"]), np.ascontiguousarray(c["Y"])
    xl = None if c["x_lengths"] is None else np.ascontiguousarray(c["x_lengths"], np.int32)
    yl = None if c["y_lengths"] is None else np.ascontiguousarray(c["y_lengths"], np.int32)
    flags = (0 if c["squared"] else UNSQUARED) | (SINGLE if single else 0)
    out = {"dist_x": np.full((b, n), np.nan, np.float32), "nearest_x": np.full((b, n), -2, np.int32), "rows": np.full((b, 2), np.nan, np.float32),
           "dX": np.full((b, n, 3), np.nan, np.float32), "dY": np.full((b, m, 3), np.nan, np.float32)}
    if not single:
        out.update(dist_y=np.full((b, m), np.nan, np.float32), nearest_y=np.full((b, m), -2, np.int32))
    sx, sy = ref.scales(b)
    fwd(np_ptr(X), np_ptr(Y), np_ptr(xl), np_ptr(yl), np_ptr(out["dist_x"]), np_ptr(out["nearest_x"]), np_ptr(out.get("dist_y")), np_ptr(out.get("nearest_y")), np_ptr(out["rows"]),
        *(() if work is None else (work,)), flags, b, n, m, *fwd_tail)
    bwd(np_ptr(X), np_ptr(Y), np_ptr(xl), np_ptr(yl), np_ptr(out["nearest_x"]), np_ptr(out.get("nearest_y")), np_ptr(sx), None if single else np_ptr(sy), np_ptr(out["dX"]), np_ptr(out["dY"]),
        flags, b, n, m, *bwd_tail)
    return out


def host_run(model, c, cus=CUS, single=False):
    return abi_run(model.model_chamfer_fwd, model.model_chamfer_bwd, c, single, fwd_tail=(cus,))


def test_host_model_against_g27(model, g27_cases):
    worst = check_against_g27(g27_cases, lambda c: host_run(model, c), "host")
    # the recorded HOST_* constants are this measurement (to the three digits they are written with)
    for k, host in MEASURED.items():
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)


def test_host_model_single_direction_and_work_item_sizes(model, g27_cases):
    """The x direction alone (dY then holds the x direction's hits), and U = 1, 2, 4 as the device grows smaller: the partial sums are
    combined in another order, within the same bounds, and the search itself does not depend on U."""
    picked = [c for c in g27_cases if c["geometry"] in ("random_257x1025", "subset_300x700")]
    check_against_g27(picked, lambda c: host_run(model, c, single=True), "host single", single=True)
    c = next(c for c in g27_cases if c["name"] == "random_1000x2500/ragged/l2")
    seen = {}
    for cus in (256, 10, 0):
        u = model.model_chamfer_points_per_lane(c["b"], c["n"], c["m"], 0, cus)
        seen[u] = host_run(model, c, cus)
        f = case_figures(c, seen[u])
        print("host U=%d " % u + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            assert v <= bounds()[k], (u, k, v)
    assert sorted(seen) == [1, 2, 4]
    assert all(np.array_equal(seen[u]["nearest_x"], seen[1]["nearest_x"]) and np.array_equal(seen[u]["nearest_y"], seen[1]["nearest_y"]) for u in seen)
    a, b = host_run(model, c), host_run(model, c)
    assert all(np.array_equal(a[k], b[k]) for k in a)
