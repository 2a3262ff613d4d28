"""Chamfer's normal term (so3_chamfer_normals_workspace_bytes, so3_chamfer_normals_fwd_f32, so3_chamfer_normals_bwd_f32 and
chamfer_distance's x_normals / y_normals / abs_cosine) without a GPU: the boundary (header, binding table, exports, argument validation,
the Python surface's errors), the G31 fixture's own consistency, and the kernels' device functions compiled for the host
(tests/host_model/chamfer_normals.cpp with SO3_HOST_MODEL) on G31.

The figures are tests/chamfer_normals_ref.py's (term, rows_n, grad, exact), all against float64 THROUGH THE RETURNED INDICES, and
`bits`, 0 or inf: on the host model (1 / sqrt correctly rounded) term_* and dN* equal the float32 restatement normals32 bit for bit,
and nearest_*, dist_* and the distance rows equal tests/host_model/chamfer.cpp's, the model of the call without normals.  On the device
rsq is a 1-ulp instruction, so there `bits` covers only what the call without normals also produces.

TOLERANCES.  MEASURED holds the largest figures of the float32 host model over G31 (abs and signed cosine, U = 1, 2, 4), measured here;
the host model is held to them as they stand, and the bound of each check on the host and on the GPU alike is 4 x that value.
tests/test_gpu_chamfer_normals.py imports the bounds and the checks; DESIGN.md section 7m quotes them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import chamfer_normals_ref as ref
from support import bits, boundary, build_host_model, lengths_of, np_ptr, on_own_thread

#                                 measured on the host       bound (4 x)
HOST_TERM = 3.289e-7;             TERM_TOL = 4 * HOST_TERM               # noqa: E702
HOST_ROWS_N = 1.207e-7;           ROWS_N_TOL = 4 * HOST_ROWS_N           # noqa: E702
HOST_GRAD = 2.723e-7;             GRAD_TOL = 4 * HOST_GRAD               # noqa: E702
MEASURED = {"term": HOST_TERM, "rows_n": HOST_ROWS_N, "grad": HOST_GRAD}

NEW_SYMBOLS = {"so3_chamfer_normals_workspace_bytes": 3, "so3_chamfer_normals_fwd_f32": 20, "so3_chamfer_normals_bwd_f32": 15}
SRC = os.path.join(ROOT, "tests", "host_model", "chamfer_normals.cpp")
PLAIN_SRC = os.path.join(ROOT, "tests", "host_model", "chamfer.cpp")
CUS = 256                           # the device the host model stands in for
UNSQUARED, SINGLE, SIGNED = 1, 2, 4


# Reasoned, not measured: what the Python surface adds in float32.  The per-cloud loss_normals is the sum of the two rows: their errors
# add, and the sum, below 4, is rounded once (half an ulp of [2, 4) is 2^-23).  A folded scale carries at most two roundings of its own
# (g / B, then / n_b), relative to the coefficient the grad figure is scaled by.
LOSS_N_TOL = 2 * ROWS_N_TOL + 2.0 ** -23
FOLDED_GRAD_TOL = GRAD_TOL + 2 * 2.0 ** -24


def bounds():
    return {"term": TERM_TOL, "rows_n": ROWS_N_TOL, "loss_n": LOSS_N_TOL, "grad": GRAD_TOL, "exact": 0.0, "bits": 0.0}


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert int(re.search(r"#define SO3_CHAMFER_SIGNED_COSINE (\d+)u", raw).group(1)) == _lib.CHAMFER_SIGNED_COSINE == SIGNED
    assert (_lib.CHAMFER_UNSQUARED, _lib.CHAMFER_SINGLE) == (UNSQUARED, SINGLE)


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error

    def fwd(b, n, m, X=p, Y=p, NX=p, NY=p, dist_x=None, near_x=None, dist_y=None, near_y=None, term_x=None, term_y=None, rows=p, rows_n=p, work=p,
            flags=0):
        return lib.so3_chamfer_normals_fwd_f32(X, Y, NX, NY, None, None, dist_x, near_x, dist_y, near_y, term_x, term_y, rows, rows_n, work, flags,
                                               b, n, m, None)

    def bwd(b, n, m, NX=p, NY=p, near_x=p, near_y=p, scale_x=p, scale_y=p, dNX=p, dNY=p, flags=0):
        return lib.so3_chamfer_normals_bwd_f32(NX, NY, None, None, near_x, near_y, scale_x, scale_y, dNX, dNY, flags, b, n, m, None)

    assert fwd(0, 8, 8, X=None, Y=None, NX=None, NY=None, rows=None, rows_n=None, work=None) == 0          # B == 0: a no-op, whatever the pointers
    assert bwd(0, 8, 8, NX=None, NY=None, near_x=None, near_y=None, scale_x=None, scale_y=None, dNX=None, dNY=None) == 0
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert fwd(b, n, m) != 0 and b"so3_chamfer_normals_fwd_f32: B/N/M" in err(), (b, n, m, err())
        assert bwd(b, n, m) != 0 and b"so3_chamfer_normals_bwd_f32: B/N/M" in err(), (b, n, m, err())
    for kw in ({"X": None}, {"Y": None}, {"NX": None}, {"NY": None}, {"rows": None}, {"rows_n": None}, {"work": None}):   # the rest is optional
        assert fwd(4, 8, 8, **kw) != 0 and b"so3_chamfer_normals_fwd_f32: null pointer" in err(), kw
    for kw in ({"dist_y": p}, {"near_y": p}, {"term_y": p}):
        assert fwd(4, 8, 8, flags=SINGLE, **kw) != 0 and b"SO3_CHAMFER_SINGLE" in err(), kw
    for kw in ({"NX": None}, {"NY": None}, {"near_x": None}, {"scale_x": None}, {"dNX": None, "dNY": None}):
        assert bwd(4, 8, 8, **kw) != 0 and b"so3_chamfer_normals_bwd_f32: null pointer" in err(), kw
    for kw in ({"near_y": None}, {"scale_y": None}, {"flags": SINGLE}, {"flags": SINGLE, "near_y": None}, {"flags": SINGLE | SIGNED, "scale_y": None}):
        assert bwd(4, 8, 8, **kw) != 0 and b"SO3_CHAMFER_SINGLE" in err(), kw
    for flags in (8, 16, 1 << 31):
        assert fwd(4, 8, 8, flags=flags) != 0 and err() == b"so3_chamfer_normals_fwd_f32: unknown flag: invalid argument", err()
        assert bwd(4, 8, 8, flags=flags) != 0 and err() == b"so3_chamfer_normals_bwd_f32: unknown flag: invalid argument", err()
    wb, plain = lib.so3_chamfer_normals_workspace_bytes, lib.so3_chamfer_workspace_bytes
    assert wb(-1, 8, 8) == 0 and wb(4, 0, 8) == 0 and wb(4, 8, 0) == 0 and wb(4, big, 8) == 0 and wb(4, 8, big) == 0 and wb(0, 8, 8) == 0
    assert wb(1, 1, 1) == 2 * 2 * 4 and wb(3, 257, 256) == 3 * (2 + 1) * 2 * 4 and wb(2, 1000, 2500) == 2 * (4 + 10) * 2 * 4
    assert all(wb(*s) == 2 * plain(*s) for s in ((1, 1, 1), (5, 1025, 257)))


def test_python_surface_without_gpu():
    import inspect
    import poseestimation_amd as pa
    names = list(inspect.signature(pa.chamfer_distance).parameters)
    assert names[-3:] == ["x_normals", "y_normals", "abs_cosine"] and names[:9] == [
        "X", "Y", "x_lengths", "y_lengths", "squared", "point_reduction", "batch_reduction", "single_directional", "return_nearest"]
    X, Y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for kw in ({"x_normals": X}, {"y_normals": Y}, {"x_normals": X, "single_directional": True}, {"y_normals": Y, "single_directional": True}):
        with pytest.raises(ValueError, match="chamfer_distance: x_normals and y_normals go together"):
            pa.chamfer_distance(X, Y, **kw)
    for fn in (lambda: pa.chamfer_distance(X, Y, x_normals=X, y_normals=Y),
               lambda: pa.chamfer_distance(X, Y, x_normals=X.clone().requires_grad_(), y_normals=Y, abs_cosine=False, return_nearest=True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    with pytest.raises(ValueError, match="chamfer_distance"):
        pa.chamfer_distance(X, Y, point_reduction="max", x_normals=X, y_normals=Y)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g31_cases():
    return ref.cases(ref.g31())


def autograd_gradients(c, signed, scale_x, scale_y):
    """Float64 torch autograd of the spelling two gathers + cosine_similarity + sum on the fixture's own indices, over the live
    points whose pair is not flat (a flat pair has term 1 and no gradient BY DEFINITION)."""
    NX = torch.tensor(c["NX"], dtype=torch.float64).nan_to_num(0.0, 0.0, 0.0).requires_grad_(True)
    NY = torch.tensor(c["NY"], dtype=torch.float64).nan_to_num(0.0, 0.0, 0.0).requires_grad_(True)
    nl, ml = lengths_of(c["x_lengths"], c["b"], c["n"]), lengths_of(c["y_lengths"], c["b"], c["m"])
    total = torch.zeros((), dtype=torch.float64)
    for k in range(c["b"]):
        nb, mb = int(nl[k]), int(ml[k])
        if nb == 0 or mb == 0:
            continue
        for own, other, own32, other32, idx, s in ((NX[k, :nb], NY[k], c["NX"][k, :nb], c["NY"][k], c["nearest_x"][k, :nb], scale_x[k]),
                                                   (NY[k, :mb], NX[k], c["NY"][k, :mb], c["NX"][k], c["nearest_y"][k, :mb], scale_y[k])):
            keep = torch.as_tensor(~ref.flat(own32, other32[idx]))
            cos = torch.nn.functional.cosine_similarity(own[keep], other[torch.as_tensor(idx)][keep], dim=-1, eps=0.0)
            total = total + float(s) * (1.0 - (cos if signed else cos.abs())).sum()
    total.backward()
    return NX.grad.numpy(), NY.grad.numpy()


def test_g31_is_self_consistent(g31_cases):
    import chamfer_ref as cref
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    assert {(c["n"], c["m"]) for c in g31_cases if c["family"] == "random"} == set(ref.SIZES)
    assert {(c["geometry"], c["lengths"]) for c in g31_cases if c["family"] == "random"} == {
        ("random_%dx%d" % s, t) for s in ref.SIZES for t in ("full", "ragged")}
    assert {c["family"] for c in g31_cases} == set(ref.FAMILIES)
    by_name = {c["name"]: c for c in g31_cases}
    for c in g31_cases:
        X, Y, NX, NY, xl, yl = c["X"], c["Y"], c["NX"], c["NY"], c["x_lengths"], c["y_lengths"]
        assert all(a.dtype == np.float32 for a in (X, Y, NX, NY)) and NX.shape == X.shape and NY.shape == Y.shape, c["name"]
        if c["lengths"] == "ragged":
            nl, ml = lengths_of(xl, c["b"], c["n"]), lengths_of(yl, c["b"], c["m"])
            assert nl[0] == 0 and ml[1] == 0 and ml[2] == 1 and nl[3] >= 1 and ml[3] >= 1, c["name"]
        f = cref.chamfer64(X, Y, xl, yl)
        assert np.array_equal(f["nearest_x"], c["nearest_x"]) and np.array_equal(f["nearest_y"], c["nearest_y"]), c["name"]
        assert ref.small_cosines(NX, NY, xl, yl, c["nearest_x"], c["nearest_y"]) == [], c["name"]          # the cosine condition
        sx, sy = ref.scales(c["b"])
        for signed in (False, True):
            w = ref.normals64(NX, NY, xl, yl, c["nearest_x"], c["nearest_y"], signed, sx, sy)
            gX, gY = autograd_gradients(c, signed, sx, sy)
            for got, want, scale in ((gX, w["dNX"], w["SX"]), (gY, w["dNY"], w["SY"])):
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, scale.max()), (c["name"], signed)
        w = ref.normals64(NX, NY, xl, yl, c["nearest_x"], c["nearest_y"], False, sx, sy)
        ws = ref.normals64(NX, NY, xl, yl, c["nearest_x"], c["nearest_y"], True, sx, sy)
        if c["family"] == "random":                        # lengths log-uniform over [2^-10, 2^10]
            ln = np.linalg.norm(np.concatenate([NX.reshape(-1, 3), NY.reshape(-1, 3)]).astype(np.float64), axis=1)
            assert 2.0 ** -10.01 <= ln.min() and ln.max() <= 2.0 ** 10.01 and (c["n"] < 255 or (ln.min() < 2.0 ** -8 and ln.max() > 2.0 ** 8))
        if c["family"] == "sphere":                        # X lies on Y: t_x near 0, and psi near 0 by cancellation (|psi| = sin / |a|, |a| = 1)
            assert 0 <= w["term_x"].max() < 1e-4 and np.abs(ref.psi64(NX[0], NY[0][c["nearest_x"][0]], False)).max() < 1e-2
        if c["family"] == "flipped":                       # abs_cosine gives the unflipped terms, signed 2 - t on the flipped pairs
            base = by_name["sphere:%s/%s" % (c["geometry"], c["lengths"])]
            wb = ref.normals64(base["NX"], base["NY"], xl, yl, c["nearest_x"], c["nearest_y"], True)
            assert np.array_equal(w["term_x"], wb["term_x"]) and np.array_equal(w["term_y"], wb["term_y"])
            odd = c["nearest_x"][0] % 2 == 1
            assert odd.any() and (~odd).any() and np.allclose(ws["term_x"][0, odd], 2 - wb["term_x"][0, odd], atol=1e-15)
            assert np.array_equal(ws["term_x"][0, ~odd], wb["term_x"][0, ~odd])
        if c["family"] == "subset":                        # X inside Y, every point twice in Y, other normals on the second copy
            half = c["m"] // 2
            assert np.array_equal(c["nearest_x"], c["pick"]) and (c["pick"] < half).all() and (f["dist_x"] == 0).all()
            assert np.array_equal(Y[:, :half], Y[:, half:]) and not (NY[:, :half] == NY[:, half:]).any()
            other = ref.term64(NX[0], NY[0, c["pick"][0] + half], False)
            assert np.abs(other - w["term_x"][0]).min() > 1e-6
        if c["family"] == "orthogonal":                    # sab == 0 exactly: t = 1, the gradient 0 under abs_cosine and not under signed
            live = c["nearest_x"] >= 0
            assert (w["term_x"][live] == 1).all() and (w["dNX"] == 0).all() and (w["dNY"] == 0).all()
            assert (np.abs(ws["dNX"]).max(-1)[live] > 0).all()
            assert (np.log2(np.abs(NX).max(-1)) % 1 == 0).all() and ((NX != 0).sum(-1) == 1).all() and ((NY != 0).sum(-1) == 1).all()
        if c["family"] == "degenerate":
            assert (NX[:-1, 0::3] == 0).all() and (NY[:-1, 1::3] == 0).all() and np.isnan(NX[-1]).any() and np.isinf(NY[-1]).any()
            assert np.isfinite(NX[:-1]).all() and np.isfinite(NY[:-1]).all()
            assert (w["term_x"][:, 0::3][c["nearest_x"][:, 0::3] >= 0] == 1).all() and np.isfinite(w["dNX"]).all() and np.isfinite(w["dNY"]).all()
        if c["family"] == "many_to_one":
            assert (c["nearest_y"] == 0).all() and np.linalg.norm(Y[0].astype(np.float64) - X[0, 0], axis=1).max() <= 1e-2 and c["m"] > 512


# ---- the checks, shared with tests/test_gpu_chamfer_normals.py ------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def case_figures(c, got, signed, single=False, plain=None, exact32=False):
    """ref.figures plus what the families promise and `bits`: against `plain`, the results of the call without normals on the same
    input (nearest_*, dist_*, rows), and with exact32 (the host model) term_* and dN* against normals32 through the returned indices."""
    f = ref.figures(c, got, signed, single)
    if f["exact"] != 0.0:
        return f
    wrong = []
    sides = ("x",) if single else ("x", "y")
    if plain is not None:
        wrong += [k + s for s in sides for k in ("nearest_", "dist_") if not same_bits(got[k + s], plain[k + s])]
        wrong += [k for k in ("rows", "loss", "dX", "dY") if k in plain and not same_bits(got[k], plain[k])]
    sx, sy = got.get("scale_x", ref.scales(c["b"])[0]), got.get("scale_y", ref.scales(c["b"])[1])
    if exact32:
        w32 = ref.normals32(c["NX"], c["NY"], c["x_lengths"], c["y_lengths"], got["nearest_x"], None if single else got["nearest_y"], signed, sx,
                            None if single else sy)
        wrong += ["term_" + s for s in sides if not same_bits(got["term_" + s], w32["term_" + s])]
        wrong += [k for k in ("dNX", "dNY") if got.get(k) is not None and not same_bits(np.asarray(got[k]) + 0.0, w32[k] + np.float32(0))]
    if wrong:
        print("%s: arrays whose bits differ: %s" % (c["name"], wrong))
    f["bits"] = np.inf if wrong else 0.0
    nl, ml = lengths_of(c["x_lengths"], c["b"], c["n"]), lengths_of(c["y_lengths"], c["b"], c["m"])
    ok = True
    for k in range(c["b"]):                                                               # padded slots and empty clouds: rows of zeros
        nb, mb = (int(nl[k]), int(ml[k])) if nl[k] > 0 and ml[k] > 0 else (0, 0)
        ok &= all(got.get(key) is None or not (np.asarray(got[key])[k, at:] != 0).any() for key, at in (("dNX", nb), ("dNY", mb)))
        for s, own, other, pb in (("x", c["NX"], c["NY"], nb),) + (() if single else (("y", c["NY"], c["NX"], mb),)):
            if pb and "term_" + s in got:                                                  # a flat pair's term is exactly 1
                fl = ref.flat(own[k, :pb], other[k][np.asarray(got["nearest_" + s])[k, :pb]])
                ok &= bool((np.asarray(got["term_" + s])[k, :pb][fl] == 1).all())
    if c["family"] == "orthogonal":                                                       # sab == 0 exactly
        for s in sides:
            if "term_" + s in got:
                ok &= bool((np.asarray(got["term_" + s])[np.asarray(got["nearest_" + s]) >= 0] == 1).all())
        for key in ("dNX", "dNY"):
            if got.get(key) is not None:
                ok &= bool((np.asarray(got[key]) != 0).any() if signed else (np.asarray(got[key]) == 0).all())
    if c["family"] == "subset":
        ok &= np.array_equal(got["nearest_x"], c["pick"])
    if c["family"] == "many_to_one" and not single:
        ok &= bool((np.asarray(got["nearest_y"]) == 0).all())
    if not ok:
        f["exact"] = np.inf
    return f


def check_against_g31(cases, run, label, single=False, bnd=None, **kw):
    """Print every figure, then hold every case to the bounds, with abs and with signed cosine.  `run(case, signed)` returns the results
    as numpy arrays (and, under "plain", those of the call without normals)."""
    bnd = bounds() if bnd is None else bnd
    worst, rows = {}, []
    for c in cases:
        for signed in (False, True):
            got = run(c, signed)
            f = case_figures(c, got, signed, single, plain=got.get("plain"), **kw)
            rows.append((c, signed, f))
            print("%s %-40s %-6s " % (label, c["name"], "signed" if signed else "abs") + "  ".join("%s %.2e" % kv for kv in f.items()))
            for k, v in f.items():
                worst[k] = max(worst.get(k, 0.0), float(v))
    print(label, "worst:", "  ".join("%s %.3e" % kv for kv in worst.items()))
    for c, signed, f in rows:
        for k, v in f.items():
            assert v <= bnd[k], (label, c["name"], signed, k, v, bnd[k])
    return worst


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib, plain = build_host_model(tmp_path_factory, "chamfer_normals", SRC), build_host_model(tmp_path_factory, "chamfer", PLAIN_SRC)
    P, I64, I32, U32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    lib.model_chamfer_normals_fwd.argtypes = [P] * 14 + [U32, I64, I32, I32, I64, I32]
    lib.model_chamfer_normals_bwd.argtypes = [P] * 10 + [U32, I64, I32, I32]
    plain.model_chamfer_fwd.argtypes = [P] * 9 + [U32, I64, I32, I32, I64]
    lib.model_chamfer_normals_fwd.restype = lib.model_chamfer_normals_bwd.restype = plain.model_chamfer_fwd.restype = None
    lib.plain = plain
    return lib


def abi_run(fwd, bwd, c, signed, single=False, squared=True, fwd_tail=(), bwd_tail=(), work=None):
    """One case through functions with the C ABI's argument order (the host model here): forward into NaN / -2 pre-filled buffers, then
    backward through the returned indices with ref.scales."""
    b, n, m = c["b"], c["n"], c["m"]
    X, Y, NX, NY = (np.ascontiguousarray(c[k]) for k in ("X", "Y", "NX", "NY"))
    xl = None if c["x_lengths"] is None else np.ascontiguousarray(c["x_lengths"], np.int32)
    yl = None if c["y_lengths"] is None else np.ascontiguousarray(c["y_lengths"], np.int32)
    flags = (0 if squared else UNSQUARED) | (SINGLE if single else 0) | (SIGNED if signed else 0)
    out = {"dist_x": np.full((b, n), np.nan, np.float32), "nearest_x": np.full((b, n), -2, np.int32), "term_x": np.full((b, n), np.nan, np.float32),
           "rows": np.full((b, 2), np.nan, np.float32), "rows_n": np.full((b, 2), np.nan, np.float32),
           "dNX": np.full((b, n, 3), np.nan, np.float32), "dNY": np.full((b, m, 3), np.nan, np.float32)}
    if not single:
        out.update(dist_y=np.full((b, m), np.nan, np.float32), nearest_y=np.full((b, m), -2, np.int32), term_y=np.full((b, m), np.nan, np.float32))
    sx, sy = ref.scales(b)
    fwd(np_ptr(X), np_ptr(Y), np_ptr(NX), np_ptr(NY), np_ptr(xl), np_ptr(yl), np_ptr(out["dist_x"]), np_ptr(out["nearest_x"]), np_ptr(out.get("dist_y")), np_ptr(out.get("nearest_y")),
        np_ptr(out["term_x"]), np_ptr(out.get("term_y")), np_ptr(out["rows"]), np_ptr(out["rows_n"]), *(() if work is None else (work,)), flags, b, n, m, *fwd_tail)
    bwd(np_ptr(NX), np_ptr(NY), np_ptr(xl), np_ptr(yl), np_ptr(out["nearest_x"]), np_ptr(out.get("nearest_y")), np_ptr(sx), None if single else np_ptr(sy), np_ptr(out["dNX"]),
        np_ptr(out["dNY"]), flags, b, n, m, *bwd_tail)
    return out


def host_run(model, c, signed, u=0, single=False, squared=True, cus=CUS):
    out = abi_run(model.model_chamfer_normals_fwd, model.model_chamfer_normals_bwd, c, signed, single, squared, fwd_tail=(cus, u))
    b, n, m = c["b"], c["n"], c["m"]
    plain = {"dist_x": np.full((b, n), np.nan, np.float32), "nearest_x": np.full((b, n), -2, np.int32), "rows": np.full((b, 2), np.nan, np.float32)}
    if not single:
        plain.update(dist_y=np.full((b, m), np.nan, np.float32), nearest_y=np.full((b, m), -2, np.int32))
    xl = None if c["x_lengths"] is None else np.ascontiguousarray(c["x_lengths"], np.int32)
    yl = None if c["y_lengths"] is None else np.ascontiguousarray(c["y_lengths"], np.int32)
    # the model of the call without normals picks U by its own rule: the rows' bits are compared where that is the U used here
    model.plain.model_chamfer_fwd(np_ptr(np.ascontiguousarray(c["X"])), np_ptr(np.ascontiguousarray(c["Y"])), np_ptr(xl), np_ptr(yl), np_ptr(plain["dist_x"]),
                                  np_ptr(plain["nearest_x"]), np_ptr(plain.get("dist_y")), np_ptr(plain.get("nearest_y")), np_ptr(plain["rows"]),
                                  (0 if squared else UNSQUARED) | (SINGLE if single else 0), b, n, m, cus)
    if u != 0:
        plain["rows"] = out["rows"]
    out["plain"] = plain
    return out


def test_host_model_against_g31(model, g31_cases):
    """The host model over G31 at U = 1, 2, 4 (the launcher's rule picks 1 at these sizes), held to MEASURED as it stands; the
    recorded constants are this measurement (to the digits they are written with)."""
    worst = {}
    for u in (0, 1, 2, 4):
        w = check_against_g31(g31_cases, lambda c, s: host_run(model, c, s, u), "host U=%d" % u, exact32=True,
                              bnd={**{k: v * 1.005 for k, v in MEASURED.items()}, "exact": 0.0, "bits": 0.0})
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, host in MEASURED.items():
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)


def test_host_model_repeats_single_direction_and_unsquared(model, g31_cases):
    picked = [c for c in g31_cases if c["geometry"] in ("random_257x1025", "subset_100x300")]
    check_against_g31(picked, lambda c, s: host_run(model, c, s, single=True), "host single", single=True, exact32=True)
    check_against_g31(picked[:2], lambda c, s: host_run(model, c, s, squared=False), "host l2", exact32=True)
    c = next(c for c in g31_cases if c["name"] == "random:random_257x1025/ragged")
    a, b = host_run(model, c, False), host_run(model, c, False)
    assert all(same_bits(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k]) for k in a if k != "plain")
    sq, l2 = host_run(model, c, True), host_run(model, c, True, squared=False)
    assert all(same_bits(sq[k], l2[k]) for k in ("term_x", "term_y", "rows_n", "dNX", "dNY"))       # the term does not see the flavour


def test_flat_pairs_and_orthogonal_normals_are_exact(model, g31_cases):
    """A flat pair (a zero, NaN or infinite normal on either side) has term exactly 1 and gives neither normal a gradient; NaN normals
    in one cloud leave the others' bits alone; axis-aligned orthogonal normals give term exactly 1 and, under abs_cosine, gradient 0."""
    c = next(c for c in g31_cases if c["name"] == "degenerate:random_256x1024/full")
    clean = next(x for x in g31_cases if x["name"] == "random:random_256x1024/full")
    for signed in (False, True):
        got = host_run(model, c, signed)
        assert all(np.isfinite(got[k]).all() for k in ("term_x", "term_y", "rows_n", "dNX", "dNY"))
        for own, other, near, term, grad in ((c["NX"], c["NY"], got["nearest_x"], got["term_x"], got["dNX"]),
                                             (c["NY"], c["NX"], got["nearest_y"], got["term_y"], got["dNY"])):
            for k in range(c["b"]):
                fl = ref.flat(own[k], other[k][near[k]])
                dead = ~np.isfinite(own[k]).all(-1) | (own[k] == 0).all(-1)
                assert fl[dead].all() and (term[k][fl] == 1).all() and (grad[k][dead] == 0).all() and dead.sum() > c["n"] // 4
        # the NaN cloud is the last one: give the clean normals to it alone and the other clouds' results keep their bits
        mixed = dict(c, NX=c["NX"].copy(), NY=c["NY"].copy())
        mixed["NX"][-1], mixed["NY"][-1] = clean["NX"][-1], clean["NY"][-1]
        other = host_run(model, mixed, signed)
        assert all(same_bits(got[k][:-1], other[k][:-1]) for k in ("term_x", "term_y", "rows_n", "dNX", "dNY"))
    c = next(c for c in g31_cases if c["name"] == "orthogonal:random_257x1025/full")
    got = host_run(model, c, False)
    assert (got["term_x"] == 1).all() and (got["term_y"] == 1).all() and (got["rows_n"] == 1).all() and (got["dNX"] == 0).all() and (got["dNY"] == 0).all()
    got = host_run(model, c, True)
    assert (got["term_x"] == 1).all() and (np.abs(got["dNX"]).max(-1) > 0).all() and (np.abs(got["dNY"]).max(-1) > 0).all()
