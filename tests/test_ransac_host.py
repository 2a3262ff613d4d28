"""ransac_align (so3_ransac_score_f32, so3_ransac_select_f32) without a GPU: the boundary (header, binding table, exports, argument
validation in its order, the Python names), the base case's premises, and the kernels' device functions compiled for the host
(tests/host_model/ransac.cpp with SO3_HOST_MODEL) against the float32 restatement of tests/ransac_ref.py -- admissibility, count and err
bit for bit GIVEN the model's own poses, the selection, weights, targets, inliers and rmse -- on the base case, on small shapes and on
cases built to stand ON each rule's branch.  The pose itself is judged against float64 (ref.POSE_BOUND = 4 x ref.MEASURED).
tests/test_gpu_ransac.py imports the checks and runs them on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import ransac_ref as ref
from support import bits, boundary, build_host_model, np_ptr, on_own_thread

NEW_SYMBOLS = {"so3_ransac_score_f32": 16, "so3_ransac_select_f32": 20}
SRC = os.path.join(ROOT, "tests", "host_model", "ransac.cpp")
TILE = 1024                          # so3_device.h: kRansacTile, the pairs of one LDS tile (test_the_constants_are_the_headers holds it there)


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, NEW_SYMBOLS)
    assert "#define SO3_RANSAC_MAX_HYPOTHESES 1048576" in raw and _lib.RANSAC_MAX_HYPOTHESES == 1 << 20


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error
    inf, nan = float("inf"), float("nan")

    def score(b, n, m=8, h=4, d=0.1, s=0.9, ptrs=None):
        a = dict(P=p, Q=p, corr=p, samples=p, T=p, count=p, err=p)
        a.update(ptrs or {})
        return lib.so3_ransac_score_f32(a["P"], a["Q"], a["corr"], None, None, a["samples"], d, s, a["T"], a["count"], a["err"], b, n, m, h, None)

    def select(b, n, m=8, h=4, d=0.1, s=None, ptrs=None):
        a = dict(P=p, Q=p, corr=p, T=p, count=p, err=p, best=p, T_best=p, inliers=p, rmse=p, weights=p, targets=p)
        a.update(ptrs or {})
        return lib.so3_ransac_select_f32(a["P"], a["Q"], a["corr"], None, None, a["T"], a["count"], a["err"], d, a["best"], a["T_best"], a["inliers"],
                                         a["rmse"], a["weights"], a["targets"], b, n, m, h, None)

    none_score = dict.fromkeys(("P", "Q", "corr", "samples", "T", "count", "err"))
    none_select = dict.fromkeys(("P", "Q", "corr", "T", "count", "err", "best", "T_best", "inliers", "rmse", "weights", "targets"))
    assert score(0, 8, ptrs=none_score) == 0 and select(0, 8, ptrs=none_select) == 0          # B == 0: a no-op, whatever the pointers
    assert score(0, 8, d=nan, s=7.0, ptrs=none_score) == 0 and select(0, 8, d=-1.0, ptrs=none_select) == 0   # ... and the two floats
    big = _lib.ADD_S_MAX_N + 1
    for name, call, keys in ((b"so3_ransac_score_f32", score, none_score), (b"so3_ransac_select_f32", select, none_select)):
        for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
            assert call(b, n, m) != 0 and err() == name + b": B/N/M: invalid argument", (b, n, m, err())
        for h in (0, -1, (1 << 20) + 1, 2**31 - 1):
            assert call(4, 8, 8, h) != 0 and err() == name + b": H: invalid argument", (h, err())
            assert call(0, 8, 8, h) != 0 and err() == name + b": H: invalid argument"                # H is checked before the no-op
            assert call(-1, 8, 8, h) != 0 and err() == name + b": B/N/M: invalid argument"           # ... and B/N/M before H
        for d in (-1e-3, inf, -inf, nan):
            assert call(4, 8, d=d, s=5.0, ptrs=keys) != 0 and err() == name + b": max_distance: invalid argument", (d, err())
        for k in keys:
            assert call(4, 8, ptrs={k: None}) != 0 and err() == name + b": null pointer: invalid argument", (k, err())
    for s in (-1e-3, 1.0 + 1e-6, inf, nan):
        assert score(4, 8, s=s, ptrs=none_score) != 0 and err() == b"so3_ransac_score_f32: edge_similarity: invalid argument", (s, err())


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import neighbors, rotation_representation as rr
    for name in ("ransac_align", "global_registration"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name) is getattr(neighbors, name)
    P, Q, corr = torch.zeros(2, 7, 3), torch.zeros(2, 9, 3), torch.zeros(2, 7, dtype=torch.long)
    for fn in (lambda: pa.ransac_align(P, Q, corr, 0.1), lambda: pa.ransac_align(P, Q, corr.int(), 0.1, samples=torch.zeros(2, 4, 3, dtype=torch.long)),
               lambda: pa.ransac_align(P.double(), Q, corr, 0.1, refine=False, return_info=True), lambda: pa.global_registration(P, Q, 0.1)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "ransac", SRC, fp_contract_off=False)     # the header's own pragmas decide, as on the device
    P, I64, I32, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    lib.model_ransac_score.argtypes = [P, P, P, P, P, P, F, F, P, P, P, I64, I32, I32, I32]
    lib.model_ransac_select.argtypes = [P, P, P, P, P, P, P, P, F, P, P, P, P, P, P, I64, I32, I32, I32]
    return lib


def test_the_constants_are_the_headers(model):
    from poseestimation_amd import _lib
    assert model.model_ransac_tile() == TILE and model.model_ransac_max_hypotheses() == _lib.RANSAC_MAX_HYPOTHESES


def host_score(model, c):
    T = np.full((c["b"], c["h"], 12), np.nan, np.float32)
    count, err = np.full((c["b"], c["h"]), -7, np.int32), np.full((c["b"], c["h"]), np.nan, np.float32)
    assert model.model_ransac_score(np_ptr(c["P"]), np_ptr(c["Q"]), np_ptr(c["corr"]), np_ptr(c["x_len"]), np_ptr(c["y_len"]), np_ptr(c["samples"]),
                                    c["max_distance"], c["edge_similarity"], np_ptr(T), np_ptr(count), np_ptr(err), c["b"], c["n"], c["m"], c["h"]) == 0
    return T, count, err


def host_select(model, c, T, count, err):
    T, count, err = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(count, np.int32), np.ascontiguousarray(err, np.float32)
    B, N = c["b"], c["n"]
    best, inliers = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    T_best, rmse = np.full((B, 12), np.nan, np.float32), np.full(B, np.nan, np.float32)
    weights, targets = np.full((B, N), np.nan, np.float32), np.full((B, N, 3), np.nan, np.float32)
    assert model.model_ransac_select(np_ptr(c["P"]), np_ptr(c["Q"]), np_ptr(c["corr"]), np_ptr(c["x_len"]), np_ptr(c["y_len"]), np_ptr(T), np_ptr(count),
                                     np_ptr(err), c["max_distance"], np_ptr(best), np_ptr(T_best), np_ptr(inliers), np_ptr(rmse), np_ptr(weights),
                                     np_ptr(targets), B, N, c["m"], T.shape[1]) == 0
    return best, T_best, inliers, rmse, weights, targets


# ---- the checks, shared with tests/test_gpu_ransac.py -----------------------------------------------------------------------
def same_bits(a, b):
    return a.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def check_score(label, c, T, count, err):
    """Admissibility is the restatement's, T the identity exactly where it fails, and count / err are the restatement's bits GIVEN T."""
    adm = ref.admissible32(c)
    assert count.dtype == np.int32 and np.array_equal(count >= 0, adm), (label, np.flatnonzero((count >= 0) != adm)[:8])
    assert same_bits(T[~adm], np.broadcast_to(ref.IDENTITY, T[~adm].shape)), label
    want_count, want_err = ref.score32(c, T, adm)
    assert np.array_equal(count, want_count), (label, np.argwhere(count != want_count)[:8])
    assert same_bits(err, want_err), (label, np.argwhere(bits(err) != bits(want_err))[:8])
    return adm


def check_select(label, c, T, count, err, got):
    """so3_ransac_select_f32's six outputs are the restatement's bits from T, count and err as given."""
    want = ref.outputs32(c, T, count, err)
    for name, g, w in zip(("best", "T_best", "inliers", "rmse", "weights", "targets"), got, want):
        g = np.asarray(g).reshape(w.shape)
        ok = same_bits(g, w) if w.dtype == np.float32 else (g.dtype == np.int32 and np.array_equal(g, w))
        assert ok, (label, name, np.argwhere(g != w)[:8])
    return want


def check_case(label, c, run_score, run_select, bound=ref.POSE_BOUND):
    """Both entries on one case.  -> (T, count, err, the select outputs, the pose deviation's four figures)."""
    T, count, err = run_score(c)
    adm = check_score(label, c, T, count, err)
    out = run_select(c, T, count, err)
    check_select(label, c, T, count, err, out)
    rot, tra, judged, total = ref.pose_deviation(c, T, adm)
    assert rot <= bound["rotation"] and tra <= bound["translation"], (label, rot, tra, bound)
    return T, count, err, out, (rot, tra, judged, total)


SHAPES = [(1, 1, 4, 1), (1, 2, 3, 2), (3, 3, 5, 63), (1, 4, 4, 64), (3, 63, 80, 65), (1, 64, 50, 255), (3, 65, 65 + 7, 256), (1, 257, 300, 257),
          (1, 40, 33, 1000)]                                       # (B, N, M, H): M != N on both sides


@pytest.fixture(scope="module")
def base():
    return ref.base_case()


def test_base_case_on_the_host_model(model, base):
    """The base case end to end: the exact checks, the pose bound, and the vote's outcome -- in every whole cloud the winner's inliers ARE the
    true pairs, the refined float64 fit on them is what the pose approximates, and the ragged clouds come out as the definition says."""
    c = base
    T, count, err, out, (rot, tra, judged, total) = check_case("base", c, lambda k: host_score(model, k), lambda k, *a: host_select(model, k, *a))
    print("host model on the base case: rotation %.3g  translation %.3g  over %d of %d admissible triples" % (rot, tra, judged, total))
    assert total >= 40 and total - judged <= 0.2 * total, (judged, total)
    assert rot <= ref.MEASURED["rotation"] and tra <= ref.MEASURED["translation"], (rot, tra)       # MEASURED is this model's own figure
    best, T_best, inliers, rmse, weights, targets = out
    full = c["full"]
    for b in list(range(full)) + [full + 4]:
        assert best[b] >= 0 and np.array_equal(weights[b] > 0, c["true"][b]) and inliers[b] == c["true"][b].sum(), b
        assert 0 < rmse[b] < c["max_distance"]
    for b in range(full, full + 4):                                              # n_b = 0 .. 3: no three distinct valid pairs that pass, or one triple
        assert (count[b] <= 3).all() and (weights[b, c["x_len"][b]:] == 0).all() and (targets[b, c["x_len"][b]:] == 0).all()
    b = full + 5                                                                 # c_b < 3: nothing admissible
    assert (count[b] == -1).all() and best[b] == -1 and inliers[b] == 0 and rmse[b] == 0 and (weights[b] == 0).all()
    assert same_bits(T_best[b], ref.IDENTITY)
    live = ~ref.valid_pairs(c)[b]
    assert same_bits(targets[b][live], c["P"][b][live])                          # an invalid pair's target is the posed point: here the point itself


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_N%d_M%d_H%d" % s)
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_shapes_on_the_host_model(model, shape, ragged):
    c = ref.shape_case(11 + shape[1] + shape[3], *shape, ragged=ragged, edge_similarity=0.5)
    check_case(("shape", shape, ragged), c, lambda k: host_score(model, k), lambda k, *a: host_select(model, k, *a))


# ---- each rule alone, ON its branch ------------------------------------------------------------------------------------------
def triangle_case(p, q, corr=(0, 1, 2), samples=((0, 1, 2),), edge_similarity=0.5, max_distance=0.05, **kw):
    """One cloud whose first three pairs are the triangle p -> q (further rows of p and q ride along)."""
    return ref.make_case(np.asarray(p, np.float32)[None], np.asarray(q, np.float32)[None], np.asarray(corr)[None], np.asarray(samples, np.int32)[None],
                         max_distance=max_distance, edge_similarity=edge_similarity, **kw)


TRI_P = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
TRI_Q = [[4, 2, 1], [5, 2, 1], [4, 3, 1]]                       # TRI_P moved by (4, 2, 1): every edge agrees exactly


def branch_cases():
    """name -> (case, the admissibility each hypothesis must have)."""
    up, down = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    out = {}
    out["plain"] = (triangle_case(TRI_P, TRI_Q), [True])
    out["repeated_index"] = (triangle_case(TRI_P, TRI_Q, samples=((0, 1, 1), (2, 1, 2), (0, 0, 1), (0, 1, 2))), [False, False, False, True])
    out["one_target_twice"] = (triangle_case(TRI_P + [[0, 1, 0]], TRI_Q, corr=(0, 1, 2, 2), samples=((0, 1, 2), (0, 1, 3), (0, 2, 3))), [True, True, False])
    # the edge (0,1) stands exactly on lp2 == s2 lq2: p_1 - p_0 = (1,0,0), q_1 - q_0 = (2,0,0), s2 = 1/4; one ulp below it fails
    q_wide = [[4, 2, 1], [6, 2, 1], [4, 3, 1]]
    out["edge_on_the_bound"] = (triangle_case(TRI_P, q_wide), [True])
    out["edge_one_ulp_below"] = (triangle_case([[0, 0, 0], [down, 0, 0], [0, 1, 0]], q_wide), [False])
    out["edge_other_side_on_the_bound"] = (triangle_case(q_wide, TRI_P), [True])               # lq2 == s2 lp2
    out["edge_other_side_below"] = (triangle_case(q_wide, [[0, 0, 0], [down, 0, 0], [0, 1, 0]]), [False])
    out["similarity_one_exact"] = (triangle_case(TRI_P, TRI_Q, edge_similarity=1.0), [True])
    out["similarity_one_off_by_an_ulp"] = (triangle_case([[0, 0, 0], [up, 0, 0], [0, 1, 0]], TRI_Q, edge_similarity=1.0), [False])
    out["similarity_zero"] = (triangle_case(TRI_P, [[0, 0, 0], [9, 0, 0], [0, 0, 0.125]], edge_similarity=0.0), [True])
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        p4 = TRI_P + [[0.5, 0.5, 0]]
        q4 = TRI_Q + [[4.5, 2.5, 1]]
        for side in ("p", "q"):
            pp, qq = np.array(p4, np.float32), np.array(q4, np.float32)
            (pp if side == "p" else qq)[2, 1] = bad
            out["%s_in_a_sampled_%s" % (name, side)] = (triangle_case(pp, qq, corr=(0, 1, 2, 3), samples=((0, 1, 2), (0, 1, 3)), edge_similarity=0.0),
                                                        [False, True])
            pp, qq = np.array(p4, np.float32), np.array(q4, np.float32)
            (pp if side == "p" else qq)[3, 1] = bad
            out["%s_in_an_unsampled_%s" % (name, side)] = (triangle_case(pp, qq, corr=(0, 1, 2, 3), samples=((0, 1, 2),), edge_similarity=0.0), [True])
    return out


@pytest.mark.parametrize("name", sorted(branch_cases()))
def test_admissibility_branches_on_the_host_model(model, name):
    c, want = branch_cases()[name]
    adm, lp2, lq2 = ref.admissible32(c, return_edges=True)
    assert adm[0].tolist() == want, (name, adm)
    s2 = np.float32(c["edge_similarity"]) ** 2
    if name == "edge_on_the_bound":                                              # reached: the compare is an equality
        assert lp2[0, 0, 0] == s2 * lq2[0, 0, 0] == 1.0
    if name == "edge_one_ulp_below":
        assert s2 * lq2[0, 0, 0] == 1.0 > lp2[0, 0, 0] >= 1.0 - 2.0 ** -22
    if name == "edge_other_side_on_the_bound":
        assert lq2[0, 0, 0] == s2 * lp2[0, 0, 0] == 1.0
    if name == "similarity_one_exact":
        assert np.array_equal(lp2, lq2)
    if name == "similarity_one_off_by_an_ulp":
        assert 1.0 + 2.0 ** -21 >= lp2[0, 0, 0] > lq2[0, 0, 0] == 1.0
    T, count, err, out, _ = check_case(name, c, lambda k: host_score(model, k), lambda k, *a: host_select(model, k, *a),
                                       bound={"rotation": np.inf, "translation": np.inf})
    if "unsampled" in name:                                                      # the bad pair is no inlier and spoils no other: 3 of the 4 rows
        assert count[0, 0] == 3 and np.isfinite(err[0, 0]) and out[4][0].tolist() == [1, 1, 1, 0]
    if "in_a_sampled" in name:                                                   # ... and sampled, it rejects its hypothesis and loses its row
        assert count[0].tolist() == [-1, 3] and out[0][0] == 1 and out[4][0].tolist() == [1, 1, 0, 1]


def select_case(n_rows, p, q, max_distance):
    return ref.make_case(np.asarray(p, np.float32)[None], np.asarray(q, np.float32)[None], np.arange(n_rows)[None], np.zeros((1, 1, 3), np.int32),
                         max_distance=max_distance)


def run_selection_rules(run_select):
    """Crafted T_hyp / count / err straight into so3_ransac_select_f32: the radius' boundary and every tie rule, each reached exactly."""
    c = select_case(3, [[0, 0, 0]] * 3, [[0.5, 0, 0], [0.5, 1.5 * 2.0 ** -13, 0], [0, 0.25, 0]], 0.5)      # d2 == r2, the next float up (0.5625 ulp added), inside
    T = np.tile(ref.IDENTITY, (1, 1, 1))
    d2 = ref.distances32(c, T)[0, 0]
    assert d2[0] == np.float32(0.25) == np.float32(0.5) * np.float32(0.5) and d2[1] == np.nextafter(np.float32(0.25), np.float32(1))
    out = run_select(c, T, np.array([[3]], np.int32), np.array([[0.5]], np.float32))
    check_select("radius", c, T, np.array([[3]], np.int32), np.array([[0.5]], np.float32), out)
    assert np.asarray(out[4]).reshape(-1).tolist() == [1.0, 0.0, 1.0]
    shifts = np.stack([np.concatenate([ref.IDENTITY[:3], [np.float32(k)], ref.IDENTITY[4:]]) for k in range(6)]).astype(np.float32)[None]
    tiny = np.nextafter(np.float32(0.5), np.float32(0))
    for label, count, err, want in (
            ("count decides", [1, 5, 4, 5, 2, -1], [0, 9, 0, 9.5, 0, 0], 1),
            ("err breaks a count tie", [5, 5, 5, 2, 5, -1], [0.5, 0.5, tiny, 0, 0.5, 0], 2),
            ("h breaks a count and err tie", [-1, 4, 5, 5, 5, 1], [0, 0, 0.5, 0.5, 0.5, 0], 2),
            ("the last one wins", [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 7], 5),
            ("all inadmissible", [-1] * 6, [0] * 6, -1),
            ("count 0 beats -1", [-1, -1, -1, 0, -1, 0], [0] * 6, 3)):
        count, err = np.array([count], np.int32), np.array([err], np.float32)
        out = run_select(c, shifts, count, err)
        check_select(label, c, shifts, count, err, out)
        best, T_best, inliers, rmse, weights, _ = (np.asarray(o) for o in out)
        assert best.reshape(-1)[0] == want, (label, best)
        assert same_bits(T_best.reshape(-1), ref.IDENTITY if want < 0 else shifts[0, want]), label
        if want < 0:
            assert inliers.reshape(-1)[0] == 0 and rmse.reshape(-1)[0] == 0 and (weights == 0).all(), label
        if label == "count 0 beats -1":
            assert inliers.reshape(-1)[0] == 0 and rmse.reshape(-1)[0] == 0


def test_selection_rules_on_the_host_model(model):
    run_selection_rules(lambda c, T, count, err: host_select(model, c, T, count, err))
