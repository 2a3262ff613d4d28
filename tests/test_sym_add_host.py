"""ADD, ADD-L1 and MSSD up to a symmetry group (so3_sym_add_f32; compute_symmetric_ADD_loss, compute_symmetric_ADD_L1_loss, compute_MSSD)
without a GPU: the boundary (header, binding table, exports, argument validation), the G26 fixture's own consistency, and the kernel's
device functions compiled for the host (tests/host_model/sym_add.cpp with SO3_HOST_MODEL) on G26.

TOLERANCES.  HOST_* are the largest absolute errors of the float32 host model against G26's float64 answers over every case of the
fixture (clouds of unit radius, poses about two units from the origin), measured here; the bound of each check, on the host and on the
GPU alike, is 4 x that value, for the reason tests/test_add_metrics_host.py states (the device's v_sqrt / v_rcp are 1-ulp
approximations and it contracts a * b + c).  A value's error is |dist - the float64 minimum over k|.  Indices are not compared for
equality: the float64 statistic at the returned k may exceed the float64 minimum by at most the value bound (near-ties and the
table's padding may legitimately resolve differently in float32).  Gradients are the largest |difference| of a dT entry against
float64 autograd THROUGH THE RETURNED INDEX, so a tie cannot enter.  The ADD gradient's figure is set by the near_symmetric family:
its residuals d = D p + dt are about 1e-2 long and carry the 1e-7 rounding of D, so a direction u = d / |d| is good to 1e-5 per point
-- the price of the definition, as for ADD-S in tests/test_add_metrics_host.py, not of a kernel.  The ADD-L1 gradient is a sum of
signs; no residual coordinate of the fixture is within rounding of 0 (a flipped sign would move an entry by up to 2 |p| / (3N)), and
the residuals are fmaf chains that the device forms bit for bit as the host does.
tests/test_gpu_sym_add.py imports the bounds from here; DESIGN.md section 7h quotes them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from support import boundary, build_host_model, np_ptr, on_own_thread
import sym_add_ref as ref

#                                 measured on the host       bound (4 x)
HOST_L2 = 8.24e-8;                L2_TOL = 4 * HOST_L2                   # noqa: E702
HOST_L1 = 6.87e-8;                L1_TOL = 4 * HOST_L1                   # noqa: E702
HOST_MSSD = 1.42e-7;              MSSD_TOL = 4 * HOST_MSSD               # noqa: E702
HOST_L2_GRAD = 5.32e-7;           L2_GRAD_TOL = 4 * HOST_L2_GRAD         # noqa: E702
HOST_L1_GRAD = 1.05e-8;           L1_GRAD_TOL = 4 * HOST_L1_GRAD         # noqa: E702

SYMBOL = "so3_sym_add_f32"
NEW_NAMES = ["compute_symmetric_ADD_loss", "compute_symmetric_ADD_L1_loss", "compute_MSSD"]
SRC = os.path.join(ROOT, "tests", "host_model", "sym_add.cpp")
VALUE_TOL = {ref.L2: L2_TOL, ref.L1: L1_TOL, ref.MAX: MSSD_TOL}
GRAD_TOL = {ref.L2: L2_GRAD_TOL, ref.L1: L1_GRAD_TOL}
STAT_KEY = {ref.L2: "stat_l2", ref.L1: "stat_l1", ref.MAX: "stat_max"}


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    raw, _ = boundary(built_library, {SYMBOL: 16})
    for name, value in (("SO3_SYM_ADD_L2", _lib.SYM_ADD_L2), ("SO3_SYM_ADD_L1", _lib.SYM_ADD_L1), ("SO3_SYM_ADD_MAX", _lib.SYM_ADD_MAX)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % name, raw).group(1)) == value
    assert (_lib.SYM_ADD_L2, _lib.SYM_ADD_L1, _lib.SYM_ADD_MAX) == (ref.L2, ref.L1, ref.MAX) and ref.L2 == 0


def test_argument_validation_without_gpu(built_library):
    """Each bad argument returns SO3_ERR_INVALID with a so3_last_error text before any launch; B == 0 is a no-op.  No device is touched."""
    on_own_thread(check_arguments)


def check_arguments():
    from poseestimation_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)             # never dereferenced: every call below returns before a launch

    def call(Tg=f, Tp=f, P=f, S=f, cls=None, C=1, K=4, dists=None, index=None, ls=None, dT=None, flags=0, B=8, N=16):
        return lib.so3_sym_add_f32(Tg, Tp, P, S, cls, C, K, dists, index, ls, dT, 1.0, flags, B, N, None)

    for kw, text in (({"K": 0}, b"K must be in [1, 64]"), ({"K": 65}, b"K must be in [1, 64]"),
                     ({"C": 0}, b"num_classes must be >= 1"), ({"C": -3}, b"num_classes must be >= 1"),
                     ({"C": 5, "K": 64, "cls": f}, b"num_classes * K must be <= 256"),
                     ({"C": 2, "cls": None}, b"class_id must be given"), ({"C": 1, "cls": f}, b"class_id must be given"),
                     ({"S": None}, b"S is null"),
                     ({"B": -1}, b": B/N"), ({"B": 2**62}, b": B/N"), ({"B": 2**31 + 1}, b": B/N"), ({"N": 0}, b": B/N"), ({"N": -3}, b": B/N"),
                     ({"N": 2**31 - 1}, b": B/N"), ({"N": 150000001}, b": B/N"),
                     ({"flags": 3}, b"unknown flag"), ({"flags": 0x100}, b"unknown flag"),
                     ({"Tg": None}, b"null pointer"), ({"Tp": None}, b"null pointer"), ({"P": None}, b"null pointer"),
                     ({"flags": _lib.SYM_ADD_MAX, "dT": f}, b"dTpred must be null with SO3_SYM_ADD_MAX"),
                     ({"flags": _lib.SYM_ADD_MAX, "dT": f, "B": 0}, b"dTpred must be null with SO3_SYM_ADD_MAX")):
        assert call(**kw) == -1, kw
        err = lib.so3_last_error()
        assert b"so3_sym_add_f32" in err and text in err, (kw, err)
    for flags in (_lib.SYM_ADD_L2, _lib.SYM_ADD_L1, _lib.SYM_ADD_MAX):
        assert call(B=0, flags=flags) == 0                                               # a no-op ...
        assert call(B=0, flags=flags, Tg=None, Tp=None, P=None) == 0                     # ... whatever the data pointers
    assert call(B=0, dT=f, dists=f, index=f, ls=f) == 0
    assert call(C=64, K=4, cls=f, B=0) == 0                                              # 256 entries: accepted
    assert call(B=0, N=150000000) == 0


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    for name in NEW_NAMES:
        assert name in pa.__all__ and hasattr(pa, name), name
    table = pa.SymmetryTable(pa.cyclic_symmetry(4, "z"))
    t, pts = torch.eye(4)[None].repeat(2, 1, 1), torch.zeros(2, 5, 3)
    for fn in (lambda: pa.compute_symmetric_ADD_loss(t, t, pts, table), lambda: pa.compute_symmetric_ADD_L1_loss(t, t, pts, table),
               lambda: pa.compute_MSSD(t, t, pts, table), lambda: pa.compute_symmetric_ADD_loss(t, t, pts[0], table, use_batch_mean=False),
               lambda: pa.compute_MSSD(t, t, pts[0], table, return_index=True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    with pytest.raises(TypeError, match="SymmetryTable"):
        pa.compute_MSSD(t, t, pts, pa.cyclic_symmetry(4, "z"))


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g26_cases():
    return ref.cases(ref.g26())


def test_g26_is_self_consistent(g26_cases):
    assert os.path.getsize(ref.GOLDEN) <= 256 * 1024
    assert {c["family"] for c in g26_cases} == set(ref.FAMILIES)
    assert {1, 64, 65} <= {c["n"] for c in g26_cases} and max(c["n"] for c in g26_cases) > 1024            # either side of a wave and of a sweep
    assert any(c["C"] > 1 for c in g26_cases) and {1, 2, 4, 7} <= {c["K"] for c in g26_cases}
    winners = set()
    for c in g26_cases:
        tag = (c["family"], c["n"], c["K"])
        assert c["pts"].dtype == c["tgt"].dtype == c["tpred"].dtype == c["S"].dtype == np.float32 and c["stat_l2"].dtype == np.float64, tag
        assert c["stat_l2"].shape == c["stat_l1"].shape == c["stat_max"].shape == (c["b"], c["K"]) and c["grad_l2"].shape == (c["b"], 4, 4), tag
        assert np.linalg.norm(c["pts"].astype(np.float64), axis=-1).max() <= 1 + 1e-6, tag
        again = ref.answers(c["tgt"], c["tpred"], c["pts"], c["S"], c["cls"])                          # the stored answers are the restatement's
        for k, v in again.items():
            assert np.allclose(v, c[k], rtol=0, atol=1e-14), (tag, k)
        assert (c["stat_max"] >= c["stat_l2"] * (1 - 2.0**-50)).all(), tag                                 # max >= mean
        assert (c["stat_l2"] >= np.sqrt(3.0) * c["stat_l1"] * (1 - 2.0**-50)).all() and (c["stat_l2"] <= 3.0 * c["stat_l1"] * (1 + 2.0**-50)).all(), tag      # |d|_1 / sqrt 3 <= |d|_2 <= |d|_1
        srows = ref.rows_of(c["S"], c["cls"], c["b"])
        assert np.array_equal(srows[:, 0], np.broadcast_to(np.eye(3), (c["b"], 3, 3))), tag                # S_0 = I
        for mode, name in ((ref.L2, "grad_l2"), (ref.L1, "grad_l1")):
            idx = np.argmin(c[STAT_KEY[mode]], axis=1)
            winners.update(idx.tolist())
            assert np.allclose(ref.grad_autograd(mode, c["tgt"], c["tpred"], c["pts"], srows, idx), c[name], rtol=0, atol=1e-12), (tag, name)
            assert (c[name][:, 3] == 0).all(), tag
        if c["family"] == "near_symmetric":
            j = np.arange(c["b"]) % c["K"]
            eq = c["stat_l2"] == c["stat_l2"][np.arange(c["b"]), j][:, None]                            # (the padding repeats the identity's value)
            assert (c["stat_l2"].min(1) == c["stat_l2"][np.arange(c["b"]), j]).all() and (c["stat_l2"].min(1) < 0.02).all(), tag
            assert (np.argmin(c["stat_l2"], axis=1) == np.argmax(eq, axis=1)).all(), tag
        if c["family"] == "exact_c4":
            for k in ("stat_l2", "stat_l1", "stat_max"):
                assert (np.diag(c[k]) == 0).all(), (tag, k)                                             # exact in float64 too
                assert c["n"] == 1 or (c[k][~np.eye(4, dtype=bool)] > 0.1).all(), (tag, k)
        if c["family"] == "identical_points":
            assert (c["pts"] == c["pts"][:, :1]).all() and (c["stat_max"][:, 0] == 0).all() and (c["grad_l2"] == 0).all() and (c["grad_l1"] == 0).all(), tag
    assert len(winners) > 3                                                                             # the winner is not always the identity


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "sym_add", SRC)
    lib.model_sym_add.restype = ctypes.c_int
    lib.model_sym_add.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32] * 2 + [ctypes.c_void_p] * 4 + [ctypes.c_float, ctypes.c_uint32,
                                                                                                            ctypes.c_int64, ctypes.c_int32]
    return lib


def host_run(model, c, grad_scale=1.0):
    """The host model on one case: {mode: {"dist", "index", "grad" (None for MSSD), "all"}} in float32 / int32, NaN / -2 pre-filled."""
    b, n = c["b"], c["n"]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    tg, tp, pts, S = f(c["tgt"]), f(c["tpred"]), f(c["pts"]), f(c["S"])
    cls = None if c["cls"] is None else np.ascontiguousarray(c["cls"], dtype=np.int32)
    out = {}
    for mode in (ref.L2, ref.L1, ref.MAX):
        dist, index = np.full(b, np.nan, np.float32), np.full(b, -2, np.int32)
        every = np.full((b, c["K"]), np.nan, np.float32)
        grad = None if mode == ref.MAX else np.full((b, 4, 4), np.nan, np.float32)
        assert model.model_sym_add(np_ptr(tg), np_ptr(tp), np_ptr(pts), np_ptr(S), np_ptr(cls), c["C"], c["K"], np_ptr(dist), np_ptr(index), np_ptr(every), np_ptr(grad),
                                   grad_scale, mode, b, n) == 0
        out[mode] = {"dist": dist, "index": index, "grad": grad, "all": every}
    return out


def figures(c, got):
    """Largest absolute errors of one case's results `got` (as host_run returns them) against the fixture: the quantities both test
    files bound.  Keys: l2, l1, mssd (values), l2_index, l1_index, mssd_index (the float64 statistic at the returned k over the float64
    minimum), l2_grad, l1_grad (against float64 autograd through the returned index)."""
    srows = ref.rows_of(c["S"], c["cls"], c["b"])
    out = {}
    for mode, name in ((ref.L2, "l2"), (ref.L1, "l1"), (ref.MAX, "mssd")):
        g = got[mode]
        assert g["index"].min() >= 0 and g["index"].max() < c["K"], (name, g["index"])
        out[name], out[name + "_index"] = ref.excess(c[STAT_KEY[mode]], g["dist"], g["index"])
        if mode != ref.MAX:
            want = ref.grad_autograd(mode, c["tgt"], c["tpred"], c["pts"], srows, g["index"])
            out[name + "_grad"] = float(np.abs(g["grad"] - want).max())
    return out


BOUNDS = {"l2": L2_TOL, "l1": L1_TOL, "mssd": MSSD_TOL, "l2_index": L2_TOL, "l1_index": L1_TOL, "mssd_index": MSSD_TOL,
          "l2_grad": L2_GRAD_TOL, "l1_grad": L1_GRAD_TOL}


def check_against_g26(cases, run, label):
    """Print every figure, then hold every case to the bounds.  `run(case)` returns the results as host_run does."""
    worst = {k: 0.0 for k in BOUNDS}
    rows = []
    for c in cases:
        got = run(c)
        f = figures(c, got)
        rows.append((c, f, got))
        print("%s %-16s N=%4d C=%d K=%d  " % (label, c["family"], c["n"], c["C"], c["K"]) + "  ".join("%s %.2e" % kv for kv in f.items()))
        for k, v in f.items():
            worst[k] = max(worst[k], float(v))
    print(label, "worst:", "  ".join("%s %.3e (bound %.3e)" % (k, v, BOUNDS[k]) for k, v in worst.items()))
    for c, f, got in rows:
        for k, v in f.items():
            assert v <= BOUNDS[k], (label, c["family"], c["n"], c["K"], k, v, BOUNDS[k])
        assert (got[ref.MAX]["dist"] >= got[ref.L2]["dist"]).all(), (label, c["family"], c["n"])          # MSSD >= symmetric ADD, every row
        for mode in (ref.L2, ref.L1):
            assert (got[mode]["grad"][:, 3] == 0).all(), (label, c["family"], c["n"])
    return worst


def test_host_model_against_g26(model, g26_cases):
    worst = check_against_g26(g26_cases, lambda c: host_run(model, c), "host")
    # the recorded HOST_* constants are this measurement (to the three digits they are written with)
    for k, host in (("l2", HOST_L2), ("l1", HOST_L1), ("mssd", HOST_MSSD), ("l2_grad", HOST_L2_GRAD), ("l1_grad", HOST_L1_GRAD)):
        assert worst[k] <= host * 1.005, (k, worst[k], host)
    # every candidate's statistic, not only the winner's, is within the value bound
    for c in g26_cases:
        got = host_run(model, c)
        for mode in (ref.L2, ref.L1, ref.MAX):
            assert np.abs(got[mode]["all"] - c[STAT_KEY[mode]]).max() <= VALUE_TOL[mode], (c["family"], c["n"], mode)
            assert np.array_equal(got[mode]["dist"], got[mode]["all"][np.arange(c["b"]), got[mode]["index"]])
            assert np.array_equal(got[mode]["index"], np.argmin(got[mode]["all"], axis=1))             # the first of equal minima


def exact_case_checks(c, got):
    """What must hold exactly, on the host and on the GPU alike."""
    tag = (c["family"], c["n"])
    if c["family"] == "exact_c4":                     # T_pred = T_gt S_j^-1 exactly: candidate j is exactly 0 in every mode, and it is chosen
        for mode in (ref.L2, ref.L1, ref.MAX):
            assert (got[mode]["dist"] == 0).all() and np.array_equal(got[mode]["index"], np.arange(4)), (tag, mode, got[mode])
        assert (got[ref.L2]["grad"] == 0).all(), tag                                                   # u = 0 at d = 0
    if c["family"] == "identical_points":
        for mode in (ref.L2, ref.L1, ref.MAX):
            assert (got[mode]["dist"] == 0).all() and (got[mode]["index"] == 0).all(), (tag, mode)
        assert (got[ref.L2]["grad"] == 0).all() and (got[ref.L1]["grad"] == 0).all(), tag
    if c["family"] == "haar" and c["C"] > 1:           # class 0 is {I} padded with the identity: every candidate ties, the smallest k wins
        for mode in (ref.L2, ref.L1, ref.MAX):
            assert (got[mode]["index"][c["cls"] == 0] == 0).all(), (tag, mode)


def test_host_model_exact_cases(model, g26_cases):
    seen = set()
    for c in g26_cases:
        exact_case_checks(c, host_run(model, c))
        seen.add(c["family"])
        if c["family"] == "exact_c4" and c["n"] > 1:   # plain ADD (the table {I}) is large where the symmetric one is 0
            plain = host_run(model, dict(c, S=c["S"][:, :1], K=1))
            assert (plain[ref.L2]["dist"][1:] > 0.1).all() and (plain[ref.MAX]["dist"][1:] > 0.1).all()
    assert {"exact_c4", "identical_points"} <= seen


def test_host_model_with_the_trivial_table_is_plain_add(model, g26_cases, tmp_path_factory):
    """Table {I}: compute_ADD_loss / compute_ADD_L1_loss's values and gradients within the bounds (not bit for bit: the sweeps' totals
    are added after the butterfly here, k_add_l1 adds per lane across sweeps).  ADD through the host model of k_add_l1<.., L2>
    (tests/host_model/add_metrics.cpp), ADD-L1 through the float64 definition."""
    import test_add_metrics_host as add_host
    add_model = build_host_model(tmp_path_factory, "add_metrics", add_host.SRC)
    eye = np.eye(3, dtype=np.float32).reshape(1, 1, 3, 3)
    for c in g26_cases:
        one = dict(c, S=eye, C=1, K=1, cls=None)
        got = host_run(model, one)
        b, n = c["b"], c["n"]
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        tg, tp, pts = f(c["tgt"]), f(c["tpred"]), f(c["pts"])
        add, g_add = np.full(b, np.nan, np.float32), np.full((b, 4, 4), np.nan, np.float32)
        add_model.model_add_l2(np_ptr(tg), np_ptr(tp), np_ptr(pts), np_ptr(add), np_ptr(g_add), ctypes.c_float(1.0), ctypes.c_int64(b), ctypes.c_int32(n))
        assert np.abs(got[ref.L2]["dist"].astype(np.float64) - add).max() <= L2_TOL and np.abs(got[ref.L2]["grad"].astype(np.float64) - g_add).max() <= L2_GRAD_TOL
        assert (got[ref.L2]["index"] == 0).all() and (got[ref.L1]["index"] == 0).all()
        d = ref.residuals(tg, tp, pts, np.broadcast_to(np.eye(3), (b, 1, 3, 3)))[:, 0]
        assert np.abs(got[ref.L1]["dist"] - np.abs(d).mean((1, 2))).max() <= L1_TOL                      # Iterative/loss.py:10-26
        assert np.abs(got[ref.L2]["dist"] - c["stat_l2"][:, 0]).max() <= L2_TOL                          # candidate 0 of any table is the plain metric


def test_host_model_class_ids_out_of_range(model, g26_cases):
    c = next(c for c in g26_cases if c["C"] > 1 and c["family"] == "haar")
    cls = c["cls"].copy()
    cls[1], cls[4] = -1, c["C"]
    got, clean = host_run(model, dict(c, cls=cls)), host_run(model, c)
    keep = np.ones(c["b"], bool)
    keep[[1, 4]] = False
    for mode in (ref.L2, ref.L1, ref.MAX):
        assert np.isnan(got[mode]["dist"][~keep]).all() and (got[mode]["index"][~keep] == -1).all()
        assert np.array_equal(got[mode]["dist"][keep], clean[mode]["dist"][keep]) and np.array_equal(got[mode]["index"][keep], clean[mode]["index"][keep])
        if mode != ref.MAX:
            assert np.isnan(got[mode]["grad"][~keep][:, :3]).all() and (got[mode]["grad"][:, 3] == 0).all()
            assert np.array_equal(got[mode]["grad"][keep], clean[mode]["grad"][keep])
