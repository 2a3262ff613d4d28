"""fpfh_features and match_features (so3_spfh_f32, so3_fpfh_f32) without a GPU: the boundary (header, binding table, exports, argument
validation, the Python names), the G32 fixture's own consistency under the margin condition, the kernels' device functions compiled
for the host (tests/host_model/fpfh.cpp with SO3_HOST_MODEL) on G32 and on the branch cases (exact swap ties, features past the outer
edges, the weight rule), and match_features -- plain torch -- against a brute-force loop.

Under the margin condition (tests/fpfh_ref.py) pairs and counts are compared EXACTLY with float64, spfh bit for bit with (100 c) / r,
and fpfh bit for bit with the numpy restatement of its defined order; fpfh against float64 is held to ref.MEASURED here and to 4 x that
on the device.  tests/test_gpu_fpfh.py imports the checks and runs them on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import fpfh_ref as ref
from support import bits, boundary, build_host_model, lengths_of, np_ptr, on_own_thread

NEW_SYMBOLS = {"so3_spfh_f32": 10, "so3_fpfh_f32": 10}
SRC = os.path.join(ROOT, "tests", "host_model", "fpfh.cpp")
GRID_CAP, BLOCK = 8192, 256          # so3proj.hip: kThreeMaxGrid, kBlock


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    boundary(built_library, NEW_SYMBOLS)
    assert _lib.KNN_MAX_K == ref.MAX_K == 64


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error

    def spfh(b, n, k=4, X=p, nrm=p, idx=p, out=p, pairs=p):
        return lib.so3_spfh_f32(X, nrm, idx, None, out, pairs, k, b, n, None)

    def fpfh(b, n, k=4, X=p, idx=p, spfh=p, pairs=p, out=p):
        return lib.so3_fpfh_f32(X, idx, None, spfh, pairs, out, k, b, n, None)

    assert spfh(0, 8, X=None, nrm=None, idx=None, out=None, pairs=None) == 0                    # B == 0: a no-op, whatever the pointers
    assert fpfh(0, 8, X=None, idx=None, spfh=None, pairs=None, out=None) == 0
    big = _lib.ADD_S_MAX_N + 1
    for name, call in ((b"so3_spfh_f32", spfh), (b"so3_fpfh_f32", fpfh)):
        for b, n in ((-1, 8), (2**62, 8), (4, 0), (4, -3), (4, big)):
            assert call(b, n) != 0 and err() == name + b": B/N: invalid argument", (b, n, err())
        for k in (0, -1, 65, 2**31 - 1):
            assert call(4, 8, k) != 0 and err() == name + b": K: invalid argument", (k, err())
            assert call(0, 8, k) != 0 and err() == name + b": K: invalid argument"               # K is checked before the no-op
            assert call(-1, 8, k) != 0 and err() == name + b": B/N: invalid argument"            # ... and B/N before K
    for kw in ({"X": None}, {"nrm": None}, {"idx": None}, {"out": None, "pairs": None}):          # both outputs NULL is an error
        assert spfh(4, 8, **kw) != 0 and err() == b"so3_spfh_f32: null pointer: invalid argument", (kw, err())
    for kw in ({"X": None}, {"idx": None}, {"spfh": None}, {"pairs": None}, {"out": None}):
        assert fpfh(4, 8, **kw) != 0 and err() == b"so3_fpfh_f32: null pointer: invalid argument", (kw, err())


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("fpfh_features", "match_features"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    X, Nr, idx = torch.zeros(2, 7, 3), torch.zeros(2, 7, 3), torch.zeros(2, 7, 4, dtype=torch.long)
    for fn in (lambda: pa.fpfh_features(X, Nr), lambda: pa.fpfh_features(X, Nr, idx), lambda: pa.fpfh_features(X.double(), Nr, idx.int(), return_spfh=True),
               lambda: pa.fpfh_features(X, Nr, None, 3, torch.tensor([1, 2])), lambda: pa.fpfh_features(X[0], Nr)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    for fx, fy in ((torch.zeros(2, 3), torch.zeros(2, 3, 4)), (torch.zeros(2, 3, 4), torch.zeros(1, 3, 4)), (torch.zeros(2, 3, 4), torch.zeros(2, 3, 5)),
                   (torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.long))):
        with pytest.raises(ValueError, match="match_features: expected fx"):
            pa.match_features(fx, fy)
    for kw in ({"x_lengths": torch.tensor([1.0, 2.0])}, {"y_lengths": torch.tensor([1, 2, 3])}, {"x_lengths": [1, 2]}):
        with pytest.raises(ValueError, match="match_features: expected [xy]_lengths"):
            pa.match_features(torch.zeros(2, 3, 4), torch.zeros(2, 5, 4), **kw)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g32_cases():
    return ref.cases(ref.g32())


def sums_of(h):
    """(B, N, 33) -> the three sub-histograms' sums (B, N, 3) in float64."""
    h = np.asarray(h, np.float64)
    return h.reshape(h.shape[:2] + (3, ref.BINS)).sum(-1)


def test_g32_is_self_consistent(g32_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    by_name = {c["name"]: c for c in g32_cases}
    assert {c["family"] for c in g32_cases} == {"sphere", "blob", "lattice_plane", "lattice_column", "coincident", "zero_normals", "mixed", "no_self",
                                                "repeated", "small_k", "k_above_n", "ragged", "nonfinite", "scaled", "moved"}
    for fam in ("sphere", "blob"):
        for n, K in ref.SURFACE_SHAPES:
            c = by_name["%s_%dx%d" % (fam, n, K)]
            assert (c["n"], c["K"]) == (n, K) and (c["pairs"] == K - 1).all(), c["name"]
    for c in g32_cases:
        X, Nr, idx, lengths = c["X"], c["normals"], c["idx"], c["lengths"]
        assert X.dtype == Nr.dtype == np.float32 and idx.dtype == np.int32, c["name"]
        f = ref.features64(X, Nr, idx, lengths)
        assert not (ref.violations(f).any(-1) & c["spfh_rows"]).any(), c["name"]                  # the margin condition
        counts, r = ref.counts_of(f["pair"], f["g"])
        rows = c["spfh_rows"]
        assert np.array_equal(counts[rows], c["counts"][rows]) and np.array_equal(r[rows], c["pairs"][rows]), c["name"]
        if c["family"] != "nonfinite":
            assert rows.all() and c["fpfh_rows"].all() and np.isfinite(X).all() and np.isfinite(Nr).all(), c["name"]
        live = (c["pairs"] > 0)[..., None]
        assert np.abs(sums_of(c["spfh"]) - 100.0 * live)[rows].max() <= 1e-4, c["name"]            # each sub-histogram sums to 100 [r > 0]
        total = sums_of(c["fpfh64"])[c["fpfh_rows"]]
        assert np.abs(total[..., None] - [0.0, 100.0, 200.0]).min(-1).max() <= 1e-9, c["name"]    # ... and of fpfh to 200, 100 or 0
        f32 = ref.fpfh32(X, idx, lengths, c["spfh"], c["pairs"])
        assert (f32[np.arange(c["n"])[None, :] >= lengths_of(lengths, c["b"], c["n"])[:, None]] == 0).all(), c["name"]   # rows past n_b are zeros
        dev = ref.relative_deviation(f32, c["fpfh64"], c["fpfh_rows"])
        assert dev <= ref.MEASURED["fpfh"], (c["name"], dev)                                        # the restatement is an accurate fpfh
    c = by_name["lattice_plane"]
    assert (c["pairs"] == 8).all() and (c["counts"][..., [5, 16, 27]] == 8).all() and (c["normals"] == [0, 0, 1]).all()
    assert (by_name["lattice_column"]["pairs"] == 0).all() and (by_name["lattice_column"]["fpfh64"] == 0).all()
    c = by_name["coincident"]
    assert np.array_equal(c["X"][:, :32], c["X"][:, 32:]) and (c["pairs"] <= 6).all()
    c = by_name["zero_normals"]
    assert (c["normals"][:, ::3] == 0).all() and (c["pairs"][:, ::3] == 0).all() and (c["pairs"][:, 1::3] > 0).all()
    c = by_name["mixed"]
    valid = (c["idx"] >= 0) & (c["idx"] < c["n"])
    assert {-1, c["n"], ref.INT32_MIN} <= set(np.unique(c["idx"][~valid]).tolist()) and (np.diff(valid.astype(int), axis=-1) > 0).any() and (c["pairs"] == 3).all()
    assert (by_name["no_self"]["idx"] != np.arange(64)[None, :, None]).all() and (by_name["no_self"]["pairs"] == 8).all()
    c = by_name["repeated"]
    assert (c["idx"][:, :, 5] == c["idx"][:, :, 2]).all() and (c["pairs"] == 7).all() and (c["counts"].max(-1) >= 2).all()   # a multiset: twice counts twice
    assert [by_name[k]["K"] for k in ("k1", "k2", "k3")] == [1, 2, 3] and (by_name["k1"]["pairs"] == 1).all()
    c = by_name["k_above_n"]
    assert c["K"] > c["n"] and (c["pairs"] == c["n"] - 1).all()
    c = by_name["ragged"]
    nl = lengths_of(c["lengths"], c["b"], c["n"])
    assert list(nl[:3]) == [0, 1, 2] and 1 < nl[3] < c["K"] and nl[4] == c["n"] and all((c["pairs"][b, nl[b]:] == 0).all() for b in range(c["b"]))
    c = by_name["nonfinite"]
    assert np.isnan(c["X"][1]).any() and np.isinf(c["X"][1]).any() and np.isnan(c["normals"][1]).any() and np.isinf(c["normals"][1]).any()
    assert c["spfh_rows"][[0, 2]].all() and c["fpfh_rows"][[0, 2]].all() and 8 <= c["fpfh_rows"][1].sum() < c["spfh_rows"][1].sum() < c["n"]
    for fam in ("sphere", "blob"):                                                              # the moved copy's premises, in float64
        c = by_name["moved_" + fam]
        assert np.array_equal(c["idx"][0], c["idx"][1]) and np.array_equal(c["counts"][0], c["counts"][1]) and np.abs(c["X"][0] - c["X"][1]).max() > 0.1
        assert not ref.moved_premises(c["X"][0], c["normals"][0], c["X"][1], c["normals"][1], c["K"]).any()
    up, down, base = by_name["blob_257x16_up"], by_name["blob_257x16_down"], by_name["blob_257x16"]
    assert np.array_equal(up["X"], base["X"] * np.float32(2.0 ** 20)) and np.array_equal(down["X"] * np.float32(2.0 ** 20), base["X"])


# ---- the checks, shared with tests/test_gpu_fpfh.py -----------------------------------------------------------------------
def check_case(label, c, spfh=None, pairs=None, fpfh=None, bound=ref.FPFH_BOUND):
    """The outputs of one case as numpy arrays (None: not requested), in the rows no non-finite value reaches: pairs and counts EXACTLY
    the float64 ones, spfh bit-equal to (100 c) / r, fpfh bit-equal to the restatement of its defined order FROM spfh and pairs as
    given (the fixture's where they are not) and within `bound` of float64.  -> fpfh's relative deviation from float64 (0.0 without)."""
    what = (label, c["name"])
    rows, frows = c["spfh_rows"], c["fpfh_rows"]
    if pairs is not None:
        assert pairs.dtype == np.int32 and np.array_equal(pairs[rows], c["pairs"][rows]), what
    if spfh is not None:
        assert spfh.dtype == np.float32
        counts = np.rint(spfh.astype(np.float64) * c["pairs"][..., None] / 100.0).astype(np.int64)
        assert np.array_equal(counts[rows], c["counts"][rows]), what
        assert np.array_equal(bits(spfh)[rows], bits(c["spfh"])[rows]), what
    if fpfh is None:
        return 0.0
    s, r = (c["spfh"] if spfh is None else spfh), (c["pairs"] if pairs is None else pairs)
    assert fpfh.dtype == np.float32 and np.array_equal(bits(fpfh)[frows], bits(ref.fpfh32(c["X"], c["idx"], c["lengths"], s, r))[frows]), what
    total = sums_of(fpfh)[frows]
    assert np.abs(total[..., None] - [0.0, 100.0, 200.0]).min(-1).max() <= 200 * 64 * 2.0 ** -23, what      # K terms of 2^-24 relative each, twice
    dev = ref.relative_deviation(fpfh, c["fpfh64"], frows)
    assert dev <= bound, (what, dev, bound)
    return dev


def check_against_g32(cases, run, label, bound=ref.FPFH_BOUND):
    """`run(case)` -> (spfh, pairs, fpfh).  -> fpfh's largest relative deviation from float64 over the fixture."""
    return max(check_case(label, c, *run(c), bound=bound) for c in cases)


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "fpfh", SRC, fp_contract_off=False)     # the header's own pragmas decide, as on the device
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.model_spfh.argtypes = [P, P, P, P, P, P, P, P, I32, I64, I32]
    lib.model_fpfh.argtypes = [P, P, P, P, P, P, I32, I64, I32]
    return lib


def _inputs(c):
    lengths = None if c["lengths"] is None else np.ascontiguousarray(c["lengths"], np.int32)
    return np.ascontiguousarray(c["X"], np.float32), np.ascontiguousarray(c["normals"], np.float32), np.ascontiguousarray(c["idx"], np.int32), lengths


def host_spfh(model, c, features=False):
    """-> (spfh, pairs), with features=True also every slot's (g (B, N, K, 3), pair (B, N, K))."""
    X, Nr, idx, lengths = _inputs(c)
    b, n, K = idx.shape
    spfh, pairs = np.full((b, n, ref.SLOTS), np.nan, np.float32), np.full((b, n), -7, np.int32)
    g = np.full((b, n, K, 3), np.nan, np.float32) if features else None
    pair = np.full((b, n, K), 9, np.uint8) if features else None
    assert model.model_spfh(np_ptr(X), np_ptr(Nr), np_ptr(idx), np_ptr(lengths), np_ptr(spfh), np_ptr(pairs), np_ptr(g), np_ptr(pair), K, b, n) == 0
    return (spfh, pairs, g, pair.astype(bool)) if features else (spfh, pairs)


def host_fpfh(model, c, spfh, pairs):
    X, _, idx, lengths = _inputs(c)
    b, n, K = idx.shape
    out = np.full((b, n, ref.SLOTS), np.nan, np.float32)
    assert model.model_fpfh(np_ptr(X), np_ptr(idx), np_ptr(lengths), np_ptr(np.ascontiguousarray(spfh, np.float32)),
                            np_ptr(np.ascontiguousarray(pairs, np.int32)), np_ptr(out), K, b, n) == 0
    return out


def host_run(model, c):
    spfh, pairs = host_spfh(model, c)
    return spfh, pairs, host_fpfh(model, c, spfh, pairs)


def test_host_model_against_g32(model, g32_cases):
    """Exact counts, exact spfh, fpfh bit-equal to the restatement and within the UN-multiplied figure of float64; twice the same bits."""
    assert model.model_fpfh_slots() == ref.SLOTS
    worst = check_against_g32(g32_cases, lambda c: host_run(model, c), "host", bound=ref.MEASURED["fpfh"])
    print("host model over G32: fpfh's largest relative deviation from float64 %.3g" % worst)
    assert ref.FPFH_BOUND == 4 * ref.MEASURED["fpfh"] and worst > ref.MEASURED["fpfh"] / 2           # the recorded figure is the measured one, not slack
    c = next(c for c in g32_cases if c["name"] == "blob_257x16")
    a, b_ = host_run(model, c), host_run(model, c)
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b_))


def test_host_model_features_stay_inside_the_margin(model, g32_cases):
    """What justifies MARGIN: the float32 features' largest distance from the float64 ones, in bins' units, over every pair of the
    fixture -- at a swap tie from the nearer of the two role assignments, which the condition makes equivalent."""
    worst, seen = 0.0, 0
    for c in g32_cases:
        _, _, g, pair = host_spfh(model, c, features=True)
        f = ref.features64(c["X"], c["normals"], c["idx"], c["lengths"])
        rows = c["spfh_rows"][..., None]
        assert np.array_equal(pair & rows, f["pair"] & rows), c["name"]
        with np.errstate(invalid="ignore"):                                                       # the slots that are no pair may hold NaN
            own, alt = np.abs(g - f["g"]).max(-1), np.abs(g - f["g_alt"]).max(-1)
        dev = np.where(f["tie"], np.minimum(own, alt), own)[f["pair"] & rows]
        worst, seen = max(worst, float(dev.max()) if dev.size else 0.0), seen + dev.size
    print("host model over G32: the largest |g32 - g64| over %d pairs %.3g" % (seen, worst))
    assert seen > 30000 and ref.MEASURED["g"] / 2 < worst <= ref.MEASURED["g"] <= ref.MARGIN / 4


def scaled_case(c, e):
    d = dict(c)
    d["X"] = c["X"] * np.float32(2.0 ** e)
    return d


def check_power_of_two(label, c, base, run, e=20):
    """Scaling the cloud by 2^+-e leaves pairs, spfh and fpfh bit-identical."""
    for ee in (e, -e):
        got = run(scaled_case(c, ee))
        assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(got, base)), (label, c["name"], ee)


def test_host_model_power_of_two(model, g32_cases):
    for c in g32_cases:
        if c["family"] in ("sphere", "blob", "lattice_plane", "coincident", "mixed", "ragged", "moved") and c["n"] <= 257:
            check_power_of_two("host", c, host_run(model, c), lambda d: host_run(model, d))


def check_nonfinite_is_contained(label, c, run):
    """The cloud with NaN and infinite values changes no other cloud, and in its own only the rows that name those values."""
    assert c["name"] == "nonfinite"
    spfh, pairs, fpfh = run(c)
    clean = dict(c)
    clean["X"], clean["normals"] = c["X"][[0, 0, 2]], c["normals"][[0, 0, 2]]
    spfh0, pairs0, fpfh0 = run(clean)
    rows, frows = c["spfh_rows"], c["fpfh_rows"]
    assert np.array_equal(bits(spfh)[rows], bits(spfh0)[rows]) and np.array_equal(pairs[rows], pairs0[rows]), label
    assert np.array_equal(bits(fpfh)[frows], bits(fpfh0)[frows]), label
    assert not np.array_equal(bits(spfh)[1], bits(spfh0)[1]), label                                # ... and it does change those


def test_host_model_nonfinite_is_contained(model, g32_cases):
    check_nonfinite_is_contained("host", next(c for c in g32_cases if c["name"] == "nonfinite"), lambda d: host_run(model, d))


# ---- where the definition branches exactly (tests/fpfh_ref.py: the branch cases) ------------------------------------------------------
def check_branch_case(label, c, spfh, pairs, fpfh):
    """A tie or outer-edge case: pairs and counts EXACTLY the float64 ones, spfh bit-equal to (100 c) / r, fpfh bit-equal to fpfh32.
    Every comparison is exact; fpfh's distance from float64 is G32's measured figure and is not judged on these inputs."""
    check_case(label, c, spfh, pairs, fpfh, bound=float("inf"))


def check_weight_case(label, c, fpfh):
    """so3_fpfh_f32 alone from the GIVEN spfh and pairs: bit-equal to fpfh32, which is finite everywhere."""
    assert fpfh.dtype == np.float32 and fpfh.shape == c["fpfh32"].shape, label
    assert np.array_equal(bits(fpfh), bits(c["fpfh32"])), (label, np.argwhere(bits(fpfh) != bits(c["fpfh32"]))[:4])


def test_branch_cases_reach_their_branches():
    """The generators assert their premises as they build; what the cases promise the tests is re-asserted here."""
    assert [1 << int(np.ceil(np.log2(K))) for K in ref.EDGE_KS] == [8, 16, 64]                   # k_spfh<8>, <16>, <64>
    for K in ref.EDGE_KS:
        ties, outer = ref.branch_cases(K)
        for c in (ties, outer):
            assert (c["b"], c["n"], c["K"]) == (ref.EDGE_B, ref.EDGE_N, K) and c["lengths"].min() < ref.EDGE_N and (c["idx"] == -1).any(), c["name"]
            live = np.array(ref.EDGE_ROWS)[None, :] < lengths_of(c["lengths"], c["b"], c["n"])[:, None]
            assert (c["pairs"][:, ref.EDGE_ROWS][live] >= min(K - 2, 2)).all(), c["name"]          # the judged rows hold the branch's pairs
            assert not ref.undecided(c["f"], c["normals"]).any(), c["name"]
        assert ref.violations(ties["f"]).sum() >= ties["ties_that_differ"] >= ties["ties"] / 2 > 100   # the margin condition rejects them
        assert min(outer["beyond"].values()) >= 2 and ref.violations(outer["f"]).sum() >= sum(outer["beyond"].values())
    w = ref.weight_case()
    assert 4 <= w["n"] <= 8 and np.isfinite(w["fpfh32"]).all()


@pytest.mark.parametrize("K", ref.EDGE_KS)
def test_host_model_swap_ties_and_outer_edges(model, K):
    ties, outer = ref.branch_cases(K)
    for c in (ties, outer):
        base = host_run(model, c)
        check_branch_case("host", c, *base)
        check_power_of_two("host", c, base, lambda d: host_run(model, d))
    _, _, g, pair = host_spfh(model, ties, features=True)                                         # float32 reaches the branch too: a1 == a2 ...
    f = ties["f"]
    assert np.array_equal(pair, f["pair"]) and np.abs(g - f["g"])[pair].max() <= ref.MARGIN / 4
    _, _, g, pair = host_spfh(model, outer, features=True)                                        # ... and g past the outer edges
    f = outer["f"]
    assert np.array_equal(pair, f["pair"])
    beyond = (f["g"] > ref.BINS + ref.OVERSHOOT) | (f["g"] < -ref.OVERSHOOT)
    assert (((g > ref.BINS) | (g < 0)) == beyond)[pair].all() and np.abs(g - f["g"])[pair[..., None] & beyond].max() <= ref.OVERSHOOT / 2


def test_host_model_weight_rule(model):
    c = ref.weight_case()
    check_weight_case("host", c, host_fpfh(model, c, c["spfh"], c["pairs"]))


# ---- match_features: plain torch, so it runs here ----------------------------------------------------------------------------
def match_loop(fx, fy, nl, ml, mutual):
    """The brute-force statement: the nearest live row of fy, the first of equal candidates; -1 past a length or, with mutual,
    where fy's row does not name the row back."""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    out = np.full(fx.shape[:2], -1, np.int64)

    def nearest(a, rows):
        best, at = np.inf, -1
        for j in range(rows.shape[0]):
            d = float(((a - rows[j]) ** 2).sum())
            if d < best:
                best, at = d, j
        return at

    for b in range(fx.shape[0]):
        for i in range(nl[b]):
            j = nearest(fx[b, i], fy[b, :ml[b]])
            if j >= 0 and (not mutual or nearest(fy[b, j], fx[b, :nl[b]]) == i):
                out[b, i] = j
    return out


@pytest.mark.parametrize("mutual", [True, False])
def test_match_features_against_the_loop(mutual):
    import poseestimation_amd as pa
    rng = np.random.default_rng(3200)
    b, n, m, d = 4, 13, 9, 5                                                                      # N != M
    fx = rng.integers(-3, 4, (b, n, d)).astype(np.float32)                                        # small integers: exact distances, many ties
    fy = rng.integers(-3, 4, (b, m, d)).astype(np.float32)
    fy[:, 4] = fy[:, 1]                                                                           # equal candidates: the first one wins
    fx[:, 7] = fx[:, 2]
    for xl, yl in ((None, None), ([13, 0, 5, 1], [9, 4, 0, 1]), ([20, 13, -1, 6], [3, 12, 9, 5])):
        nl, ml = lengths_of(xl, b, n), lengths_of(yl, b, m)
        for dtype in (torch.int32, torch.int64):
            got = pa.match_features(torch.from_numpy(fx), torch.from_numpy(fy), None if xl is None else torch.tensor(xl, dtype=dtype),
                                    None if yl is None else torch.tensor(yl, dtype=dtype), mutual=mutual)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), match_loop(fx, fy, nl, ml, mutual)), (xl, yl)
    want = match_loop(fx, fy, [n] * b, [m] * b, mutual)
    assert (want >= 0).any() and (mutual or (want >= 0).all()) and (not mutual or (want < 0).any())
    assert not (match_loop(fx, fy, [n] * b, [m] * b, False) == 4).any()                            # row 4 repeats row 1: never the first candidate
    assert np.array_equal(pa.match_features(torch.from_numpy(fx).double(), torch.from_numpy(fy), mutual=mutual).numpy(), want)


def test_match_features_empty_sides_and_identity():
    import poseestimation_amd as pa
    for n, m in ((0, 5), (5, 0), (0, 0)):
        got = pa.match_features(torch.zeros(2, n, 4), torch.zeros(2, m, 4))
        assert got.shape == (2, n) and got.dtype == torch.int64 and (got == -1).all()
    assert pa.match_features(torch.zeros(0, 3, 4), torch.zeros(0, 2, 4)).shape == (0, 3)
    f = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 40, 33)).astype(np.float32))
    perm = torch.from_numpy(np.random.default_rng(6).permutation(40))
    got = pa.match_features(f, f[:, perm])                                                        # a permuted copy: the inverse permutation
    assert (f[:, perm].gather(1, got[..., None].expand(-1, -1, 33)) == f).all() and (got >= 0).all()
    f.requires_grad_(True)
    assert not pa.match_features(f, f).requires_grad
