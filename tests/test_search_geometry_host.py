"""The work splits of the two N^2 kernels (k_add_s, k_icp_step) without a GPU: what tests/test_gpu_search_geometry.py expects is proven
here.  The geometry table of tests/search_geometry_ref.py at 256 compute units; the exact (lattice) families' self-consistency -- exact
in float32, the float64 restatement gives the integers' answer, the ties and the last-point cases are what they claim --; the two host
models (tests/host_model/add_metrics.cpp, icp.cpp) on the exact families, index for index, and on one random case per tile, unroll and
chunk edge at the bounds the GPU tests use (test_add_metrics_host.BOUNDS, test_icp_host.bounds(): unchanged); and the condition on the
random ICP families: by the float64 reference alone at most 5 % of the clouds of any case have a step that is not unique, none at
N >= 255 (N < 3 aside, where no step is).  The host models loop in index order: they have no tiles, chunks or grid, and stay that way."""
import numpy as np
import pytest
import torch

import add_metrics_ref as aref
import f32_exact as fx
import icp_ref
import search_geometry_ref as geo
import test_add_metrics_host as ahost
import test_icp_host as ihost
from test_add_metrics_host import model as adds_model          # noqa: F401 -- the host models' fixtures, under their own names
from test_icp_host import model as icp_model                   # noqa: F401

CASES = geo.cases(geo.CUS)
CPU_PAIRS = 1 << 24                  # float64 pairs per case here: the GPU file checks 32 times as many


@pytest.fixture(scope="module", autouse=True)
def _release_the_shared_batches():
    yield
    geo.adds_shared.cache_clear()                    # G5's batch is a few hundred MB on the host
    geo.icp_shared.cache_clear()


def test_the_geometry_table_at_256_compute_units():
    c = CASES
    assert list(c) == geo.IDS
    assert (c["G1"]["u"], geo.chunks(2500, 1), -(-2500 // geo.TILE), 2500 % geo.TILE, -2500 % geo.UNROLL) == (1, 10, 3, 452, 4)
    assert (c["G2"]["b"], c["G2"]["u"], geo.chunks(1025, 2), 1025 - 2 * 512) == (171, 2, 3, 1) and geo.rule(170, 1025, 256) == 1
    assert (c["G3"]["b"], c["G3"]["u"], geo.chunks(1025, 4)) == (256, 4, 2) and geo.rule(255, 1025, 256) == 2
    assert (c["G4"]["b"], c["G4"]["u"], c["G4"]["u_adds"]) == (64 * 256 + 37, 4, 4) and c["G4"]["items"] > c["G4"]["cap"] and c["G4"]["b"] > 4 * 8 * 256
    assert (c["G5"]["b"], c["G5"]["u"], c["G5"]["items"]) == (32 * 256 + 5, 4, 64 * 256 + 10) and c["G5"]["items"] > c["G5"]["cap"]
    assert c["G4"]["b"] > 4 * 16 * 256                                                   # k_icp_finish's grid: 16 workgroups of 4 waves per CU
    for k, v in c.items():
        if k[:2] in ("G6", "G7"):
            assert v["b"] == 2 and v["u"] == 1 and v["u_adds"] == 1, k
        assert v["u"] == v["u_adds"] or k == "G4", k
    assert {v["u"] for v in c.values()} == {1, 2, 4} == {v["u_adds"] for v in c.values()}
    pairs = {(v["n"], v["m"]) for v in c.values()}
    assert pairs >= {(1025, 1023), (257, 2049), (geo.ICP_N4, geo.ICP_M4), (1025, 1025)}
    assert max(v["b"] * v["n"] * v["m"] for v in c.values()) < 9e9
    # batches of <= 64 clouds, which the bitwise checks re-run a case in, are U = 1 at both of its sizes
    assert geo.rule(64, 1025, 256) == 1 and geo.rule(64, geo.ICP_N4, 256) == 1 and geo.rule(64, geo.ADDS_N4, 256) == 1


# ---- the exact families ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adds_families():
    return [geo.exact_adds_family(name, n, b, geo.exact_seed(name, n)) for name, n, b in geo.EXACT_ADDS] + \
        [geo.exact_adds_family("identical", 1025, CASES[k]["b"], geo.exact_seed("identical", 1025)) for k in ("G2", "G3")]


@pytest.fixture(scope="module")
def search_families():
    return [geo.exact_search_family(name, n, geo.exact_seed(name, n) + 1) for name, n in geo.EXACT_SEARCH]


def _on_lattice(a, limit):
    k = np.asarray(a, np.float64) / geo.QUANTUM
    return bool((k == np.round(k)).all() and np.abs(k).max() <= limit)


def test_exact_families_are_what_they_claim(adds_families, search_families):
    for f in adds_families:
        tag = (f["name"], f["n"], f["b"])
        n = f["n"]
        assert f["pts"].dtype == np.float32 and _on_lattice(f["pts"], 64) and _on_lattice(f["tgt"][:, :3, 3], 132) and _on_lattice(f["tpred"][:, :3, 3], 128), tag
        for T in (f["tgt"], f["tpred"]):
            R = T[:, :3, :3].astype(np.float64)
            assert (np.abs(R).sum(1) == 1).all() and (np.abs(R).sum(2) == 1).all() and (np.linalg.det(R) == 1).all() and (T[:, 3] == [0, 0, 0, 1]).all(), tag
        if f["name"] == "identical":
            assert np.array_equal(f["tgt"], f["tpred"]) and (f["d2"] == 0).all() and (f["count"] == 1).all(), tag
            assert (f["nearest"] == np.arange(n)).all(), tag
        if f["name"] == "ties":
            assert n == 2049 and np.array_equal(f["tgt"], f["tpred"]) and (f["d2"] == 0).all(), tag
            want = np.arange(n)
            for dup, first in geo.TIES.items():
                want[dup] = first
            assert (f["nearest"] == want).all() and (f["count"][:, [5, 1023, 1024, 2048]] == 4).all() and (f["count"][:, [1030, 2047]] == 2).all(), tag
            assert (f["count"].sum(1) == n + 4 * 3 + 2).all(), tag                    # no other duplicates
            assert {1023 // geo.TILE, 1024 // geo.TILE, 2048 // geo.TILE} == {0, 1, 2}
        if f["name"] == "last_wins":
            assert n % geo.UNROLL == 1 and len(f["special"]) == 3, tag
            sp = f["special"] + [n - 1]
            assert (f["nearest"][:, sp] == n - 1).all() and (f["count"][:, sp] == 1).all(), tag      # the unique nearest: the last point
            assert (f["d2"][:, f["special"]] == 1).all() and (f["d2"][:, n - 1] == 16).all(), tag
        # float32 arithmetic is exact on these inputs: posing in float32 gives the integers, so float64 has nothing to add
        if f["b"] <= 4:
            tg, tp, p = (torch.as_tensor(f[k], dtype=torch.float64) for k in ("tgt", "tpred", "pts"))
            x32 = (torch.as_tensor(f["pts"]) @ torch.as_tensor(f["tgt"])[:, :3, :3].transpose(1, 2) + torch.as_tensor(f["tgt"])[:, None, :3, 3]).double()
            assert torch.equal(x32, aref.pose64(tg, p)), tag
            for i in range(f["b"]):
                pd, nn = aref.adds_parts64(tg[i:i + 1], tp[i:i + 1], p[i:i + 1])
                assert np.array_equal(nn[0].numpy(), f["nearest"][i]) and np.abs(pd[0].numpy() - geo.lattice_dist(f["d2"][i])).max() <= 1e-15, tag      # (torch's vectorised root: 1 ulp of float64)
                assert abs(aref.diameter64(p[i:i + 1]).item() - np.sqrt(geo.lattice_diameter2(f["ints"][i])) * geo.QUANTUM) <= 1e-15, tag
    for f in search_families:
        tag = (f["name"], f["n"])
        assert _on_lattice(f["X"], 68) and _on_lattice(f["Y"], 64), tag
        d, idx = icp_ref.nearest64(f["X"], f["Y"])
        assert np.array_equal(idx, f["nearest"]) and np.abs(d - geo.lattice_dist(f["d2"])).max() <= 1e-15, tag
        if f["name"] == "ties":
            assert (f["d2"] == 0).all() and (f["nearest"][:, [1023, 1024, 2048]] == 5).all() and (f["nearest"][:, 2047] == 1030).all(), tag
        else:
            assert (f["nearest"][:, f["special"] + [f["n"] - 1]] == f["n"] - 1).all() and (f["count"][:, f["special"]] == 1).all(), tag


def adds_case(tgt, tpred, pts):
    """An add_metrics case as test_add_metrics_host.figures reads it, its float64 answers from add_metrics_ref one cloud at a time."""
    tgt, tpred, pts = (np.ascontiguousarray(a, dtype=np.float32) for a in (tgt, tpred, pts))
    parts = [aref.answers(tgt[i:i + 1], tpred[i:i + 1], pts[i:i + 1]) for i in range(len(pts))]
    return {"family": "geometry", "b": len(pts), "n": pts.shape[1], "tgt": tgt, "tpred": tpred, "pts": pts,
            **{k: np.concatenate([p[k] for p in parts]) for k in parts[0]}}


def test_host_models_on_the_exact_families(adds_model, icp_model, adds_families, search_families):
    """Index for index, the distance the correctly rounded root of the exact square, the gradient of an exact zero exactly zero."""
    for f in adds_families:
        tag = (f["name"], f["n"], f["b"])
        f = dict(f, b=min(f["b"], 6), **{k: f[k][:6] for k in ("tgt", "tpred", "pts", "d2", "nearest")})      # (a large batch repeats four clouds)
        got = ahost.host_run(adds_model, f)
        want = geo.lattice_dist(f["d2"]).astype(np.float32)
        assert np.array_equal(got["nearest"], f["nearest"]) and np.array_equal(got["point_dist"], want), tag
        assert (np.abs(got["adds"] - want.astype(np.float64).sum(1) / f["n"]) <= geo.ulp32(got["adds"])).all(), tag
        diam = np.array([np.sqrt(geo.lattice_diameter2(f["ints"][i % len(f["ints"])])) * geo.QUANTUM for i in range(f["b"])])
        assert np.array_equal(got["diam"], diam.astype(np.float32)), tag
        if f["name"] in ("identical", "ties"):
            assert (got["grad_adds"] == 0).all() and (got["point_dist"] == 0).all(), tag
    for f in search_families:
        c = {"kind": "search", "b": 2, "n": f["n"], "m": f["m"], "shared": False, "P": f["X"], "Q": f["Y"]}
        got = ihost.host_run(icp_model, c)
        assert np.array_equal(got["nearest"], f["nearest"]) and np.array_equal(got["dist"], geo.lattice_dist(f["d2"]).astype(np.float32)), (f["name"], f["n"])


# ---- the host models on one random case per edge, at the GPU file's bounds --------------------------------------------------------------
EDGES = [k for k in geo.IDS if k[:2] in ("G6", "G7")]


@pytest.mark.parametrize("case_id", EDGES)
def test_host_add_metrics_at_every_edge(adds_model, case_id):
    c = CASES[case_id]
    tg, tp, pts = geo.adds_inputs(c["b"], c["n_adds"], 600 + geo.IDS.index(case_id))
    case = adds_case(tg.numpy(), tp.numpy(), pts.numpy())
    got = ahost.host_run(adds_model, case)
    f = ahost.figures(case, got)
    # the defined bits: both clouds through pose_point's fmaf order, pair_dist2, the first of equal candidates -- indices EQUAL
    posed = [fx.pose_point32(case[k].reshape(-1, 16)[:, :12], case["pts"]) for k in ("tgt", "tpred")]
    assert np.array_equal(got["nearest"], geo.nearest32(*posed)), case_id
    print("host %-8s " % case_id + "  ".join("%s %.2e" % kv for kv in f.items()))
    for k, v in f.items():
        assert v <= ahost.BOUNDS[k], (case_id, k, v, ahost.BOUNDS[k])


def icp_case(case, d, shared, max_distance, iterations):
    return {"kind": "step", "b": case["b"], "n": case["n"], "m": case["m"], "shared": shared, "P": d["Ps"] if shared else d["P"],
            "Q": d["Qs"] if shared else d["Q"], "w": d["w"], "R0": d["R0"], "t0": d["t0"], "max_distance": max_distance, "iterations": iterations}


def split_step_figures(P, Q, w, R0, t0, max_distance, got, unique, it=0):
    """test_icp_host.step_figures over a batch whose clouds are judged in full where `unique`, on properties where not."""
    f = {}
    for keep, check in ((unique, icp_ref.FULL), (~unique, icp_ref.PROPERTIES)):
        if not keep.any():
            continue
        sub = {k: (v[:, keep] if k in ("rmse", "inliers") else v[keep]) for k, v in got.items()}
        part = ihost.step_figures(P[keep], Q if np.ndim(Q) == 2 else Q[keep], None if w is None else w[keep], R0[keep], t0[keep], max_distance, sub, check, it)
        for k, v in part.items():
            f[k] = max(f.get(k, 0.0), v if np.ndim(v) == 0 else max(v))
    return f


@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("case_id", EDGES)
def test_host_icp_at_every_edge(icp_model, case_id, shared):
    c = CASES[case_id]
    d = geo.icp_case_inputs(c, geo.CUS)
    case = icp_case(c, d, shared, None, 1)
    got = ihost.host_run(icp_model, case)
    R0, t0 = geo.initial64(d, c["b"])
    X = icp_ref.pose_points(case["P"], R0, t0)
    dmin, idx = icp_ref.nearest64(X, case["Q"])
    f = ihost.search_figures(X, case["Q"], got["dist"], got["nearest"], dmin)
    assert d["R0"] is None and np.array_equal(got["nearest"], geo.nearest32(case["P"], case["Q"])), case_id      # unposed: the raw points' defined bits
    unique = geo.unique_step(icp_ref.step_from(case["P"], case["Q"], idx, dmin, R0, t0, case["w"], None))
    f.update(split_step_figures(case["P"], case["Q"], case["w"], R0, t0, None, got, unique))
    print("host %-8s %-6s " % (case_id, "shared" if shared else "own") + "  ".join("%s %.2e" % kv for kv in f.items()))
    for k, v in f.items():
        assert v <= ihost.bounds()[k], (case_id, k, v, ihost.bounds()[k])


def test_host_icp_on_the_whole_of_g4(icp_model):
    """G4 weighted and trimmed over two iterations, every cloud, the second iteration judged from the first one's returned pose.  Among
    16 421 clouds of about ten inliers some pass the uniqueness criterion with (s2 + s3) / s1 = 0.16 and s3 / s1 = 0.003: their rotation
    amplifies the rounding of H sixfold, and the host model itself exceeds G21's R_TOL and T_TOL on them.  So those two bounds are defined
    for this shape by the host model on this shape: test_icp_host.HOST_R_G4 / HOST_T_G4 are this measurement, bounds_g4() is 4 x them.
    Every other figure stays within bounds()."""
    c = CASES["G4"]
    d = geo.icp_case_inputs(c, geo.CUS)
    worst = {}
    for shared in (False, True):
        P, Q = (d["Ps"], d["Qs"]) if shared else (d["P"], d["Q"])
        R0, t0 = geo.initial64(d, c["b"])
        md = geo.max_distance_for(P, Q, d["w"], R0, t0, 2)
        one = ihost.host_run(icp_model, icp_case(c, d, shared, md, 1))
        two = ihost.host_run(icp_model, icp_case(c, d, shared, md, 2))
        assert np.array_equal(two["rmse"][0], one["rmse"][0]) and np.array_equal(two["inliers"][0], one["inliers"][0])
        T0 = np.concatenate([d["R0"], d["t0"][:, :, None]], 2).reshape(-1, 12)       # the first search: the source through pose_point32, indices EQUAL
        assert np.array_equal(one["nearest"], geo.nearest32(fx.pose_point32(T0, P), Q)), shared
        for got, (Ra, ta), it in ((one, (R0, t0), 0), (two, (one["R"].astype(np.float64), one["t"].astype(np.float64)), 1)):
            X = icp_ref.pose_points(P, Ra, ta)
            dmin, idx = icp_ref.nearest64(X, Q)
            f = ihost.search_figures(X, Q, got["dist"], got["nearest"], dmin)
            unique = geo.unique_step(icp_ref.step_from(P, Q, idx, dmin, Ra, ta, d["w"], md))
            f.update(split_step_figures(P, Q, d["w"], Ra, ta, md, got, unique, it))
            print("host G4 %-6s iteration %d " % ("shared" if shared else "own", it) + "  ".join("%s %.3e" % kv for kv in f.items()))
            for k, v in f.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= ihost.bounds_g4()[k], (shared, it, k, v, ihost.bounds_g4()[k])
    for k, host in (("R", ihost.HOST_R_G4), ("T", ihost.HOST_T_G4)):
        assert host * 0.995 <= worst[k] <= host * 1.005, (k, worst[k], host)


# ---- the condition on the random ICP families -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", geo.IDS)
def test_at_most_one_cloud_in_twenty_has_no_unique_step(case_id):
    """From the float64 reference alone.  G2, G3 and G5 are sampled here (every k-th cloud within CPU_PAIRS pairs); G4 is whole."""
    c = CASES[case_id]
    if c["n"] < 3:
        return                                                                             # no step of fewer than three points is unique
    d = geo.icp_case_inputs(c, geo.CUS)
    weighted, trimmed, posed, iterations = geo.icp_mode(case_id)
    keep = geo.f64_sample(c["b"], c["n"] * c["m"], CPU_PAIRS)
    for shared in (False, True):
        P, Q = (d["Ps"] if shared else d["P"])[keep], d["Qs"] if shared else d["Q"][keep]
        w = None if d["w"] is None else d["w"][keep]
        R, t = (a[keep] for a in geo.initial64(d, c["b"]))
        md = geo.max_distance_for(P, Q, w, R, t, iterations) if trimmed else None
        for it in range(iterations):
            dmin, idx = icp_ref.nearest64(icp_ref.pose_points(P, R, t), Q)
            s = icp_ref.step_from(P, Q, idx, dmin, R, t, w, md)
            bad = int((~geo.unique_step(s)).sum())
            print("%-8s %-6s iteration %d: %d of %d clouds without a unique step, max_distance %s" % (case_id, "shared" if shared else "own", it, bad, len(keep), md))
            assert bad <= 0.05 * len(keep) and (bad == 0 or c["n"] < 255), (case_id, shared, it, bad, len(keep))
            if trimmed:
                inl = s["inliers"] / c["n"]
                assert 0.5 < inl.mean() < 0.95, (case_id, inl.mean())                         # the trimming trims
            R, t = s["R"], s["t"]
