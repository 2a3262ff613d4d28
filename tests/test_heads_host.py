"""The forward rotation heads without a GPU: the float32 host model of the kernels' own templates (oracle/kernel_model.cpp: OpQuat, OpEuler,
OpOrtho5d, OpExpMap, OpOrtho6d, OpSe3Update and their backwards) on every edge family of tests/heads_ref.py, every row against its
float64 answer.  This is where the constants of heads_ref are MEASURED: each HOST_* value there is the largest figure printed here, and
the bound used on the host and on the GPU alike (tests/test_gpu_heads.py) is 4 x it."""
import numpy as np
import pytest

from conftest import load_golden
import heads_ref as hr


@pytest.fixture(scope="module")
def km():
    from oracle import kernel_model
    if kernel_model.clangxx() is None:
        pytest.skip("clang++ is not available (ext_vector_type)")
    kernel_model.lib()
    return kernel_model


def run_fwd(km, op, d):
    if op == "se3_update":
        return km.se3_update(d["x"], d["t"], hr.FX, hr.FY).reshape(-1, 16)
    return km.head(op, d["x"]).reshape(-1, 9)


def run_bwd(km, op, d):
    if op == "se3_update":
        return km.se3_update_bwd(d["x"], d["t"], d["g"], hr.FX, hr.FY)
    return km.head_bwd(op, d["x"], d["g"])


def _per_family(d, fig):
    return {name: fig[d["fam"] == i].max() for i, name in enumerate(d["names"])}


@pytest.mark.parametrize("op", hr.OPS)
def test_every_row_of_every_family_is_within_its_bound_and_the_constants_are_the_measured_ones(km, op):
    d = hr.data(op)
    assert set(np.bincount(d["fam"])) == {hr.ROWS} and 128 <= hr.ROWS <= 256
    fwd, bwd = run_fwd(km, op, d), run_bwd(km, op, d)
    assert np.isfinite(fwd).all() and np.isfinite(bwd).all()               # inside the range no row is NaN
    ffig, bfig = hr.forward_figure(op, fwd), hr.backward_figure(op, bwd)
    for name, (f, b) in {k: (v, _per_family(d, bfig)[k]) for k, v in _per_family(d, ffig).items()}.items():
        print("%-10s %-16s forward %7.3f u cond   backward %7.3f u |G|_1 cond gunit" % (op, name, f, b))
    print("%-10s measured %.3f / %.3f   recorded %.2f / %.2f   bounds %.2f / %.2f" % (op, ffig.max(), bfig.max(), hr.HOST_FWD[op], hr.HOST_BWD[op],
                                                                                  hr.C_FWD[op], hr.C_BWD[op]))
    # the recorded constants ARE the measurement (rounded up in the last digit), and the bound is 4 x
    assert 0.95 * hr.HOST_FWD[op] <= ffig.max() <= hr.HOST_FWD[op]
    assert 0.95 * hr.HOST_BWD[op] <= bfig.max() <= hr.HOST_BWD[op]
    assert hr.C_FWD[op] == 4 * hr.HOST_FWD[op] <= 64 and hr.C_BWD[op] == 4 * hr.HOST_BWD[op] <= 64
    if op == "se3_update":                                                 # rows without a gap: a rotation all the same
        assert hr.se3_rotation_defect(fwd).max() < 1e-5
        assert (d["gap"] < hr.SE3_MIN_GAP).sum() >= hr.ROWS - 8            # the rank-one family


def test_the_exp_maps_kink_is_where_heads_ref_says(km):
    """Outside the band every row takes the float64 side of the clamp; inside it rows may take either, and some do take the other one
    (or the band would be untested).  Judged against the wrong side such a row is off by up to hundreds of u
    (the via_theta term: how much depends on the row's G)."""
    d = hr.data("expmap")
    got = run_bwd(km, "expmap", d).astype(np.float64)
    unit = hr.U * np.abs(d["g"]).astype(np.float64).sum(1)[:, None]
    main, alt = (np.abs(got - d["dx64"]) / unit).max(1), (np.abs(got - d["dx64_alt"]) / unit).max(1)
    other_side = alt < main
    straddle = d["fam"] == d["names"].index("straddle")
    print("rows in the band: %d of the straddle family's %d; on the float64 side %d, on the other %d; worst wrong-side figure %.0f u" %
          (d["kink"].sum(), straddle.sum(), (d["kink"] & ~other_side).sum(), other_side.sum(), np.maximum(main, alt)[d["kink"]].max()))
    assert not (other_side & ~d["kink"]).any()
    assert other_side.any() and (d["kink"] & ~other_side).any()
    assert 8 <= d["kink"].sum() <= straddle.sum() // 2 and (main[other_side] > hr.C_BWD["expmap"]).any()
    # the forward is continuous across the clamp: no exclusion there
    assert hr.forward_figure("expmap", run_fwd(km, "expmap", d))[straddle].max() <= hr.C_FWD["expmap"]


@pytest.mark.parametrize("op", hr.OUTSIDE_OPS)
def test_outside_the_range_the_rows_are_what_heads_ref_says(km, op):
    o = hr.outside(op)
    got = km.head(op, o["x"]).reshape(-1, 9)
    assert hr.outside_matches(op, got), got[[0, -1]]
    back = km.head_bwd(op, o["x"], np.ones((len(o["x"]), 9), np.float32))
    if op == "quat":
        assert (back == 0).all()                                           # 1 / |q| = 0: no gradient
    else:
        assert np.isnan(back).any(1).all()


def test_quaternion_of_norm_zero_is_the_identity_with_no_gradient(km):
    d = hr.data("quat")
    zero = d["fam"] == d["names"].index("zero")
    assert (d["x"][zero] == 0).all()
    assert np.array_equal(run_fwd(km, "quat", d)[zero], np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (zero.sum(), 1)))
    assert (run_bwd(km, "quat", d)[zero] == 0).all() and (d["dx64"][zero] == 0).all()


def test_sampler_restatement_and_its_constant():
    s = hr.sampler()
    fig = hr.sampler_figure(hr.sampler_f32(s["theta"], s["axis"]))
    for i, name in enumerate(s["names"]):
        print("%-24s %.3f u" % (name, fig[s["fam"] == i].max()))
    assert 0.95 * hr.HOST_SAMPLER <= fig.max() <= hr.HOST_SAMPLER and hr.C_SAMPLER == 4 * hr.HOST_SAMPLER <= 64
    eye = np.eye(3).reshape(9)
    assert (s["r64"][s["fam"] % 4 == 0] == eye).all()                       # a zero axis: the identity, whatever theta


def test_g23_the_float64_restatement_takes_the_references_clamps():
    """tests/golden/g23_head_edges.npz: the reference's own outputs and autograd on every fourth row of every family.  In float64 the
    restatement in oracle/so3_oracle.py and the reference agree to float64 round-off -- at |q| below and beside 1e-8, below and beside
    |v|^2 = 1e-4 and at every magnitude; the reference's float32 run is within the bound its naive arithmetic allows.  At q = 0 the
    reference's gradient is NaN (the derivative of sqrt at 0); heads_ref and the kernels give 0 there."""
    g = load_golden("g23_head_edges.npz")
    tiny = 1e-4                                                              # in units of u: 6e-12 cond
    for op in hr.OPS:
        d = hr.data(op)
        rows = g[op + "_rows"].astype(np.int64)
        assert len(rows) == len(d["x"]) // 4 and np.array_equal(g[op + "_x"], d["x"][rows])        # the same rows, bit for bit
        ffig32 = hr.forward_figure(op, g[op + "_r"], rows)
        defined = np.isfinite(g[op + "_dx"]).all(1)
        bfig32 = hr.backward_figure(op, np.where(defined[:, None], g[op + "_dx"], 0.0), rows)[defined]
        print("%-10s reference float32: forward %.2f, backward %.2f (in the units of the bounds); rows with a NaN gradient: %d" %
              (op, ffig32.max(), bfig32.max(), (~defined).sum()))
        if op + "_r_f64" in g:
            assert hr.forward_figure(op, g[op + "_r_f64"], rows).max() <= tiny, op
            dx = g[op + "_dx_f64"]
            ok = np.isfinite(dx).all(1)
            assert hr.backward_figure(op, np.where(ok[:, None], dx, 0.0), rows)[ok].max() <= tiny, op
            nan_rows = rows[~ok]
            if op == "quat":
                assert len(nan_rows) == hr.ROWS // 4 and (d["fam"][nan_rows] == d["names"].index("zero")).all()
            else:
                assert len(nan_rows) == 0, op
        else:
            assert op in ("ortho5d", "se3_update")
