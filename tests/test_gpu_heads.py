"""The forward rotation heads on the GPU (so3_quat_*, so3_euler_*, so3_ortho5d_*, so3_expmap_*, so3_ortho6d_*, so3_se3_update_*_f32 and
so3_rotations_axis_angle_f32) through the raw C ABI, on every way their rows are sent: the remainder kernel alone (B < 64), the streaming
engine with and without a remainder, one pass of the engine's whole grid -1, +0, +1, +64, three passes + 5.  The input is
tests/heads_ref.py's edge families tiled with a prime period coprime to a pass; the float64 answers are GATHERED with the same index, never
recomputed, and every row is judged by the bound of heads_ref (4 x what the float32 host model of the same templates reaches,
tests/test_heads_host.py).  A row computed from another round's input is another family's row: it misses its bound by many orders.

WHAT THESE TESTS CATCH (the first by construction, the others tried on a copy of the host model, worst figure against the bound):
  * the engine's row base of round k >= 1 taken from round k - 1 (or any earlier round): the tiling's period is a prime above the
    fixture's length (heads_ref.tile_period), coprime to the rows of a pass for every operation -- asserted in tiled() -- so rows a whole
    number of passes apart never hold the same fixture row, and at round + 64 the second round's rows are compared with answers gathered
    for OTHER fixture rows (apart from the families whose rows are all alike: q = 0, v = 0, e = 0);
  * kQuatMinNorm applied as |q| + 1e-8: the 1.01e-8 family misses by 2.5e7 u (n is halved), 1e-6 by 6.6e5 u;
  * 1 / 30 -> 1 / 24 in the exp map's a1s: backward, 0.01_to_1 4.7e4 and around_1 4.4e4 against 7.1;
  * sincosf -> the hardware sine (argument reduced in float32 turns) in OpEuler: pm1e4 1.5e4, pm1e6 1.6e6 against 7.2;
  * k0 truncated to 2.41 in OpOrtho5d: 17 of 20 family / direction pairs, up to 9.5e4 against 14.5;
  * the `clamped` mask dropped from OpQuat<true>: backward, 1e-9 2.5e4 and 0.99e-8 2.6e7 against 23.4."""
import math
import re

import numpy as np
import pytest
import torch

import heads_ref as hr
from test_gpu_float64_metrics import _p, _st

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -777.0
# rows in one pass of the engine's whole grid, per CU, as the issue tabulates them: CUs x 4 SIMDs x WPS waves x NPL x 64 rows.  _round() does
# not use this table: it reads NPL and WPS from the name of the instantiation the library launched (so3_last_kernel), and
# test_a_pass_is_what_the_library_launches holds the table against that.
ROWS_PER_CU = {("quat", 0): 1536, ("euler", 0): 1536, ("ortho5d", 0): 1536, ("expmap", 0): 1536, ("ortho6d", 0): 2048, ("se3_update", 0): 1024,
               ("quat", 1): 1536, ("euler", 1): 1536, ("ortho5d", 1): 1536, ("expmap", 1): 1536, ("ortho6d", 1): 2048, ("se3_update", 1): 768}
ENGINE_OP = {("quat", 0): "OpQuat<false>", ("quat", 1): "OpQuat<true>", ("euler", 0): "OpEuler<false>", ("euler", 1): "OpEuler<true>",
             ("ortho5d", 0): "OpOrtho5d<false>", ("ortho5d", 1): "OpOrtho5d<true>", ("expmap", 0): "OpExpMap<false>", ("expmap", 1): "OpExpMap<true>",
             ("ortho6d", 0): "OpOrtho6d", ("ortho6d", 1): "OpOrtho6dBwd", ("se3_update", 0): "OpSe3Update", ("se3_update", 1): "OpSe3UpdateBwd"}
SIZE_IDS = ["1", "63", "64", "65", "round-1", "round", "round+1", "round+64", "3round+5"]
CASES = [(op, bwd) for op in hr.OPS for bwd in (0, 1)]
CASE_IDS = ["%s-%s" % (op, "bwd" if bwd else "fwd") for op, bwd in CASES]


_ROUND = {}


def _round(lib, op, bwd):
    """Rows in one pass of the grid the library launches for this operation: one unit is sent, and NPL, WPS and the block size are read
    from the instantiation's name, so3::k_rows<Op, NPL, WPS, BLOCK, false> (launch_rows caps the grid at CUs x 4 x WPS / waves workgroups
    of `waves` waves, each wave taking NPL units of 64 rows per round)."""
    if (op, bwd) not in _ROUND:
        t = small(op, 64)
        launch(lib, op, bwd, t["x"], t["g"], t["t"])
        name = lib.so3_last_kernel().decode()
        m = re.fullmatch(r"so3::k_rows<so3::%s, (\d+), (\d+), (\d+), false>" % re.escape(ENGINE_OP[(op, bwd)]), name)
        assert m, name
        npl, wps, block = (int(v) for v in m.groups())
        waves = block // 64
        workgroups = torch.cuda.get_device_properties(0).multi_processor_count * 4 * wps // waves
        _ROUND[(op, bwd)] = workgroups * waves * npl * 64
    return _ROUND[(op, bwd)]


def _sizes(lib, op, bwd):
    r = _round(lib, op, bwd)
    return [1, 63, 64, 65, r - 1, r, r + 1, r + 64, 3 * r + 5]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def rr():
    from poseestimation_amd import rotation_representation
    return rotation_representation


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_TILED = {}


def tiled(lib, op):
    """The op's fixture tiled to its largest size, on the device, with the index it was gathered by (built once per op)."""
    if op not in _TILED:
        _TILED.clear()                                                     # one op's 3 rounds + 5 rows at a time
        d = hr.data(op)
        period = hr.tile_period(len(d["x"]))
        for bwd in (0, 1):                                                 # rows a whole number of passes apart: never the same fixture row
            assert math.gcd(period, _round(lib, op, bwd)) == 1, (op, bwd, period, _round(lib, op, bwd))
        n = max(max(_sizes(lib, op, 0)), max(_sizes(lib, op, 1)))
        idx = hr.tile_index(n, len(d["x"]))
        t = dict(idx=idx, period=period, x=_dev(d["x"][idx]), g=_dev(d["g"][idx]))
        if op == "se3_update":
            t["t"] = _dev(d["t"][idx])
        _TILED[op] = t
    return _TILED[op]


def small(op, n):
    """The first n rows of the same tiling, built for the call (the tests that need a few hundred rows)."""
    d = hr.data(op)
    idx = hr.tile_index(n, len(d["x"]))
    return dict(idx=idx, x=_dev(d["x"][idx]), g=_dev(d["g"][idx]), t=_dev(d["t"][idx]) if op == "se3_update" else None)


def launch(lib, op, bwd, x, g=None, t=None):
    """One call of the C function into a sentinel-filled output with one guard row behind it; every slot written, the guard intact."""
    b = x.shape[0]
    out = torch.full((b + 1, hr.WIDTH[op] if bwd else hr.OUT_WIDTH[op]), SENTINEL, dtype=torch.float32, device=DEV)
    if op == "se3_update":
        args = (_p(x), _p(t), _p(g), _p(out)) if bwd else (_p(x), _p(t), _p(out))
        name = "so3_se3_update_bwd_f32" if bwd else "so3_se3_update_f32"
        code = getattr(lib, name)(*args, hr.FX, hr.FY, b, _st())
    else:
        name = "so3_%s_%s_f32" % (op, "bwd" if bwd else "fwd")
        code = getattr(lib, name)(*((_p(x), _p(g), _p(out)) if bwd else (_p(x), _p(out))), b, _st())
    assert code == 0, (name, code, lib.so3_last_error())
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all(), name
    return out[:b]


def figure(op, bwd, got, idx):
    got = got.cpu().numpy()
    assert not (got == SENTINEL).all(1).any()                               # a row left unwritten
    return (hr.backward_figure if bwd else hr.forward_figure)(op, got, idx)


def bound(op, bwd):
    return (hr.C_BWD if bwd else hr.C_FWD)[op]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(t, op, lo, hi):
    return dict(x=t["x"][lo:hi], g=t["g"][lo:hi], t=t["t"][lo:hi] if op == "se3_update" else None)


@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_a_pass_is_what_the_library_launches(lib, op, bwd):
    """`round` comes from the launched instantiation's NPL and WPS; the issue's table says the same.  If a launch template changes, this
    test says so while the size tests go on straddling the real pass."""
    assert _round(lib, op, bwd) == torch.cuda.get_device_properties(0).multi_processor_count * ROWS_PER_CU[(op, bwd)]


@pytest.mark.parametrize("which", range(len(SIZE_IDS)), ids=SIZE_IDS)
@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_every_row_within_its_bound_on_every_route(lib, op, bwd, which):
    b = _sizes(lib, op, bwd)[which]
    t = tiled(lib, op)
    got = launch(lib, op, bwd, **_inputs(t, op, 0, b))
    fig = figure(op, bwd, got, t["idx"][:b])
    worst = int(np.nanargmax(fig)) if not np.isnan(fig).all() else 0
    d = hr.data(op)
    print("%s %s B = %d: worst figure %.3f (bound %.2f, host %.2f) at row %d, family %s" %
          (op, "bwd" if bwd else "fwd", b, fig[worst], bound(op, bwd), (hr.HOST_BWD if bwd else hr.HOST_FWD)[op], worst, d["names"][d["fam"][t["idx"][worst]]]))
    assert torch.isfinite(got).all()
    assert (fig <= bound(op, bwd)).all(), (op, bwd, b, worst, fig[worst])
    if op == "se3_update" and not bwd:
        assert hr.se3_rotation_defect(got.cpu().numpy()).max() < 1e-5
    # copies of a position's row sit one period apart: the same bits wherever the engine computed them
    m, done = t["period"], (b // 64) * 64
    if done > m:
        assert same_bits(got[m:done], got[: done - m])


@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_every_fixture_row_through_the_remainder_kernel(lib, op, bwd):
    """The sizes above send the tiling's first 63 rows to the one-row-per-thread kernel and the rest to the engine.  Here every fixture row
    goes through the remainder kernel, 63 at a time."""
    d = hr.data(op)
    x, g = _dev(d["x"]), _dev(d["g"])
    t = _dev(d["t"]) if op == "se3_update" else None
    got = torch.cat([launch(lib, op, bwd, x[lo:lo + 63], g[lo:lo + 63], t[lo:lo + 63] if t is not None else None) for lo in range(0, len(x), 63)])
    assert torch.isfinite(got).all()
    fig = figure(op, bwd, got, None)
    print("%s %s remainder kernel: worst figure %.3f (bound %.2f)" % (op, "bwd" if bwd else "fwd", fig.max(), bound(op, bwd)))
    assert (fig <= bound(op, bwd)).all()


@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_position_independence_within_the_engine_and_within_the_remainder(lib, op, bwd):
    """31 fixture rows (one from every few families) repeated: 31 is coprime to the 64 lanes and to the engine's rows per lane, so a row
    visits every lane and slot.  One pass + 64 rows on the engine, then 62 rows -- two copies of each -- in the remainder kernel.  Copies
    agree bit for bit within each part; between the parts the bound applies (the two instantiations may contract a * b + c differently)."""
    d = hr.data(op)
    pick = (np.arange(31) * (len(d["x"]) // 31 + 1)) % len(d["x"])
    done = _round(lib, op, bwd) + 64
    b = done + 62
    idx = pick[np.arange(b) % 31]
    x, g = _dev(d["x"][idx]), _dev(d["g"][idx])
    got = launch(lib, op, bwd, x, g, _dev(d["t"][idx]) if op == "se3_update" else None)
    assert same_bits(got[31:done], got[: done - 31])
    assert same_bits(got[done + 31:], got[done:done + 31])
    assert (figure(op, bwd, got[done - 31:], idx[done - 31:]) <= bound(op, bwd)).all()


@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_inputs_four_byte_but_not_sixteen_byte_aligned(lib, op, bwd):
    b = 64 * 5 + 17
    t = small(op, b)
    ins = _inputs(t, op, 0, b)
    want = launch(lib, op, bwd, **ins)
    shifted = {}
    for k, v in ins.items():
        if v is not None:
            base = torch.empty(v.numel() + 1, dtype=torch.float32, device=DEV)
            base[1:] = v.reshape(-1)
            shifted[k] = base[1:].view(v.shape)
            assert shifted[k].data_ptr() % 16 == 4
    got = launch(lib, op, bwd, **shifted)
    assert same_bits(got, want)
    assert (figure(op, bwd, got, t["idx"][:b]) <= bound(op, bwd)).all()


@pytest.mark.parametrize("op,bwd", CASES, ids=CASE_IDS)
def test_nan_inf_and_out_of_range_rows_change_no_other_row(lib, op, bwd):
    """A NaN row, an inf row and (quat, 5D) rows outside the documented range, in the middle of an engine unit -- next to the row that
    shares their lane where the engine holds two rows per lane -- and in the remainder: every other row keeps its bits."""
    b = 64 * 4 + 23
    t = small(op, b)
    ins = {k: (v.clone() if v is not None else None) for k, v in _inputs(t, op, 0, b).items()}
    clean = launch(lib, op, bwd, **ins)
    bad = {70: float("nan"), 101: float("inf"), 64 * 4 + 5: float("nan"), 64 * 4 + 11: float("-inf")}
    for row, v in bad.items():
        ins["x"][row] = v
    rows = list(bad)
    if op in hr.OUTSIDE_OPS:
        o = _dev(hr.outside(op)["x"])
        extra = [133, 134, 64 * 4 + 17, 64 * 4 + 18]
        ins["x"][extra] = o[[0, -1, 1, -2]]
        rows += extra
    got = launch(lib, op, bwd, **ins)
    keep = torch.ones(b, dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert same_bits(got[keep], clean[keep])
    if not bwd:
        width = 9 if op != "se3_update" else 11                             # the update's last row (0 0 0 1) is constant
        assert torch.isnan(got[[70, 64 * 4 + 5], :width]).all()            # a NaN row gives a NaN row


@pytest.mark.parametrize("op", hr.OUTSIDE_OPS)
def test_outside_the_range_the_kernels_return_what_the_header_says(lib, op):
    """include/so3proj.h, 'input range of the heads': pinned on the engine (rows 0 .. 63) and in the remainder kernel (rows 64 .. 79)."""
    o = hr.outside(op)
    n = len(o["x"])
    x = _dev(np.concatenate([o["x"]] * 5))                                  # 80 rows: one unit and a remainder of 16
    got = launch(lib, op, 0, x).cpu().numpy()
    for k in range(5):
        assert hr.outside_matches(op, got[k * n:(k + 1) * n]), (op, k)


@pytest.mark.parametrize("b", [1, 255, 256, 257])
def test_sampler_on_its_families(lib, b):
    s = hr.sampler()
    idx = hr.tile_index(b, len(s["theta"]))
    theta, axis = _dev(s["theta"][idx]), _dev(s["axis"][idx])
    out = torch.full((b + 1, 9), SENTINEL, dtype=torch.float32, device=DEV)
    code = lib.so3_rotations_axis_angle_f32(_p(theta), _p(axis), _p(out), b, _st())
    assert code == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all()
    fig = hr.sampler_figure(out[:b].cpu().numpy(), idx)
    print("sampler B = %d: worst figure %.3f (bound %.2f)" % (b, fig.max(), hr.C_SAMPLER))
    assert (fig <= hr.C_SAMPLER).all()


def test_python_surface_dtypes_and_the_6d_shape_rule(rr):
    heads = {"quat": rr.compute_rotation_matrix_from_quaternion, "euler": rr.compute_rotation_matrix_from_euler,
             "ortho5d": rr.compute_rotation_matrix_from_ortho5d, "expmap": rr.vec_3d_to_SO3, "ortho6d": rr.compute_rotation_matrix_from_ortho6d}
    for op, fn in heads.items():
        d = hr.data(op)
        rows = np.flatnonzero(np.abs(d["x"]).max(1) < 1e3)[::7][:100]       # magnitudes bfloat16 and the sum below keep finite
        for dtype in (torch.bfloat16, torch.float64):
            x = _dev(d["x"][rows]).to(dtype).requires_grad_(True)
            y = fn(x)
            assert y.dtype == torch.float32 and y.shape == (len(rows), 3, 3)
            (gx,) = torch.autograd.grad(y.sum(), x)
            assert gx.dtype == dtype and gx.shape == x.shape
    # (..., 6) -> (..., 3, 3) at an edge family: the nearly parallel halves at sine 1e-5
    d = hr.data("ortho6d")
    fam = np.flatnonzero(d["fam"] == d["names"].index("parallel_1e-05"))[:120]
    x = _dev(d["x"][fam]).view(2, 3, 20, 6).clone().requires_grad_(True)
    y = rr.compute_rotation_matrix_from_ortho6d(x)
    assert y.shape == (2, 3, 20, 3, 3)
    assert (hr.forward_figure("ortho6d", y.detach().reshape(-1, 9).cpu().numpy(), fam) <= hr.C_FWD["ortho6d"]).all()
    g = _dev(d["g"][fam]).view(2, 3, 20, 3, 3)
    (gx,) = torch.autograd.grad(y, x, g)
    assert gx.shape == x.shape
    assert (hr.backward_figure("ortho6d", gx.reshape(-1, 6).cpu().numpy(), fam) <= hr.C_BWD["ortho6d"]).all()
