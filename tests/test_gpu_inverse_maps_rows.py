"""The inverse maps on the GPU, row by row (so3_mat_to_quat_*, so3_logmap_*, so3_mat_to_euler_*, so3_relative_log_* through the raw C ABI):
every row of G18 and of the edge families of tests/inverse_maps_ref.py -- next to and below the Euler gradient's floor, r0^2 + r2^2
among the subnormals, rotation vectors of 1e-30 .. 1e-2, residuals R2 = R1 exp(delta) down to delta = 0, pairs on the cut theta = pi --
against the float64 definition evaluated on the same float32 row, each row held to ITS family's bound (ROW_TOL of
tests/test_inverse_maps_host.py: 4 x what the float32 host model of the same templates reaches on that family; never a figure of the
device's).  No row is left out: none within 0.05 rad of gimbal lock, none compared up to sign or by closure.  (The relative maps' rows
within 1e-6 of the cut are held to the nearer of the float64 answers at v and at -v: inverse_maps_ref.on_cut says why.)

ROUTES.  Each of the ten entry points -- three forwards, three backwards, the relative forward, so3_relative_log_bwd_f32 with both
gradients, with dR1 alone and with dR2 alone -- is sent 1, 63, 64, 65 rows and pass - 1, pass, pass + 1, pass + 64, 3 pass + 5 rows of ITS
OWN pass: NPL, WPS and BLOCK are read from the name of the instantiation the library launched (so3_last_kernel), not from a table.  The
input is the table tiled with a prime period above its length, coprime to every pass (asserted); the float64 answers are gathered by the
same index and never recomputed, so a row computed from another pass's input is another family's row and misses its bound by orders.
(tests/test_gpu_inverse_maps.py keeps the 1 000 003-row case, the closures, the dtypes and the graph capture.)

WHAT THESE TESTS CATCH, tried on copies of the host model (tests/host_model/inverse_maps.cpp over a mutated so3_rows.h); `old` is the
twelve tests this file's host companion had before, `new` test_every_row_within_its_family_bound, worst figure against its bound:
  * kEulerMinCos 1e-6 -> 5e-3: old passes; new fails on 925 rows of euler_grad: 0.9998 in euler_floor (bound 9.2e-7), euler_underflow
    (6.4e-7), gimbal_exact (9.4e-7) and axis_aligned (4.5e-7), 0.998 in gimbal_near (9.7e-7), 0.576 in tie_half_turn (8.6e-7);
  * kEulerMinCos 1e-6 -> 1e-8: old passes; new fails on 478 rows of euler_grad: 99.0 (the gradient 100 times too large) in euler_floor,
    euler_underflow, gimbal_exact and axis_aligned against the same bounds -- the 1e-8 .. 1e-16 rows and lock; the 0.99e-6 rows by 0.01;
  * the log map's k zeroed when n < 1e-6: old passes; new fails on log with relative error 1.0 in log_small (bound 4.3e-7, 151 rows) and
    theta_small (6.2e-7), and on rel in rel_residual, 1.11e-7 against 8.6e-8 (18 rows);
  * the `lock` select of OpMatToEuler dropped: old FAILS already (test_forward_values_ranges_and_closure: the Euler closure is NaN;
    test_gradients_against_float64_autograd: not finite); new fails too (euler, euler_grad: NaN rows at lock).
The device fault these tests found: with `lock` as h <= 0, all 144 rows with 0 < r0^2 + r2^2 < 2^-126 came out NaN on the MI355X, forward
and backward (v_rsq_f32 reads a subnormal as 0); the host model, whose rsq is libm's, returned finite rows."""
import math
import re

import numpy as np
import pytest
import torch

import heads_ref as hr
import inverse_maps_ref as ref
from test_gpu_float64_metrics import _p, _st
from test_inverse_maps_host import ROW_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -777.0
# entry point -> (the engine operation it launches, the C symbol, the checks of ref.CHECKS its outputs answer, in output order)
ENTRIES = {
    "mat_to_quat_fwd": ("OpMatToQuat<false>", "so3_mat_to_quat_fwd_f32", ("quat",)),
    "logmap_fwd": ("OpLogMap<false>", "so3_logmap_fwd_f32", ("log",)),
    "mat_to_euler_fwd": ("OpMatToEuler<false>", "so3_mat_to_euler_fwd_f32", ("euler",)),
    "relative_log_fwd": ("OpRelLog<false, false>", "so3_relative_log_fwd_f32", ("rel",)),
    "mat_to_quat_bwd": ("OpMatToQuat<true>", "so3_mat_to_quat_bwd_f32", ("quat_grad",)),
    "logmap_bwd": ("OpLogMap<true>", "so3_logmap_bwd_f32", ("log_grad",)),
    "mat_to_euler_bwd": ("OpMatToEuler<true>", "so3_mat_to_euler_bwd_f32", ("euler_grad",)),
    "relative_log_bwd_both": ("OpRelLog<true, true>", "so3_relative_log_bwd_f32", ("rel_grad1", "rel_grad2")),
    "relative_log_bwd_dR1": ("OpRelLog<true, false>", "so3_relative_log_bwd_f32", ("rel_grad1",)),
    "relative_log_bwd_dR2": ("OpRelLog<true, false>", "so3_relative_log_bwd_f32", ("rel_grad2",)),
}
WIDTH = {"quat": 4, "log": 3, "euler": 3, "rel": 3}
SIZE_IDS = ["1", "63", "64", "65", "pass-1", "pass", "pass+1", "pass+64", "3pass+5"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pa(lib):
    import poseestimation_amd
    return poseestimation_amd


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def launch(lib, entry, r, r2, g):
    """One call of the C function into sentinel-filled outputs with one guard row behind each -> {check: (b, w) tensor}; the guard intact."""
    _, symbol, checks = ENTRIES[entry]
    b = r.shape[0]
    outs = [torch.full((b + 1, WIDTH.get(c, 9)), SENTINEL, dtype=torch.float32, device=DEV) for c in checks]
    g3 = g[:, :3].contiguous()
    if entry.startswith("relative_log_bwd"):
        by_check = dict(zip(checks, outs))
        args = (_p(r), _p(r2), _p(g3), _p(by_check.get("rel_grad1")), _p(by_check.get("rel_grad2")))
    elif entry == "relative_log_fwd":
        args = (_p(r), _p(r2), _p(outs[0]))
    elif entry.endswith("_bwd"):
        args = (_p(r), _p(g if entry == "mat_to_quat_bwd" else g3), _p(outs[0]))
    else:
        args = (_p(r), _p(outs[0]))
    code = getattr(lib, symbol)(*args, b, _st())
    assert code == 0, (entry, code, lib.so3_last_error())
    torch.cuda.synchronize()
    for c, out in zip(checks, outs):
        assert (out[b] == SENTINEL).all(), (entry, c)
    return {c: out[:b] for c, out in zip(checks, outs)}


_PASS = {}


def _pass(lib, entry):
    """Rows in one pass of the grid the library launches for this entry point: 64 rows are sent, and NPL, WPS and the block size are
    read from the instantiation's name, so3::k_rows<Op, NPL, WPS, BLOCK, false> (the grid is capped at CUs x 4 x WPS / waves workgroups
    of `waves` waves, each wave taking NPL units of 64 rows per round) -> (rows, NPL, WPS, BLOCK)."""
    if entry not in _PASS:
        t = ref.rows()
        launch(lib, entry, _dev(t["r"][:64]), _dev(t["r2"][:64]), _dev(t["g"][:64]))
        name = lib.so3_last_kernel().decode()
        m = re.fullmatch(r"so3::k_rows<so3::%s, (\d+), (\d+), (\d+), false>" % re.escape(ENTRIES[entry][0]), name)
        assert m, (entry, name)
        npl, wps, block = (int(v) for v in m.groups())
        waves = block // 64
        workgroups = torch.cuda.get_device_properties(0).multi_processor_count * 4 * wps // waves
        _PASS[entry] = (workgroups * waves * npl * 64, npl, wps, block)
    return _PASS[entry]


def _sizes(lib, entry):
    p = _pass(lib, entry)[0]
    return [1, 63, 64, 65, p - 1, p, p + 1, p + 64, 3 * p + 5]


@pytest.fixture(scope="module")
def tiled(lib):
    """The table tiled to the largest size of any entry point, on the device, with the index it was gathered by."""
    t = ref.rows()
    m = len(t["r"])
    period = hr.tile_period(m)
    for entry in ENTRIES:                                          # rows a whole number of passes apart: never the same table row
        assert math.gcd(period, _pass(lib, entry)[0]) == 1, (entry, period, _pass(lib, entry))
    n = max(max(_sizes(lib, entry)) for entry in ENTRIES)
    idx = hr.tile_index(n, m)
    assert (np.bincount(idx[:period], minlength=m) >= 1).all()
    return dict(table=t, idx=idx, period=period, r=_dev(t["r"][idx]), r2=_dev(t["r2"][idx]), g=_dev(t["g"][idx]))


def judge(entry, got, table, idx, what):
    """Every row of every output of one call against its family's bound; prints the worst row of each check before asserting."""
    for check, out in got.items():
        out = out.cpu().numpy()
        assert not (out == SENTINEL).all(1).any(), (entry, check, what)           # a row left unwritten
        assert np.isfinite(out).all(), (entry, check, what, np.flatnonzero(~np.isfinite(out).all(1))[:8])
        fig, bound = ref.row_error(check, out, table, idx), ref.row_bound(check, ROW_TOL, table, idx)
        ratio = np.where(fig > 0, fig / np.maximum(bound, 1e-300), 0.0)
        worst = int(np.argmax(ratio))
        row = worst if idx is None else int(idx[worst])
        print("%s %s %s: worst row %d (table row %d, family %s) figure %.3e, bound %.3e" % (
            entry, check, what, worst, row, table["names"][table["fam"][row]], fig[worst], bound[worst]))
        assert (fig <= bound).all(), (entry, check, what, worst, row, table["names"][table["fam"][row]], fig[worst], bound[worst], int((fig > bound).sum()))
        if check in ("log", "rel"):                                                 # an answer that is exactly 0 comes out exactly 0
            want = table["want"][check] if idx is None else table["want"][check][idx]
            assert (out[(want == 0).all(1)] == 0).all(), (entry, check, what)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_pass_is_what_the_library_launches(lib, entry):
    """The inverse maps run two matrices per lane and four waves per SIMD, 2048 rows per CU; so3_relative_log_bwd_f32 with both
    gradients runs three waves per SIMD, three quarters of that, as DESIGN 7a says, and the one-gradient instantiation is launched
    with the same shape (so3proj.hip: SO3_RELLOG_BWD_WPS).  If a launch template changes, this test says so while the size tests go on
    straddling the real pass."""
    rows, npl, wps, block = _pass(lib, entry)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("%s: NPL %d, WPS %d, BLOCK %d, %d rows per pass" % (entry, npl, wps, block, rows))
    assert rows == cus * 4 * wps * npl * 64
    if entry.startswith("relative_log_bwd"):
        assert (npl, wps, block) == (2, 3, 256) and 4 * rows == 3 * _pass(lib, "relative_log_fwd")[0] and rows == cus * 1536
    else:
        assert (npl, wps, block) == (2, 4, 256) and rows == cus * 2048


@pytest.mark.parametrize("which", range(len(SIZE_IDS)), ids=SIZE_IDS)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_row_within_its_family_bound_on_every_route(lib, tiled, entry, which):
    b = _sizes(lib, entry)[which]
    got = launch(lib, entry, tiled["r"][:b], tiled["r2"][:b], tiled["g"][:b])
    judge(entry, got, tiled["table"], tiled["idx"][:b], "B = %d" % b)
    # copies of a position's row sit one period apart: the same bits wherever the engine computed them
    m, done = tiled["period"], (b // 64) * 64
    if done > m:
        for out in got.values():
            assert torch.equal(out[m:done].view(torch.int32), out[: done - m].view(torch.int32)), entry


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_table_row_through_the_remainder_kernel(lib, entry):
    """The sizes above send at most 63 rows to the one-row-per-thread kernel.  Here every row of the table goes through it, 63 at a time."""
    t = ref.rows()
    r, r2, g = _dev(t["r"]), _dev(t["r2"]), _dev(t["g"])
    parts = [launch(lib, entry, r[lo:lo + 63], r2[lo:lo + 63], g[lo:lo + 63]) for lo in range(0, len(r), 63)]
    judge(entry, {c: torch.cat([p[c] for p in parts]) for c in parts[0]}, t, None, "remainder kernel")


def test_one_gradient_alone_against_both(lib):
    """dR2 alone is the both-gradients dR2 bit for bit; dR1 alone off the cut too.  Within 1e-3 of theta = pi a row of dR1 alone is
    judged by its family's bound in the route test above, like every other row."""
    t = ref.rows()
    r, r2, g = _dev(t["r"]), _dev(t["r2"]), _dev(t["g"])
    both = launch(lib, "relative_log_bwd_both", r, r2, g)
    o1, o2 = launch(lib, "relative_log_bwd_dR1", r, r2, g)["rel_grad1"], launch(lib, "relative_log_bwd_dR2", r, r2, g)["rel_grad2"]
    off_cut = torch.as_tensor(np.pi - np.linalg.norm(t["want"]["rel"], axis=1) > 1e-3).to(DEV)
    assert torch.equal(o2, both["rel_grad2"]) and torch.equal(o1[off_cut], both["rel_grad1"][off_cut])


def test_python_surface_gives_the_c_abi_bits_on_the_edge_rows(lib, pa):
    t = ref.rows()
    edge = np.flatnonzero(t["fam"] >= t["names"].index(ref.EDGE_FAMILIES[0]))
    r, r2, g = _dev(t["r"][edge]), _dev(t["r2"][edge]), _dev(t["g"][edge])
    g3 = g[:, :3].contiguous()
    for fn, fwd, bwd in ((pa.matrix_to_euler, "mat_to_euler_fwd", "mat_to_euler_bwd"), (pa.so3_log_map, "logmap_fwd", "logmap_bwd")):
        x = r.view(-1, 3, 3).clone().requires_grad_(True)
        y = fn(x)
        y.backward(g3)
        (want,), (want_grad,) = launch(lib, fwd, r, r2, g).values(), launch(lib, bwd, r, r2, g).values()
        assert torch.equal(y.detach(), want) and torch.equal(x.grad.reshape(-1, 9), want_grad), fwd
    x1, x2 = r.view(-1, 3, 3).clone().requires_grad_(True), r2.view(-1, 3, 3).clone().requires_grad_(True)
    y = pa.relative_rotation_vector(x1, x2)
    y.backward(g3)
    both = launch(lib, "relative_log_bwd_both", r, r2, g)
    assert torch.equal(y.detach(), launch(lib, "relative_log_fwd", r, r2, g)["rel"])
    assert torch.equal(x1.grad.reshape(-1, 9), both["rel_grad1"]) and torch.equal(x2.grad.reshape(-1, 9), both["rel_grad2"])
    judge("matrix_to_euler", {"euler": pa.matrix_to_euler(r.view(-1, 3, 3))}, t, edge, "python surface")
