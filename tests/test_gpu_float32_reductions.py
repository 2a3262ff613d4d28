"""The float32 and bfloat16 losses and metrics (K3 so3_frob_fwd_bwd_v2_*, K3' so3_frob_loss_v2_f32, K4 so3_angle_error_v2, K1+K4
so3_project_angle_error_v2_f32, so3_geodesic_eps_f32, K4s / K3s) on every way their rows are sent and their sums finished, against plain
high-precision references: math.fsum of float64 per-row values, the float64 oracle, torch's round-to-nearest-even.

Rows go one of three ways: the one-workgroup kernel (B <= 1024), the streaming engine plus a remainder kernel for the last B mod 64 rows,
or the tile kernels alone (a bfloat16 view at an odd row offset is not dword aligned).  Sums finish one of three ways: the workspace
ticket, a memset plus atomics, or caller-zeroed accumulators (SO3_PREZEROED).  Every reducing launch here has kFixedRounds = 0, so one
round of the engine's grid is CUs x 4 SIMDs x WPS x NPL x 64 = CUs x 1024 rows for each of them (so3proj.hip: launch_rows)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_float64_metrics import _haar_rows, _p, _st, _timed
from test_gpu_symmetry import assert_angles, trace_margin
from test_symmetry_host import sym_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0**-53                               # unit round-off of float64
U32 = 2.0**-24                             # and of float32
PREZEROED, EXACT_F64 = 0x2, 0x4
DEG = 180.0 / np.pi
ROW_REL = 12 * U32                         # one float32 row norm ||a - b||: the subtraction, 9 fmas, v_rsq_f32 (1 ulp), one product
N_MAX = 1_000_003


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def pa(lib):
    import poseestimation_amd
    return poseestimation_amd


def _round():
    """Rows in one round of the engine's whole grid, for every reducing op here."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 1024


def _sizes():
    r = _round()
    return [1, 63, 64, 65, 1024, 1025, r - 64, r, r + 81, 3 * r + 5, N_MAX]


SIZE_IDS = ["1", "63", "64", "65", "1024", "1025", "round-64", "round", "round+81", "3round+5", "1000003"]


@pytest.fixture(scope="module")
def data(lib):
    gen = torch.Generator(device=DEV).manual_seed(32)
    n = N_MAX + 2
    t = _haar_rows(n, gen).float()
    p = _haar_rows(n, gen).float()
    x = torch.randn(n, 9, device=DEV, generator=gen)
    return dict(t=t, p=p, x=x)


def _f64(k, v=777.0):
    return torch.full((k,), v, dtype=torch.float64, device=DEV)


def _f32(k, v=-1.0):
    return torch.full((k,), v, dtype=torch.float32, device=DEV)


def _ws(lib):
    return torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)


def _depth(n, ws):
    """A generous count of the float64 additions one row's value passes on its way into the sum: the lane's own rounds, the wave's 6
    shuffle levels, the workgroup's waves, then the ticket's slots -- or, with atomics, one add per workgroup of the engine (<= 2 x CUs)
    and of the tile kernel (<= 2048)."""
    d = 128
    if not ws:
        d += 2 * _round() // 1024 + 2048
    return d


def _row_norms(a, b):
    d = a.double() - b.double()                                  # exact: float32 data
    return torch.sqrt((d * d).sum(1)).cpu().numpy()


def _sum_bound(vals, n, ws, row_rel):
    s = math.fsum(np.abs(vals).tolist())
    return row_rel * s + _depth(n, ws) * U * s


def _zeroed(ws):
    torch.cuda.synchronize()
    return int(torch.count_nonzero(ws).item()) == 0


def _sample_rows(n):
    """Row 0, the first and last units, every unit boundary near the end of the engine's share, and a spread in between."""
    idx = np.unique(np.concatenate((np.arange(min(n, 256)), np.arange(max(0, n - 256), n), np.linspace(0, n - 1, 2048).astype(np.int64))))
    return idx


def _oracle_rows(x, idx):
    from oracle import so3_oracle as so
    xs = x[idx].double().cpu().numpy()
    ref, s, d = so.symmetric_orthogonalization_np(xs, return_parts=True)
    gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]
    return xs, ref.reshape(-1, 9), s, gap


# ------------------------------------------------------------------------------------------------
# 1. K3 float32: every size, every finish, the four R / dM instantiations
# ------------------------------------------------------------------------------------------------
def _k3(lib, x, t, want_r, want_dm, ws, flags=0, bf16=False, ls=None):
    n = x.shape[0]
    r = torch.full((n, 9), 7.0, device=DEV) if want_r else None
    dm = (torch.full((n, 9), 7.0, device=DEV, dtype=x.dtype)) if want_dm else None
    ls = _f64(1) if ls is None else ls
    mean = _f32(1)
    entry = lib.so3_frob_fwd_bwd_v2_bf16 if bf16 else lib.so3_frob_fwd_bwd_v2_f32
    assert entry(_p(x), _p(t), _p(r), _p(dm), _p(ls), _p(mean), _p(ws), flags, n, _st()) == 0
    return r, dm, ls, mean


@pytest.mark.parametrize("idx", range(11), ids=SIZE_IDS)
def test_frob_head_f32_every_size_and_finish(lib, data, idx):
    from oracle import so3_oracle as so
    n = _sizes()[idx]
    x, t = data["x"][:n], data["t"][:n]
    ws = _ws(lib)
    r0, dm0, ls0, mean0 = _k3(lib, x, t, True, True, ws)
    s0 = ls0.item()
    nrm = _row_norms(r0, t)                                     # ||T - R|| of the kernel's own R
    exact = math.fsum(nrm.tolist())
    assert abs(s0 - exact) <= _sum_bound(nrm, n, True, ROW_REL), (n, s0, exact)
    assert mean0.item() == float(np.float32(s0 * (1.0 / n)))
    # the four instantiations give the same loss bits on the workspace path, and the same rows
    for want_r, want_dm in ((True, True), (True, False), (False, True), (False, False)):
        r, dm, ls, mean = _k3(lib, x, t, want_r, want_dm, ws)
        assert ls.item() == s0 and mean.item() == mean0.item(), (n, want_r, want_dm)
        if want_r:
            assert torch.equal(r, r0)
        if want_dm:
            assert torch.equal(dm, dm0)
    assert _zeroed(ws)
    # no workspace (memset + atomics above 1024 rows), and caller-zeroed accumulators
    for flags in (0, PREZEROED):
        acc = _f64(1, 0.0 if flags else 777.0)
        r, dm, ls, mean = _k3(lib, x, t, True, True, None, flags, ls=acc)
        assert torch.equal(r, r0) and torch.equal(dm, dm0)
        assert abs(ls.item() - exact) <= _sum_bound(nrm, n, False, ROW_REL), (n, flags, ls.item(), exact)
        assert mean.item() == float(np.float32(ls.item() * (1.0 / n)))
        if n <= 1024:
            assert ls.item() == s0
    # per-row values against the oracle on a sample: R in the conditioned measure, dM as the projection backward of (R - T)/(B ||R - T||)
    rows = _sample_rows(n)
    xs, ref, s, gap = _oracle_rows(x, rows)
    rk = r0[rows].double().cpu().numpy()
    assert (np.abs(rk - ref).max(1) * gap).max() < 2e-6, n
    diff = rk - t[rows].double().cpu().numpy()
    g = diff / (n * np.linalg.norm(diff, axis=1, keepdims=True))
    dref = so.projection_backward_np(xs, g).reshape(-1, 9)
    rel = np.abs(dm0[rows].double().cpu().numpy() - dref).max(1) * n * gap * gap * s[:, 0]
    assert rel.max() < 2e-5, (n, rel.max())


# ------------------------------------------------------------------------------------------------
# 2. K3 bfloat16: even row offsets (engine) and odd ones (tile kernels alone, grid-stride past 524 288 rows)
# ------------------------------------------------------------------------------------------------
BF16_SIZES = [1, 65, 1025, "round+81", 524_289, N_MAX]


def _bf16_size(v):
    return _round() + 81 if v == "round+81" else v


@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("size", BF16_SIZES, ids=[str(v) for v in BF16_SIZES])
def test_frob_head_bf16_even_and_odd_offsets(lib, data, size, off):
    n = _bf16_size(size)
    xb_all = data["x"][:n + 2].bfloat16()
    xb, t = xb_all[off:off + n], data["t"][off:off + n]
    assert (xb.data_ptr() % 4 == 0) == (off % 2 == 0)
    xf = xb.float()                                              # the same values in float32 storage
    ws = _ws(lib)
    rb, dmb, lsb, meanb = _k3(lib, xb, t, True, True, ws, bf16=True)
    rf, dmf, lsf, _ = _k3(lib, xf, t, True, True, ws)
    assert dmb.dtype == torch.bfloat16
    nrm = _row_norms(rb, t)
    exact = math.fsum(nrm.tolist())
    tile_only = off % 2 == 1 and n > 1024                        # memset + atomics although a workspace is passed
    assert abs(lsb.item() - exact) <= _sum_bound(nrm, n, not tile_only, ROW_REL), (n, off, lsb.item(), exact)
    assert _zeroed(ws)
    rne = dmf.to(torch.bfloat16)                                 # torch: round to nearest even
    if not tile_only:
        # the same route as the float32 call: the same float32 arithmetic, then round-to-nearest-even of every element
        assert torch.equal(rb, rf)
        assert torch.equal(dmb.view(torch.int16), rne.view(torch.int16)), (n, off)
        assert lsb.item() == lsf.item()
    else:
        # the tile kernel's projection is not the engine's (project_rotation_frames against the quaternion fast path): R to the oracle,
        # dM within 1 bf16 ulp of the float32 call's rounding wherever the singular gap leaves the two float32 answers 1e-5 apart at most
        rows = _sample_rows(n)
        _, ref, s, gap = _oracle_rows(xf, rows)
        assert (np.abs(rb[rows].double().cpu().numpy() - ref).max(1) * gap).max() < 2e-6
        sv = np.linalg.svd(xf.double().cpu().numpy().reshape(-1, 3, 3), compute_uv=False)
        det = np.linalg.det(xf.double().cpu().numpy().reshape(-1, 3, 3))
        g_all = np.where(det < 0, sv[:, 1] - sv[:, 2], sv[:, 1] + sv[:, 2]) / sv[:, 0]
        ok = g_all > 1e-2
        got = dmb.float().cpu().numpy()
        want = rne.float().cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) * 2.0**16        # float32 spacing x 2^16 = one bf16 ulp
        ulp = np.maximum(ulp, 2.0**-133)
        err = np.abs(got.astype(np.float64) - want)
        assert (err[ok] <= ulp[ok]).all(), (n, (err / ulp)[ok].max())
        assert np.isfinite(got).all()
    # the Python spellings on the view: frobenius_head and the projection's backward
    from poseestimation_amd import rotation_representation as rr
    xv = xb.detach().requires_grad_(True)
    loss, r = rr.frobenius_head(xv, t.view(n, 3, 3))
    loss.backward()
    assert torch.equal(r.reshape(n, 9), rb)
    assert torch.equal(xv.grad.view(torch.int16), dmb.view(torch.int16))
    assert abs(loss.item() - meanb.item()) <= 1e-6 * meanb.item()
    if n <= 65_536 or tile_only:
        g = torch.randn(n, 3, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
        xv = xb.detach().requires_grad_(True)
        rr.symmetric_orthogonalization(xv).backward(g)
        xf2 = xf.detach().requires_grad_(True)
        rr.symmetric_orthogonalization(xf2).backward(g)
        assert xv.grad.dtype == torch.bfloat16
        if off % 2 == 0:                                         # K2 on the same route: the float32 gradient, rounded to nearest even
            assert torch.equal(xv.grad.view(torch.int16), xf2.grad.to(torch.bfloat16).view(torch.int16))
        assert torch.isfinite(xv.grad.float()).all()


# ------------------------------------------------------------------------------------------------
# 3. K3' float32
# ------------------------------------------------------------------------------------------------
def _k3p(lib, p, t, want_grad, ws, flags=0, ls=None):
    n = p.shape[0]
    g = torch.full((n, 9), 7.0, device=DEV) if want_grad else None
    ls = _f64(1) if ls is None else ls
    mean = _f32(1)
    assert lib.so3_frob_loss_v2_f32(_p(p), _p(t), _p(g), _p(ls), _p(mean), _p(ws), flags, n, _st()) == 0
    return g, ls, mean


@pytest.mark.parametrize("idx", range(11), ids=SIZE_IDS)
def test_frob_loss_f32_every_size_and_finish(lib, data, idx):
    n = _sizes()[idx]
    p, t = data["p"][:n], data["t"][:n]
    ws = _ws(lib)
    nrm = _row_norms(p, t)
    exact = math.fsum(nrm.tolist())
    d = (p.double() - t.double()).cpu().numpy()
    gref = d / (n * nrm[:, None])
    g0, ls0, mean0 = _k3p(lib, p, t, True, ws)
    s0 = ls0.item()
    assert abs(s0 - exact) <= _sum_bound(nrm, n, True, ROW_REL), (n, s0, exact)
    assert mean0.item() == float(np.float32(s0 * (1.0 / n)))
    err = np.abs(g0.double().cpu().numpy() - gref).max(1) / np.abs(gref).max(1)
    assert err.max() <= 1e-6, (n, err.max())
    for _ in range(2):                                           # without the gradient, and again: the same bits
        _, ls, mean = _k3p(lib, p, t, False, ws)
        assert ls.item() == s0 and mean.item() == mean0.item()
    assert _zeroed(ws)
    for want_grad in (True, False):
        for flags in (0, PREZEROED):
            g, ls, mean = _k3p(lib, p, t, want_grad, None, flags, ls=_f64(1, 0.0 if flags else 777.0))
            assert abs(ls.item() - exact) <= _sum_bound(nrm, n, False, ROW_REL), (n, want_grad, flags)
            assert mean.item() == float(np.float32(ls.item() * (1.0 / n)))
            if want_grad:
                assert torch.equal(g, g0)


# ------------------------------------------------------------------------------------------------
# 4. the gradient of rows whose difference is tiny or zero, on every route
# ------------------------------------------------------------------------------------------------
def _tiny_kinds():
    """(entries of one row's difference) -- an exact zero, one entry of 1e-20 / 1e-19 / 3e-19, n2 just under and just over 1e-37 and
    2^-100, several tiny entries, the smallest subnormal."""
    f = lambda v: float(np.float32(v))
    return [[], [f(1e-20)], [f(1e-19)], [f(3e-19)], [f(math.sqrt(0.9e-37))], [f(math.sqrt(1.1e-37))],
            [f(2.0**-50 * 0.999)], [f(2.0**-50 * 1.001)], [f(1e-20), f(-2e-20), f(5e-21)], [2.0**-149], [f(1e-19), f(1e-3)]]


def _place(n, nunits_rows, kinds):
    """Rows for each kind: at row 0.., in the last engine unit, and in the remainder."""
    k = len(kinds)
    starts = [0, nunits_rows - 64, nunits_rows] if nunits_rows > 0 else [0]
    rows = []
    for s in starts:
        rows.append(list(range(s, s + k)))
    assert all(r < n for rr_ in rows for r in rr_)
    return rows


OFFDIAG = [1, 2, 3, 5, 6, 7]


def _perturb(base, rows, kinds):
    """base[row] at the off-diagonal positions holds exact zeros; write the kind's entries there (row's difference = -entries)."""
    out = base.clone()
    for r, kind in zip(rows, kinds):
        for j, v in zip(OFFDIAG, kind):
            out[r, j] = out[r, j] - v
    return out


def _check_tiny_grad(got, diff, n, label):
    """got: (k, 9) float32 gradient rows; diff: (k, 9) float64 exact differences.  Zero difference -> exactly 0; otherwise
    diff / (n ||diff||) to 1e-6 relative, finite."""
    assert np.isfinite(got).all(), (label, got)
    nrm = np.sqrt((diff.astype(np.longdouble) ** 2).sum(1)).astype(np.float64)
    for i in range(len(got)):
        if nrm[i] == 0:
            assert not got[i].any(), (label, i, got[i])
        else:
            want = diff[i] / (n * nrm[i])
            assert np.abs(got[i] - want).max() <= 1e-6 * np.abs(want).max(), (label, i, got[i], want)


def test_tiny_and_zero_differences_on_every_route(lib, pa, data):
    kinds = _tiny_kinds()
    k = len(kinds)
    # K3' and K3s: T with zeros off the diagonal in the chosen rows, P = T minus the kind's entries
    for n in (_round() + 81, 1000, 64 * 20 + 17):
        t = data["t"][:n].clone()
        nunits_rows = (n // 64) * 64 if n > 1024 else 0
        placed = _place(n, nunits_rows, kinds)
        for rows in placed:
            for r in rows:
                t[r] = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], device=DEV)
        p = t.clone()
        for rows in placed:
            p = _perturb(p, rows, kinds)
        ws = _ws(lib)
        grads = []
        for w in (ws, None):
            g, ls, _ = _k3p(lib, p, t, True, w)
            nrm = _row_norms(p, t)
            assert abs(ls.item() - math.fsum(nrm.tolist())) <= _sum_bound(nrm, n, w is not None, ROW_REL) + 1e-30
            gn = g.double().cpu().numpy()
            d = (p.double() - t.double()).cpu().numpy()
            for rows in placed:
                _check_tiny_grad(gn[rows], d[rows], n, ("K3'", n, rows[0], w is None))
            grads.append(g)
        assert torch.equal(grads[0], grads[1])
        # every position of one call: the same bits (one arithmetic, frob_row, on every route)
        for rows in placed[1:]:
            assert torch.equal(grads[0][rows], grads[0][placed[0]]), ("K3'", n, rows[0])
        # K3s with the table {I}: the same rows, the same gradient for both arguments
        table = pa.SymmetryTable([pa.cyclic_symmetry(1, "z")])
        S = table.matrices.float().reshape(1, 1, 9).contiguous().to(DEV)
        dp, dt = torch.full((n, 9), 7.0, device=DEV), torch.full((n, 9), 7.0, device=DEV)
        ls, mean = _f64(1), _f32(1)
        assert lib.so3_sym_frob_loss_f32(_p(p), _p(t), _p(S), None, 1, 1, _p(dp), _p(dt), None, _p(ls), _p(mean), _p(ws), 0, n, _st()) == 0
        assert torch.equal(dp, grads[0]) and torch.equal(dt, -grads[0]), ("K3s", n)
        assert _zeroed(ws)
    # K3: M = I in the chosen rows projects to exactly I; T = R of a first call minus the kind's entries off the diagonal
    from oracle import so3_oracle as so
    for n, bf16, off in ((_round() + 81, False, 0), (1000, False, 0), (4 * 1024 + 3, True, 1), (_round() + 81, True, 0)):
        xs = data["x"][:n + 1].clone()
        nunits_rows = (n // 64) * 64 if (n > 1024 and off % 2 == 0) else 0
        placed = _place(n, nunits_rows, kinds) if nunits_rows else [list(range(0, k)), list(range(n - k, n))]
        for rows in placed:
            for r in rows:
                xs[off + r] = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], device=DEV)
        x = (xs.bfloat16() if bf16 else xs)[off:off + n]
        t0 = data["t"][:n]
        r1, _, _, _ = _k3(lib, x, t0, True, False, None, bf16=bf16)
        allrows = sum(placed, [])
        assert (r1[allrows][:, OFFDIAG] == 0).all(), "the projection of I is expected to be exactly I"
        t = r1.clone()
        for rows in placed:
            t = _perturb(t, rows, kinds)
        ws = _ws(lib)
        for w in (ws, None):
            r, dm, ls, _ = _k3(lib, x, t, True, True, w, bf16=bf16)
            assert torch.equal(r, r1)
            d = (r.double() - t.double()).cpu().numpy()
            nrm = np.sqrt((d ** 2).sum(1))
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(nrm[:, None] > 0, d / (n * nrm[:, None]), 0.0)
            dref = so.projection_backward_np(x[allrows].double().cpu().numpy(), g[allrows]).reshape(-1, 9)
            got = dm[allrows].double().cpu().numpy()
            assert np.isfinite(got).all(), ("K3", n, bf16, off)
            zero = nrm[allrows] == 0
            assert not got[zero].any()
            scale = np.abs(dref).max(1, keepdims=True)
            tol = 1e-6 * scale + (2.0**-8 * scale if bf16 else 0.0)
            assert (np.abs(got - dref) <= tol).all(), ("K3", n, bf16, off, np.abs(got - dref).max(), scale.max())
            full = _row_norms(r, t)
            assert abs(ls.item() - math.fsum(full.tolist())) <= _sum_bound(full, n, w is not None, ROW_REL) + 1e-30
        assert _zeroed(ws)


# ------------------------------------------------------------------------------------------------
# 5. a NaN row: NaN out, promptly, on every route
# ------------------------------------------------------------------------------------------------
def test_nan_rows_are_nan_and_prompt_on_every_route(lib, data):
    n = _round() + 81
    nunits_rows = (n // 64) * 64
    t = data["t"][:n]
    ws = _ws(lib)
    for row in (0, nunits_rows - 1, n - 1):
        p = data["p"][:n].clone()
        p[row, 4] = float("nan")
        x = data["x"][:n].clone()
        x[row, 4] = float("nan")
        for w in (ws, None):
            _k3p(lib, data["p"][:n], t, True, w)                                    # warm
            (g, ls, mean), ms = _timed(lambda: _k3p(lib, p, t, True, w))
            assert math.isnan(ls.item()) and math.isnan(mean.item()) and ms < 5.0, ("K3'", row, ms)
            (r, dm, ls, mean), ms = _timed(lambda: _k3(lib, x, t, True, True, w))
            assert math.isnan(ls.item()) and ms < 5.0, ("K3", row, ms)
            sc = _f64(2)
            (_, ms) = _timed(lambda: lib.so3_angle_error_v2(_p(p), _p(t), None, _p(sc), None, _p(w), 0, n, _st()))
            assert math.isnan(sc[0].item()) and ms < 5.0, ("K4", row, ms)
        assert _zeroed(ws)
    p = data["p"][:1000].clone()
    p[999, 0] = float("nan")
    _, ls, _ = _k3p(lib, p, t[:1000], True, None)
    assert math.isnan(ls.item())


# ------------------------------------------------------------------------------------------------
# 6. sums without per-row values: K4, K1+K4 (float64 and float32 sums), geodesic
# ------------------------------------------------------------------------------------------------
def _angle_row_bound_f32_sum(deg):
    """so3_rows.h (angle_sum_f32): outside the band |c| >= 1 - 5e-7 a row differs from its float64 angle by at most 2e-7 / sin(theta)
    rad (the float32 trace's round-off through acos) plus the polynomial's 1.2e-9 rad; inside it the float64 arithmetic runs."""
    th = np.radians(deg)
    return (2e-7 / np.maximum(np.sin(th), 1e-3) + 2e-9) * DEG


@pytest.mark.parametrize("idx", range(11), ids=SIZE_IDS)
def test_angle_sums_against_fsum(lib, data, idx):
    n = _sizes()[idx]
    p, t, x = data["p"][:n], data["t"][:n], data["x"][:n]
    ws = _ws(lib)
    st = _st()
    # K4: the per-row float64 angles, then the sum alone
    deg = _f64(n)
    assert lib.so3_angle_error_v2(_p(p), _p(t), _p(deg), None, None, None, 0, n, st) == 0
    dn = deg.cpu().numpy()
    exact = math.fsum(dn.tolist())
    sums = []
    for w, flags in ((ws, 0), (ws, 0), (None, 0), (None, PREZEROED)):
        sc, fl = _f64(2, 0.0 if flags else 777.0), torch.full((1,), 0 if flags else 9, dtype=torch.int32, device=DEV)
        assert lib.so3_angle_error_v2(_p(p), _p(t), None, _p(sc), _p(fl), _p(w), flags, n, st) == 0
        s, cnt = sc.tolist()
        assert cnt == n and fl.item() == 0
        assert abs(s - exact) <= _depth(n, w is not None) * U * exact, (n, w is None, flags, s, exact)
        sums.append(s)
    assert sums[0] == sums[1]
    assert _zeroed(ws)
    # K1 + K4: per-row angles of the materialised R, then the float64 sum (SO3_EXACT_F64) and the float32 one
    r = torch.empty(n, 9, device=DEV)
    deg = _f64(n)
    assert lib.so3_project_angle_error_v2_f32(_p(x), _p(t), _p(r), _p(deg), None, None, None, 0, n, st) == 0
    dn = deg.cpu().numpy()
    exact = math.fsum(dn.tolist())
    bound_f32 = math.fsum(_angle_row_bound_f32_sum(dn).tolist())
    for exact_flag in (EXACT_F64, 0):
        runs = []
        for w, flags in ((ws, 0), (ws, 0), (None, 0), (None, PREZEROED)):
            sc = _f64(2, 0.0 if flags else 777.0)
            r2 = torch.empty(n, 9, device=DEV) if n % 64 else None
            assert lib.so3_project_angle_error_v2_f32(_p(x), _p(t), _p(r2), None, _p(sc), None, _p(w), flags | exact_flag, n, st) == 0
            s, cnt = sc.tolist()
            assert cnt == n
            bound = _depth(n, w is not None) * U * exact + (bound_f32 if (exact_flag == 0 and n > 1024) else 0.0)
            assert abs(s - exact) <= bound, (n, exact_flag, w is None, flags, s - exact, bound)
            runs.append(s)
        assert runs[0] == runs[1]
    assert _zeroed(ws)
    # geodesic with eps: float32 theta per row, the float64 sum of them, sum and mean
    eps = 1e-7
    th, acc0 = _f32(n), _f64(1)
    assert lib.so3_geodesic_eps_f32(_p(p), _p(t), _p(th), _p(acc0), None, 0, eps, _p(ws), n, st) == 0     # theta of the summing op
    tn = th.double().cpu().numpy()
    exact = math.fsum(tn.tolist())
    for mean in (0, 1):
        res = []
        for w in (ws, ws, None):
            acc, out = _f64(1), _f32(1)
            assert lib.so3_geodesic_eps_f32(_p(p), _p(t), None, _p(acc), _p(out), mean, eps, _p(w), n, st) == 0
            s = acc.item()
            assert abs(s - exact) <= _depth(n, w is not None) * U * exact, (n, mean, w is None)
            if w is not None:
                assert s == acc0.item()
            assert out.item() == float(np.float32(s * (1.0 / n) if mean else s))
            res.append(s)
        assert res[0] == res[1]
    assert _zeroed(ws)


@pytest.mark.parametrize("n", [3, 1088, 1091])
def test_projected_angle_rows_and_sum_in_one_call(lib, data, n):
    """K1 + K4 writing the per-row angles AND their sum (OpProjectAngle<4, WR, true, true, false>, with SO3_EXACT_F64 and without: the
    float32 sum exists for the sum alone), R given and, where no remainder needs it (17 whole units), left out: one workgroup, the
    engine alone, engine + remainder + workspace finish.  The sum against fsum of the rows the same call wrote."""
    t, x = data["t"][:n], data["x"][:n]
    ws, st = _ws(lib), _st()
    for exact_flag in (EXACT_F64, 0):
        for with_r in ((True, False) if n % 64 == 0 else (True,)):
            for w in (ws, None):
                r = torch.empty(n, 9, device=DEV) if with_r else None
                deg, sc = _f64(n), _f64(2, 777.0)
                assert lib.so3_project_angle_error_v2_f32(_p(x), _p(t), _p(r), _p(deg), _p(sc), None, _p(w), exact_flag, n, st) == 0
                s, cnt = sc.tolist()
                exact = math.fsum(deg.cpu().numpy().tolist())
                assert cnt == n
                assert abs(s - exact) <= _depth(n, w is not None) * U * exact, (n, exact_flag, with_r, w is None, s - exact)
    assert _zeroed(ws)


# ------------------------------------------------------------------------------------------------
# 7. SO3_PREZEROED accumulating over several calls, one per shard
# ------------------------------------------------------------------------------------------------
def test_prezeroed_accumulates_over_shards(lib, data):
    r = _round()
    n = 3 * r + 5
    cuts = [0, 1000, 1000 + r + 81, 1000 + r + 81 + 63, n]          # a one-workgroup shard, engine + remainder, 63 rows, the rest
    p, t, x = data["p"][:n], data["t"][:n], data["x"][:n]
    st = _st()
    # K3'
    nrm = _row_norms(p, t)
    exact = math.fsum(nrm.tolist())
    acc = _f64(1, 0.0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        _k3p(lib, p[a:b], t[a:b], False, None, PREZEROED, ls=acc)
    assert abs(acc.item() - exact) <= _sum_bound(nrm, n, False, ROW_REL) * 2, (acc.item(), exact)
    # K3: the one-call sum against the shards' (rows differ by route: each within its row bound)
    r1, _, ls1, _ = _k3(lib, x, t, True, False, None)
    nrm = _row_norms(r1, t)
    acc = _f64(1, 0.0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        _k3(lib, x[a:b], t[a:b], False, True, None, PREZEROED, ls=acc)
    assert abs(acc.item() - ls1.item()) <= 2 * _sum_bound(nrm, n, False, 4 * ROW_REL), (acc.item(), ls1.item())
    # K4 and K1+K4 (float64 rows on every route): sum and range flag
    deg = _f64(n)
    assert lib.so3_angle_error_v2(_p(p), _p(t), _p(deg), None, None, None, 0, n, st) == 0
    exact = math.fsum(deg.cpu().numpy().tolist())
    for bad_shard in (None, 0, 1, 3):
        tt = t.clone()
        if bad_shard is not None:
            tt[cuts[bad_shard] + 7] = 3.0 * p[cuts[bad_shard] + 7]
        sc, fl = _f64(2, 0.0), torch.zeros(1, dtype=torch.int32, device=DEV)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert lib.so3_angle_error_v2(_p(p[a:b]), _p(tt[a:b]), None, _p(sc), _p(fl), None, PREZEROED, b - a, st) == 0
        assert fl.item() == (0 if bad_shard is None else 1), bad_shard
        if bad_shard is None:
            assert abs(sc[0].item() - exact) <= 2 * _depth(n, False) * U * exact
    deg = _f64(n)
    rr_ = torch.empty(n, 9, device=DEV)
    assert lib.so3_project_angle_error_v2_f32(_p(x), _p(t), _p(rr_), _p(deg), None, None, None, 0, n, st) == 0
    dn = deg.cpu().numpy()
    exact = math.fsum(dn.tolist())
    for flags, bound in ((EXACT_F64, 2 * _depth(n, False) * U * exact),
                         (0, 2 * _depth(n, False) * U * exact + math.fsum(_angle_row_bound_f32_sum(dn).tolist()))):
        sc, fl = _f64(2, 0.0), torch.zeros(1, dtype=torch.int32, device=DEV)
        r2 = torch.empty(n, 9, device=DEV)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert lib.so3_project_angle_error_v2_f32(_p(x[a:b]), _p(t[a:b]), _p(r2[a:b]), None, _p(sc), _p(fl), None, PREZEROED | flags,
                                                      b - a, st) == 0
        assert fl.item() == 0 and abs(sc[0].item() - exact) <= bound, (flags, sc[0].item() - exact, bound)


# ------------------------------------------------------------------------------------------------
# 8. the range flag from every share of the grid
# ------------------------------------------------------------------------------------------------
def test_range_flag_from_every_share(lib, data):
    r = _round()
    st = _st()
    ws = _ws(lib)
    for n in (3 * r + 5, r + 81, 1000):
        p, t0, x = data["p"][:n], data["t"][:n], data["x"][:n]
        from poseestimation_amd import rotation_representation as rr
        rx = rr.symmetric_orthogonalization(x.view(n, 3, 3)).reshape(n, 9)
        nunits_rows = (n // 64) * 64 if n > 1024 else 0
        cases = {"first workgroup": [3], "remainder": [n - 1] if n % 64 else [n - 2], "every workgroup": list(range(5, n, 64))}
        if nunits_rows and n % 64:
            cases["last engine unit"] = [nunits_rows - 2]
        for name, rows in cases.items():
            t = t0.clone()
            t[rows] = 3.0 * p[rows]
            tb = t0.clone()
            tb[rows] = 3.0 * rx[rows]                                    # for K1+K4: Rtrue = 3 proj(M), cosine 4
            for w, flags in ((ws, 0), (None, 0), (None, PREZEROED)):
                for entry, a, b_ in (("K4", p, t), ("K1+K4", x, tb)):
                    for want_sum in (True, False):
                        sc = _f64(2, 0.0) if want_sum else None
                        fl = torch.full((1,), 0 if flags else 9, dtype=torch.int32, device=DEV)
                        rbuf = torch.empty(n, 9, device=DEV)
                        if entry == "K4":
                            rc = lib.so3_angle_error_v2(_p(a), _p(b_), None, _p(sc), _p(fl), _p(w), flags, n, st)
                        else:
                            rc = lib.so3_project_angle_error_v2_f32(_p(a), _p(b_), _p(rbuf), None, _p(sc), _p(fl), _p(w), flags, n, st)
                        assert rc == 0 and fl.item() == 1, (n, name, entry, w is None, flags, want_sum)
                        fl = torch.full((1,), 0 if flags else 9, dtype=torch.int32, device=DEV)
                        sc = _f64(2, 0.0) if want_sum else None
                        if entry == "K4":
                            rc = lib.so3_angle_error_v2(_p(a), _p(t0), None, _p(sc), _p(fl), _p(w), flags, n, st)
                        else:
                            rc = lib.so3_project_angle_error_v2_f32(_p(a), _p(t0), _p(rbuf), None, _p(sc), _p(fl), _p(w), flags, n, st)
                        assert rc == 0 and fl.item() == 0, (n, name, entry, "clean")
            assert _zeroed(ws)


# ------------------------------------------------------------------------------------------------
# 9. symmetry tables at their limits
# ------------------------------------------------------------------------------------------------
def _sym_call(lib, p, t, S, cls, C, K, ws):
    n = p.shape[0]
    st = _st()
    deg, idx, fo = _f64(n), torch.full((n,), 99, dtype=torch.int32, device=DEV), torch.full((1,), 9, dtype=torch.int32, device=DEV)
    assert lib.so3_sym_angle_error_f32(_p(p), _p(t), _p(S), _p(cls), C, K, _p(deg), _p(idx), _p(fo), 0, n, st) == 0
    dp, dt = torch.full((n, 9), 7.0, device=DEV), torch.full((n, 9), 7.0, device=DEV)
    lidx, ls, mean = torch.full((n,), 99, dtype=torch.int32, device=DEV), _f64(1), _f32(1)
    assert lib.so3_sym_frob_loss_f32(_p(p), _p(t), _p(S), _p(cls), C, K, _p(dp), _p(dt), _p(lidx), _p(ls), _p(mean), _p(ws), 0, n, st) == 0
    return deg, idx, fo, dp, dt, lidx, ls, mean


@pytest.mark.parametrize("which", ["C64", "4x64", "256x1"])
def test_symmetry_tables_at_their_limits(lib, pa, data, which):
    r = _round()
    if which == "C64":
        table = pa.SymmetryTable([pa.cyclic_symmetry(64, "z")])
    elif which == "4x64":
        table = pa.SymmetryTable([pa.cyclic_symmetry(64, "z"), pa.cyclic_symmetry(32, "x"), pa.cyclic_symmetry(7, [1.0, 2.0, 3.0]),
                                  pa.cyclic_symmetry(1, "z")])
    else:
        table = pa.SymmetryTable([pa.cyclic_symmetry(1, "z")] * 256)
    mats = table.matrices
    C, K = mats.shape[0], mats.shape[1]
    assert (which, C, K) in (("C64", 1, 64), ("4x64", 4, 64), ("256x1", 256, 1))
    S = mats.float().reshape(C, K, 9).contiguous().to(DEV)
    Sn = mats.float().numpy()
    gen = torch.Generator(device=DEV).manual_seed(7)
    for n in (1, 1025, r + 81, 3 * r + 5):
        p, t = data["p"][:n], data["t"][:n]
        cls = torch.randint(0, C, (n,), device=DEV, generator=gen, dtype=torch.int32) if C > 1 else None
        ws = _ws(lib)
        deg, idx, fo, dp, dt, lidx, ls, mean = _sym_call(lib, p, t, S, cls, C, K, ws)
        assert _zeroed(ws)
        deg2, idx2, fo2, dp2, dt2, lidx2, ls2, _ = _sym_call(lib, p, t, S, cls, C, K, None)
        assert torch.equal(deg, deg2) and torch.equal(idx, idx2) and torch.equal(dp, dp2) and torch.equal(dt, dt2) and torch.equal(lidx, lidx2)
        assert fo.item() == 0 and fo2.item() == 0
        assert mean.item() == float(np.float32(ls.item() * (1.0 / n)))
        rows = _sample_rows(n)
        pn, tn = p[rows].cpu().numpy(), t[rows].cpu().numpy()
        cn = None if cls is None else cls[rows].cpu().numpy()
        o = sym_oracle(pn, tn, Sn, cn)
        assert_angles(deg[rows].cpu().numpy(), o["deg"], (which, n))
        c0 = np.zeros(len(rows), np.int64) if cn is None else cn
        sure = trace_margin(pn, tn, Sn, c0) >= 1e-6
        assert np.array_equal(idx[rows].cpu().numpy()[sure], o["idx"][sure]), (which, n)
        sure_l = trace_margin(pn, tn, Sn, c0, loss=True) >= 1e-5
        assert np.array_equal(lidx[rows].cpu().numpy()[sure_l], o["loss_idx"][sure_l]), (which, n)
        tol = (2e-6 + 4e-7 / o["dist"]) / len(rows)
        for got, ref in ((dp, o["dp"]), (dt, o["dt"])):
            gg = got[rows].double().cpu().numpy().reshape(-1, 3, 3) * (n / len(rows))      # the oracle's 1/B is the sample's
            err = np.abs(gg - ref).max(axis=(1, 2))
            assert np.all((err <= tol)[sure_l]), (which, n, (err / tol)[sure_l].max())
        # the loss against fsum of the oracle's per-row distances (a near tie may select the other branch: 1e-5 of trace)
        if n <= r + 81:
            dist = np.concatenate([sym_oracle(p[a:a + 16384].cpu().numpy(), t[a:a + 16384].cpu().numpy(), Sn,
                                              None if cls is None else cls[a:a + 16384].cpu().numpy())["dist"] for a in range(0, n, 16384)])
            exact = math.fsum(dist.tolist())
            for got, w in ((ls, True), (ls2, False)):
                assert abs(got.item() - exact) <= _sum_bound(dist, n, w, ROW_REL) + 1e-5 * n, (which, n, got.item(), exact)
        else:
            assert abs(ls.item() - ls2.item()) <= 2 * _depth(n, False) * U * ls.item()
        if which == "256x1":
            # K = 1: the angle is so3_angle_error_v2's, bit for bit, index 0; the loss is so3_frob_loss_v2_f32's to float32 rounding
            ref = _f64(n)
            assert lib.so3_angle_error_v2(_p(p), _p(t), _p(ref), None, None, None, 0, n, _st()) == 0
            assert torch.equal(deg, ref) and (idx == 0).all() and (lidx == 0).all()
            _, lsf, _ = _k3p(lib, p, t, False, _ws(lib))
            assert abs(ls.item() - lsf.item()) <= 1e-6 * lsf.item()
        if which == "4x64" and n >= 1025:
            # padding with the identity ties exactly with k = 0, and the smallest k wins: C_1 rows pick 0, C_7 rows k < 7, C_32 rows k < 32
            cn_all = cls.cpu().numpy()
            ia, il = idx.cpu().numpy(), lidx.cpu().numpy()
            for c, size in ((3, 1), (2, 7), (1, 32)):
                assert (ia[cn_all == c] < size).all() and (il[cn_all == c] < size).all(), (which, n, c)
        # class ids out of range: NaN, index -1, flag bit 1, the loss NaN
        if C > 1:
            bad_cls = cls.clone()
            bad_cls[n // 2] = C
            bad_cls[0] = -1 if n > 1 else C
            deg, idx, fo, dp, dt, lidx, ls, _ = _sym_call(lib, p, t, S, bad_cls, C, K, ws)
            bad = (bad_cls < 0) | (bad_cls >= C)
            assert fo.item() == 2 and math.isnan(ls.item())
            assert torch.isnan(deg[bad]).all() and (idx[bad] == -1).all() and (lidx[bad] == -1).all()
            assert torch.isnan(dp[bad]).all() and torch.isnan(dt[bad]).all()
            assert torch.equal(deg[~bad], deg2[~bad]) and torch.equal(idx[~bad], idx2[~bad]) and torch.equal(dp[~bad], dp2[~bad])
            assert _zeroed(ws)
