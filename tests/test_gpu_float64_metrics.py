"""The float64 twins of the metrics and the loss (csrc/so3proj.hip: k_angle_f64, k_frob_loss_f64, k_angle_bwd_f64) and the float64 acos
every angle of the library goes through (csrc/so3_rows.h: acos_f64), on the device, against plain high-precision references: numpy float64,
math.fsum, np.longdouble.  Double tensors reach these kernels through every metric spelling and loss_frobenius (the reference accepts them,
and the float64 head returns them).

The batch sizes are chosen to hit each way a reduction is finished (so3proj.hip: reduce_how): one workgroup up to 1024 rows (how = 1), the
ticket finish on a caller's workspace (how = 2), atomics onto accumulators zeroed by an init launch (how = 0), and the grid-stride loop past
the grid cap -- 2 x CUs workgroups of 256 rows for the reducing entries, 2048 for the others."""
import math

import numpy as np
import pytest
import torch

from conftest import metric_grad_check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0**-53                              # unit round-off of float64
RADIANS, PREZEROED, EXACT_F64, GRAD_SCALAR, F64_MATH = 0x1, 0x2, 0x4, 0x8, 0x10      # include/so3proj.h
ERR_INVALID = -1
BLOCK = 256                               # rows per workgroup and sweep of the float64 kernels (so3proj.cpp: kBlock)
DEG = 180.0 / np.pi


@pytest.fixture(scope="module")
def pa():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import poseestimation_amd as pa_
    from poseestimation_amd import _lib
    _lib.load()                                   # fail loudly if the HIP extension is missing
    return pa_


@pytest.fixture(scope="module")
def rr(pa):
    from poseestimation_amd import rotation_representation
    return rotation_representation


@pytest.fixture(scope="module")
def lib(pa):
    from poseestimation_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _reduce_sizes():
    """1, 1024 (one workgroup), 1025 (the first batch that needs a workspace or atomics), 2 x CUs x 256 +- 1 (the reducing entries' grid
    cap: one row over it is the first second sweep), 2048 x 256 + 1 (the other entries' cap) and 1 000 003."""
    cap = 2 * _cus() * BLOCK
    return [1, 1024, 1025, cap - 1, cap + 1, 2048 * BLOCK + 1, 1_000_003]


def _haar_rows(n, gen):
    q = torch.randn(n, 4, device=DEV, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                        2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).contiguous()


def _grid(n, cap):
    return min((n + BLOCK - 1) // BLOCK, cap)


def _sum_depth(n, how, grid):
    """How many additions one row's angle (or norm) passes through on its way into the kernel's float64 sum, at most: the thread's own rows
    (grid-stride), block_sum (6 shuffle levels, then the 4 waves' partials in a row), and then -- ticket finish -- each thread's slots,
    6 shuffle levels and 4 waves again, or -- atomics -- the chain of the grid's atomicAdds on one address.  Every term is >= 0, so each
    addition errs by at most U times the whole sum, and the sum by at most depth * U * sum.  The ordered finishes stay below 64; the
    atomics' chain is as long as the grid, and their bound says so."""
    d = -(-n // (grid * BLOCK)) + 6 + 4
    if how == 2:
        d += -(-grid // BLOCK) + 6 + 4
    elif how == 0:
        d += grid
    assert how == 0 or d <= 64, d
    return max(d, 64)


def _cos_np(a, b):
    a = np.asarray(a, np.float64).reshape(-1, 9)
    b = np.asarray(b, np.float64).reshape(-1, 9)
    return ((a * b).sum(1) - 1.0) / 2.0


def _cond_err(got_rad, ref_rad):
    """|d theta| * max(sin theta, 1e-8): a cosine known to a few float64 ulps fixes theta to that over sin(theta), no better."""
    return np.abs(got_rad - ref_rad) * np.maximum(np.sin(ref_rad), 1e-8)


# ------------------------------------------------------------------------------------------------
# 1. acos_f64 through the device, exactly
# ------------------------------------------------------------------------------------------------
def _exact_cosine_rows(c, dtype):
    """R1 = I, R2 = diag(1, c, c): tr = 1 + 2c and c_raw = (tr - 1)/2 = c with no rounding in float64 (and for float32 data, which the
    float64 kernels widen first), so each row's angle is exactly the kernel's acos of c."""
    n = c.shape[0]
    r1 = torch.zeros(n, 9, dtype=dtype)
    r1[:, 0] = r1[:, 4] = r1[:, 8] = 1.0
    r2 = torch.zeros(n, 9, dtype=dtype)
    r2[:, 0] = 1.0
    ct = torch.from_numpy(c).to(dtype)
    r2[:, 4] = ct
    r2[:, 8] = ct
    return r1.to(DEV), r2.to(DEV)


def _sweep_cosines():
    k = np.arange(-2**20, 2**20 + 1, dtype=np.float64)
    j = np.arange(-2048, 2049, dtype=np.float64)
    i = np.arange(0, 4096, dtype=np.float64)
    c = np.concatenate(([0.0, -0.0, 1.0, -1.0],
                        k * 2.0**-20,                                           # 2^21 + 1 cosines over [-1, 1]
                        0.5 + j * 2.0**-34, -0.5 + j * 2.0**-34,                # the branch switch of acos_f64
                        0.5 + j * 2.0**-25, -0.5 + j * 2.0**-25,
                        1.0 - i * 2.0**-20, -1.0 + i * 2.0**-20,                # c = +-(1 - j 2^-20)
                        1.0 - i * 2.0**-44, -1.0 + i * 2.0**-44))
    return c if len(c) % 64 else np.append(c, 0.25)        # not a multiple of 64 rows: the float32 engine's remainder kernel runs too


def _check_acos(got, c):
    ref = np.arccos(c.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert err.max() <= 1.5e-14, (err.max(), c[err.argmax()])
    big = (c > 0.5) & (c < 1.0)
    rel = err[big] / ref[big].astype(np.float64)
    assert rel.max() <= 1e-14, (rel.max(), c[big][rel.argmax()])
    assert (got[c == 1.0] == 0.0).all() and (got[c == -1.0] == np.pi).all()


def test_device_acos_exactly_against_long_double(lib):
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double for the reference"
    c = _sweep_cosines()
    n = c.shape[0]
    st = _st()
    for dtype, entry in ((torch.float64, lib.so3_angle_error_v2_f64), (torch.float32, lib.so3_angle_error_v2)):
        cc = c.astype(np.float32).astype(np.float64) if dtype is torch.float32 else c      # what the kernel reads
        r1, r2 = _exact_cosine_rows(cc, dtype)
        rad = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
        deg = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
        fl = torch.full((1,), 9, dtype=torch.int32, device=DEV)
        assert entry(_p(r1), _p(r2), _p(rad), None, _p(fl), None, RADIANS, n, st) == 0
        assert entry(_p(r1), _p(r2), _p(deg), None, None, None, 0, n, st) == 0
        rad, deg = rad.cpu().numpy(), deg.cpu().numpy()
        assert fl.item() == 0
        _check_acos(rad, cc)
        # degrees: the same acos times 180/pi, one more rounding
        ref_deg = np.arccos(cc.astype(np.longdouble)) * (np.longdouble(180) / np.arccos(np.longdouble(-1)))
        err = np.abs(deg.astype(np.longdouble) - ref_deg).astype(np.float64)
        assert (err <= 1.5e-14 * DEG + 2 * U * np.abs(deg)).all(), err.max()
        if dtype is torch.float64:
            theta = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)          # compute_geodesic_distance's twin: the hard clamp
            assert lib.so3_geodesic_f64(_p(r1), _p(r2), _p(theta), n, st) == 0
            assert np.array_equal(theta.cpu().numpy(), rad)


def test_device_eps_clamps_at_their_bound(lib):
    """geodesic's clamp to [-1 + 1e-7, 1 - 1e-7]: so3_geodesic_eps_f64 on the exact rows against long double acos of the clamped cosine,
    so3_geodesic_eps_f32 against oracle.geodesic_eps_np to 2 float32 ulps of theta, and both AT the bound equal to acos of the bound."""
    from oracle import so3_oracle as so
    st = _st()
    eps = 1e-7
    # float64: c = 1 - j 2^-24 straddles 1 - 1e-7 (j = 1 above it, j = 2 below), and its mirror image at -1; plus the sweep
    j = np.arange(0, 64, dtype=np.float64)
    c = np.concatenate((1.0 - j * 2.0**-24, -1.0 + j * 2.0**-24, _sweep_cosines()[::7]))
    n = c.shape[0]
    r1, r2 = _exact_cosine_rows(c, torch.float64)
    theta = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    assert lib.so3_geodesic_eps_f64(_p(r1), _p(r2), _p(theta), None, None, 0, eps, n, st) == 0
    got = theta.cpu().numpy()
    cl = np.clip(c, -1.0 + eps, 1.0 - eps)
    _check_acos(got, cl)
    hi, lo = 1.0 - eps, -1.0 + eps
    bound_hi = float(np.arccos(np.longdouble(hi)))
    bound_lo = float(np.arccos(np.longdouble(lo)))
    assert np.abs(got[c >= hi] - bound_hi).max() <= 1e-14 * bound_hi and np.abs(got[c <= lo] - bound_lo).max() <= 1.5e-14
    near1, near_m1 = got[:64], got[64:128]
    assert (near1[:2] == near1[0]).all() and (near1[2:] > near1[0]).all() and (near_m1[:2] == near_m1[0]).all() and (near_m1[2:] < near_m1[0]).all()
    hard = torch.full((n,), 7.0, dtype=torch.float64, device=DEV)
    assert lib.so3_geodesic_f64(_p(r1), _p(r2), _p(hard), n, st) == 0
    hard = hard.cpu().numpy()
    assert hard[0] == 0.0 and hard[64] == np.pi                               # c = +-1: the hard clamp does not move them
    # float32: through a float32 trace only even j reach the kernel exactly (1 + 2c = 3 - j 2^-23 is a float32 for even j), and
    # float32(1 - 1e-7) = 1 - 2^-23 is j = 2: j = 0 is clamped, 2 sits on the bound, 4.. pass through
    j32 = np.arange(0, 64, 2, dtype=np.float64)
    c32 = np.concatenate((1.0 - j32 * 2.0**-24, -1.0 + j32 * 2.0**-24))
    n32 = c32.shape[0]
    a, b = _exact_cosine_rows(c32, torch.float32)
    th32 = torch.full((n32,), 7.0, dtype=torch.float32, device=DEV)
    assert lib.so3_geodesic_eps_f32(_p(a), _p(b), _p(th32), None, None, 0, eps, None, n32, st) == 0
    got32 = th32.cpu().numpy()
    ref32 = so.geodesic_eps_np(a.cpu().numpy(), b.cpu().numpy(), "none")
    ulp = np.spacing(np.abs(ref32).astype(np.float32)).astype(np.float64)
    assert (np.abs(got32.astype(np.float64) - ref32.astype(np.float64)) <= 2 * ulp).all()
    at_hi = np.arccos(np.float32(1 - eps))
    for row in (0, 1):                                                        # j = 0 (clamped) and j = 2 (on the bound)
        assert abs(float(got32[row]) - float(at_hi)) <= 2 * float(np.spacing(at_hi)), (row, got32[row], at_hi)
    assert got32[0] == got32[1] < got32[2]


# ------------------------------------------------------------------------------------------------
# 3. every float64 reduction path against math.fsum
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def haar_pairs(pa):
    gen = torch.Generator(device=DEV).manual_seed(64)
    n = max(_reduce_sizes())
    return _haar_rows(n, gen), _haar_rows(n, gen)


def _f64(k, v=777.0):
    return torch.full((k,), v, dtype=torch.float64, device=DEV)


def _flag():
    return torch.full((1,), 9, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("idx", range(7))
def test_angle_error_f64_reductions_against_fsum(lib, haar_pairs, idx):
    from oracle import so3_oracle as so
    n = _reduce_sizes()[idx]
    a, b = haar_pairs[0][:n], haar_pairs[1][:n]
    st = _st()
    ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    grid = _grid(n, 2 * _cus())
    ref = so.angle_error_np(a.cpu().numpy(), b.cpu().numpy())
    ref_rad = ref / DEG
    for w in (ws, None):
        how = 1 if n <= 1024 else (2 if w is not None else 0)
        deg, sc, fl = _f64(n), _f64(2), _flag()
        assert lib.so3_angle_error_v2_f64(_p(a), _p(b), _p(deg), _p(sc), _p(fl), _p(w), 0, n, st) == 0
        got = deg.cpu().numpy()
        assert _cond_err(got / DEG, ref_rad).max() <= 4e-15, (n, how, _cond_err(got / DEG, ref_rad).max())
        exact = math.fsum(got.tolist())
        s, cnt = sc.tolist()
        assert cnt == n and fl.item() == 0
        assert abs(s - exact) <= _sum_depth(n, how, grid) * U * exact, (n, how, s, exact)
        if w is not None:
            runs = [s]
            for _ in range(2):
                sc2 = _f64(2)
                assert lib.so3_angle_error_v2_f64(_p(a), _p(b), _p(deg), _p(sc2), _p(fl), _p(w), 0, n, st) == 0
                runs.append(sc2[0].item())
            assert runs[0] == runs[1] == runs[2]                               # the same bits, call after call
        # one output at a time: deg only, sum only, flag only
        deg2 = _f64(n)
        assert lib.so3_angle_error_v2_f64(_p(a), _p(b), _p(deg2), None, None, _p(w), 0, n, st) == 0
        assert torch.equal(deg2, deg)
        sc2 = _f64(2)
        assert lib.so3_angle_error_v2_f64(_p(a), _p(b), None, _p(sc2), None, _p(w), 0, n, st) == 0
        assert sc2[1].item() == n and abs(sc2[0].item() - exact) <= _sum_depth(n, how, grid) * U * exact
        if how != 0:
            assert sc2[0].item() == s
        fl2 = _flag()
        assert lib.so3_angle_error_v2_f64(_p(a), _p(b), None, None, _p(fl2), _p(w), 0, n, st) == 0
        assert fl2.item() == 0
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws).item()) == 0                           # slots, flag and ticket left zeroed


def test_angle_error_f64_range_flag_from_every_share_of_the_grid(lib, haar_pairs):
    """A row with cosine 4 (R2 = 3 R1) in the first workgroup's share, the last one's, or the second grid-stride sweep raises the flag with
    the ticket finish and with the atomics; the next clean call on the same workspace clears it."""
    n = 1_000_003
    grid = _grid(n, 2 * _cus())
    assert n > grid * BLOCK
    a, b0 = haar_pairs[0][:n], haar_pairs[1][:n]
    st = _st()
    ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for row in (0, 17, (grid - 1) * BLOCK + 3, grid * BLOCK + 5, n - 1):
        b = b0.clone()
        b[row] = 3.0 * a[row]
        for w in (ws, None):
            fl, sc = _flag(), _f64(2)
            assert lib.so3_angle_error_v2_f64(_p(a), _p(b), None, _p(sc), _p(fl), _p(w), RADIANS, n, st) == 0
            assert fl.item() == 1 and sc[1].item() == n, (row, w is None)
            fl = _flag()
            assert lib.so3_angle_error_v2_f64(_p(a), _p(b0), None, None, _p(fl), _p(w), RADIANS, n, st) == 0
            assert fl.item() == 0, (row, w is None)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws).item()) == 0


def test_angle_error_f64_refuses_unknown_flags_and_writes_nothing(lib, haar_pairs):
    st = _st()
    for n in (1000, 5000):
        a, b = haar_pairs[0][:n], haar_pairs[1][:n]
        ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
        for flags in (PREZEROED, EXACT_F64, GRAD_SCALAR, F64_MATH, 0x20, 0x80000000, RADIANS | PREZEROED, RADIANS | EXACT_F64):
            for w in (ws, None):
                deg, sc, fl = _f64(n), _f64(2), _flag()
                assert lib.so3_angle_error_v2_f64(_p(a), _p(b), _p(deg), _p(sc), _p(fl), _p(w), flags, n, st) == ERR_INVALID
                torch.cuda.synchronize()
                assert (deg == 777.0).all() and sc.tolist() == [777.0, 777.0] and fl.item() == 9, (n, flags)
        assert int(torch.count_nonzero(ws).item()) == 0
    assert lib.so3_frob_loss_v2_f64(_p(a), _p(b), None, _p(sc), None, None, RADIANS, n, st) == ERR_INVALID


@pytest.mark.parametrize("idx", range(7))
def test_frob_loss_f64_against_fsum_and_the_closed_form(lib, haar_pairs, idx):
    n = _reduce_sizes()[idx]
    gen = torch.Generator(device=DEV).manual_seed(n)
    p = haar_pairs[0][:n] + 1e-3 * torch.randn(n, 9, device=DEV, generator=gen, dtype=torch.float64)
    t = haar_pairs[1][:n].clone()
    z = n // 2
    t[z] = p[z]                                                               # a zero difference: its gradient is exactly 0
    st = _st()
    ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    grid = _grid(n, 2 * _cus())
    d = (p - t).cpu().numpy()                                                 # the same float64 subtraction the kernel makes
    nrm = np.sqrt((d.astype(np.longdouble) ** 2).sum(1))
    exact = math.fsum(nrm.astype(np.float64).tolist())
    dref = d.astype(np.longdouble) / (n * np.where(nrm > 0, nrm, 1))[:, None]
    for w in (ws, None):
        how = 1 if n <= 1024 else (2 if w is not None else 0)
        runs = []
        for want_grad in (True, False, False):
            g = torch.full((n, 9), 7.0, dtype=torch.float64, device=DEV) if want_grad else None
            ls, mean = _f64(1), _f64(1)
            assert lib.so3_frob_loss_v2_f64(_p(p), _p(t), _p(g), _p(ls), _p(mean), _p(w), 0, n, st) == 0
            s = ls.item()
            runs.append(s)
            # the norms' own round-off (a few U each, relative) is inside the summation bound's slack
            assert abs(s - exact) <= _sum_depth(n, how, grid) * U * exact, (n, how, s, exact)
            assert mean.item() == s * (1.0 / n)
            if want_grad:
                got = g.cpu().numpy()
                err = np.abs(got.astype(np.longdouble) - dref).astype(np.float64)
                assert (err <= 1e-15 * np.abs(dref).astype(np.float64)).all(), (n, how, err.max())
                assert not got[z].any()
        if how != 0:
            assert runs[0] == runs[1] == runs[2]
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws).item()) == 0


def test_frob_loss_f64_of_no_rows_writes_zeros(lib):
    st = _st()
    ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for w in (ws, None):
        ls, mean = _f64(1), _f64(1)
        assert lib.so3_frob_loss_v2_f64(None, None, None, _p(ls), _p(mean), _p(w), 0, 0, st) == 0
        assert ls.item() == 0.0 and mean.item() == 0.0
        sc, fl = _f64(2), _flag()
        assert lib.so3_angle_error_v2_f64(None, None, None, _p(sc), _p(fl), _p(w), 0, 0, st) == 0
        assert sc.tolist() == [0.0, 0.0] and fl.item() == 0


@pytest.mark.parametrize("idx", range(7))
def test_geodesic_eps_f64_reductions_against_fsum(lib, haar_pairs, idx):
    """none, sum and mean.  This entry has no workspace: every workgroup adds its partial with one atomic, in whatever order the workgroups
    retire, so the sum's last bits differ from call to call -- its accuracy is asserted, not its bits."""
    n = _reduce_sizes()[idx]
    a, b = haar_pairs[0][:n], haar_pairs[1][:n]
    st = _st()
    eps = 1e-7
    c = _cos_np(a.cpu().numpy(), b.cpu().numpy())
    ref = np.arccos(np.clip(c, -1 + eps, 1 - eps).astype(np.longdouble)).astype(np.float64)
    theta = _f64(n)
    assert lib.so3_geodesic_eps_f64(_p(a), _p(b), _p(theta), None, None, 0, eps, n, st) == 0
    got = theta.cpu().numpy()
    assert _cond_err(got, ref).max() <= 4e-15
    exact = math.fsum(got.tolist())
    bound = _sum_depth(n, 0, _grid(n, 2048)) * U * exact
    for mean in (0, 1):
        acc, out, th2 = _f64(1), _f64(1), _f64(n)
        assert lib.so3_geodesic_eps_f64(_p(a), _p(b), _p(th2), _p(acc), _p(out), mean, eps, n, st) == 0
        s = acc.item()
        assert abs(s - exact) <= bound, (n, s, exact)
        assert out.item() == (s * (1.0 / n) if mean else s)
        assert torch.equal(th2, theta)
        acc = _f64(1)
        assert lib.so3_geodesic_eps_f64(_p(a), _p(b), None, _p(acc), None, mean, eps, n, st) == 0
        assert abs(acc.item() - exact) <= bound
    acc, out = _f64(1), _f64(1)
    assert lib.so3_geodesic_eps_f64(None, None, None, _p(acc), _p(out), 1, eps, 0, st) == 0
    assert acc.item() == 0.0 and math.isnan(out.item())                       # torch: the mean of nothing is NaN, the sum 0
    assert lib.so3_geodesic_eps_f64(None, None, None, _p(acc), _p(out), 0, eps, 0, st) == 0
    assert acc.item() == 0.0 and out.item() == 0.0


@pytest.mark.parametrize("eps,flags", [(0.0, 0), (0.0, RADIANS), (1e-7, RADIANS)])
def test_angle_bwd_f64_at_a_million_rows(lib, haar_pairs, eps, flags):
    from oracle import so3_oracle as so
    n = 1_000_003
    a, b = haar_pairs[0][:n].clone(), haar_pairs[1][:n].clone()
    b[7] = a[7]                                                                       # 0 degrees
    b[8] = (a[8].view(3, 3) @ torch.diag(torch.tensor([1.0, -1.0, -1.0], device=DEV, dtype=torch.float64))).reshape(9)   # 180
    gen = torch.Generator(device=DEV).manual_seed(3)
    w = torch.randn(n, device=DEV, generator=gen, dtype=torch.float64)
    one = torch.full((1,), 3.0, dtype=torch.float64, device=DEV)
    an, bn, wn = a.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy()
    unit = 1.0 if flags & RADIANS else DEG
    st = _st()
    for scalar in (False, True):
        div = float(n) if scalar else 1.0
        d1r, d2r, c = so.metric_backward_np(an, bn, 3.0 if scalar else wn, eps=eps, unit=unit, divisor=div)
        for want in ("d1", "d2", "both"):
            d1 = torch.full((n, 9), 7.0, dtype=torch.float64, device=DEV) if want != "d2" else None
            d2 = torch.full((n, 9), 7.0, dtype=torch.float64, device=DEV) if want != "d1" else None
            g = one if scalar else w
            assert lib.so3_angle_bwd_f64(_p(a), _p(b), _p(g), div, eps, flags | (GRAD_SCALAR if scalar else 0), _p(d1), _p(d2), n, st) == 0
            g1 = d1.cpu().numpy() if d1 is not None else d1r
            g2 = d2.cpu().numpy() if d2 is not None else d2r
            metric_grad_check(g1, g2, d1r, d2r, c, eps, 1e-15, 1e-14, (eps, flags, scalar, want))
            assert np.isfinite(g1).all() and np.isfinite(g2).all()


# ------------------------------------------------------------------------------------------------
# 4. the Python spellings on doubles at size
# ------------------------------------------------------------------------------------------------
def test_python_spellings_on_doubles_at_size(rr, haar_pairs):
    from oracle import so3_oracle as so
    n = 100_003
    gen = torch.Generator(device=DEV).manual_seed(4)
    wrow = torch.randn(n + 1, device=DEV, generator=gen, dtype=torch.float64)
    for lo in (0, 1):                                                         # 16-byte aligned, and a view one row (72 bytes) in
        base_a = haar_pairs[0][:n + 1].reshape(-1, 3, 3)
        base_b = haar_pairs[1][:n + 1].reshape(-1, 3, 3)
        a0, b0, w = base_a[lo:lo + n], base_b[lo:lo + n], wrow[lo:lo + n]
        an, bn, wn = a0.cpu().numpy(), b0.cpu().numpy(), w.cpu().numpy()
        c = _cos_np(an, bn)
        exact_rad = np.arccos(np.clip(c, -1, 1).astype(np.longdouble)).astype(np.float64)
        # angle_error: float64 degrees
        a, b = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
        deg = rr.angle_error(a, b)
        assert deg.dtype == torch.float64 and deg.shape == (n,)
        ref = so.angle_error_np(an, bn)
        assert _cond_err(deg.detach().cpu().numpy() / DEG, ref / DEG).max() <= 4e-15
        deg.backward(w)
        d1, d2, cc = so.metric_backward_np(an, bn, wn, unit=DEG)
        metric_grad_check(a.grad.cpu().numpy(), b.grad.cpu().numpy(), d1, d2, cc, 0.0, 1e-15, 1e-14, ("angle_error", lo))
        assert a.grad.dtype == torch.float64
        # compute_geodesic_distance_from_two_matrices: float64 radians, hard clamp
        a, b = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
        th = rr.compute_geodesic_distance_from_two_matrices(a, b)
        assert th.dtype == torch.float64 and th.shape == (n,)
        assert _cond_err(th.detach().cpu().numpy(), exact_rad).max() <= 4e-15
        th.backward(w)
        d1, d2, cc = so.metric_backward_np(an, bn, wn)
        metric_grad_check(a.grad.cpu().numpy(), b.grad.cpu().numpy(), d1, d2, cc, 0.0, 1e-15, 1e-14, ("cgd", lo))
        # geodesic(., ., r): the arguments' dtype, eps = 1e-7
        eps_rad = np.arccos(np.clip(c, -1 + 1e-7, 1 - 1e-7).astype(np.longdouble)).astype(np.float64)
        exact = math.fsum(eps_rad.tolist())
        for red in ("none", "sum", "mean"):
            a, b = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
            y = rr.geodesic(a, b, red)
            assert y.dtype == torch.float64
            if red == "none":
                assert y.shape == (n,) and _cond_err(y.detach().cpu().numpy(), eps_rad).max() <= 4e-15
                y.backward(w)
                up, div = wn, 1.0
            else:
                want = exact / n if red == "mean" else exact
                assert y.dim() == 0 and abs(y.item() - want) <= (_sum_depth(n, 0, _grid(n, 2048)) + 4) * U * want, (red, y.item(), want)
                y.backward()
                up, div = 1.0, float(n) if red == "mean" else 1.0
            d1, d2, cc = so.metric_backward_np(an, bn, up, eps=1e-7, divisor=div)
            metric_grad_check(a.grad.cpu().numpy(), b.grad.cpu().numpy(), d1, d2, cc, 1e-7, 1e-15, 1e-14, ("geodesic", red, lo))
        # loss_frobenius: mean_b ||R_true - R_pred||_F in float64
        p, t = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
        loss = rr.loss_frobenius(p, t)
        assert loss.dtype == torch.float64 and loss.dim() == 0
        d = (an - bn).reshape(n, 9)
        nrm = np.sqrt((d.astype(np.longdouble) ** 2).sum(1))
        want = math.fsum(nrm.astype(np.float64).tolist()) / n
        assert abs(loss.item() - want) <= 64 * U * want
        (2.0 * loss).backward()
        dref = (2.0 * d.astype(np.longdouble) / (n * nrm[:, None])).astype(np.float64)
        assert np.abs(p.grad.cpu().numpy().reshape(n, 9) - dref).max() <= 1e-15 * np.abs(dref).max()
        assert torch.equal(t.grad, -p.grad)
    # mixed float32 / float64: the reference casts both to double (angle_error) or lets torch promote the difference (loss_frobenius);
    # its bmm / matmul spellings of the other two metrics refuse mixed dtypes, so there is no promoted result to match there
    a64, b64 = haar_pairs[0][:n].reshape(-1, 3, 3), haar_pairs[1][:n].reshape(-1, 3, 3)
    a32 = a64.float()
    deg = rr.angle_error(a32, b64)
    assert deg.dtype == torch.float64
    ref = so.angle_error_np(a32.cpu().numpy(), b64.cpu().numpy())
    assert _cond_err(deg.cpu().numpy() / DEG, ref / DEG).max() <= 4e-15
    assert torch.equal(rr.angle_error(b64, a32), deg)
    p32 = a32.detach().requires_grad_(True)
    loss = rr.loss_frobenius(p32, b64)
    ref_loss = so.loss_frobenius_np(a32.cpu().numpy(), b64.cpu().numpy())
    assert loss.dtype == torch.float64 and abs(loss.item() - ref_loss) <= 64 * U * ref_loss
    loss.backward()
    assert p32.grad.dtype == torch.float32


def test_angle_error_raises_on_the_last_of_a_million_double_rows(rr, haar_pairs):
    n = 1_000_003
    a, b = haar_pairs[0][:n].reshape(-1, 3, 3), haar_pairs[1][:n].reshape(-1, 3, 3).clone()
    b[n - 1] = 3.0 * a[n - 1]
    with pytest.raises(ValueError, match="angle out of range, input probably not proper rotation matrices"):
        rr.angle_error(a, b)
    assert rr.angle_error(a, b, check=False).shape == (n,)
    b[n - 1] = haar_pairs[1][n - 1].reshape(3, 3)
    assert rr.angle_error(a, b).shape == (n,)                                  # and the next clean call does not


# ------------------------------------------------------------------------------------------------
# 5. a NaN partial must not stall the ticket finish
# ------------------------------------------------------------------------------------------------
def _timed(fn):
    """(result, milliseconds on the device between two events around the call)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return out, start.elapsed_time(stop)


def _nan_bits(k, pattern):
    return torch.tensor([pattern - (1 << 64) if pattern >= 1 << 63 else pattern] * k, dtype=torch.int64).view(torch.float64).to(DEV)


def test_nan_partials_do_not_stall_the_reduction(rr, lib, haar_pairs):
    """A float64 partial can be the NaN 0xFFFF...F -- a Rpred row of 0xFF bytes keeps that payload through -, fma, sqrt and +, and a Rtrue
    NaN 0x7FFF...F comes out of Rpred - Rtrue with its sign flipped -- and a slot stores its partial's bits plus one, 0 meaning "not here
    yet".  The loss must be NaN, the call quick (the summing workgroup polled such a slot for 0.1 s before it gave up), the workspace
    left zeroed, and the next clean call on it exact."""
    from poseestimation_amd import rotation_representation as rrm
    n = 4097
    p0, t0 = haar_pairs[0][:n].clone(), haar_pairs[1][:n].clone()
    st = _st()
    ws = rrm._workspace(torch.device(DEV), st)
    clean = math.fsum(np.sqrt(((p0 - t0).cpu().numpy().astype(np.longdouble) ** 2).sum(1)).astype(np.float64).tolist()) / n
    rr.loss_frobenius(p0, t0)                                                 # warm: module load and the workspace's zero-fill
    cases = []
    p = p0.clone()
    p[100] = _nan_bits(9, 0xFFFFFFFFFFFFFFFF)
    cases.append(("Rpred 0xFF..F", p, t0))
    t = t0.clone()
    t[n - 1] = _nan_bits(9, 0x7FFFFFFFFFFFFFFF)
    cases.append(("Rtrue 0x7F..F", p0, t))
    times = {}
    for name, pp, tt in cases:
        loss, ms = _timed(lambda: rr.loss_frobenius(pp.reshape(-1, 3, 3), tt.reshape(-1, 3, 3)))
        times[name] = ms
        assert math.isnan(loss.item()), name
        assert ms < 5.0, (name, ms)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(ws).item()) == 0, name
        again = rr.loss_frobenius(p0, t0).item()
        assert abs(again - clean) <= 64 * U * clean, (name, again, clean)
        # the same rows through the C ABI's sum of angles: k_angle_f64's ticket finish
        sc = _f64(2)
        assert lib.so3_angle_error_v2_f64(_p(p0), _p(t0), None, _p(sc), None, _p(ws), RADIANS, n, st) == 0     # warm
        _, ms = _timed(lambda: lib.so3_angle_error_v2_f64(_p(pp), _p(tt), None, _p(sc), None, _p(ws), RADIANS, n, st))
        assert math.isnan(sc[0].item()) and sc[1].item() == n and ms < 5.0, (name, ms)
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(ws).item()) == 0, name
    from conftest import REPORT_LINES
    REPORT_LINES.append("float64 NaN partials, loss_frobenius on 4097 rows: " + ", ".join("%s %.3f ms" % kv for kv in times.items()))
    # float32 data cannot make that pattern (widening leaves the low 29 bits zero): a guard on the float32 reductions
    m = 100_003
    x = torch.full((m, 9), -1, dtype=torch.int32, device=DEV).view(torch.float32)         # 0xFF bytes
    r32 = haar_pairs[1][:m].float().reshape(-1, 3, 3)
    for name, fn in (("frobenius_head", lambda v: rr.frobenius_head(v.reshape(-1, 9), r32, return_rotation=False)),
                     ("loss_frobenius", lambda v: rr.loss_frobenius(v.reshape(-1, 3, 3), r32)),
                     ("angle_error_sum_count", lambda v: rr.angle_error_sum_count(v.reshape(-1, 3, 3), r32)),
                     ("angle_error", lambda v: rr.angle_error(v.reshape(-1, 3, 3), r32))):
        fn(r32)                                                               # warm
        out, ms = _timed(lambda: fn(x))
        assert torch.isnan(out.reshape(-1)[0]).item() and ms < 5.0, (name, ms)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws).item()) == 0
