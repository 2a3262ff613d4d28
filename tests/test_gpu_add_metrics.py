"""compute_ADD_loss, compute_ADD_S_loss and cloud_diameter on the GPU: G19 through the Python surface and through the raw C ABI at the
bounds of tests/test_add_metrics_host.py (4 x the float32 host model's error; see its docstring), the exact cases, the plumbing, the
gradient through a training step, and the speed condition against the torch composition the feature replaces."""

import numpy as np
import pytest
import torch

import add_metrics_ref as ref
from support import dev  # noqa: F401
import test_add_metrics_host as host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g19_cases():
    return ref.cases(ref.g19())


def _poses(b, dev, err=None, seed=0):
    from oracle import so3_oracle as so
    g = torch.Generator().manual_seed(seed)
    def one(rot9):
        t = torch.eye(4).repeat(b, 1, 1)
        t[:, :3, :3] = torch.from_numpy(so.symmetric_orthogonalization_np(rot9.numpy()).astype(np.float32)).reshape(b, 3, 3)
        return t
    tg = one(torch.randn(b, 9, generator=g))
    tg[:, :3, 3] = torch.randn(b, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 2.0])
    if err is None:
        tp = one(torch.randn(b, 9, generator=g))
        tp[:, :3, 3] = tg[:, :3, 3] + 0.05 * torch.randn(b, 3, generator=g)
    else:
        tp = one(tg[:, :3, :3].reshape(b, 9) + err * torch.randn(b, 9, generator=g))
        tp[:, :3, 3] = tg[:, :3, 3] + err * torch.randn(b, 3, generator=g)
    return tg.to(dev), tp.to(dev)


def _cloud(b, n, dev, seed=1):
    p = torch.randn(b, n, 3, generator=torch.Generator().manual_seed(seed))
    if n > 1:                                          # (a single point stays where it is, on the unit sphere: centred it would be 0 / 0)
        p = p - p.mean(1, keepdim=True)
    return (p / p.norm(dim=-1).amax(1)[:, None, None]).to(dev)


def _pairwise64(x, y):
    """(b,n,n) float64 distances from coordinate differences, as the definition forms them (torch.cdist's own difference kernel
    cannot be launched at every shape used here, and its matrix-product mode is the expanded form)."""
    return torch.linalg.vector_norm(x[:, :, None, :] - y[:, None, :, :], dim=-1)


def surface_run(c, dev):
    """One G19 case through the Python surface, results named as host.host_run names them."""
    import poseestimation_amd as pa
    tg, pts = torch.from_numpy(c["tgt"]).to(dev), torch.from_numpy(c["pts"]).to(dev)
    tp = torch.from_numpy(c["tpred"]).to(dev).requires_grad_(True)
    add = pa.compute_ADD_loss(tg, tp, pts, use_batch_mean=False)
    (g_add,) = torch.autograd.grad(add.sum(), tp)
    adds, nearest = pa.compute_ADD_S_loss(tg, tp, pts, use_batch_mean=False, return_nearest=True)
    (g_adds,) = torch.autograd.grad(adds.sum(), tp)
    assert nearest.dtype == torch.int32 and nearest.shape == (c["b"], c["n"]) and not nearest.requires_grad
    # the per-point distances are the raw ABI's; the surface returns the metric and the indices
    return {"add": add.detach().cpu().numpy(), "adds": adds.detach().cpu().numpy(), "nearest": nearest.cpu().numpy(),
            "diam": pa.cloud_diameter(pts).cpu().numpy(), "grad_add": g_add.cpu().numpy(), "grad_adds": g_adds.cpu().numpy(),
            "point_dist": abi_run(c, dev)["point_dist"]}


def abi_run(c, dev):
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n = c["b"], c["n"]
    tg, tp, pts = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("tgt", "tpred", "pts"))
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    pd, nn, adds, add, diam, work, g_add, g_adds = f32(b, n), torch.full((b, n), -1, dtype=torch.int32, device=dev), f32(b), f32(b), f32(b), f32(b, n), f32(b, 4, 4), f32(b, 4, 4)
    total = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: t.data_ptr()
    _lib.check(lib.so3_add_s_fwd_f32(P(tg), P(tp), P(pts), P(pd), P(nn), P(adds), P(total), b, n, s), "so3_add_s_fwd_f32")
    _lib.check(lib.so3_add_s_bwd_f32(P(tg), P(tp), P(pts), P(nn), None, 1.0, P(g_adds), b, n, s), "so3_add_s_bwd_f32")
    _lib.check(lib.so3_add_l2_f32(P(tg), P(tp), P(pts), P(add), P(total) + 8, P(g_add), 1.0, b, n, s), "so3_add_l2_f32")
    _lib.check(lib.so3_cloud_diameter_f32(P(pts), P(work), P(diam), b, n, s), "so3_cloud_diameter_f32")
    torch.cuda.synchronize()
    tot = total.cpu().numpy()
    assert abs(tot[0] - adds.double().sum().item()) <= 1e-6 * max(1.0, b) and abs(tot[1] - add.double().sum().item()) <= 1e-6 * max(1.0, b)
    # without indices and without rows: the same distances; the total alone (one workgroup) agrees with the rows' sum
    pd2, tot2 = f32(b, n), torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.so3_add_s_fwd_f32(P(tg), P(tp), P(pts), P(pd2), None, None, P(tot2), b, n, s), "so3_add_s_fwd_f32")
    assert torch.equal(pd2, pd) and abs(tot2.item() - tot[0]) <= 1e-12 * max(1.0, b)
    return {"add": add.cpu().numpy(), "adds": adds.cpu().numpy(), "nearest": nn.cpu().numpy(), "diam": diam.cpu().numpy(),
            "grad_add": g_add.cpu().numpy(), "grad_adds": g_adds.cpu().numpy(), "point_dist": pd.cpu().numpy()}


# ---- against G19 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["surface", "abi"])
def test_g19_values_indices_and_gradients(dev, g19_cases, route):
    run = (lambda c: surface_run(c, dev)) if route == "surface" else (lambda c: abi_run(c, dev))
    host.check_against_g19(g19_cases, run, "gpu/" + route)


def test_g19_exact_cases(dev, g19_cases):
    for c in g19_cases:
        got = surface_run(c, dev)
        if c["family"] == "identical":
            assert (got["add"] == 0).all() and (got["adds"] == 0).all() and (got["point_dist"] == 0).all(), c["n"]
            assert (got["nearest"] == np.arange(c["n"])).all(), c["n"]
            assert (got["grad_add"] == 0).all() and (got["grad_adds"] == 0).all(), c["n"]
        if c["family"] == "twofold":
            assert (got["adds"] <= host.ADDS_TOL).all() and (got["add"] > 0.1).all(), c["n"]
        assert (got["grad_add"][:, 3] == 0).all() and (got["grad_adds"][:, 3] == 0).all()


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_shared_cloud_batch_mean_and_stream(dev):
    import poseestimation_amd as pa
    b, n = 7, 300
    tg, tp = _poses(b, dev)
    one = _cloud(1, n, dev)[0]
    full = one.unsqueeze(0).expand(b, -1, -1).contiguous()
    for fn in (pa.compute_ADD_loss, pa.compute_ADD_S_loss):
        rows = fn(tg, tp, full, use_batch_mean=False)
        assert rows.shape == (b,) and torch.equal(fn(tg, tp, one, use_batch_mean=False), rows)              # (N,3) broadcast = the expanded call
        mean = fn(tg, tp, full)
        assert mean.dim() == 0 and abs(mean.item() - rows.double().mean().item()) <= 2.0**-23 * max(1.0, abs(mean.item()))
    assert pa.cloud_diameter(one).dim() == 0 and torch.equal(pa.cloud_diameter(one), pa.cloud_diameter(full)[0])
    want = pa.compute_ADD_S_loss(tg, tp, full, use_batch_mean=False, return_nearest=True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = pa.compute_ADD_S_loss(tg, tp, full, use_batch_mean=False, return_nearest=True)
        diam = pa.cloud_diameter(full)
    side.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(diam, pa.cloud_diameter(full))


@pytest.mark.parametrize("b,n", [(3, 4096), (5000, 64), (4, 1), (64, 1024), (2, 1500)])
def test_shapes_against_float64_and_bitwise_repeatable(dev, b, n):
    """(3, 4096): a cloud split over workgroups and several LDS tiles; (5000, 64): many small clouds; N = 1; (2, 1500): a tail tile."""
    import poseestimation_amd as pa
    tg, tp = _poses(b, dev, seed=b)
    pts = _cloud(b, n, dev, seed=n)
    tpg = tp.clone().requires_grad_(True)
    adds, nn = pa.compute_ADD_S_loss(tg, tpg, pts, use_batch_mean=False, return_nearest=True)
    w = torch.randn(b, generator=torch.Generator().manual_seed(3)).to(dev)
    (grad,) = torch.autograd.grad((adds * w).sum(), tpg)
    add = pa.compute_ADD_loss(tg, tp, pts, use_batch_mean=False)
    diam = pa.cloud_diameter(pts)
    again = pa.compute_ADD_S_loss(tg, tp, pts, use_batch_mean=False, return_nearest=True)
    assert torch.equal(again[0], adds.detach()) and torch.equal(again[1], nn) and torch.equal(pa.cloud_diameter(pts), diam)      # bitwise
    assert torch.equal(pa.compute_ADD_S_loss(tg, tp, pts), pa.compute_ADD_S_loss(tg, tp, pts))
    assert int(nn.min()) >= 0 and int(nn.max()) < n
    # float64 on the device, in slices of the batch (the (B,N,N) table of the definition is what the feature avoids)
    T = lambda t: t.double()
    step = max(1, (1 << 24) // (n * n))
    for lo in range(0, b, step):
        sl = slice(lo, min(b, lo + step))
        x, y = ref.pose64(T(tg[sl]), T(pts[sl])), ref.pose64(T(tp[sl]), T(pts[sl]))
        d = _pairwise64(x, y)
        pd = d.min(-1).values
        sel = torch.gather(d, 2, nn[sl].long()[:, :, None])[:, :, 0]
        assert float((sel - pd).max()) <= host.POINT_TOL                                        # the index check, every point
        assert float((adds.detach()[sl].double() - pd.mean(-1)).abs().max()) <= host.ADDS_TOL
        assert float((add[sl].double() - (x - y).norm(dim=-1).mean(-1)).abs().max()) <= host.ADD_TOL
        assert float((diam[sl].double() - _pairwise64(T(pts[sl]), T(pts[sl])).flatten(1).amax(1)).abs().max()) <= host.DIAM_TOL
        tp64 = T(tp[sl]).clone().requires_grad_(True)
        ysel = torch.gather(ref.pose64(tp64, T(pts[sl])), 1, nn[sl].long()[:, :, None].expand(-1, -1, 3))
        ((torch.linalg.vector_norm(x - ysel, dim=-1).mean(-1) * T(w[sl])).sum()).backward()
        assert float((grad[sl].double() - tp64.grad).abs().max()) <= host.ADDS_GRAD_TOL * float(w[sl].abs().max().clamp(min=1.0))
    if n == 1:
        # one point: ADD-S is ADD.  Not bit for bit -- ADD forms (R_gt - R_pred) p + (t_gt - t_pred), ADD-S the difference of the two
        # posed points -- but both are within their bounds of the same float64 number
        assert float((adds.detach() - add).abs().max()) <= host.ADD_TOL + host.ADDS_TOL and (diam == 0).all() and (nn == 0).all()


# ---- gradient through a training step ------------------------------------------------------------------------------------
def test_backward_through_the_se3_update(dev):
    import poseestimation_amd as pa
    b, n = 16, 500
    tg, t_init = _poses(b, dev, err=0.05, seed=5)
    pts = _cloud(b, n, dev, seed=6)
    out = (0.05 * torch.randn(b, 12, generator=torch.Generator().manual_seed(7))).to(dev)
    out[:, [0, 4, 8]] += 1.0
    out.requires_grad_(True)
    for fn in (pa.compute_ADD_S_loss, pa.compute_ADD_loss):
        out.grad = None
        tpred = pa.calculate_T_pred(out, t_init)
        tpred.retain_grad()
        loss = fn(tg, tpred, pts)
        loss.backward()
        assert out.grad is not None and torch.isfinite(out.grad).all() and float(out.grad.abs().max()) > 0
        # the pose gradient that entered the update's backward is the restated one (float64, through the returned indices)
        T = lambda t: t.detach().double().cpu()
        if fn is pa.compute_ADD_S_loss:
            _, nn = pa.compute_ADD_S_loss(tg, tpred.detach(), pts, return_nearest=True)
            want, tol = ref.grad_adds64(T(tg), T(tpred), T(pts), nn.cpu().numpy()) / b, host.ADDS_GRAD_TOL
        else:
            want, tol = ref.grad_add64(T(tg), T(tpred), T(pts)) / b, host.ADD_GRAD_TOL
        assert float((tpred.grad.double().cpu() - want).abs().max()) <= tol
    with pytest.raises(RuntimeError):                                                            # once_differentiable: no double backward
        tp = tpred.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(pa.compute_ADD_S_loss(tg, tp, pts), tp, create_graph=True)
        g.sum().backward()


def test_constants_warn_once(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    tg, tp = _poses(2, dev)
    pts = _cloud(2, 10, dev).requires_grad_(True)
    rr._WARNED.discard("compute_ADD_S_loss_constants")
    with pytest.warns(RuntimeWarning, match="TCO_pred only"):
        pa.compute_ADD_S_loss(tg, tp, pts)
    rr._WARNED.discard("cloud_diameter")
    with pytest.warns(RuntimeWarning, match="no gradient"):
        assert not pa.cloud_diameter(pts).requires_grad


# ---- speed, as a condition --------------------------------------------------------------------------------------------------
def test_add_s_is_not_slower_than_the_torch_composition(dev):
    """B = 256, N = 1024, HIP events, 5 warm-ups, median of 20: compute_ADD_S_loss(use_batch_mean=False) under no_grad against
    torch.cdist(x, y).min(-1).values.mean(-1) on pre-posed clouds, in the same process on the same device."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n = 256, 1024
    tg, tp = _poses(b, dev, seed=11)
    pts = _cloud(b, n, dev, seed=12)
    x = (pts @ tg[:, :3, :3].transpose(1, 2) + tg[:, None, :3, 3]).contiguous()
    y = (pts @ tp[:, :3, :3].transpose(1, 2) + tp[:, None, :3, 3]).contiguous()

    def median_ms(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    with torch.no_grad():
        ours = median_ms(lambda: pa.compute_ADD_S_loss(tg, tp, pts, use_batch_mean=False))
        theirs = median_ms(lambda: torch.cdist(x, y).min(-1).values.mean(-1))
        got, want = pa.compute_ADD_S_loss(tg, tp, pts, use_batch_mean=False), torch.cdist(x.double(), y.double()).min(-1).values.mean(-1)
    line = "ADD-S B=256 N=1024: compute_ADD_S_loss %.4f ms, torch.cdist().min().mean() %.4f ms (x%.1f); %.3g pairs/s" % (
        ours, theirs, theirs / ours, b * n * n / (ours * 1e-3))
    print(line)
    REPORT_LINES.append(line)
    assert float((got.double() - want).abs().max()) <= host.ADDS_TOL
    assert ours <= theirs, line
