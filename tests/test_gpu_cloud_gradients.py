"""Gradients of the cloud entry points on the MI355X: kabsch_rotation through K5b (so3_kabsch_bwd_f32) and rotate_point_clouds
through a7b (so3_rotate_clouds_bwd_f32), against the reference's autograd (G16) and the float64 chain rule on the C oracle's K2."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, well_conditioned

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def rr():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib
    from poseestimation_amd import rotation_representation
    _lib.load()
    return rotation_representation


def cloud_rel_err(got, ref):
    """Per cloud: max |got - ref| over the cloud's entries / max |ref|."""
    b = ref.shape[0]
    got = np.asarray(got, np.float64).reshape(b, -1)
    ref = np.asarray(ref, np.float64).reshape(b, -1)
    return np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-30)


def svd_mask(h):
    h = np.asarray(h, np.float64)
    return well_conditioned(np.linalg.svd(h, compute_uv=False), np.linalg.det(h))


def kabsch_grads(rr, p, q, g_r, g_h, need_p=True, need_q=True):
    """(R, H, dP, dQ) of (R*gR).sum() [+ (H*gH).sum()] through kabsch_rotation on the device."""
    pd = p.detach().clone().requires_grad_(need_p)
    qd = q.detach().clone().requires_grad_(need_q)
    if g_h is None:
        r = rr.kabsch_rotation(pd, qd)
        h = None
        loss = (r * g_r).sum()
    else:
        r, h = rr.kabsch_rotation(pd, qd, return_h=True)
        loss = (r * g_r).sum() + (h * g_h).sum()
    wrt = [t for t, n in ((pd, need_p), (qd, need_q)) if n]
    grads = list(torch.autograd.grad(loss, wrt))
    dp = grads.pop(0) if need_p else None
    dq = grads.pop(0) if need_q else None
    return r, h, dp, dq


def kabsch_oracle(c_oracle, p, q, h, g_r, g_h):
    """dH = K2(H, gR) (C oracle, float64 inside) + gH, then dP = dH^T q and dQ = dH p in float64."""
    dh = c_oracle.project_bwd(h, g_r).astype(np.float64)
    if g_h is not None:
        dh = dh + np.asarray(g_h, np.float64)
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    return np.einsum("bac,bia->bic", dh, q), np.einsum("bac,bic->bia", dh, p)


def rotation_bound(p, g):
    """Per-entry bound for dR = sum_i g_i p_i^T summed by a wave: (N/64 + 8) * 6e-8 * sum_i |g_i| |p_i|."""
    n = p.shape[1]
    s = (np.linalg.norm(g, axis=2) * np.linalg.norm(p, axis=2)).sum(1)
    return (n / 64 + 8) * 6e-8 * s


def check_rotation(p, r, g_nat, dp, dr):
    """g_nat: the upstream in the (B,N,3) layout.  dP = R^T g exact to a few ulp of |g|, dR within rotation_bound."""
    p, r, g_nat = (np.asarray(a, np.float64) for a in (p, r, g_nat))
    if dp is not None:
        ref = np.einsum("bac,bia->bic", r.reshape(-1, 3, 3), g_nat)
        err = np.abs(np.asarray(dp, np.float64) - ref).max(2)
        assert (err <= 6e-7 * np.linalg.norm(g_nat, axis=2) + 1e-30).all(), err.max()
    if dr is not None:
        ref = np.einsum("bia,bic->bac", g_nat, p)
        err = np.abs(np.asarray(dr, np.float64).reshape(-1, 3, 3) - ref).reshape(len(ref), -1).max(1)
        assert (err <= rotation_bound(p, g_nat) + 1e-30).all(), (err / rotation_bound(p, g_nat)).max()


def random_pairs(rr, b, n, noise=0.01, seed=0):
    """Anisotropic clouds (distinct singular values) and q = R p + noise, on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = (torch.rand(b, n, 3, device=DEV, generator=gen) - 0.5) * torch.tensor([1.0, 0.6, 0.3], device=DEV)
    r = rr.get_sampled_rotation_matrices_by_axisAngle(b, DEV, generator=gen)
    q = rr.rotate_point_clouds(p, r) + noise * torch.randn(b, n, 3, device=DEV, generator=gen)
    return p, q, r


def ends(b, k=48):
    return np.arange(b) if b <= 2 * k else np.concatenate([np.arange(k), np.arange(b - k, b)])


# ---- 1. G16: the reference's autograd ----------------------------------------------------------------------------
def test_g16_kabsch_gradients_match_the_reference(rr):
    g = load_golden("g16_cloud_gradients.npz")
    p, q = torch.from_numpy(g["p"]).to(DEV), torch.from_numpy(g["q"]).to(DEV)
    g_r, g_h = torch.from_numpy(g["g_r"]).to(DEV), torch.from_numpy(g["g_h"]).to(DEV)
    ok = svd_mask(g["kabsch_f64_h"])
    assert ok.sum() >= 8
    for case, gh in (("r", None), ("rh", g_h)):
        _, _, dp, dq = kabsch_grads(rr, p, q, g_r, gh)
        for name, got in (("dp", dp), ("dq", dq)):
            ref = g["kabsch_%s_f64_%s" % (case, name)]
            err = cloud_rel_err(got.cpu().numpy(), ref)[ok]
            err32 = cloud_rel_err(g["kabsch_%s_f32_%s" % (case, name)], ref)[ok]
            assert np.median(err) < 1e-5 and err.max() < 1e-3, (case, name, np.median(err), err.max())
            assert np.median(err) <= 2 * np.median(err32) + 1e-6 and err.max() <= 2 * err32.max() + 1e-6, (case, name, err, err32)
            assert np.isfinite(got.cpu().numpy()).all()


@pytest.mark.parametrize("layout", ["out", "gg"])
def test_g16_rotation_gradients_match_the_reference(rr, layout):
    g = load_golden("g16_cloud_gradients.npz")
    pc = torch.from_numpy(g["pc1"]).to(DEV).requires_grad_(True)
    rot = torch.from_numpy(g["gt_rmat"]).to(DEV).requires_grad_(True)
    y = rr.rotate_point_clouds(pc, rot, transposed=layout == "gg")
    y.backward(torch.from_numpy(g["u_" + layout]).to(DEV))
    pc64, up = g["pc1"].astype(np.float64), g["u_" + layout].astype(np.float64)
    g_nat = up if layout == "out" else up.transpose(0, 2, 1)
    bound = rotation_bound(pc64, g_nat)
    assert (np.abs(pc.grad.cpu().numpy() - g["rot_%s_f64_dpc" % layout]).max(2) <= bound[:, None]).all()
    assert (np.abs(rot.grad.cpu().numpy() - g["rot_%s_f64_dr" % layout]).reshape(len(bound), -1).max(1) <= bound).all()
    check_rotation(pc64, g["gt_rmat"], g_nat, pc.grad.cpu().numpy(), rot.grad.cpu().numpy())


# ---- 2. ragged and at-size shapes against the C oracle ------------------------------------------------------------
SHAPES = [(1, 1), (3, 7), (5, 64), (17, 65), (70, 200), (300, 1024), (4100, 256), (65536, 64), (300000, 33), (65536, 1024)]


@pytest.mark.parametrize("b,n", SHAPES)
def test_kabsch_backward_shapes_against_the_oracle(rr, c_oracle, b, n):
    p, q, _ = random_pairs(rr, b, n, seed=b + n)
    g_r = torch.randn(b, 3, 3, device=DEV)
    g_h = torch.randn(b, 3, 3, device=DEV)
    _, h, dp, dq = kabsch_grads(rr, p, q, g_r, g_h)
    assert torch.isfinite(dp).all() and torch.isfinite(dq).all()
    idx = torch.from_numpy(ends(b)).to(DEV)
    hh = h[idx].detach().cpu().numpy()
    ref_dp, ref_dq = kabsch_oracle(c_oracle, p[idx].cpu().numpy(), q[idx].cpu().numpy(), hh, g_r[idx].cpu().numpy(), g_h[idx].cpu().numpy())
    ok = svd_mask(hh) & np.isfinite(ref_dp).reshape(len(idx), -1).all(1) & np.isfinite(ref_dq).reshape(len(idx), -1).all(1)
    if n >= 3:
        assert ok.mean() > 0.9, ok.mean()
    for got, ref in ((dp, ref_dp), (dq, ref_dq)):
        if ok.any():
            err = cloud_rel_err(got[idx].cpu().numpy(), ref)[ok]
            assert np.median(err) < 1e-5 and err.max() < 1e-3, (b, n, np.median(err), err.max())


@pytest.mark.parametrize("b,n", SHAPES)
def test_rotation_backward_shapes_against_the_chain_rule(rr, b, n):
    p, _, r = random_pairs(rr, b, n, seed=7 * b + n)
    idx = torch.from_numpy(ends(b)).to(DEV)
    for transposed in (False, True):
        pd, rd = p.clone().requires_grad_(True), r.clone().requires_grad_(True)
        y = rr.rotate_point_clouds(pd, rd, transposed=transposed)
        g = torch.randn_like(y)
        dp, dr = torch.autograd.grad(y, (pd, rd), g)
        g_nat = (g.transpose(1, 2) if transposed else g)[idx].cpu().numpy()
        check_rotation(p[idx].cpu().numpy(), r[idx].cpu().numpy(), g_nat, dp[idx].cpu().numpy(), dr[idx].cpu().numpy())


# ---- 3. one-sided gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", [(17, 65), (4100, 256)])
def test_one_sided_gradients_equal_the_two_sided_ones(rr, b, n):
    p, q, r = random_pairs(rr, b, n, seed=3)
    g_r, g_h = torch.randn(b, 3, 3, device=DEV), torch.randn(b, 3, 3, device=DEV)
    _, _, dp, dq = kabsch_grads(rr, p, q, g_r, g_h)
    _, _, dp1, none_q = kabsch_grads(rr, p, q, g_r, g_h, need_q=False)
    _, _, none_p, dq1 = kabsch_grads(rr, p, q, g_r, g_h, need_p=False)
    assert none_q is None and none_p is None
    assert torch.equal(dp, dp1) and torch.equal(dq, dq1)
    for transposed in (False, True):
        pd, rd = p.clone().requires_grad_(True), r.clone().requires_grad_(True)
        y = rr.rotate_point_clouds(pd, rd, transposed=transposed)
        g = torch.randn_like(y)
        dpc, drr = torch.autograd.grad(y, (pd, rd), g)
        pd1 = p.clone().requires_grad_(True)
        (dpc1,) = torch.autograd.grad(rr.rotate_point_clouds(pd1, r, transposed=transposed), (pd1,), g)
        rd1 = r.clone().requires_grad_(True)
        (drr1,) = torch.autograd.grad(rr.rotate_point_clouds(p, rd1, transposed=transposed), (rd1,), g)
        assert torch.equal(dpc, dpc1) and torch.equal(drr, drr1)


# ---- 4. the gH path ------------------------------------------------------------------------------------------------
def test_h_output_is_differentiable(rr, c_oracle):
    b, n = 200, 100
    p, q, _ = random_pairs(rr, b, n, seed=4)
    w = torch.randn(b, 3, 3, device=DEV)
    rt = rr.get_sampled_rotation_matrices_by_axisAngle(b, DEV)
    pd, qd = p.clone().requires_grad_(True), q.clone().requires_grad_(True)
    r, h = rr.kabsch_rotation(pd, qd, return_h=True)
    r.retain_grad()
    loss = rr.loss_frobenius(r, rt) + (h * w).sum()
    loss.backward()
    hh = h.detach().cpu().numpy()
    ref_dp, ref_dq = kabsch_oracle(c_oracle, p.cpu().numpy(), q.cpu().numpy(), hh, r.grad.cpu().numpy(), w.cpu().numpy())
    ok = svd_mask(hh)
    for got, ref in ((pd.grad, ref_dp), (qd.grad, ref_dq)):
        err = cloud_rel_err(got.cpu().numpy(), ref)[ok]
        assert np.median(err) < 1e-5 and err.max() < 1e-3, (np.median(err), err.max())
    # H alone: dQ = W p and dP = W^T q exactly as the chain rule has it
    pd2, qd2 = p.clone().requires_grad_(True), q.clone().requires_grad_(True)
    _, h2 = rr.kabsch_rotation(pd2, qd2, return_h=True)
    (h2 * w).sum().backward()
    ref_dp, ref_dq = kabsch_oracle(c_oracle, p.cpu().numpy(), q.cpu().numpy(), hh, np.zeros((b, 3, 3), np.float32), w.cpu().numpy())
    assert cloud_rel_err(pd2.grad.cpu().numpy(), ref_dp).max() < 1e-6
    assert cloud_rel_err(qd2.grad.cpu().numpy(), ref_dq).max() < 1e-6


# ---- 5. degenerate clouds ------------------------------------------------------------------------------------------
def test_degenerate_clouds(rr, c_oracle):
    b, n = 192, 96
    p, _, r = random_pairs(rr, b, n, seed=5)
    planar = p.clone()
    planar[..., 2] = 0.0
    q_planar = rr.rotate_point_clouds(planar, r)
    g_r = torch.randn(b, 3, 3, device=DEV)
    _, _, dp, dq = kabsch_grads(rr, planar, q_planar, g_r, None)
    hh = rr.kabsch_rotation(planar, q_planar, return_h=True)[1].cpu().numpy()        # the H the backward saw
    ref_dp, ref_dq = kabsch_oracle(c_oracle, planar.cpu().numpy(), q_planar.cpu().numpy(), hh, g_r.cpu().numpy(), None)
    for got, ref in ((dp, ref_dp), (dq, ref_dq)):
        err = cloud_rel_err(got.cpu().numpy(), ref)
        assert np.median(err) < 1e-5 and err.max() < 1e-3, (np.median(err), err.max())
    t = torch.rand(b, n, 1, device=DEV) - 0.5
    line = t * torch.nn.functional.normalize(torch.randn(b, 1, 3, device=DEV), dim=2)
    zero = torch.zeros(b, n, 3, device=DEV)
    for pp, qq in ((line, rr.rotate_point_clouds(line, r)), (zero, zero)):
        _, _, dp, dq = kabsch_grads(rr, pp, qq, g_r, torch.randn(b, 3, 3, device=DEV))
        assert torch.isfinite(dp).all() and torch.isfinite(dq).all()


# ---- 6. edge cases -------------------------------------------------------------------------------------------------
def test_empty_clouds_give_a_zero_rotation_gradient(rr):
    b = 70
    r = rr.get_sampled_rotation_matrices_by_axisAngle(b, DEV).requires_grad_(True)
    pc = torch.zeros(b, 0, 3, device=DEV, requires_grad=True)
    for transposed in (False, True):
        dpc, dr = torch.autograd.grad(rr.rotate_point_clouds(pc, r, transposed=transposed).sum(), (pc, r))
        assert dpc.shape == (b, 0, 3) and dr.shape == (b, 3, 3)
        assert torch.equal(dr, torch.zeros_like(dr))
    q = torch.zeros(b, 0, 3, device=DEV, requires_grad=True)
    rk = rr.kabsch_rotation(pc, q)
    dp, dq = torch.autograd.grad((rk * torch.randn_like(rk)).sum(), (pc, q))
    assert dp.shape == (b, 0, 3) and dq.shape == (b, 0, 3)


def test_float64_and_non_contiguous_arguments(rr, c_oracle):
    b, n = 33, 130
    p32, q32, r32 = random_pairs(rr, b, n, seed=6)
    p = p32.double().transpose(1, 2).contiguous().transpose(1, 2)          # (B,N,3) float64, not contiguous
    q = q32.double()
    assert not p.is_contiguous()
    pd, qd = p.clone().requires_grad_(True), q.clone().requires_grad_(True)          # (clone keeps the strides)
    assert not pd.is_contiguous()
    r = rr.kabsch_rotation(pd, qd)
    g_r = torch.randn(b, 3, 3, device=DEV)
    (r * g_r).sum().backward()
    assert pd.grad.dtype == torch.float64 and pd.grad.shape == pd.shape
    assert qd.grad.dtype == torch.float64 and qd.grad.shape == qd.shape
    _, _, dp32, dq32 = kabsch_grads(rr, p32, q32, g_r, None)
    assert torch.equal(pd.grad, dp32.double()) and torch.equal(qd.grad, dq32.double())
    rot = r32.double().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)     # non-contiguous (B,3,3) float64
    pcd = p.detach().clone().requires_grad_(True)
    y = rr.rotate_point_clouds(pcd, rot, transposed=True)
    g = torch.randn_like(y)
    y.backward(g)
    assert rot.grad.dtype == torch.float64 and rot.grad.shape == rot.shape
    assert pcd.grad.dtype == torch.float64 and pcd.grad.shape == pcd.shape
    check_rotation(p32.cpu().numpy(), r32.cpu().numpy(), g.transpose(1, 2).cpu().numpy(), pcd.grad.cpu().numpy(), rot.grad.cpu().numpy())


def test_forward_is_bit_identical_with_and_without_grad(rr):
    b, n = 500, 300
    p, q, r = random_pairs(rr, b, n, seed=8)
    r0, h0 = rr.kabsch_rotation(p, q, return_h=True)
    r1, h1 = rr.kabsch_rotation(p.clone().requires_grad_(True), q.clone().requires_grad_(True), return_h=True)
    r2 = rr.kabsch_rotation(p, q.clone().requires_grad_(True))
    assert torch.equal(r0, r1.detach()) and torch.equal(h0, h1.detach()) and torch.equal(r0, r2.detach())
    for transposed in (False, True):
        y0 = rr.rotate_point_clouds(p, r, transposed=transposed)
        y1 = rr.rotate_point_clouds(p.clone().requires_grad_(True), r.clone().requires_grad_(True), transposed=transposed)
        assert torch.equal(y0, y1.detach())


def test_backward_on_a_side_stream(rr):
    b, n = 1000, 200
    p, q, r = random_pairs(rr, b, n, seed=9)
    g_r, g_h = torch.randn(b, 3, 3, device=DEV), torch.randn(b, 3, 3, device=DEV)
    g = torch.randn(b, 3, n, device=DEV)
    _, _, dp0, dq0 = kabsch_grads(rr, p, q, g_r, g_h)
    pd, rd = p.clone().requires_grad_(True), r.clone().requires_grad_(True)
    dpc0, dr0 = torch.autograd.grad(rr.rotate_point_clouds(pd, rd, transposed=True), (pd, rd), g)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _, _, dp1, dq1 = kabsch_grads(rr, p, q, g_r, g_h)
        pd, rd = p.clone().requires_grad_(True), r.clone().requires_grad_(True)
        dpc1, dr1 = torch.autograd.grad(rr.rotate_point_clouds(pd, rd, transposed=True), (pd, rd), g)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(dp0, dp1) and torch.equal(dq0, dq1) and torch.equal(dpc0, dpc1) and torch.equal(dr0, dr1)


# ---- 7. end to end ------------------------------------------------------------------------------------------------
def test_kabsch_in_a_loss_matches_float64_autograd(rr):
    from oracle import so3_oracle as so
    b, n = 128, 150
    p, q, _ = random_pairs(rr, b, n, noise=0.05, seed=10)
    rt = rr.get_sampled_rotation_matrices_by_axisAngle(b, DEV)
    pd, qd = p.clone().requires_grad_(True), q.clone().requires_grad_(True)
    r = rr.kabsch_rotation(pd, qd)
    loss = rr.loss_frobenius(r, rt) + rr.geodesic(r, rt)
    loss.backward()
    p64 = p.cpu().double().requires_grad_(True)
    q64 = q.cpu().double().requires_grad_(True)
    rt64 = rt.cpu().double()
    r64 = so.kabsch_torch(p64, q64)
    cos = (torch.einsum("bij,bij->b", r64, rt64) - 1) / 2
    ref = so.loss_frobenius_torch(r64, rt64) + torch.acos(torch.clamp(cos, -1 + 1e-7, 1 - 1e-7)).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    ok = svd_mask(torch.bmm(q.transpose(1, 2), p).double().cpu().numpy())
    for got, want in ((pd.grad, p64.grad), (qd.grad, q64.grad)):
        err = cloud_rel_err(got.cpu().numpy(), want.numpy())[ok]
        assert np.median(err) < 1e-4 and err.max() < 1e-2, (np.median(err), err.max())


# ---- 8. the entry points that stay non-differentiable -------------------------------------------------------------
def test_non_differentiable_cloud_calls_warn_once(rr):
    b, n = 8, 32
    p = torch.rand(b, n, 3, device=DEV).requires_grad_(True)
    rg = rr.get_sampled_rotation_matrices_by_axisAngle(b, DEV)
    theta = torch.rand(b, device=DEV).requires_grad_(True)
    axis = torch.randn(b, 3, device=DEV)
    calls = {"kabsch_rotation_synthetic": lambda: rr.kabsch_rotation_synthetic(p, rg, 0.01, 1),
             "pc_normalize": lambda: rr.pc_normalize(p),
             "rotations_from_axis_angle_draws": lambda: rr.rotations_from_axis_angle_draws(theta, axis)}
    for key, call in calls.items():
        rr._WARNED.discard(key)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            call()
            call()
        hits = [w for w in seen if issubclass(w.category, RuntimeWarning) and key in str(w.message)]
        assert len(hits) == 1, (key, [str(w.message) for w in seen])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # the differentiable calls do not warn
        rr.kabsch_rotation(p, p.detach())
        rr.rotate_point_clouds(p, rg)
