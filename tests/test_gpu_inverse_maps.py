"""The inverse maps on the GPU (so3_mat_to_quat_*, so3_logmap_*, so3_mat_to_euler_*, so3_relative_log_* and their Python spellings
matrix_to_quaternion, so3_log_map, matrix_to_euler, matrix_to_ortho6d, relative_rotation_vector, inverse_head_functions): closure through
this package's own heads, values against G18's float64 answers, ranges, the geodesic identity, gradients against float64 autograd through
the definitions restated in tests/inverse_maps_ref.py (projected to the tangent space), on every way the rows are sent -- the remainder
kernel alone (B < 64), the streaming engine with and without a remainder, one round of the engine's grid +-1, three rounds + 5, 1 000 003.

TOLERANCES are those of tests/test_inverse_maps_host.py: 4 x the largest error of the float32 host-model instantiation of the very
operation on G18 (measured values and bounds are named constants at the top of that file), the same on the host and here."""
import numpy as np
import pytest
import torch

import inverse_maps_ref as ref
from test_gpu_float64_metrics import _p, _st
from test_inverse_maps_host import (COPY_CLOSURE_TOL, EULER_CLOSURE_TOL, EULER_GRAD_GIMBAL_BAND, EULER_GRAD_TOL, EULER_VALUE_TOL, LOG_CLOSURE_TOL,
                                    LOG_GRAD_TOL, LOG_VALUE_TOL, NORM_TOL, QUAT_CLOSURE_TOL, QUAT_GRAD_TOL, QUAT_VALUE_TOL, REL_GRAD_TOL, REL_VALUE_TOL)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_MAX = 1_000_003
SENTINEL = -777.0


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
    """Rows in one round of the engine's whole grid for the inverse maps: CUs x 4 SIMDs x 4 waves x 2 matrices per lane x 64 lanes
    (so3proj.hip: SO3_INV_NPL, SO3_INV_WPS; so3_relative_log_bwd_f32 runs 3 waves per SIMD, its round is three quarters of this)."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 2048


def _sizes():
    r = _round()
    return [1, 63, 64, 65, r - 1, r, r + 1, 3 * r + 5, N_MAX]


SIZE_IDS = ["1", "63", "64", "65", "round-1", "round", "round+1", "3round+5", "1000003"]


@pytest.fixture(scope="module")
def data(lib):
    """G18 tiled to the largest size, with its float64 answers alongside.  The stride 929 is coprime with the fixture's length, so every
    tiling is a permutation of it, and the first 63 .. 65 rows cross at least eight families with the gimbal band at the fixture's share
    (7.7 - 7.9 % of them are within 0.05 rad of gimbal lock; the fixture: 8.6 %)."""
    d = ref.g18()
    m = len(d["r"])
    n = max(_sizes())
    idx = (np.arange(n, dtype=np.int64) * 929) % m
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a[idx]), dtype=dt).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(18)
    return dict(g18=d, idx=idx, r=t(d["r"].reshape(m, 9), torch.float32), r2=t(d["r"][d["perm"]].reshape(m, 9), torch.float32),
                quat=d["quat"][idx], rotvec=d["rotvec"][idx], euler=d["euler"][idx], rel=d["rel_rotvec"][idx],
                g=torch.randn(n, 4, device=DEV, generator=gen))


def _out(b, w):
    """(b, w) output with one guard row behind it."""
    return torch.full((b + 1, w), SENTINEL, dtype=torch.float32, device=DEV)


def _call(lib, name, *args):
    code = getattr(lib, name)(*args)
    assert code == 0, (name, code, lib.so3_last_error())


def c_fwd(lib, sym, r, w):
    b = r.shape[0]
    out = _out(b, w)
    _call(lib, "so3_%s_fwd_f32" % sym, _p(r), _p(out), b, _st())
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all(), sym
    return out[:b]


def c_bwd(lib, sym, r, g):
    b = r.shape[0]
    out = _out(b, 9)
    _call(lib, "so3_%s_bwd_f32" % sym, _p(r), _p(g), _p(out), b, _st())
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all(), sym
    return out[:b]


def c_rel(lib, r1, r2, g=None, want1=True, want2=True):
    b = r1.shape[0]
    if g is None:
        out = _out(b, 3)
        _call(lib, "so3_relative_log_fwd_f32", _p(r1), _p(r2), _p(out), b, _st())
        torch.cuda.synchronize()
        assert (out[b] == SENTINEL).all()
        return out[:b]
    d1 = _out(b, 9) if want1 else None
    d2 = _out(b, 9) if want2 else None
    _call(lib, "so3_relative_log_bwd_f32", _p(r1), _p(r2), _p(g), _p(d1), _p(d2), b, _st())
    torch.cuda.synchronize()
    for d in (d1, d2):
        assert d is None or (d[b] == SENTINEL).all()
    return (d1[:b] if want1 else None), (d2[:b] if want2 else None)


def _closure(head, x, r):
    return (head(x).reshape(-1, 9).double() - r.reshape(-1, 9).double()).abs().max().item()


def _check(figures):
    for what, (got, tol) in figures.items():
        print("%-22s %.3e  (bound %.3e)" % (what, got, tol))
    for what, (got, tol) in figures.items():
        assert got <= tol, (what, got, tol)


def _exempt(quat, rotvec, euler, rel):
    return dict(quat=np.abs(quat[:, 0]) < 1e-3, rotvec=np.pi - np.linalg.norm(rotvec, axis=1) < 1e-3,
                euler=np.abs(np.abs(euler[:, 2]) - np.pi / 2) < 1e-2, rel=np.pi - np.linalg.norm(rel, axis=1) < 1e-3)


@pytest.mark.parametrize("which", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_forward_on_every_route(lib, pa, data, which):
    b = _sizes()[which]
    r, r2 = data["r"][:b].contiguous(), data["r2"][:b].contiguous()
    want = {k: data[k][:b] for k in ("quat", "rotvec", "euler", "rel")}
    ex = _exempt(want["quat"], want["rotvec"], want["euler"], want["rel"])
    q, v, e = c_fwd(lib, "mat_to_quat", r, 4), c_fwd(lib, "logmap", r, 3), c_fwd(lib, "mat_to_euler", r, 3)
    rel = c_rel(lib, r, r2)
    # the Python spellings run the same kernels: the same bits
    r33 = r.view(b, 3, 3)
    assert torch.equal(pa.matrix_to_quaternion(r33), q) and torch.equal(pa.so3_log_map(r33), v) and torch.equal(pa.matrix_to_euler(r33), e)
    assert torch.equal(pa.relative_rotation_vector(r33, r2.view(b, 3, 3)), rel)
    qn, vn, en, reln = (t.cpu().numpy() for t in (q, v, e, rel))
    _check({
        "quat value": (ref.up_to_sign_error(qn, want["quat"], ex["quat"]).max(), QUAT_VALUE_TOL),
        "log value": (ref.up_to_sign_error(vn, want["rotvec"], ex["rotvec"]).max(), LOG_VALUE_TOL),
        "euler value": (np.where(ex["euler"], 0.0, ref.angle_wrap_error(en, want["euler"])).max(), EULER_VALUE_TOL),
        "relative value": (ref.up_to_sign_error(reln, want["rel"], ex["rel"]).max(), REL_VALUE_TOL),
        "quat closure": (_closure(pa.compute_rotation_matrix_from_quaternion, q, r), QUAT_CLOSURE_TOL),
        "log closure": (_closure(pa.so3_exp_map, v, r), LOG_CLOSURE_TOL),
        "euler closure": (_closure(pa.compute_rotation_matrix_from_euler, e, r), EULER_CLOSURE_TOL),
    })
    # ranges
    assert (q[:, 0] >= 0).all()
    assert (q.double().norm(dim=1) - 1).abs().max().item() <= NORM_TOL
    assert v.double().norm(dim=1).max().item() <= ref.PI32 and rel.double().norm(dim=1).max().item() <= ref.PI32
    assert e[:, 2].double().abs().max().item() <= np.pi / 2 and e[:, :2].double().abs().max().item() <= ref.PI32
    # the geodesic identity: |log(R1^T R2)| against the package's metric in float64 on the same rows.  The metric is acos of the trace,
    # and the rows are float32-ROUNDED rotations: each entry is off by 2^-24 relative, the cosine (tr - 1) / 2 by u_c <= 2^-24 x 3
    # (sum |a_ij b_ij| <= 3), and acos turns that into u_c / sin(theta) -- at most sqrt(2 u_c) where sin(theta) is smaller than that.
    geo = pa.compute_geodesic_distance_from_two_matrices(r33.double(), r2.view(b, 3, 3).double())
    assert geo.dtype == torch.float64
    u_c = 3 * 2.0**-24
    slack = torch.minimum(2 * u_c / torch.sin(geo).abs().clamp_min(1e-30), torch.full_like(geo, 2 * np.sqrt(2 * u_c)))
    excess = ((rel.double().norm(dim=1) - geo).abs() - slack).max().item()
    print("geodesic identity      %.3e  beyond the metric's own conditioning (bound %.3e)" % (excess, REL_VALUE_TOL * np.sqrt(3)))
    assert excess <= REL_VALUE_TOL * np.sqrt(3)


@pytest.mark.parametrize("which", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_backward_on_every_route(lib, pa, data, which):
    b = _sizes()[which]
    r, r2, g4 = data["r"][:b].contiguous(), data["r2"][:b].contiguous(), data["g"][:b].contiguous()
    g3 = g4[:, :3].contiguous()
    keep = torch.as_tensor(np.abs(np.abs(data["euler"][:b, 2]) - np.pi / 2) > EULER_GRAD_GIMBAL_BAND).to(DEV)
    assert (~keep).double().mean().item() < 0.10                         # the rows left out of the Euler gradient check, at every size
    figures = {}
    for sym, fn, g, tol in (("mat_to_quat", ref.quat64, g4, QUAT_GRAD_TOL), ("logmap", ref.log64, g3, LOG_GRAD_TOL), ("mat_to_euler", ref.euler64, g3, EULER_GRAD_TOL)):
        got = c_bwd(lib, sym, r, g)
        assert torch.isfinite(got).all(), sym
        (want,) = ref.autograd_tangent_t(fn, g, r)
        err = (got.double() - want.reshape(b, 9)).abs().max(1)[0] / want.reshape(b, 9).abs().max(1)[0].clamp_min(1.0)
        if sym == "mat_to_euler":
            err = torch.where(keep, err, torch.zeros_like(err))
        figures[sym + " gradient"] = (err.max().item(), tol)
    d1, d2 = c_rel(lib, r, r2, g3)
    w1, w2 = ref.autograd_tangent_t(ref.rel64, g3, r, r2)
    for got, want, side in ((d1, w1, "dR1"), (d2, w2, "dR2")):
        err = (got.double() - want.reshape(b, 9)).abs().max(1)[0] / want.reshape(b, 9).abs().max(1)[0].clamp_min(1.0)
        figures["relative_log " + side] = (err.max().item(), REL_GRAD_TOL)
    _check(figures)
    # one gradient alone: the same numbers, except on the cut theta = pi (there log(D^T) = -log(D) fails)
    off_cut = torch.as_tensor(np.pi - np.linalg.norm(data["rel"][:b], axis=1) > 1e-3).to(DEV)
    o1, none2 = c_rel(lib, r, r2, g3, want2=False)
    none1, o2 = c_rel(lib, r, r2, g3, want1=False)
    assert none1 is None and none2 is None
    assert torch.equal(o2, d2) and torch.equal(o1[off_cut], d1[off_cut])


def test_closure_for_every_table_key_on_all_of_g18(pa, data):
    d = data["g18"]
    r = torch.as_tensor(d["r"]).to(DEV)
    heads = dict(pa.head_functions)
    heads["3D"] = pa.transform_output["3D"][1]
    tol = {"SVD": COPY_CLOSURE_TOL, "6D": COPY_CLOSURE_TOL, "Quat": QUAT_CLOSURE_TOL, "quat": QUAT_CLOSURE_TOL, "Euler": EULER_CLOSURE_TOL, "3D": LOG_CLOSURE_TOL}
    assert set(pa.inverse_head_functions) == set(tol) and "5D" not in pa.inverse_head_functions
    figures = {}
    for key, inverse in pa.inverse_head_functions.items():
        x = inverse(r)
        assert x.dtype == torch.float32 and x.shape == (len(r), {"SVD": 9, "6D": 6, "Quat": 4, "quat": 4, "Euler": 3, "3D": 3}[key])
        per_row = (heads[key](x).reshape(-1, 9).double() - r.reshape(-1, 9).double()).abs().max(1)[0].cpu().numpy()
        figures["closure " + key] = (per_row.max(), tol[key])
        for fam in ("gimbal_near", "gimbal_exact", "theta_near_pi", "theta_pi_random_axis", "theta_pi_coordinate_axis"):
            rows = d["family"] == list(d["family_names"]).index(fam)
            assert per_row[rows].max() <= tol[key], (key, fam, per_row[rows].max())
    _check(figures)
    ex = ref.exemptions(d)
    assert (ex["quat"] | ex["rotvec"] | ex["euler"]).mean() < 0.25


def test_gradients_through_autograd_with_fixture_and_random_g(pa, data):
    d = data["g18"]
    r = torch.as_tensor(d["r"]).to(DEV)
    keep = torch.as_tensor(np.abs(np.abs(d["euler"][:, 2]) - np.pi / 2) > EULER_GRAD_GIMBAL_BAND).to(DEV)
    assert (~keep).double().mean().item() < 0.10
    gen = torch.Generator(device=DEV).manual_seed(7)
    figures = {}
    for label, g4 in (("fixture g", torch.as_tensor(d["g"]).to(DEV)), ("random g", torch.randn(len(r), 4, device=DEV, generator=gen))):
        g3 = g4[:, :3].contiguous()
        for name, fn, f64, g, tol in (("quaternion", pa.matrix_to_quaternion, ref.quat64, g4, QUAT_GRAD_TOL), ("log map", pa.so3_log_map, ref.log64, g3, LOG_GRAD_TOL),
                                      ("euler", pa.matrix_to_euler, ref.euler64, g3, EULER_GRAD_TOL)):
            x = r.clone().requires_grad_(True)
            fn(x).backward(g)
            (want,) = ref.autograd_tangent_t(f64, g, r)
            err = (x.grad.double() - want).abs().reshape(len(r), 9).max(1)[0] / want.abs().reshape(len(r), 9).max(1)[0].clamp_min(1.0)
            if name == "euler":
                assert torch.isfinite(x.grad).all()
                err = torch.where(keep, err, torch.zeros_like(err))
            figures["%s, %s" % (name, label)] = (err.max().item(), tol)
    _check(figures)


def test_quaternion_loss_through_the_svd_head_matches_float64_chain(pa):
    """L = |matrix_to_quaternion(symmetric_orthogonalization(M)) - q_target|^2: dM against the float64 torch chain (SVD projection, the
    quaternion definition).  The tangent-space gradient chained through a head is exact, so the bound is the heads' own."""
    from oracle import so3_oracle as so
    gen = torch.Generator(device=DEV).manual_seed(3)
    m = torch.randn(4096, 9, device=DEV, generator=gen)
    qt = torch.randn(4096, 4, device=DEV, generator=gen)
    qt = qt / qt.norm(dim=1, keepdim=True)
    x = m.clone().requires_grad_(True)
    loss = ((pa.matrix_to_quaternion(pa.symmetric_orthogonalization(x)) - qt) ** 2).sum()
    loss.backward()
    x64 = m.double().cpu().clone().requires_grad_(True)
    q64 = ref.quat64(so.symmetric_orthogonalization_torch(x64))
    # the float32 forward may sit on the other side of w = 0 for a row next to it; compare where both agree on the sign
    loss64 = ((q64 - qt.double().cpu()) ** 2).sum()
    loss64.backward()
    m64 = m.double().cpu().numpy().reshape(-1, 3, 3)
    s = np.linalg.svd(m64, compute_uv=False)
    gap = (s[:, 1] + s[:, 2] * np.sign(np.linalg.det(m64))) / s[:, 0]          # the head's backward divides by (s2 + s3') / s1
    # rows next to w = 0 may sit on the other side of the sign flip in float32; rows without a gap have no well-defined gradient
    ok = torch.as_tensor((gap > 0.05) & (np.abs(q64.detach().numpy()[:, 0]) > 1e-3))
    assert ok.double().mean().item() > 0.9
    want, got = x64.grad.reshape(-1, 9)[ok], x.grad.cpu().double().reshape(-1, 9)[ok]
    # the chain adds nothing to the head's own backward error (the tangent-space gradient is exact behind a head): float32 round-off
    # 2^-24 over some 64 operations, divided by the relative gap
    bound = torch.as_tensor(64 * 2.0**-24 / gap)[ok]
    err = (got - want).abs().max(1)[0] / want.abs().max(1)[0].clamp_min(1.0)
    print("dM through head and quaternion: max error %.3e, max error / bound %.3f" % (err.max().item(), (err / bound).max().item()))
    assert abs(loss.item() - loss64.item()) <= 1e-5 * loss64.item()
    assert (err <= bound).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_dtypes_shapes_and_views(pa, data, dtype):
    r32 = data["r"][:300]
    base = pa.matrix_to_quaternion(r32.to(dtype).float().view(-1, 3, 3))
    for shape in ((300, 3, 3), (300, 9)):
        x = r32.to(dtype).view(shape).clone().requires_grad_(True)
        for fn, w in ((pa.matrix_to_quaternion, 4), (pa.so3_log_map, 3), (pa.matrix_to_euler, 3), (pa.matrix_to_ortho6d, 6)):
            y = fn(x)
            assert y.dtype == torch.float32 and y.shape == (300, w)
            (gx,) = torch.autograd.grad(y.sum(), x)
            assert gx.dtype == dtype and gx.shape == x.shape
        assert torch.equal(pa.matrix_to_quaternion(x), base)
        y = pa.relative_rotation_vector(x, x.detach().flip(0))
        (gx,) = torch.autograd.grad(y.sum(), x)
        assert gx.dtype == dtype and gx.shape == x.shape
    # a non-contiguous view: every second matrix, and a transposed batch
    wide = data["r"][:600].view(600, 3, 3)
    assert torch.equal(pa.so3_log_map(wide[::2]), pa.so3_log_map(wide[::2].contiguous()))
    t = wide[:300].transpose(1, 2)
    assert not t.is_contiguous() and torch.equal(pa.matrix_to_euler(t), pa.matrix_to_euler(t.contiguous()))
    six = pa.matrix_to_ortho6d(wide[:300])
    assert torch.equal(six, torch.cat((wide[:300, :, 0], wide[:300, :, 1]), 1))


def test_empty_batch_and_wrong_shapes(lib, pa):
    empty = torch.empty(0, 3, 3, device=DEV)
    for fn, w in ((pa.matrix_to_quaternion, 4), (pa.so3_log_map, 3), (pa.matrix_to_euler, 3), (pa.matrix_to_ortho6d, 6)):
        assert fn(empty).shape == (0, w)
    assert pa.relative_rotation_vector(empty, empty).shape == (0, 3)
    x = empty.clone().requires_grad_(True)
    pa.so3_log_map(x).sum().backward()
    assert x.grad.shape == (0, 3, 3)
    with pytest.raises(RuntimeError):
        pa.matrix_to_quaternion(torch.zeros(4, 3, device=DEV))
    with pytest.raises(RuntimeError):
        pa.relative_rotation_vector(torch.zeros(4, 3, 3, device=DEV), torch.zeros(5, 3, 3, device=DEV))


def test_side_stream(pa, data):
    r = data["r"][:70_001].view(-1, 3, 3)
    want = pa.so3_log_map(r)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = r.clone().requires_grad_(True)
        got = pa.so3_log_map(x)
        got.sum().backward()
    side.synchronize()
    assert torch.equal(got.detach(), want) and torch.isfinite(x.grad).all()


NAN_ROWS_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import poseestimation_amd as pa
DEV = "cuda:0"
d = np.load(sys.argv[2])
r = torch.as_tensor(np.resize(d["r"], (100_000, 3, 3))).to(DEV)
r[::7] = float("nan")
r[1::7] = 0.0
r[2::7] = -torch.eye(3, device=DEV)                              # not a rotation
g = torch.ones(len(r), 4, device=DEV)
outs = []
for fn, w in ((pa.matrix_to_quaternion, 4), (pa.so3_log_map, 3), (pa.matrix_to_euler, 3)):
    x = r.clone().requires_grad_(True)
    y = fn(x)
    y.backward(g[:, :w])
    outs += [y.detach(), x.grad]
x1, x2 = r.clone().requires_grad_(True), r.flip(0).clone().requires_grad_(True)
y = pa.relative_rotation_vector(x1, x2)
y.backward(g[:, :3])
torch.cuda.synchronize()
for y in outs[0::2]:
    assert torch.isnan(y[::7]).all()                             # a NaN row gives a NaN row, in every map
q = outs[0]
assert (q[1::7] - torch.tensor([1.0, 0, 0, 0], device=DEV)).abs().max().item() <= 4 * 2.0**-23      # the zero matrix: the identity's quaternion
clean = torch.ones(len(r), dtype=torch.bool, device=DEV)
clean[::7] = clean[1::7] = clean[2::7] = False
for o in outs:
    assert torch.isfinite(o[clean]).all()
    bad = o[~clean]
    assert (torch.isfinite(bad) | torch.isnan(bad) | torch.isinf(bad)).all()
print("nan rows ok")
"""


def test_nan_and_zero_rows_return_within_a_timeout(lib, tmp_path):
    """NaN rows, zero matrices and -I in every map, forward and backward, in a child process that is ended after 120 s: a hang fails the
    test instead of stopping the suite.  (The kernels have no loop; the guard is the point.)"""
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / "nan_rows.py"
    script.write_text(NAN_ROWS_SCRIPT)
    done = subprocess.run([sys.executable, str(script), ROOT, ref.GOLDEN], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "nan rows ok" in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])


def test_capture_and_replay_in_a_graph(pa, data):
    r = data["r"][:8256].clone().view(-1, 3, 3)
    r2 = data["r2"][:8256].clone().view(-1, 3, 3)
    g = data["g"][:8256, :3].contiguous()
    x1, x2 = r.clone().requires_grad_(True), r2.clone().requires_grad_(True)

    def step():
        v = pa.relative_rotation_vector(x1, x2)
        q = pa.matrix_to_quaternion(x1)
        d1, d2 = torch.autograd.grad([v, q], [x1, x2], [g, torch.ones_like(q)])
        return v.detach(), q.detach(), d1, d2

    want = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # new inputs in the captured buffers, replayed
    with torch.no_grad():
        x1.copy_(r2)
        x2.copy_(r)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], pa.relative_rotation_vector(r2, r))
