#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE in the build container.

Run once, here, with /root/reference mounted:   python tools/gen_golden.py
The reference never travels: only the inputs and the outputs it produced are committed
(SURVEY.md section 8c).  Nothing under tests/, bench.py or the package imports this script.

How the reference code is executed
  * rotation_representation.py imports cleanly (torch, numpy only) -> imported as a module.
  * loss_frobenius (3D-Pose/loss.py:7-11) and the rotation sampler
    (point_cloud/prepare.py:12-49) live in files whose *module-level imports* need packages that
    are not installed (spatialmath, trimesh).  Their function bodies need only torch/numpy, so the
    function definitions are compiled straight from the reference files with `ast` and executed --
    the reference's own code runs, nothing is retyped.
  * Two reference functions hard-code `.cuda()` (rotation_representation.py:218-219,
    point_cloud/prepare.py:23,25).  There is no GPU here, so `Tensor.cuda` is made the identity
    for the duration of this script; arithmetic is unchanged.
"""
import ast
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self          # CPU container: see docstring
torch.set_num_threads(1)                                # deterministic LAPACK path

sys.path.insert(0, REF)
import rotation_representation as rr  # noqa: E402


def functions_from(path, names):
    """Compile the named top-level functions of a reference file without importing the file."""
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in keep} == set(names), (path, names)
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


(loss_frobenius,) = functions_from(os.path.join(REF, "3D-Pose", "loss.py"), ["loss_frobenius"])
normalize_vector, sample_rot = functions_from(
    os.path.join(REF, "point_cloud", "prepare.py"),
    ["normalize_vector", "get_sampled_rotation_matrices_by_axisAngle"])


def svd_parts(x):
    """s and det(u v^T) exactly as the reference computes them (rotation_representation.py:200-202)."""
    m = x.view(-1, 3, 3)
    u, s, v = torch.svd(m)
    det = torch.det(torch.matmul(u, torch.transpose(v, 1, 2)))
    return s, det


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()})
    print("%-28s %7.1f KB" % (name, os.path.getsize(path) / 1024))


def g7_ortho6d():
    """Next row f2: the 6D Gram-Schmidt head (rotation_representation.py:21-36), forward + autograd backward."""
    torch.manual_seed(6)
    p = torch.randn(300, 6, requires_grad=True)
    g = torch.randn(300, 3, 3)
    r = rr.compute_rotation_matrix_from_ortho6d(p)
    r.backward(g)
    pd = p.detach().double().requires_grad_(True)
    rd = rr.compute_rotation_matrix_from_ortho6d(pd)
    rd.backward(g.double())
    shaped = torch.randn(2, 5, 6)
    save("g7_ortho6d.npz", p=p.detach(), r=r.detach(), g=g, dp=p.grad, r_f64=rd.detach(), dp_f64=pd.grad,
         p_shaped=shaped, r_shaped=rr.compute_rotation_matrix_from_ortho6d(shaped))


def g8_se3_update():
    """Next row f1: calculate_T_pred (Iterative/utility.py:90-128) forward + autograd backward.

    The reference's helper `combine` (utility.py:63-71) reads two names that are not in its scope
    (`model_output`, `R_new`) and raises NameError as committed; the function compiled from the reference file is
    therefore run with a `combine` that does what that helper plainly intends (ones(B,4,4); [:3,:3]=R; column 3 =
    (tx,ty,tz); [3,:3]=0).  Everything else -- head, focal lengths, translation update, einsum -- is the
    reference's own code."""
    def combine(R, tx, ty, tz, device="cpu"):
        T = torch.ones((R.shape[0], 4, 4))
        T[:, :3, :3] = R
        T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = tx, ty, tz
        T[:, 3, :3] = 0
        return T
    calc, scene = functions_from(os.path.join(REF, "Iterative", "utility.py"), ["calculate_T_pred", "get_scene_parameters"])
    calc.__globals__.update(symmetric_orthogonalization=rr.symmetric_orthogonalization, combine=combine, get_scene_parameters=scene)
    torch.manual_seed(8)
    b = 200
    out = torch.randn(b, 12)
    out[:, 9:11] *= 20.0                                   # pixel-scale offsets
    out[:, 11] = 1.0 + 0.1 * torch.randn(b)                 # depth ratio near 1
    t_init = torch.zeros(b, 4, 4)
    t_init[:, :3, :3] = rr.symmetric_orthogonalization(torch.randn(b, 9))
    t_init[:, :3, 3] = torch.tensor([0.0, 0.0, 2.5]) + 0.3 * torch.randn(b, 3)
    t_init[:, 3, 3] = 1.0
    g = torch.randn(b, 4, 4)
    o = out.clone().requires_grad_(True)
    tp = calc(o, t_init, "cpu")
    tp.backward(g)
    # (no float64 run: the reference casts R_k with .float(), utility.py:123, so a double input raises)
    save("g8_se3_update.npz", out=out, t_init=t_init, g=g, t_pred=tp.detach(), dout=o.grad, fx=scene()[0], fy=scene()[1])


def g9_sampler():
    """Next row f4: the rotation sampler (point_cloud/prepare.py:21-49) with its random draws recorded.
    The sampler takes theta from numpy's global RNG and the axis from torch's; both are re-seeded so the draws
    can be replayed and stored next to the matrices the reference made from them."""
    b = 500
    np.random.seed(11)
    theta = np.random.uniform(-1, 1, b) * np.pi                      # what prepare.py:23 will draw
    torch.manual_seed(11)
    axis = torch.randn(b, 3)                                         # what prepare.py:25 will draw
    np.random.seed(11)
    torch.manual_seed(11)
    r = sample_rot(b)
    save("g9_sampler.npz", theta=theta.astype(np.float32), axis=axis, r=r)


def g11_add_l1():
    """Next row f6: compute_ADD_L1_loss / compute_disentangled_ADD_L1_loss (Iterative/loss.py:10-70) and their
    autograd w.r.t. the predicted pose, float32 as the training loop runs them and float64."""
    add_l1, add_l1_dis, _ = functions_from(os.path.join(REF, "Iterative", "loss.py"),
                                           ["compute_ADD_L1_loss", "compute_disentangled_ADD_L1_loss", "transform_pts"])
    add_l1.__globals__["transform_pts"] = _
    torch.manual_seed(21)
    b, n = 24, 200                                                        # N not a multiple of 64: ragged tail
    def poses(noise):
        t = torch.eye(4).repeat(b, 1, 1)
        t[:, :3, :3] = rr.symmetric_orthogonalization(torch.randn(b, 9))
        t[:, :3, 3] = torch.randn(b, 3) * 0.3 + torch.tensor([0.0, 0.0, 2.0])
        return t
    t_gt = poses(0)
    t_pred = t_gt.clone()
    t_pred[:, :3, :3] = torch.matmul(rr.symmetric_orthogonalization(torch.eye(3).reshape(1, 9) + 0.2 * torch.randn(b, 9)), t_gt[:, :3, :3])
    t_pred[:, :3, 3] += 0.1 * torch.randn(b, 3)
    t_pred[0] = t_gt[0]                                                   # an exact hit: every |.| sits at its kink
    t_pred[1, :3, 3] = t_gt[1, :3, 3]                                     # rotation error only
    t_pred[2, :3, :3] = t_gt[2, :3, :3]                                   # translation error only
    pts = torch.randn(b, n, 3) * 0.2
    out = {"t_gt": t_gt, "t_pred": t_pred, "points": pts}
    for tag, dt in (("", torch.float32), ("_f64", torch.float64)):
        tg, p = t_gt.to(dt), pts.to(dt)
        tp = t_pred.to(dt).clone().requires_grad_(True)
        loss = add_l1(tg, tp, p)
        loss.backward()
        out.update({"add" + tag: loss.detach(), "add_grad" + tag: tp.grad, "add_dists" + tag: add_l1(tg, tp.detach(), p, use_batch_mean=False)})
        tp = t_pred.to(dt).clone().requires_grad_(True)
        loss = add_l1_dis(tp, tg, p)
        loss.backward()
        out.update({"dis" + tag: loss.detach(), "dis_grad" + tag: tp.grad})
    save("g11_add_l1.npz", **out)


def g12_clouds():
    """Row a7: pc_normalize (point_cloud/prepare.py:51-56, the reference function, numpy float64) and the training
    loop's pairing rule (point_cloud/main.py:173-183), whose four statements are replayed here verbatim on CPU."""
    (pc_normalize,) = functions_from(os.path.join(REF, "point_cloud", "prepare.py"), ["pc_normalize"])
    rng = np.random.RandomState(12)
    clouds = (rng.rand(6, 200, 3) - 0.5) * np.array([1.0, 2.0, 0.5]) + np.array([0.3, -1.0, 2.0])
    norm, cent, scale = zip(*(pc_normalize(c) for c in clouds))
    torch.manual_seed(12)
    np.random.seed(12)
    batch, point_num = 6, 200
    pc1 = torch.tensor(np.stack(norm)).float()
    gt_rmat = sample_rot(batch)
    gt_rmats = gt_rmat.contiguous().view(batch, 1, 3, 3).expand(batch, point_num, 3, 3).contiguous().view(-1, 3, 3)   # :176-177
    pc2 = torch.bmm(gt_rmats, pc1.view(-1, 3, 1))                                                                      # :180
    pc_out = pc2.view(batch, point_num, 3)                                                                             # :181
    gg = pc_out.transpose(1, 2)                                                                                        # :183
    save("g12_clouds.npz", clouds=clouds, norm=np.stack(norm), centroid=np.stack(cent), scale=np.array(scale),
         pc1=pc1, gt_rmat=gt_rmat, pc_out=pc_out, gg=gg.contiguous())


def g10_heads():
    """Next row f5: the quaternion / Euler / 5D / exp-map heads (rotation_representation.py:39-171, 245-321) and
    their autograd, float32 as the reference runs them; float64 too where the reference's code keeps float64."""
    heads = {"quat": (4, rr.compute_rotation_matrix_from_quaternion), "euler": (3, rr.compute_rotation_matrix_from_euler),
             "ortho5d": (5, rr.compute_rotation_matrix_from_ortho5d), "expmap": (3, rr.vec_3d_to_SO3)}
    out = {}
    for seed, (name, (n, fn)) in enumerate(sorted(heads.items())):
        torch.manual_seed(100 + seed)
        b = 192
        x = torch.randn(b, n)
        x[:32] *= 4.0                                       # large angles / magnitudes
        x[32:64] *= 0.05                                    # small ones
        if name == "expmap":
            x[64:80] *= 0.004                               # |v|^2 < 1e-4: the clamped branch
            x[80:96] = x[80:96] / x[80:96].norm(dim=1, keepdim=True) * torch.linspace(0.9, 1.1, 16).view(-1, 1)   # around theta = 1
        g = torch.randn(b, 3, 3)
        xf = x.clone().requires_grad_(True)
        r = fn(xf)
        r.backward(g)
        out.update({name + "_x": x, name + "_r": r.detach(), name + "_g": g, name + "_dx": xf.grad})
        if name != "ortho5d":                               # its float64 run goes through float32 zeros (:82)
            xd = x.double().requires_grad_(True)
            rd = fn(xd)
            rd.backward(g.double())
            assert rd.dtype == torch.float64
            out.update({name + "_r_f64": rd.detach(), name + "_dx_f64": xd.grad})
    save("g10_heads.npz", **out)


def g13_dtype_fidelity():
    """Output dtypes and float64 values of the loss and the two metrics (3D-Pose/loss.py:7-11,
    rotation_representation.py:209-242) for float32 and float64 arguments."""
    torch.manual_seed(13)
    r1 = rr.symmetric_orthogonalization(torch.randn(300, 9).double())
    r2 = rr.symmetric_orthogonalization(torch.randn(300, 9).double())
    out = {"r1": r1, "r2": r2}
    for tag, cast in (("f32", torch.float32), ("f64", torch.float64)):
        a, b = r1.to(cast), r2.to(cast)
        ar = a.clone().requires_grad_(True)
        loss = loss_frobenius(ar, b)
        loss.backward()
        geo = rr.compute_geodesic_distance_from_two_matrices(a, b)
        ang = rr.angle_error(a, b)
        out.update({"loss_" + tag: loss.detach(), "dloss_" + tag: ar.grad, "geo_" + tag: geo, "ang_" + tag: ang,
                    "dtypes_" + tag: np.array([str(loss.dtype), str(ar.grad.dtype), str(geo.dtype), str(ang.dtype)])})
    save("g13_dtype_fidelity.npz", **out)


def g14_geodesic_reduction():
    """geodesic(R1, R2, reduction) of point_cloud/main.py:61-73 (the eps-clamped geodesic with "none" / "mean" / "sum"), run from
    the reference file on G3's pairs (0 and 180 degrees included: the clamp is what differs from the other geodesic) and on 2000
    Haar-like pairs."""
    (geodesic,) = functions_from(os.path.join(REF, "point_cloud", "main.py"), ["geodesic"])
    g3 = np.load(os.path.join(OUT, "g3_angles.npz"))
    r1, r2 = torch.from_numpy(g3["r1"]), torch.from_numpy(g3["r2"])
    torch.manual_seed(14)
    a = rr.symmetric_orthogonalization(torch.randn(2000, 9))
    b = rr.symmetric_orthogonalization(torch.randn(2000, 9))
    out = {"a": a, "b": b}
    for tag, (p, q) in (("g3", (r1, r2)), ("haar", (a, b))):
        out.update({tag + "_none": geodesic(p, q, "none"), tag + "_mean": geodesic(p, q, "mean"), tag + "_sum": geodesic(p, q, "sum")})
    assert geodesic(a, b, "median") is None                 # any other string falls through the if-chain
    out["dtypes"] = np.array([str(out["haar_none"].dtype), str(out["haar_mean"].dtype), str(out["haar_sum"].dtype)])
    save("g14_geodesic_reduction.npz", **out)


def g15_metric_gradients():
    """Autograd through the three metric spellings, as the reference's training loops can use them (`lossfunc` hooks:
    point_cloud/main.py:194-197, UPNA/main.py:56-59): geodesic(R1, R2, reduction) (point_cloud/main.py:61-73, whose eps exists for
    this gradient), compute_geodesic_distance_from_two_matrices and angle_error (rotation_representation.py:209-242).  Pairs: G3's
    (their first 64: 0 and 180 degrees, 1e-4 and 3e-3 rad included; outside the clamp the reference's masked fill gives exactly 0) and the first 128 of G14's Haar-like pairs; float32 and float64; gradients with respect to BOTH arguments; a per-row
    upstream gradient for the unreduced forms."""
    (geodesic,) = functions_from(os.path.join(REF, "point_cloud", "main.py"), ["geodesic"])
    g3 = np.load(os.path.join(OUT, "g3_angles.npz"))
    g14 = np.load(os.path.join(OUT, "g14_geodesic_reduction.npz"))
    sets = {"g3": (torch.from_numpy(g3["r1"][:64]), torch.from_numpy(g3["r2"][:64])),       # rows 0-4: 0, 180, 179.96, 0.044, 0.155 degrees
            "haar": (torch.from_numpy(g14["a"][:128]), torch.from_numpy(g14["b"][:128]))}
    out = {}
    for tag, (p, q) in sets.items():
        torch.manual_seed(15)
        w = torch.randn(p.shape[0])                        # upstream gradient of the per-row forms
        out[tag + "_r1"], out[tag + "_r2"], out[tag + "_w"] = p, q, w
        for dt_tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            def run(fn, upstream):
                a = p.to(dt).clone().requires_grad_(True)
                b = q.to(dt).clone().requires_grad_(True)
                y = fn(a, b)
                if upstream is None:
                    y.backward()
                else:
                    y.backward(upstream.to(y.dtype))
                return y.detach(), a.grad, b.grad
            cases = {
                "geo_mean": (lambda a, b: geodesic(a, b, "mean"), None),
                "geo_sum": (lambda a, b: geodesic(a, b, "sum"), None),
                "geo_none": (lambda a, b: geodesic(a, b, "none"), w),
                "cgd": (rr.compute_geodesic_distance_from_two_matrices, w),
                "ang": (rr.angle_error, w),
                "ang_mean": (lambda a, b: rr.angle_error(a, b).mean(), None),
            }
            for name, (fn, up) in cases.items():
                y, da, db = run(fn, up)
                key = "%s_%s_%s" % (tag, name, dt_tag)
                out[key + "_y"], out[key + "_d1"], out[key + "_d2"] = y, da, db
    out["dtypes"] = np.array([str(out["haar_ang_f32_y"].dtype), str(out["haar_ang_f32_d1"].dtype), str(out["haar_geo_mean_f32_d1"].dtype),
                              str(out["haar_cgd_f64_d1"].dtype)])
    save("g15_metric_gradients.npz", **out)


def g16_cloud_gradients():
    """Autograd through the cloud side.  Kabsch: the reference's symmetric_orthogonalization (rotation_representation.py:192-206,
    torch.svd's autograd) on torch.bmm(Q^T, P), for 12 clouds of 48 points -- 6 noisy pairs q = R p + 0.01 n, 4 independent pairs (det
    flips among them) and 2 planar clouds (z = 0, q = R p exactly: rank-2 H) --, losses (R*gR).sum() and (R*gR).sum() + (H*gH).sum(),
    float32 and float64.  Rotation: the four pairing statements of point_cloud/main.py:176-183 replayed verbatim with requires_grad on
    pc1 and gt_rmat, a random upstream on pc_out and on gg (the transposed layout), float32 and float64."""
    torch.manual_seed(16)
    np.random.seed(16)
    b, n = 12, 48
    p = torch.rand(b, n, 3) - 0.5
    p[10:, :, 2] = 0.0                                                    # planar clouds
    r_gt = sample_rot(b)
    q = torch.bmm(r_gt, p.transpose(1, 2)).transpose(1, 2).contiguous()
    q[:6] += 0.01 * torch.randn(6, n, 3)
    q[6:10] = torch.rand(4, n, 3) - 0.5                                   # independent pairs
    for c in (8, 9):                                                      # two of them mirrored where needed: det(H) < 0 (K1's flip)
        if torch.det(q[c].T @ p[c]) > 0:
            q[c, :, 0] = -q[c, :, 0]
    g_r, g_h = torch.randn(b, 3, 3), torch.randn(b, 3, 3)
    out = {"p": p, "q": q, "g_r": g_r, "g_h": g_h}
    for dt_tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for case in ("r", "rh"):
            pa = p.to(dt).clone().requires_grad_(True)
            qa = q.to(dt).clone().requires_grad_(True)
            h = torch.bmm(qa.transpose(1, 2), pa)
            r = rr.symmetric_orthogonalization(h)
            loss = (r * g_r.to(dt)).sum()
            if case == "rh":
                loss = loss + (h * g_h.to(dt)).sum()
            loss.backward()
            key = "kabsch_%s_%s" % (case, dt_tag)
            out[key + "_dp"], out[key + "_dq"] = pa.grad, qa.grad
            if case == "r":
                out["kabsch_%s_r" % dt_tag], out["kabsch_%s_h" % dt_tag] = r.detach(), h.detach()
    batch, point_num = 4, 48
    pc = torch.rand(batch, point_num, 3) - 0.5
    rot = sample_rot(batch)
    u_out, u_gg = torch.randn(batch, point_num, 3), torch.randn(batch, 3, point_num)
    out.update(pc1=pc, gt_rmat=rot, u_out=u_out, u_gg=u_gg)
    for dt_tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for layout, up in (("out", u_out), ("gg", u_gg)):
            pc1 = pc.to(dt).clone().requires_grad_(True)
            gt_rmat = rot.to(dt).clone().requires_grad_(True)
            gt_rmats = gt_rmat.contiguous().view(batch, 1, 3, 3).expand(batch, point_num, 3, 3).contiguous().view(-1, 3, 3)   # :176-177
            pc2 = torch.bmm(gt_rmats, pc1.view(-1, 3, 1))                                                                      # :180
            pc_out = pc2.view(batch, point_num, 3)                                                                             # :181
            gg = pc_out.transpose(1, 2)                                                                                        # :183
            y = pc_out if layout == "out" else gg
            (y * up.to(dt)).sum().backward()
            key = "rot_%s_%s" % (layout, dt_tag)
            out[key + "_dpc"], out[key + "_dr"] = pc1.grad, gt_rmat.grad
            out[key + "_y"] = y.detach().contiguous()
    save("g16_cloud_gradients.npz", **out)


def g17_symmetry():
    """Symmetry-aware angle error and Frobenius loss.  The group acts on the prediction from the right, as rotate_by_180
    (3D-Pose/loss.py:14-24: R_guess @ Rx(pi), Ry(pi), Rz(pi); spatialmath is not installed, so the flips are written as the diagonal
    matrices they are).  Three tables: rotate_by_180's {I, Rx, Ry, Rz}, C_4 about y, and three classes {I}, C_2(z), C_4(y) padded with
    the identity.  Every candidate R_pred @ S_k is formed in float64 from float32 R_pred and the float32-rounded table; the reference's
    angle_error runs on it, and loss_frobenius (3D-Pose/loss.py:7-11) on each row for the per-candidate distances.  The loss of the
    selected branches and its autograd gradients are the reference's loss_frobenius over the batch, in float64.  Rows 0..3 of each table
    are exact ties (integer matrices), the next four 'nearly' rotations of G3's kind (1.05 I: clamped, no raise); bad_* are rows on
    which angle_error raises (1.5 I) beside rows on which it does not."""
    torch.manual_seed(17)
    eye = np.eye(3)
    flip = np.stack([eye, np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])])
    ry = lambda c, s_: np.array([[c, 0.0, s_], [0.0, 1.0, 0.0], [-s_, 0.0, c]])
    c4y = np.stack([ry(1, 0), ry(0, 1), ry(-1, 0), ry(0, -1)])
    c2z = np.stack([eye, np.diag([-1.0, -1, 1]), eye, eye])
    tables = {"flip": flip[None], "c4y": c4y[None], "multi": np.stack([np.stack([eye] * 4), c2z, c4y])}
    rz90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    ties = {"flip": [(eye, rz90, 0), (rz90 @ flip[1], eye, 0), (flip[1], eye, 0), (rz90, rz90.T, 0)],
            "c4y": [(flip[1], eye, 0), (rz90, rz90.T, 0), (eye, flip[3], 0), (c4y[1], c4y[3], 0)],
            "multi": [(flip[1], eye, 1), (flip[1], eye, 2), (eye, rz90, 0), (c4y[1], c4y[3], 2)]}
    out = {}
    n_rand = 160
    for tag, table in tables.items():
        s32 = torch.from_numpy(table).float()                                   # (C, K, 3, 3): what the device holds
        c, k = s32.shape[:2]
        t_rand = rr.symmetric_orthogonalization(torch.randn(n_rand, 9))
        p_rand = rr.symmetric_orthogonalization(torch.randn(n_rand, 9))
        # a third of the random rows are near a symmetric copy of the target: the best candidate is then not the identity
        cls_rand = torch.randint(0, c, (n_rand,), dtype=torch.int32)
        near = torch.arange(n_rand) % 3 == 0
        j = torch.randint(0, k, (n_rand,))
        s_pick = s32[cls_rand.long(), j]
        noise = rr.symmetric_orthogonalization(torch.eye(3).reshape(1, 9) + 0.05 * torch.randn(n_rand, 9))
        p_near = torch.bmm(torch.bmm(t_rand, noise), s_pick.transpose(1, 2))
        p_rand = torch.where(near[:, None, None], p_near, p_rand).float()
        tie_p = torch.tensor(np.stack([a for a, _, _ in ties[tag]])).float()
        tie_t = torch.tensor(np.stack([b for _, b, _ in ties[tag]])).float()
        tie_c = torch.tensor([cc for _, _, cc in ties[tag]], dtype=torch.int32)
        nearly_p = 1.05 * torch.eye(3).repeat(4, 1, 1)
        nearly_t = rr.symmetric_orthogonalization(torch.randn(4, 9)) * 0 + torch.eye(3)
        nearly_c = torch.arange(4, dtype=torch.int32) % c
        p = torch.cat([tie_p, nearly_p, p_rand]).contiguous()
        t = torch.cat([tie_t, nearly_t, t_rand.float()]).contiguous()
        cls = torch.cat([tie_c, nearly_c, cls_rand]) if c > 1 else torch.zeros(p.shape[0], dtype=torch.int32)
        b = p.shape[0]
        s_row = s32[cls.long()].double()                                        # (B, K, 3, 3)
        deg_all = np.zeros((b, k))
        dist_all = np.zeros((b, k))
        for kk in range(k):
            cand = torch.bmm(p.double(), s_row[:, kk])                          # float64 product of float32 values
            deg_all[:, kk] = rr.angle_error(cand, t).numpy()
            for row in range(b):
                dist_all[row, kk] = float(loss_frobenius(t[row:row + 1].double(), cand[row:row + 1]))
        idx = np.argmin(deg_all, axis=1)
        loss_idx = np.argmin(dist_all, axis=1)
        pa = p.double().clone().requires_grad_(True)
        ta = t.double().clone().requires_grad_(True)
        s_sel = s_row[torch.arange(b), torch.from_numpy(loss_idx)]
        loss = loss_frobenius(ta, torch.bmm(pa, s_sel))                         # call order of 3D-Pose/main.py:85 (R, out)
        loss.backward()
        out.update({tag + "_S": s32, tag + "_p": p, tag + "_t": t, tag + "_cls": cls, tag + "_deg_all": deg_all,
                    tag + "_deg": deg_all.min(axis=1), tag + "_idx": idx.astype(np.int32), tag + "_dist_all": dist_all,
                    tag + "_loss_idx": loss_idx.astype(np.int32), tag + "_loss": loss.detach(), tag + "_dp": pa.grad, tag + "_dt": ta.grad})
    bad_p = torch.eye(3).repeat(6, 1, 1)
    bad_p[1] = 1.5 * torch.eye(3)                   # cos 1.75: raises
    bad_p[3] = 1.05 * torch.eye(3)                  # cos 1.075: clamped, no raise
    bad_p[4] = -0.5 * torch.eye(3)                  # cos -1.25: raises
    bad_t = torch.eye(3).repeat(6, 1, 1)
    raises = []
    for row in range(6):
        try:
            rr.angle_error(bad_p[row:row + 1], bad_t[row:row + 1])
            raises.append(False)
        except ValueError:
            raises.append(True)
    out.update(bad_p=bad_p, bad_t=bad_t, bad_raises=np.array(raises))
    save("g17_symmetry.npz", **out)


def g18_inverse_maps():
    """The inverse maps (matrix -> quaternion / rotation vector / Euler angles, log(R1^T R2)): about 4 000 float32 rotations made in
    float64 and then rounded, with the float64 answers for each row.  Families (`family`, names in `family_names`): uniform random;
    theta in [0, 1e-3]; theta in [pi - 1e-3, pi]; theta exactly 0 and exactly pi about random and about coordinate axes; the 24
    axis-aligned rotations; |e2| within 1e-3 of pi/2 and exactly pi/2; rows where two of (tr, r0, r4, r8) tie (rotations about a
    coordinate axis: two equal diagonal entries; half turns about (s, s, t) and (0, s, t): r0 = r4, tr = r0).
    Answers: scipy's Rotation.as_quat (reordered to (w,x,y,z), w >= 0) and as_rotvec of the NEAREST rotation (from_matrix projects the
    rounded matrix), the Euler triple of compute_rotation_matrix_from_euler's convention by the definition in float64
    (e2 = asin(clamp(-r1)), e1 = atan2(r2, r0), e0 = atan2(s3 r3 - c3 r5, c3 r8 - s3 r6), atan2(0, 0) = 0), and log(R1^T R2) for the
    shuffled pairing `perm`.  The reference's forward maps (compute_rotation_matrix_from_quaternion, so3_exp_map,
    compute_rotation_matrix_from_euler, run in float64, stored as float32) applied to those answers are kept for every fourth row
    (`fwd_rows`).  `g` is a fixed upstream gradient (its first three columns serve the three-vectors).
    The rows exempt from a signed value comparison (|w| < 1e-3, pi - theta < 1e-3, | |e2| - pi/2 | < 1e-2) stay below 25 %."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(18)
    fam_names, mats, fam = [], [], []

    def add(name, m):
        m = np.asarray(m, np.float64).reshape(-1, 3, 3)
        if name not in fam_names:
            fam_names.append(name)
        mats.append(m)
        fam.append(np.full(len(m), fam_names.index(name)))

    def unit(n):
        a = rng.standard_normal((n, 3))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    def euler_matrix(e):
        return rr.compute_rotation_matrix_from_euler(torch.as_tensor(np.asarray(e, np.float64))).numpy()

    add("random", Rotation.random(2400, random_state=18).as_matrix())
    add("theta_small", Rotation.from_rotvec(unit(300) * rng.uniform(0.0, 1e-3, (300, 1))).as_matrix())
    add("theta_near_pi", Rotation.from_rotvec(unit(300) * (np.pi - rng.uniform(0.0, 1e-3, (300, 1)))).as_matrix())
    add("theta_zero", np.tile(np.eye(3), (8, 1, 1)))
    ax = unit(100)
    add("theta_pi_random_axis", 2.0 * ax[:, :, None] * ax[:, None, :] - np.eye(3))
    add("theta_pi_coordinate_axis", [np.diag(d) for d in ([1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.])])
    axis_aligned = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, perm[i]] = signs[i]
            if np.linalg.det(m) > 0:
                axis_aligned.append(m)
    assert len(axis_aligned) == 24
    add("axis_aligned", axis_aligned)
    e = rng.uniform(-np.pi, np.pi, (250, 3))
    e[:, 2] = rng.choice([-1.0, 1.0], 250) * (np.pi / 2 - rng.uniform(0.0, 1e-3, 250))
    add("gimbal_near", euler_matrix(e))
    e = rng.uniform(-np.pi, np.pi, (50, 3))
    e[:, 2] = rng.choice([-1.0, 1.0], 50) * (np.pi / 2)
    add("gimbal_exact", euler_matrix(e))
    ang = rng.uniform(-np.pi, np.pi, 150)
    add("tie_diagonal", Rotation.from_rotvec(np.eye(3)[np.arange(150) % 3] * ang[:, None]).as_matrix())
    s_ = np.cos(rng.uniform(0.0, np.pi, 60))
    half = []
    for k, s0 in enumerate(s_):
        a = np.array([s0, s0, 1.0]) if k % 2 == 0 else np.array([0.0, s0, 1.0])
        a = np.roll(a, k % 3) / np.linalg.norm(a)
        half.append(2.0 * np.outer(a, a) - np.eye(3))
    add("tie_half_turn", half)

    r = np.concatenate(mats).astype(np.float32)
    family = np.concatenate(fam).astype(np.int16)
    n = len(r)
    near = Rotation.from_matrix(r.astype(np.float64))            # the nearest rotation of each rounded matrix
    q = near.as_quat()[:, [3, 0, 1, 2]]
    q = np.where(q[:, :1] < 0, -q, q)
    v = near.as_rotvec()
    m = near.as_matrix().reshape(n, 9)
    e2 = np.arcsin(np.clip(-m[:, 1], -1.0, 1.0))
    e1 = np.arctan2(m[:, 2], m[:, 0])
    s3, c3 = np.sin(e1), np.cos(e1)
    e0 = np.arctan2(s3 * m[:, 3] - c3 * m[:, 5], c3 * m[:, 8] - s3 * m[:, 6])
    euler = np.stack([e0, e1, e2], 1)
    perm = rng.permutation(n)
    rel = (near.inv() * near[perm]).as_rotvec()
    fwd_rows = np.arange(0, n, 4)
    f32 = lambda t: t.numpy().astype(np.float32)
    r_from_quat = f32(rr.compute_rotation_matrix_from_quaternion(torch.as_tensor(q[fwd_rows])))
    r_from_rotvec = f32(rr.so3_exp_map(torch.as_tensor(v[fwd_rows])))
    r_from_euler = f32(rr.compute_rotation_matrix_from_euler(torch.as_tensor(euler[fwd_rows])))
    theta = np.linalg.norm(v, axis=1)
    exempt = (np.abs(q[:, 0]) < 1e-3) | (np.pi - theta < 1e-3) | (np.abs(np.abs(e2) - np.pi / 2) < 1e-2)
    assert exempt.mean() < 0.25, exempt.mean()
    print("g18: %d rows, %.1f %% exempt from a signed comparison" % (n, 100 * exempt.mean()))
    save("g18_inverse_maps.npz", r=r, family=family, family_names=np.array(fam_names), quat=q, rotvec=v, euler=euler, perm=perm.astype(np.int32),
         rel_rotvec=rel, fwd_rows=fwd_rows.astype(np.int32), r_from_quat=r_from_quat, r_from_rotvec=r_from_rotvec, r_from_euler=r_from_euler,
         g=rng.standard_normal((n, 4)).astype(np.float32))


def g19_add_metrics():
    """ADD, ADD-S, per-point distances, nearest indices, diameters and the gradients w.r.t. the estimated pose: float32 inputs, float64
    answers from tests/add_metrics_ref.py (the reference has no evaluation metric for Iterative/; the definitions are the
    literature's).  Clouds are normalised to the unit sphere; fixed seeds."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import add_metrics_ref as ref
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(19)

    def haar(b):
        return Rotation.random(b, random_state=rng).as_matrix()

    def poses(rot, t):
        T = np.tile(np.eye(4), (len(rot), 1, 1))
        T[:, :3, :3], T[:, :3, 3] = rot, t
        return T.astype(np.float32)

    def unit_sphere(p):                                   # centred on the bounding sphere's proxy (the mean), largest radius 1
        p = p - p.mean(1, keepdims=True)
        r = np.linalg.norm(p, axis=-1).max(1)
        return (p / np.where(r > 0, r, 1.0)[:, None, None]).astype(np.float32)

    def cloud(b, n):
        return unit_sphere(rng.standard_normal((b, n, 3)))

    def near(T, err):
        """T with a rotation error of `err` rad about a random axis and a translation error of `err`."""
        b = len(T)
        ax = rng.standard_normal((b, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        dt = rng.standard_normal((b, 3))
        dt *= err / np.linalg.norm(dt, axis=1, keepdims=True)
        rot = Rotation.from_rotvec(ax * err).as_matrix() @ T[:, :3, :3].astype(np.float64)
        return poses(rot, T[:, :3, 3].astype(np.float64) + dt)

    plan = []                                             # (family, n, tgt, tpred, pts)
    tr = lambda b: rng.standard_normal((b, 3)) * 0.3 + np.array([0.0, 0.0, 2.0])
    for n in ref.SIZES:
        t = tr(2)                                         # Haar rotations; the translations differ a little (not at N = 1: ADD-S <= diameter = 0)
        plan.append(("haar", n, poses(haar(2), t), poses(haar(2), t + (0.05 * rng.standard_normal((2, 3)) if n > 1 else 0.0)), cloud(2, n)))
    for n in (64, 256, 1000):
        tg = poses(haar(1), tr(1))
        plan.append(("small_error", n, tg, near(tg, 1e-3), cloud(1, n)))
    for n in (1, 3, 100, 256):
        tg = poses(haar(1), tr(1))
        plan.append(("identical", n, tg, tg.copy(), cloud(1, n)))
    half_turn = np.diag([-1.0, -1.0, 1.0])
    for n in (64, 100, 256):                              # p and (-x, -y, z): an exact 2-fold symmetry in float32
        h = rng.standard_normal((1, n // 2, 3))
        h[..., 2] -= h[..., 2].mean()
        h = (h / np.linalg.norm(h, axis=-1).max()).astype(np.float32)
        pts = np.concatenate([h, h * np.array([-1, -1, 1], np.float32)], 1)
        tg = poses(haar(1), tr(1))
        tp = poses(tg[:, :3, :3].astype(np.float64) @ half_turn, tg[:, :3, 3].astype(np.float64))     # exact: sign flips of two columns
        plan.append(("twofold", n, tg, tp, pts))
    for n in (3, 100):
        d = rng.standard_normal(3)
        pts = unit_sphere(rng.standard_normal((1, n, 1)) * (d / np.linalg.norm(d)))
        plan.append(("collinear", n, poses(haar(1), tr(1)), poses(haar(1), tr(1)), pts))
    for n in (64, 100):
        pts = cloud(1, n)
        pts[:, n // 2:] = pts[:, :n - n // 2]              # every point of the first half appears twice
        tg = poses(haar(1), tr(1))
        plan.append(("duplicated", n, tg, near(tg, 0.05), pts))

    out = {k: [] for k in ref.PER_CLOUD + ref.PER_POINT}
    fam, ns, bs = [], [], []
    for family, n, tg, tp, pts in plan:
        assert pts.shape[1] == n and pts.dtype == np.float32 and np.linalg.norm(pts, axis=-1).max() <= 1 + 1e-6
        ans = ref.answers(tg, tp, pts)
        ans.update(tgt=tg, tpred=tp, pts=pts)
        for k in ref.PER_CLOUD:
            out[k].append(ans[k])
        for k in ref.PER_POINT:
            out[k].append(ans[k].reshape((-1,) + ans[k].shape[2:]))
        fam.append(ref.FAMILIES.index(family)); ns.append(n); bs.append(len(tg))
        print("g19 %-12s N=%4d  ADD %.3e  ADD-S %.3e  diam %.4f" % (family, n, ans["add"][0], ans["adds"][0], ans["diam"][0]))
    save("g19_add_metrics.npz", family_names=np.array(ref.FAMILIES), case_family=np.array(fam, np.int32), case_n=np.array(ns, np.int32),
         case_b=np.array(bs, np.int32), **{k: np.concatenate(v) for k, v in out.items()})


def g26_sym_add():
    """so3_sym_add_f32: ADD, ADD-L1 and MSSD up to a symmetry group.  float32 poses, clouds and tables; float64 answers from
    tests/sym_add_ref.py for the three modes and EVERY candidate k, and the float64 winner's gradient for the two losses (no reference
    code exists for these metrics, as for G19: the definitions are the literature's, restated from include/so3proj.h).  Clouds of unit
    radius, poses about two units from the origin, fixed seeds.  Families: haar (unrelated poses), near_symmetric (T_pred within 1e-2 of
    T_gt S_j^-1: the winner is j), exact_c4 (T_pred = T_gt S_j^-1 exactly, quarter turns about z), identical_points (a cloud of one
    repeated point at T_pred = T_gt: d = 0 everywhere)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import sym_add_ref as ref
    rng = np.random.default_rng(26)
    eye = np.eye(3)

    def haar(b):
        q, r = np.linalg.qr(rng.standard_normal((b, 3, 3)))
        q = q * np.sign(np.einsum("bii->bi", r))[:, None, :]
        q[:, :, 0] *= np.linalg.det(q)[:, None]
        return q

    def cyclic(n, axis):                                  # C_n about a coordinate axis; quarter and half turns exact
        th = 2.0 * np.pi * np.arange(n) / n
        c, s_ = np.cos(th), np.sin(th)
        c[np.abs(c) < 1e-15] = 0.0
        s_[np.abs(s_) < 1e-15] = 0.0
        a = np.zeros(3)
        a["xyz".index(axis)] = 1.0
        k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        return c[:, None, None] * eye + (1.0 - c)[:, None, None] * np.outer(a, a) + s_[:, None, None] * k

    def table(groups):                                    # SymmetryTable's layout: identity first, padded with the identity
        k = max(len(g) for g in groups)
        t = np.broadcast_to(eye, (len(groups), k, 3, 3)).copy()
        for c, g in enumerate(groups):
            t[c, :len(g)] = g
        return t.astype(np.float32)

    def poses(rot, t):
        T = np.tile(np.eye(4), (len(rot), 1, 1))
        T[:, :3, :3], T[:, :3, 3] = rot, t
        return T.astype(np.float32)

    def cloud(b, n):
        p = rng.standard_normal((b, n, 3))
        if n > 1:
            p = p - p.mean(1, keepdims=True)
        return (p / np.linalg.norm(p, axis=-1).max(1)[:, None, None]).astype(np.float32)

    def small_rotation(b, err):
        v = rng.standard_normal((b, 3))
        v *= err / np.linalg.norm(v, axis=1, keepdims=True)
        th = np.linalg.norm(v, axis=1)[:, None, None]
        k = np.zeros((b, 3, 3))
        k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
        k = k / th
        return eye + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)

    tr = lambda b: rng.standard_normal((b, 3)) * 0.3 + np.array([0.0, 0.0, 2.0])
    one = {"c2z": table([cyclic(2, "z")]), "c4y": table([cyclic(4, "y")]), "c7x": table([cyclic(7, "x")]), "i": table([eye[None]])}
    multi = table([eye[None], cyclic(2, "z"), cyclic(4, "y"), cyclic(6, "x")])
    plan = []                                             # (family, tgt, tpred, pts, S, cls)
    for n, tag in ((1, "c2z"), (3, "c4y"), (64, "c7x"), (100, "i"), (1000, "c4y"), (1500, "c2z")):
        t = tr(2)
        plan.append(("haar", poses(haar(2), t), poses(haar(2), t + 0.05 * rng.standard_normal((2, 3))), cloud(2, n), one[tag], None))
    for n in (65, 300):
        b = 8
        cls = rng.integers(0, 4, b).astype(np.int32)
        t = tr(b)
        plan.append(("haar", poses(haar(b), t), poses(haar(b), t + 0.05 * rng.standard_normal((b, 3))), cloud(b, n), multi, cls))
    for n, S, cls in ((64, one["c4y"], None), (256, one["c7x"], None), (1100, one["c2z"], None), (100, multi, np.array([0, 1, 2, 3, 3, 2], np.int32))):
        b = S.shape[1] if cls is None else len(cls)
        rows = ref.rows_of(S, cls, b)
        j = np.arange(b) % S.shape[1]
        rg, t = haar(b), tr(b)
        rp = small_rotation(b, 1e-2) @ rg @ np.transpose(rows[np.arange(b), j], (0, 2, 1))
        plan.append(("near_symmetric", poses(rg, t), poses(rp, t + 1e-3 * rng.standard_normal((b, 3))), cloud(b, n), S, cls))
    c4z = table([cyclic(4, "z")])
    for n in (1, 100, 1030):
        tg = poses(haar(4), tr(4))
        tp = tg.copy()
        tp[:, :3, :3] = np.einsum("bil,bjl->bij", tg[:, :3, :3], c4z[0])          # T_gt S_j^-1: signed column permutations, exact in float32
        plan.append(("exact_c4", tg, tp, cloud(4, n), c4z, None))
    for n in (5, 200):
        tg = poses(haar(1), tr(1))
        plan.append(("identical_points", tg, tg.copy(), np.repeat(cloud(1, 1), n, axis=1), one["c4y"], None))

    out, fam = {}, []
    for i, (family, tg, tp, pts, S, cls) in enumerate(plan):
        assert pts.dtype == np.float32 and S.dtype == np.float32 and np.linalg.norm(pts, axis=-1).max() <= 1 + 1e-6
        ans = ref.answers(tg, tp, pts, S, cls)
        ans.update(tgt=tg, tpred=tp, pts=pts, S=S, cls=np.zeros(0, np.int32) if cls is None else cls)
        out.update({"%d_%s" % (i, k): ans[k] for k in ref.PER_CASE})
        fam.append(ref.FAMILIES.index(family))
        print("g26 %-16s B=%d N=%4d C=%d K=%d  ADD %s" % (family, len(tg), pts.shape[1], S.shape[0], S.shape[1], np.round(ans["stat_l2"][0], 4)))
    save("g26_sym_add.npz", family_names=np.array(ref.FAMILIES), case_family=np.array(fam, np.int32), **out)


def g20_rigid_align():
    """rigid_align: float32 clouds, weights and upstream gradients, float64 answers (R, t, H, centroids) from tests/rigid_align_ref.py
    (the reference has no registration layer: the definition is the weighted Kabsch / Umeyama solution without scale).  Clouds of
    unit radius, Q = R_gt P + t_gt + sigma * noise with Haar R_gt; fixed seeds.  The per-point gradients are not stored (they
    would triple the file): both test files compute them from the stored inputs with ref.grads64."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import rigid_align_ref as ref
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(20)

    def ball(n):                                           # n points in the unit ball
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * rng.uniform(0, 1, (n, 1)) ** (1 / 3)

    def weights(kind, n):
        """(w as stored, the number of real points): the mask keeps at least three points, so that R stays unique."""
        if kind in ("none", "ones"):
            return np.ones(n), n
        if kind == "random":
            return rng.uniform(0.05, 1.0, n), n
        if kind == "zero":
            return np.zeros(n), n
        valid = min(n, max(3, n // 2))
        return (np.arange(n) < valid).astype(np.float64), valid

    def well_conditioned(p, q, w):
        """Is the rotation well determined?  (s2 + s3) / s1 >= 0.1 for the float64 H's singular values: a nearly collinear triple
        is a degenerate cloud in all but name, and its R amplifies any rounding of H by s1 / (s2 + s3)."""
        h = ref.answers(p[None].astype(np.float32), q[None].astype(np.float32), w[None].astype(np.float32))["H"][0]
        s = np.linalg.svd(h, compute_uv=False)
        return s[0] > 0 and (s[1] + s[2]) / s[0] >= 0.1

    def haar_cloud(n, kind, offset, sigma):
        while True:
            p, q, w = draw_cloud(n, kind, offset, sigma)
            if n < 3 or kind == "zero" or well_conditioned(p, q, w):
                return p, q, w

    def draw_cloud(n, kind, offset, sigma):
        w, valid = weights(kind, n)
        p = ball(n) + offset
        t_gt = max(offset, 1.0) * rng.uniform(-1, 1, 3)
        q = p @ Rotation.random(random_state=rng).as_matrix().T + t_gt + sigma * rng.standard_normal((n, 3))
        if valid < n:                                      # the masked tail: finite junk up to 10 x the radius around the clouds
            p[valid:] = offset + rng.uniform(-10, 10, (n - valid, 3))
            q[valid:] = q[:valid].mean(0) + rng.uniform(-10, 10, (n - valid, 3))
        return p, q, w

    plan = []                                              # (family, kind, n, offset, check, [(p, q, w, sigma), ...])
    for n in ref.SIZES:
        if n in ref.SMALL_SIZES:
            combos = [(k, o) for k in ref.WEIGHTS for o in ref.OFFSETS]
        else:                                              # a covering selection: every kind and every offset at every large size
            i = ref.SIZES.index(n)
            combos = [("none", 100.0), ("random", ref.OFFSETS[i % 3]), ("mask", ref.OFFSETS[(i + 1) % 3]), ("ones", ref.OFFSETS[(i + 2) % 3]),
                      ("zero", 10.0)]
        for kind, off in combos:
            sig = ref.SIGMAS if n in ref.SMALL_SIZES else (ref.SIGMAS[(ref.WEIGHTS.index(kind) + n) % 2],)
            check = ref.ZERO if kind == "zero" else ref.PROPERTIES if n < 3 else ref.FULL
            plan.append(("haar", kind, n, off, check, [haar_cloud(n, kind, off, s) + (s,) for s in sig]))
    for n, off in ((64, 0.0), (65, 10.0)):                 # Q = diag(1, 1, -1) P (about the offset): the best R is not the reflection
        p = ball(n)
        plan.append(("reflected", "none", n, off, ref.PROPERTIES, [(p + off, p * np.array([1.0, 1.0, -1.0]) + off, np.ones(n), 0.0)]))
    for n, off in ((3, 0.0), (65, 10.0)):
        d = rng.standard_normal(3)
        p = rng.uniform(-1, 1, (n, 1)) * (d / np.linalg.norm(d)) + off
        q = (p - off) @ Rotation.random(random_state=rng).as_matrix().T + off
        plan.append(("collinear", "random", n, off, ref.PROPERTIES, [(p, q, rng.uniform(0.05, 1.0, n), 0.0)]))
    for n, off in ((3, 0.0), (64, 100.0)):
        p, q = np.tile(ball(1) + off, (n, 1)), np.tile(ball(1) - off, (n, 1))
        plan.append(("coincident", "none", n, off, ref.PROPERTIES, [(p, q, np.ones(n), 0.0)]))

    out = {k: [] for k in ref.PER_CLOUD + ref.PER_POINT}
    meta = {k: [] for k in ref.PER_CASE}
    for family, kind, n, off, check, clouds in plan:
        b = len(clouds)
        P = np.stack([c[0] for c in clouds]).astype(np.float32)
        Q = np.stack([c[1] for c in clouds]).astype(np.float32)
        w = np.stack([c[2] for c in clouds]).astype(np.float32)
        ans = ref.answers(P, Q, w)
        ans.update(P=P, Q=Q, w=w, sigma=np.array([c[3] for c in clouds]), gR=rng.standard_normal((b, 3, 3)).astype(np.float32),
                   gt=rng.standard_normal((b, 3)).astype(np.float32), gH=rng.standard_normal((b, 3, 3)).astype(np.float32))
        for k in ref.PER_CLOUD:
            out[k].append(ans[k])
        for k in ref.PER_POINT:
            out[k].append(ans[k].reshape((-1,) + ans[k].shape[2:]))
        for k, v in zip(ref.PER_CASE, (ref.FAMILIES.index(family), n, b, ref.WEIGHTS.index(kind), off, check)):
            meta[k].append(v)
    print("g20: %d cases, %d clouds, %d points" % (len(plan), sum(meta["b"]), sum(len(x) for x in out["P"])))
    save("g20_rigid_align.npz", family_names=np.array(ref.FAMILIES), weight_names=np.array(ref.WEIGHTS),
         case_family=np.array(meta["family"], np.int32), case_n=np.array(meta["n"], np.int32), case_b=np.array(meta["b"], np.int32),
         case_weights=np.array(meta["weights"], np.int32), case_offset=np.array(meta["offset"]), case_check=np.array(meta["check"], np.int32),
         **{k: np.concatenate(v) for k, v in out.items()})


def g21_icp():
    """nearest_neighbors and icp_align: float32 clouds, initial poses and weights, float64 answers from tests/icp_ref.py (the reference
    has no registration layer: the definition is brute-force closest points and rigid_align's pose, restated there).  Clouds of unit
    radius; fixed seeds.  What the generator asserts about its own cases is what the tests rely on: the trimming margin of every
    trimmed step, exact convergence of the exact cases within 10 float64 iterations, settled correspondences of the noisy ones."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import icp_ref as ref
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(21)

    def ball(n):
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * rng.uniform(0, 1, (n, 1)) ** (1 / 3)

    def spaced_ball(n, spacing, quantum=None):
        """n points of the unit ball, no two closer than `spacing`; with `quantum`, coordinates are integer multiples of it."""
        pts = []
        while len(pts) < n:
            c = ball(1)[0] * 0.98
            if quantum is not None:
                c = np.round(c / quantum) * quantum
            if all(np.linalg.norm(c - o) >= spacing for o in pts):
                pts.append(c)
        return np.array(pts)

    def small_motion(deg, shift):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        d = rng.standard_normal(3)
        return (Rotation.from_rotvec(axis * np.deg2rad(rng.uniform(0.25 * deg, deg))).as_matrix(),
                d / np.linalg.norm(d) * rng.uniform(0.25 * shift, shift))

    cases = []

    def add(kind, name, P, Q, w=None, R0=None, t0=None, iterations=0, max_distance=None, weights="none", offset=0.0, check=ref.FULL, **answers):
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        cases.append(dict(kind=kind, name=name, P=f32(P), Q=f32(Q), w=f32(w), R0=f32(R0), t0=f32(t0), iterations=iterations,
                          max_distance=max_distance, weights=weights, offset=offset, check=check, shared=np.ndim(Q) == 2, **answers))
        return cases[-1]

    # ---- search -------------------------------------------------------------------------------------------------------------
    for n, m in ref.SIZES:
        for shared in (False, True):
            b = 2 if shared or (n, m) in ref.SMALL_SIZES else 1
            c = add("search", "search %dx%d %s" % (n, m, "shared" if shared else "own"), np.stack([ball(n) for _ in range(b)]),
                    ball(m) if shared else np.stack([ball(m) for _ in range(b)]))
            c["dist"], c["nearest"] = ref.nearest64(c["P"], c["Q"])
    Y = ball(300)
    Y[150:200] = Y[50:100]                                                    # duplicated target points: the first one is the answer
    pick = np.concatenate([rng.permutation(300)[:80], np.arange(150, 200, 2), [299, 0]])
    c = add("search", "subset with duplicates", np.stack([Y[pick], Y[pick[::-1]]]), Y)
    c["dist"], c["nearest"] = ref.nearest64(c["P"], c["Q"])
    first = np.where((pick >= 150) & (pick < 200), pick - 100, pick)
    assert (c["dist"] == 0).all() and (c["nearest"][0] == first).all() and (c["nearest"][1] == first[::-1]).all()

    # ---- single steps ---------------------------------------------------------------------------------------------------------
    def step_case(n, m, weights, trimmed, offset, axis, shared=False, b=1, empty=False):
        P, Q, W, R0, T0 = [], [], [], [], []
        identity = weights == "none" and offset == 0.0 and not trimmed           # these start from the default pose
        q_shared = ball(m) + offset * np.eye(3)[axis]
        for _ in range(b):
            q = q_shared if shared else ball(m) + offset * np.eye(3)[axis]
            if identity:
                r_gt, t_gt = small_motion(3.0, 0.03)
            else:
                r_gt, t_gt = Rotation.random(random_state=rng).as_matrix(), max(offset, 1.0) * rng.uniform(-1, 1, 3)
            src = q[rng.permutation(m)[:n]] + 0.03 * rng.standard_normal((n, 3))
            P.append((src - t_gt) @ r_gt)                                        # p = R_gt^T (q + noise - t_gt)
            dr, dt = small_motion(3.0, 0.03)
            R0.append(r_gt @ dr)
            T0.append(t_gt + dt)
            W.append(None if weights == "none" else rng.uniform(0.05, 1.0, n) if weights == "random" else (rng.uniform(0, 1, n) < 0.7).astype(np.float64))
            Q.append(q)
        c = add("step", "step %dx%d %s %s off %g%s" % (n, m, weights, "trimmed" if trimmed else "all", offset, " shared" if shared else ""),
                np.stack(P), q_shared if shared else np.stack(Q), None if weights == "none" else np.stack(W),
                None if identity else np.stack(R0), None if identity else np.stack(T0), iterations=1, weights=weights, offset=offset)
        R0_, t0_ = (np.broadcast_to(np.eye(3), (b, 3, 3)), np.zeros((b, 3))) if identity else (c["R0"].astype(np.float64), c["t0"].astype(np.float64))
        d, idx = ref.nearest64(ref.pose_points(c["P"], R0_, t0_), c["Q"])
        if trimmed or empty:
            flat = np.sort(d.reshape(-1))
            md = None
            if empty:
                md = 0.5 * flat[0]
            else:
                for k in range(max(1, int(0.6 * len(flat))), len(flat)):
                    if flat[k] - flat[k - 1] > 4 * ref.MARGIN:
                        md = 0.5 * (flat[k] + flat[k - 1])
                        break
                if md is None:
                    md = flat[-1] + 0.01
            assert np.abs(d - md).min() > ref.MARGIN and md > ref.MARGIN, (c["name"], md)
            c["max_distance"] = float(np.float32(md))
            assert np.abs(d - c["max_distance"]).min() > ref.MARGIN
        ans = ref.icp64(c["P"], c["Q"], None if identity else c["R0"], None if identity else c["t0"], 1, c["max_distance"], c["w"])
        s = ref.step_from(c["P"], c["Q"], idx, d, R0_, t0_, c["w"], c["max_distance"])
        sv = np.linalg.svd(s["H"], compute_uv=False)
        good = (s["wp"] > 0).sum(1).min() >= 3 and (sv[:, 0] > 0).all() and ((sv[:, 1] + sv[:, 2]) / np.maximum(sv[:, 0], 1e-300)).min() >= 0.1
        c["check"] = ref.FULL if good or empty else ref.PROPERTIES
        if empty:
            assert (ans["inliers"] == 0).all() and (ans["rmse"] == 0).all() and np.array_equal(ans["R"], R0_) and np.array_equal(ans["t"], t0_)
        c.update({k: ans[k] for k in ("R", "t", "rmse", "inliers", "nearest", "dist")})
        return c

    for n, m in ref.SMALL_SIZES:
        for wk in ref.WEIGHTS:
            for trimmed in (False, True):
                for ax, off in enumerate(ref.OFFSETS):
                    step_case(n, m, wk, trimmed, off, ax, b=2)
    for i, (n, m) in enumerate(ref.SIZES[2:]):                                    # a covering selection at the large sizes
        for j, (wk, trimmed) in enumerate((("none", False), ("random", True), ("mask", True), ("random", False))):
            step_case(n, m, wk, trimmed, ref.OFFSETS[(i + j) % 3] if j else 0.0, (i + j) % 3)
    step_case(257, 1025, "random", True, 10.0, 1, shared=True, b=2)
    step_case(255, 1023, "mask", False, 0.0, 0, empty=True)
    step_case(3, 7, "none", False, 10.0, 2, empty=True, b=2)

    # ---- convergence: Q = T_gt (P permuted) EXACTLY in float32 ----------------------------------------------------------------
    # P on the lattice 25 * 2^-14, R_gt = Rz Rx of the (3, 4, 5) triangle (entries are multiples of 1/25), t_gt on 2^-14: every
    # coordinate of Q is an integer multiple of 2^-14 below 4, exact in float32, so the float64 fixed point is T_gt itself.
    c5, s5 = 3.0 / 5.0, 4.0 / 5.0
    rz5, rx5 = np.array([[c5, -s5, 0], [s5, c5, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0], [0, c5, -s5], [0, s5, c5]])
    r_exact = [rz5 @ rx5, (rz5 @ rx5).T, rx5 @ rz5, (rx5 @ rz5).T]

    def registration(name, kind, exact, extra, sigma, seed_tries=20):
        n, b = 300, 4
        for _ in range(seed_tries):
            P, Q, R0, T0, RG, TG, PERM = [], [], [], [], [], [], []
            for cloud in range(b):
                p = spaced_ball(n, 0.12, 25 * 2.0**-14 if exact else None)
                r_gt = r_exact[cloud] if exact else Rotation.random(random_state=rng).as_matrix()
                t_gt = np.round(rng.uniform(-0.5, 0.5, 3) * 2**14) / 2**14
                slots = rng.permutation(n + extra)
                q = np.zeros((n + extra, 3))
                if exact:                                  # integers throughout: R_gt = R25 / 25 and p = 25 k 2^-14 give R_gt p = (R25 k) 2^-14
                    image = (np.round(p * 2.0**14 / 25) @ np.round(25 * r_gt).T) * 2.0**-14 + t_gt
                else:
                    image = p @ r_gt.T + t_gt + sigma * rng.standard_normal((n, 3))
                q[slots[:n]] = image
                d = rng.standard_normal((extra, 3))
                q[slots[n:]] = (t_gt + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.5, 2.0, (extra, 1))).astype(np.float32)      # beyond max_distance
                dr, dt = small_motion(2.0, 0.02)
                P.append(p); Q.append(q); R0.append(r_gt @ dr); T0.append(t_gt + dt); RG.append(r_gt); TG.append(t_gt); PERM.append(slots[:n])
            c = dict(P=np.stack(P).astype(np.float32), Q=np.stack(Q).astype(np.float32), R0=np.stack(R0).astype(np.float32), t0=np.stack(T0).astype(np.float32))
            md = 0.2 if extra else None
            ans = ref.icp64(c["P"], c["Q"], c["R0"], c["t0"], 20, md, None)
            perm = np.stack(PERM)
            if exact:
                assert np.array_equal(c["P"].astype(np.float64), np.stack(P)) and np.array_equal(c["Q"].astype(np.float64), np.stack(Q))
                ok = (ans["rmse"][9:] < 1e-12).all() and np.array_equal(ans["nearest"], perm)
            else:                                          # the correspondences have settled by iteration 10 and are far from a tie
                early = ref.icp64(c["P"], c["Q"], c["R0"], c["t0"], 10, md, None)
                ok = np.array_equal(early["nearest"], ans["nearest"]) and ref.runner_up_gap(c["P"], c["Q"], ans["R"], ans["t"]) > 1e-3
            if ok:
                break
        else:
            raise AssertionError("no seed converged for " + name)
        add(kind, name, c["P"], c["Q"], None, c["R0"], c["t0"], iterations=20, max_distance=md, Rgt=np.stack(RG), tgt=np.stack(TG), perm=perm,
            **{k: ans[k] for k in ("R", "t", "rmse", "inliers", "nearest", "dist")})
        print("g21 %-28s rmse %s" % (name, " ".join("%.1e" % v for v in ans["rmse"][:6, 0])))

    registration("converge exact", "converge", True, 0, 0.0)
    registration("converge exact superset", "converge", True, 40, 0.0)
    registration("noise", "noise", False, 0, 0.01)
    registration("noise superset", "noise", False, 40, 0.01)

    arrays = {}
    for i, c in enumerate(cases):
        for k in ref.ARRAYS:
            if c.get(k) is not None and not (c["kind"] == "step" and k in ("dist", "nearest")):      # a step is checked from what the call returns
                arrays["c%d_%s" % (i, k)] = c[k].astype(np.int32) if k in ("nearest", "perm", "inliers") else c[k]
    wn = list(ref.WEIGHTS)
    print("g21: %d cases" % len(cases))
    save("g21_icp.npz", kind_names=np.array(ref.KINDS), weight_names=np.array(wn), case_kind=np.array([ref.KINDS.index(c["kind"]) for c in cases], np.int32),
         case_name=np.array([c["name"] for c in cases]), case_weights=np.array([wn.index(c["weights"]) for c in cases], np.int32),
         case_offset=np.array([c["offset"] for c in cases]), case_iterations=np.array([c["iterations"] for c in cases], np.int32),
         case_max_distance=np.array([-1.0 if c["max_distance"] is None else c["max_distance"] for c in cases]),
         case_shared=np.array([c["shared"] for c in cases]), case_check=np.array([c["check"] for c in cases], np.int32), **arrays)


def g22_pointnet(seed=24):
    """farthest_point_sample and query_ball_point (point_cloud/pointnet_utils.py:53-97), the reference's own functions on the CPU in
    float32, at the reference model's settings: clouds normalised by pc_normalize, level one 1024 -> 512 centres with (r, K) = (0.1, 32)
    and (0.2, 64), level two 512 -> 128 centres (of level one's centres) with (0.4, 64) and (0.8, 128), and an odd-sized 3 x 300 -> 77.
    torch is seeded and centroids[:, 0] is the recorded start.  Every ball-query case stores near_boundary (tests/pointnet_ref.py);
    the generator asserts that the reference differs from the float64 restatement only inside that mask and that the mask covers at
    most 1 % of a case's rows.  (Seeds 22 and 23 put 4 and 3 of level two's 256 rows into the mask: 1.6 % and 1.2 %; 24 is the first
    seed that meets the cap in every case.)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import pointnet_ref as ref
    names = ["square_distance", "index_points", "farthest_point_sample", "query_ball_point"]
    fns = functions_from(os.path.join(REF, "point_cloud", "pointnet_utils.py"), names)
    for f in fns:                                                 # the functions call each other by name
        f.__globals__.update(dict(zip(names, fns)))
    _, index_points, farthest_point_sample, query_ball_point = fns
    (pc_normalize,) = functions_from(os.path.join(REF, "point_cloud", "prepare.py"), ["pc_normalize"])
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)

    def clouds(b, n):
        raw = (rng.rand(b, n, 3) - 0.5) * np.array([1.0, 0.8, 0.6]) + np.array([0.3, -1.0, 2.0])
        return torch.tensor(np.stack([pc_normalize(c)[0] for c in raw])).float()

    arrays = {}
    level = {1024: clouds(2, 1024), 300: clouds(3, 300)}
    arrays["cloud0"], arrays["cloud2"] = level[1024], level[300]
    fps_idx = {}
    for k, (b, n, npoint) in enumerate(ref.FPS_CASES):
        idx = farthest_point_sample(level[n], npoint)
        assert idx.shape == (b, npoint) and int(idx.max()) < n
        assert np.array_equal(ref.fps(level[n].numpy(), npoint, idx[:, 0].numpy()), idx.numpy()), "the restatement is not the reference's sequence"
        fps_idx[n] = idx
        arrays["fps%d_idx" % k] = idx.numpy().astype(np.uint16)
        if n == 1024:
            level[512] = index_points(level[1024], idx)             # level two's cloud: level one's centres
    centres = {1024: level[512], 512: index_points(level[512], fps_idx[512])}
    for k, (n, s, radius, nsample) in enumerate(ref.BALL_CASES):
        xyz, c = level[n], centres[n]
        assert c.shape == (2, s, 3)
        idx = query_ball_point(radius, nsample, xyz, c).numpy()
        want, _ = ref.ball_query(radius, nsample, xyz.numpy(), c.numpy(), np.float64)
        near = ref.near_boundary(radius, xyz.numpy(), c.numpy())
        differ = (idx != want).any(-1)
        assert not (differ & ~near).any(), "the reference differs from the float64 restatement outside the boundary mask"
        assert near.mean() <= ref.BOUNDARY_CAP, (k, near.mean())
        ref.row_properties(idx, n)
        print("g22 ball N=%d S=%d r=%g K=%d: %d rows near the boundary (%.2f %%), %d differ" % (n, s, radius, nsample, near.sum(), 100 * near.mean(), differ.sum()))
        arrays["ball%d_idx" % k] = idx.astype(np.uint16)
        arrays["ball%d_near" % k] = near
    save("g22_pointnet.npz", **arrays)


def g24_three_nn(seed=24):
    """three_nn and three_interpolate: the reference's own statements on the CPU in float32 -- the `if S == 1: ... else: ...` of
    PointNetFeaturePropagation.forward (point_cloud/pointnet_utils.py:283-293: square_distance, sort, the weight lines, index_points),
    taken out of the method with `ast` and executed, nothing retyped -- on anisotropic Gaussian clouds, D = 16, torch seeded.  The
    clouds go through pc_normalize (centred on their bounding box and scaled by its diagonal: radius at most 0.5) and are then scaled
    to radius 1, the scale near_tie's and near_zero's thresholds are stated for: at pc_normalize's own scale no cloud of 512 known
    points can meet the near_zero cap (a bounding box of diagonal 1 holds at most 0.19 of volume, so more than 1.1 % of uniformly
    placed unknown points lie within 0.01 of a known one; a Gaussian cloud at that scale puts 1.8 % of the rows near a tie).
    Cases (tests/three_nn_ref.py: CASES): disjoint clouds at 2 x 1024 <- 512, 2 x 512 <- 128 and 3 x 300 <- 77 (unknown and known
    points drawn and normalised together, then split); `subset` at 2 x 1024 <- 512, case 0's unknown cloud with the known points
    chosen from it by the reference's farthest_point_sample, as the model's fp1 has them; 2 x 128 <- 1.  Every case stores near_tie and
    near_zero (float64); the generator asserts that the reference's indices differ from the restatement's only inside near_tie, that
    near_tie covers at most 1 % of a case's rows and, for the disjoint cases, that near_tie | near_zero does.  ref_dev is the largest
    |reference - float64 restatement| of the interpolated features outside both masks.  The subset case's values are NOT stored: half its
    rows have a true distance of 0, where the reference's expanded form is cancellation noise; the number of rows with a negative
    reference weight is recorded instead."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import three_nn_ref as ref
    path = os.path.join(REF, "point_cloud", "pointnet_utils.py")
    names = ["square_distance", "index_points", "farthest_point_sample"]
    fns = functions_from(path, names)
    for f in fns:
        f.__globals__.update(dict(zip(names, fns)))
    square_distance, index_points, farthest_point_sample = fns
    (pc_normalize,) = functions_from(os.path.join(REF, "point_cloud", "prepare.py"), ["pc_normalize"])
    with open(path) as fh:
        tree = ast.parse(fh.read(), filename=path)
    layer = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PointNetFeaturePropagation")
    forward = next(n for n in layer.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    branch = next(n for n in forward.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare) and getattr(n.test.left, "id", "") == "S")
    assert (branch.lineno, branch.end_lineno) == (283, 293)
    code = compile(ast.Module(body=[branch], type_ignores=[]), path, "exec")

    def reference(xyz1, xyz2, points2):
        ns = {"torch": torch, "square_distance": square_distance, "index_points": index_points, "xyz1": xyz1, "xyz2": xyz2, "points2": points2,
              "B": xyz1.shape[0], "N": xyz1.shape[1], "S": xyz2.shape[1]}
        exec(code, ns)
        return ns["interpolated_points"], ns.get("idx"), ns.get("weight")

    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)

    def clouds(b, n):
        raw = rng.randn(b, n, 3) * np.array([1.0, 0.8, 0.6]) + np.array([0.3, -1.0, 2.0])
        pc = np.stack([pc_normalize(c)[0] for c in raw])
        return torch.tensor(pc / np.linalg.norm(pc, axis=-1).max(1)[:, None, None]).float()

    arrays = {}
    for k, (kind, b, n, s) in enumerate(ref.CASES):
        if kind == "subset":
            xyz1, feat = arrays["xyz1_0"], arrays["feat_0"]
            fps = farthest_point_sample(xyz1, s)
            xyz2 = index_points(xyz1, fps)
            arrays["fps_%d" % k] = fps.numpy().astype(np.uint16)
        else:
            both = clouds(b, n + s)
            xyz1, xyz2 = both[:, :n].contiguous(), both[:, n:].contiguous()
            feat = torch.randn(b, s, ref.D_FIXTURE)
            arrays["xyz1_%d" % k], arrays["xyz2_%d" % k], arrays["feat_%d" % k] = xyz1, xyz2, feat
        out, idx, weight = reference(xyz1, xyz2, feat)
        assert out.shape == (b, n, ref.D_FIXTURE) and out.dtype == torch.float32
        d3, want, w = ref.three_nn(xyz1.numpy(), xyz2.numpy())
        tie, zero = ref.masks(xyz1.numpy(), xyz2.numpy())
        ref_idx = np.zeros((b, n, 3), np.int64) if idx is None else idx.numpy()
        differ = (ref_idx != want).any(-1)
        assert not (differ & ~tie).any(), "the reference's indices differ from the restatement's outside near_tie"
        assert tie.mean() <= ref.MASK_CAP, (k, tie.mean())
        arrays["ref_idx_%d" % k], arrays["near_tie_%d" % k], arrays["near_zero_%d" % k] = ref_idx.astype(np.uint16), tie, zero
        line = "g24 %s %dx%d<-%d: near_tie %.2f %%, near_zero %.2f %%, either %.2f %%, %d rows differ" % (
            kind, b, n, s, 100 * tie.mean(), 100 * zero.mean(), 100 * (tie | zero).mean(), differ.sum())
        if kind == "subset":
            negative = int((weight < 0).any(-1).sum())
            arrays["ref_negative_weights_%d" % k] = np.int64(negative)
            line += "; the reference has a negative weight in %d of %d rows" % (negative, b * n)
        else:
            if kind == "disjoint":
                assert (tie | zero).mean() <= ref.MASK_CAP, (k, (tie | zero).mean())
            keep = ~(tie | zero)
            dev = float(np.abs(out.numpy().astype(np.float64) - ref.interpolate(feat.numpy(), want, w)[0])[keep].max())
            arrays["ref_out_%d" % k], arrays["ref_dev_%d" % k] = out, np.float64(dev)
            line += "; ref_dev %.3g" % dev
        print(line)
    save("g24_three_nn.npz", **arrays)


def g25_grouping(seed=25):
    """group_points: the reference's own CLASSES on the CPU, torch seeded -- PointNetSetAbstraction (group_all false and true) and
    PointNetSetAbstractionMsg (two radii) of point_cloud/pointnet_utils.py, constructed with EMPTY MLP lists, so the tensor entering
    torch.max(., 2) is exactly the permuted grouped tensor (B, C, K, S).  While a forward runs, torch.max and the module's
    farthest_point_sample and query_ball_point are wrapped to record that tensor T, the FPS indices (their first column is the
    start), every idx and new_xyz; nothing of the reference is retyped.  Recorded beside them: the reference's own autograd gradients
    of sum_i (T_i * G_i).sum() with respect to xyz (B, 3, N) and points (B, D, N), G_i = tests/grouping_ref.py: seeded_g(i, T_i.shape)
    (regenerated by the tests, not stored).  2 x 256 points, 64 centres, D = 5, (r, K) = (0.2, 16) and (0.4, 32) (the single-scale
    layer takes the second) on pc_normalize'd clouds scaled to radius 1; 2 x 40 points for group_all.  Asserted here: no recorded idx
    holds N (every centre is a cloud point and hits itself)."""
    import importlib.util
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import grouping_ref as ref
    spec = importlib.util.spec_from_file_location("reference_pointnet_utils", os.path.join(REF, "point_cloud", "pointnet_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (pc_normalize,) = functions_from(os.path.join(REF, "point_cloud", "prepare.py"), ["pc_normalize"])
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)

    def clouds(b, n):
        raw = rng.randn(b, n, 3) * np.array([1.0, 0.8, 0.6]) + np.array([0.3, -1.0, 2.0])
        pc = np.stack([pc_normalize(c)[0] for c in raw])
        return torch.tensor(pc / np.linalg.norm(pc, axis=-1).max(1)[:, None, None]).float()

    def run(layer, xyz, points):
        """-> (new_xyz (B, 3, S), [T_i], [fps], [idx_i], grad_xyz (B, 3, N), grad_points (B, D, N))"""
        rec = {"t": [], "fps": [], "idx": []}
        real_max, real_fps, real_ball = torch.max, mod.farthest_point_sample, mod.query_ball_point

        def max_(x, *a, **k):
            if x.dim() == 4:                        # the layer's own call; farthest_point_sample's argmax is (B, N)
                rec["t"].append(x)
            return real_max(x, *a, **k)

        def fps_(*a, **k):
            rec["fps"].append(real_fps(*a, **k))
            return rec["fps"][-1]

        def ball_(*a, **k):
            rec["idx"].append(real_ball(*a, **k).clone())
            return rec["idx"][-1].clone()

        x, p = xyz.transpose(1, 2).contiguous().requires_grad_(True), points.transpose(1, 2).contiguous().requires_grad_(True)
        torch.max, mod.farthest_point_sample, mod.query_ball_point = max_, fps_, ball_
        try:
            new_xyz, _ = layer(x, p)
        finally:
            torch.max, mod.farthest_point_sample, mod.query_ball_point = real_max, real_fps, real_ball
        sum((t * torch.tensor(ref.seeded_g(i, tuple(t.shape)))).sum() for i, t in enumerate(rec["t"])).backward()
        return new_xyz.detach(), [t.detach() for t in rec["t"]], rec["fps"], rec["idx"], x.grad, p.grad

    n, s, d = ref.N_FIXTURE, ref.S_FIXTURE, ref.D_FIXTURE
    xyz, points = clouds(2, n), torch.randn(2, n, d)
    arrays = {"xyz": xyz, "points": points}
    (r0, k0), (r1, k1) = ref.RADII
    layers = {"sa": mod.PointNetSetAbstraction(s, r1, k1, 3 + d, [], False), "msg": mod.PointNetSetAbstractionMsg(s, [r0, r1], [k0, k1], d, [[], []])}
    for tag, layer in layers.items():
        new_xyz, ts, fps, idxs, gx, gp = run(layer, xyz, points)
        assert len(fps) == 1 and len(ts) == len(idxs) == (1 if tag == "sa" else 2)
        arrays["fps_" + tag], arrays["new_xyz_" + tag] = fps[0].numpy().astype(np.uint16), new_xyz
        arrays["grad_xyz_" + tag], arrays["grad_points_" + tag] = gx, gp
        for i, (t, idx) in enumerate(zip(ts, idxs)):
            assert t.shape == (2, 3 + d, idx.shape[2], s) and t.dtype == torch.float32
            assert int(idx.max()) < n and int(idx.min()) >= 0, "a recorded idx holds N"
            arrays["t_%s_%d" % (tag, i)], arrays["idx_%s_%d" % (tag, i)] = t.contiguous(), idx.numpy().astype(np.uint16)
            print("g25 %s radius %d: K = %d, %.1f %% of the slots are padding" % (
                tag, i, idx.shape[2], 100 * float((idx[:, :, 1:] == idx[:, :, :1]).float().mean())))
    xyz_all, points_all = clouds(2, ref.N_ALL), torch.randn(2, ref.N_ALL, d)
    new_xyz, ts, fps, idxs, gx, gp = run(mod.PointNetSetAbstraction(None, None, None, 3 + d, [], True), xyz_all, points_all)
    assert not fps and not idxs and len(ts) == 1 and ts[0].shape == (2, 3 + d, ref.N_ALL, 1)
    arrays.update(xyz_all=xyz_all, points_all=points_all, new_xyz_all=new_xyz, t_all=ts[0].contiguous(), grad_xyz_all=gx, grad_points_all=gp)
    save("g25_grouping.npz", **arrays)
    assert os.path.getsize(os.path.join(OUT, "g25_grouping.npz")) <= 512 * 1024


def g23_head_edges():
    """The forward heads at their edges (tests/heads_ref.py: every family, every fourth row -- 32 of 128): the reference's own float32
    outputs and autograd gradients, float64 too where the reference's code keeps float64 (not the 5D head: float32 zeros, :82; not
    calculate_T_pred: .float(), utility.py:123).  Shows that oracle/so3_oracle.py's float64 restatement takes the reference's clamps
    (max(|q|, 1e-8), clamp(|v|^2, 1e-4)) at the edges G10's randn rows never reach."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import heads_ref as hr
    heads = {"quat": rr.compute_rotation_matrix_from_quaternion, "euler": rr.compute_rotation_matrix_from_euler,
             "ortho5d": rr.compute_rotation_matrix_from_ortho5d, "expmap": rr.vec_3d_to_SO3, "ortho6d": rr.compute_rotation_matrix_from_ortho6d}
    out = {}
    for name, fn in heads.items():
        d = hr.data(name)
        rows = np.arange(0, len(d["x"]), 4)
        x, g = torch.as_tensor(d["x"][rows].copy()), torch.as_tensor(d["g"][rows].copy()).view(-1, 3, 3)
        xf = x.clone().requires_grad_(True)
        r = fn(xf)
        r.backward(g)
        out.update({name + "_rows": rows.astype(np.int32), name + "_x": x, name + "_r": r.detach().reshape(-1, 9), name + "_dx": xf.grad})
        if name != "ortho5d":
            xd = x.double().requires_grad_(True)
            rd = fn(xd)
            rd.backward(g.double())
            assert rd.dtype == torch.float64
            out.update({name + "_r_f64": rd.detach().reshape(-1, 9), name + "_dx_f64": xd.grad})

    def combine(R, tx, ty, tz, device="cpu"):                 # see g8_se3_update
        T = torch.ones((R.shape[0], 4, 4))
        T[:, :3, :3] = R
        T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = tx, ty, tz
        T[:, 3, :3] = 0
        return T
    calc, scene = functions_from(os.path.join(REF, "Iterative", "utility.py"), ["calculate_T_pred", "get_scene_parameters"])
    calc.__globals__.update(symmetric_orthogonalization=rr.symmetric_orthogonalization, combine=combine, get_scene_parameters=scene)
    d = hr.data("se3_update")
    rows = np.arange(0, len(d["x"]), 4)
    o = torch.as_tensor(d["x"][rows].copy()).requires_grad_(True)
    tp = calc(o, torch.as_tensor(d["t"][rows].copy()).view(-1, 4, 4), "cpu")
    tp.backward(torch.as_tensor(d["g"][rows].copy()).view(-1, 4, 4))
    assert abs(scene()[0] - hr.FX) < 1e-9 and abs(scene()[1] - hr.FY) < 1e-9
    out.update(se3_update_rows=rows.astype(np.int32), se3_update_x=o.detach(), se3_update_r=tp.detach().reshape(-1, 16), se3_update_dx=o.grad)
    save("g23_head_edges.npz", **out)


def g27_chamfer():
    """chamfer_distance: no reference code exists, so the fixture holds the inputs (clouds of unit radius at every work split, ragged
    lengths with an empty source, an empty target and a one-point target, X inside Y with duplicates, 2500 points whose nearest
    neighbour is ONE point) and the float64 restatement's indices and rows -- tests/chamfer_ref.py: generate, which asserts that no
    non-zero nearest distance lies below MIN_DISTANCE."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import chamfer_ref as ref
    arrays = ref.generate()
    save("g27_chamfer.npz", **arrays)
    assert os.path.getsize(os.path.join(OUT, "g27_chamfer.npz")) <= os.path.getsize(os.path.join(OUT, "g21_icp.npz"))


def g28_knn():
    """knn_points: no reference code exists, so the fixture holds the inputs (clouds of unit radius at the shapes of tests/knn_ref.py:
    SHAPES, each full and ragged -- an empty source, an empty target, a one-point target and a target shorter than K -- and the exact
    families: X inside Y with duplicates, an all-equal target, lattice points with exact ties, many-to-one) and the float32
    restatement's outputs -- tests/knn_ref.py: generate, which asserts the float64 excess bound on every case."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import knn_ref as ref
    save("g28_knn.npz", **ref.generate())
    assert os.path.getsize(os.path.join(OUT, "g28_knn.npz")) <= 512 * 1024


def g29_local_frames():
    """local_frames: no reference code exists, so the fixture holds the inputs (clouds of unit radius, their index rows, lengths and
    viewpoints: the surface families at tests/local_frames_ref.py: SURFACE_SHAPES and at K = 3, the sphere shifted by 100, the exact
    lattice plane, collinear points, the octahedron and the cube, all-equal neighbours, r = 1 and r = 2, rows whose valid slots are
    no prefix, ragged lengths, a viewpoint inside and one outside the sphere) and the outputs of the float32 restatement of the
    covariance and of float64 numpy.linalg.eigh -- tests/local_frames_ref.py: generate, which asserts the covariance's bound against
    float64 and the share of small-gap rows on every case."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import local_frames_ref as ref
    save("g29_local_frames.npz", **ref.generate())
    assert os.path.getsize(os.path.join(OUT, "g29_local_frames.npz")) <= 512 * 1024


def g30_icp_plane():
    """icp_align_plane: no reference code exists, so the fixture holds float32 clouds, normals (stored, or the analytic ellipsoid
    normals tests/icp_plane_ref.py derives from the target), initial poses and weights, and the answers of the float64 restatement
    -- tests/icp_plane_ref.py: generate, which asserts the trimming margins, the share of non-unique steps, the degenerate systems,
    exact convergence and the comparison case's property."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import icp_plane_ref as ref
    save("g30_icp_plane.npz", **ref.generate())
    assert os.path.getsize(os.path.join(OUT, "g30_icp_plane.npz")) <= 512 * 1024


def g31_chamfer_normals():
    """Chamfer's normal term: no reference code exists, so the fixture holds float32 clouds and normals at every work split (ragged
    lengths as G27's) in seven families and the float64 search's indices -- tests/chamfer_normals_ref.py: generate, which redraws a
    normal whose cosine through those indices lies in (0, MIN_COSINE).  The float64 expectations are re-formed from these on load."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import chamfer_normals_ref as ref
    save("g31_chamfer_normals.npz", **ref.generate())
    assert os.path.getsize(os.path.join(OUT, "g31_chamfer_normals.npz")) <= 512 * 1024


def g32_fpfh():
    """fpfh_features: no reference code exists, so the fixture holds float32 clouds, normals and index rows (tests/fpfh_ref.py: the
    sphere and the blob at SURFACE_SHAPES, the exact lattices, coincident points, zero normals, rows with invalid, missing and repeated
    indices, K = 1, 2, 3, K > n_b, ragged lengths, non-finite values, and the moved copies) and the float64 counts -- tests/fpfh_ref.py:
    generate, which redraws points until the margin condition holds and asserts every family's premise.  The expectations are
    re-formed from the counts on load."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import fpfh_ref as ref
    save("g32_fpfh.npz", **ref.generate())
    assert os.path.getsize(os.path.join(OUT, "g32_fpfh.npz")) <= 512 * 1024


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "g32":
        return g32_fpfh()
    if len(sys.argv) > 1 and sys.argv[1] == "g31":
        return g31_chamfer_normals()
    if len(sys.argv) > 1 and sys.argv[1] == "g30":
        return g30_icp_plane()
    if len(sys.argv) > 1 and sys.argv[1] == "g29":
        return g29_local_frames()
    if len(sys.argv) > 1 and sys.argv[1] == "g28":
        return g28_knn()
    if len(sys.argv) > 1 and sys.argv[1] == "g27":
        return g27_chamfer()
    if len(sys.argv) > 1 and sys.argv[1] == "g26":
        return g26_sym_add()
    if len(sys.argv) > 1 and sys.argv[1] == "g25":
        return g25_grouping()
    if len(sys.argv) > 1 and sys.argv[1] == "g24":
        return g24_three_nn()
    if len(sys.argv) > 1 and sys.argv[1] == "g23":
        return g23_head_edges()
    if len(sys.argv) > 1 and sys.argv[1] == "g22":
        return g22_pointnet()
    if len(sys.argv) > 1 and sys.argv[1] == "g21":
        return g21_icp()
    if len(sys.argv) > 1 and sys.argv[1] == "g20":
        return g20_rigid_align()
    if len(sys.argv) > 1 and sys.argv[1] == "g19":
        return g19_add_metrics()
    if len(sys.argv) > 1 and sys.argv[1] == "g18":
        return g18_inverse_maps()
    if len(sys.argv) > 1 and sys.argv[1] == "g17":
        return g17_symmetry()
    if len(sys.argv) > 1 and sys.argv[1] == "g16":
        return g16_cloud_gradients()
    if len(sys.argv) > 1 and sys.argv[1] == "g15":
        return g15_metric_gradients()
    if len(sys.argv) > 1 and sys.argv[1] == "g14":
        return g14_geodesic_reduction()
    if len(sys.argv) > 1 and sys.argv[1] == "g13":
        return g13_dtype_fidelity()
    if len(sys.argv) > 1 and sys.argv[1] == "g9":
        return g9_sampler()
    if len(sys.argv) > 1 and sys.argv[1] == "g7":        # regenerate one fixture without touching the others
        return g7_ortho6d()
    if len(sys.argv) > 1 and sys.argv[1] == "g8":
        return g8_se3_update()
    if len(sys.argv) > 1 and sys.argv[1] == "g10":
        return g10_heads()
    if len(sys.argv) > 1 and sys.argv[1] == "g11":
        return g11_add_l1()
    if len(sys.argv) > 1 and sys.argv[1] == "g12":
        return g12_clouds()
    g7_ortho6d()
    g8_se3_update()
    g9_sampler()
    g10_heads()
    g11_add_l1()
    g12_clouds()
    g13_dtype_fidelity()
    g19_add_metrics()
    g26_sym_add()
    g20_rigid_align()
    g21_icp()
    g27_chamfer()
    g28_knn()
    g29_local_frames()
    g30_icp_plane()
    g31_chamfer_normals()
    g32_fpfh()
    g22_pointnet()
    g23_head_edges()
    # ---- G1: config #1, 256 Gaussian rows ------------------------------------------------------
    torch.manual_seed(0)
    x = torch.randn(256, 9)
    r = rr.symmetric_orthogonalization(x)
    s, det = svd_parts(x)
    r64 = rr.symmetric_orthogonalization(x.double())
    save("g1_gaussian256.npz", x=x, r=r, s=s, det=det, r_f64=r64)

    # ---- G2: adversarial inputs ------------------------------------------------------------------
    torch.manual_seed(2)
    q = rr.symmetric_orthogonalization(torch.randn(4, 9))
    cases, names = [], []

    def add(name, m):
        names.append(name)
        cases.append(torch.as_tensor(m, dtype=torch.float32).reshape(3, 3))
    add("zero", torch.zeros(3, 3))
    add("identity", torch.eye(3))
    add("reflection_z", torch.diag(torch.tensor([1., 1., -1.])))
    add("neg_identity", -torch.eye(3))
    add("rank1_e1", torch.diag(torch.tensor([2., 0., 0.])))
    add("rank1_ones", torch.ones(3, 3))
    add("rank2_diag", torch.diag(torch.tensor([1., 1., 0.])))
    add("rank2_rot", q[0] @ torch.diag(torch.tensor([3., 0.5, 0.])) @ q[1].T)
    add("rotation", q[2])
    add("rotation_scaled_1e-20", q[2] * 1e-20)
    add("rotation_scaled_1e+15", q[2] * 1e15)
    add("improper_rotation", q[3] @ torch.diag(torch.tensor([1., 1., -1.])))
    add("near_equal_sv", q[0] @ torch.diag(torch.tensor([1.0, 1.0 - 1e-6, 1.0 - 2e-6])) @ q[1].T)
    add("near_equal_sv_flip", q[0] @ torch.diag(torch.tensor([1.0, 0.7, -0.3])) @ q[1].T)
    add("flip_close_s2_s3", q[0] @ torch.diag(torch.tensor([1.0, 0.5, -0.499])) @ q[1].T)
    add("tiny_s3_pos", q[2] @ torch.diag(torch.tensor([1.0, 0.5, 1e-6])) @ q[3].T)
    add("tiny_s3_neg", q[2] @ torch.diag(torch.tensor([1.0, 0.5, -1e-6])) @ q[3].T)
    add("graded", q[1] @ torch.diag(torch.tensor([1e3, 1.0, 1e-3])) @ q[0].T)
    add("upper_triangular", torch.tensor([[1., 2., 3.], [0., 4., 5.], [0., 0., 6.]]))
    add("permutation_odd", torch.tensor([[0., 1., 0.], [1., 0., 0.], [0., 0., 1.]]))
    add("permutation_even", torch.tensor([[0., 1., 0.], [0., 0., 1.], [1., 0., 0.]]))
    xa = torch.stack(cases).reshape(-1, 9)
    ra = rr.symmetric_orthogonalization(xa)
    sa, deta = svd_parts(xa)
    save("g2_adversarial.npz", x=xa, r=ra, s=sa, det=deta, names=np.array(names),
         r_f64=rr.symmetric_orthogonalization(xa.double()))
    # view semantics: any shape with numel % 9 == 0 (rotation_representation.py:199)
    torch.manual_seed(3)
    xs = torch.randn(2, 5, 9)
    save("g2_shape_2x5x9.npz", x=xs, r=rr.symmetric_orthogonalization(xs))

    # ---- G3: angle_error / geodesic ----------------------------------------------------------------
    torch.manual_seed(4)
    r1 = rr.symmetric_orthogonalization(torch.randn(256, 9))
    r2 = rr.symmetric_orthogonalization(torch.randn(256, 9))
    r2[0] = r1[0]                                                   # 0 degrees
    r2[1] = r1[1] @ torch.diag(torch.tensor([1., -1., -1.]))        # 180 degrees
    r2[2] = r1[2] @ torch.diag(torch.tensor([-1., -1., 1.]))        # 180 degrees
    small = rr.so3_exp_map(torch.tensor([[1e-4, 0., 0.], [0., 3e-3, 0.]])) if hasattr(rr, "so3_exp_map") else None
    if small is not None and small.shape == (2, 3, 3):
        r2[3] = r1[3] @ small[0].float()
        r2[4] = r1[4] @ small[1].float()
    deg = rr.angle_error(r1, r2)
    rad = rr.compute_geodesic_distance_from_two_matrices(r1, r2)
    bad1 = torch.eye(3).repeat(3, 1, 1)
    bad2 = torch.eye(3).repeat(3, 1, 1)
    bad2[1] = 1.5 * torch.eye(3)          # trace 4.5 -> cos 1.75 > 1.1 : must raise
    raised = False
    try:
        rr.angle_error(bad1, bad2)
    except ValueError as exc:
        raised = True
        msg = str(exc)
    assert raised
    nearly = torch.eye(3).repeat(2, 1, 1)
    nearly2 = nearly.clone()
    nearly2[1] = 1.05 * torch.eye(3)      # cos = 1.075: inside the tolerance band, clamped, no raise
    deg_nearly = rr.angle_error(nearly, nearly2)
    save("g3_angles.npz", r1=r1, r2=r2, deg=deg, rad=rad, bad1=bad1, bad2=bad2, raise_msg=np.array(msg),
         nearly1=nearly, nearly2=nearly2, deg_nearly=deg_nearly)

    # ---- G4: config #4, 512 rows bf16-rounded, Frobenius loss forward + backward ------------------
    torch.manual_seed(0)
    x4 = torch.randn(512, 9).bfloat16()
    torch.manual_seed(1)
    rt = rr.symmetric_orthogonalization(torch.randn(512, 9))
    xf = x4.float().requires_grad_(True)
    out = rr.symmetric_orthogonalization(xf)
    loss = loss_frobenius(rt, out)                      # call order of 3D-Pose/main.py:85 (R, out)
    loss.backward()
    # generic upstream gradient through the head alone (K2)
    torch.manual_seed(5)
    g = torch.randn(512, 3, 3)
    xg = x4.float().requires_grad_(True)
    rr.symmetric_orthogonalization(xg).backward(g)
    # float64 versions of both gradients (the reference code, double input)
    xd = x4.double().requires_grad_(True)
    lossd = loss_frobenius(rt.double(), rr.symmetric_orthogonalization(xd))
    lossd.backward()
    xgd = x4.double().requires_grad_(True)
    rr.symmetric_orthogonalization(xgd).backward(g.double())
    save("g4_frobenius512.npz", x_bf16_bits=x4.view(torch.int16), r_true=rt, r=out.detach(), loss=loss.detach(),
         dx=xf.grad, g=g, dx_g=xg.grad, loss_f64=lossd.detach(), dx_f64=xd.grad, dx_g_f64=xgd.grad)

    # ---- G5: Kabsch pairs (config #3 contract), 6 clouds x 1024 + 24 clouds x 64 --------------------
    for tag, (b, n) in {"6x1024": (6, 1024), "24x64": (24, 64)}.items():
        torch.manual_seed(7)
        np.random.seed(7)
        p = torch.rand(b, n, 3) - 0.5
        r_gt = sample_rot(b)                                         # point_cloud/prepare.py:21-49
        qpts = torch.bmm(r_gt, p.transpose(1, 2)).transpose(1, 2).contiguous()   # point_cloud/main.py:176-181
        qn = qpts + 0.01 * torch.randn(b, n, 3)
        h = torch.bmm(qn.transpose(1, 2), p)
        save("g5_kabsch_%s.npz" % tag, p=p, q=qn, r_gt=r_gt, h=h, r=rr.symmetric_orthogonalization(h),
             r_f64=rr.symmetric_orthogonalization(torch.bmm(qn.double().transpose(1, 2), p.double())))

    # ---- G6: scalar statistics at config #2's full size (inputs regenerated from the seeds) -------
    torch.set_num_threads(8)
    torch.manual_seed(0)
    xb = torch.randn(1_000_000, 9)
    torch.manual_seed(1)
    tb = rr.symmetric_orthogonalization(torch.randn(1_000_000, 9))
    rb = rr.symmetric_orthogonalization(xb)
    sb, detb = svd_parts(xb)
    ang = rr.angle_error(rb, tb)
    rb64 = rr.symmetric_orthogonalization(xb.double())
    ang64 = rr.angle_error(rb64, tb.double())
    orth = torch.linalg.matrix_norm(rb.transpose(1, 2) @ rb - torch.eye(3), ord="fro")
    save("g6_stats_1m.npz", n=1_000_000, seed_x=0, seed_t=1,
         mean_angle_deg=ang.mean(), mean_angle_deg_f64=ang64.mean(),
         flip_count=(detb < 0).sum(), max_orth_err=orth.max(),
         x_head=xb[:64], r_head=rb[:64], t_head=tb[:64], x_checksum=xb.double().sum(), t_checksum=tb.double().sum(),
         flip_bits=np.packbits((detb < 0).numpy()))


if __name__ == "__main__":
    main()
