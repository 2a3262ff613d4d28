#!/usr/bin/env python3
"""Times every C-ABI entry point at the BASELINE.json configs (secondary kernels; bench.py is the headline).
Each call is launched back-to-back on rotating buffers; reported per call with the algorithmic bytes it moves."""
import ctypes, math, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from poseestimation_amd import _lib
from poseestimation_amd import rotation_representation as rr

P = ctypes.c_void_p
dev = torch.device("cuda:0")
if os.environ.get("SO3_LIB"):                    # another build of the library (tools/build_variant.sh), for A/B runs
    _lib.LIB_PATH = os.path.abspath(os.environ["SO3_LIB"])
lib = _lib.load()
ONLY = os.environ.get("SO3_BENCH_ONLY")          # time only the lines whose name contains this
st = P(torch.cuda.current_stream().cuda_stream)
NB = 6


QUICK = os.environ.get("SO3_BENCH_QUICK") == "1"      # 2 calls per entry: for rocprofv3 --pmc passes (kernels are serialised)


def timeit(name, fn, bytes_per_call, iters=60, warm=5):
    if ONLY and ONLY not in name:
        return
    if QUICK:
        iters, warm = 2, 1
    us = float("inf")
    for rep in range(1 if QUICK else 3):          # the best of three blocks: a line's first block reads up to 2 us high after a line of another kernel
        for i in range(warm): fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters): fn(i)
        e1.record(); torch.cuda.synchronize()
        us = min(us, e0.elapsed_time(e1) / iters * 1e3)
    print("%-58s %9.2f us/call  %7.0f GB/s (%4.1f%% of 8 TB/s)" % (name, us, bytes_per_call / us * 1e-3, bytes_per_call / us * 1e-3 / 80))


def main():
    n = 1_000_000
    x = [torch.randn(n, 9, device=dev) for _ in range(NB)]
    xb = [t.bfloat16() for t in x]
    g = [torch.randn(n, 9, device=dev) for _ in range(NB)]
    r = [torch.empty(n, 9, device=dev) for _ in range(NB)]
    dm = [torch.empty(n, 9, device=dev) for _ in range(NB)]
    dmb = [torch.empty(n, 9, device=dev, dtype=torch.bfloat16) for _ in range(NB)]
    rt = [rr.symmetric_orthogonalization(torch.randn(n, 9, device=dev)).reshape(n, 9) for _ in range(NB)]
    flip = torch.empty(n, dtype=torch.uint8, device=dev)
    ls = torch.empty(1, dtype=torch.float64, device=dev)
    deg = torch.empty(n, dtype=torch.float64, device=dev)
    th = torch.empty(n, dtype=torch.float32, device=dev)
    sc = torch.empty(2, dtype=torch.float64, device=dev)
    fl = torch.empty(1, dtype=torch.int32, device=dev)
    p = lambda t: P(t.data_ptr())
    # the chip's clock needs tens of milliseconds of load to come up: keep it busy for ~80 ms before the first line
    import time
    t_warm = time.perf_counter()
    while time.perf_counter() - t_warm < 0.08:
        for i in range(64):
            lib.so3_project_fwd_f32(p(x[i % NB]), p(r[i % NB]), None, n, st)
        torch.cuda.synchronize()
    print("--- 1M rows (config #2 shape) ---")
    timeit("K1 so3_project_fwd_f32", lambda i: lib.so3_project_fwd_f32(p(x[i % NB]), p(r[i % NB]), None, n, st), 72 * n)
    timeit("K1 so3_project_fwd_f32 + flip flags", lambda i: lib.so3_project_fwd_f32(p(x[i % NB]), p(r[i % NB]), p(flip), n, st), 73 * n)
    timeit("K1 so3_project_fwd_bf16 (bf16 in, f32 out)", lambda i: lib.so3_project_fwd_bf16(p(xb[i % NB]), p(r[i % NB]), None, n, st), 54 * n)
    timeit("K2 so3_project_bwd_f32", lambda i: lib.so3_project_bwd_f32(p(x[i % NB]), p(g[i % NB]), p(dm[i % NB]), n, st), 108 * n)
    timeit("K2 so3_project_bwd_bf16", lambda i: lib.so3_project_bwd_bf16(p(xb[i % NB]), p(g[i % NB]), p(dmb[i % NB]), n, st), 72 * n)
    # the reducing entry points exist once (round 4): workspace nullable, a flags word.  "atomics" = no workspace (a zero-fill launch in front,
    # one atomic per workgroup behind); "workspace" = caller-owned, one launch, what the Python mirror passes for K3 / K3';
    # "zeroed slots" = SO3_PREZEROED, one launch, what the mirror passes for the metrics
    ws = torch.zeros(lib.so3_reduce_workspace_bytes(), dtype=torch.uint8, device=dev)
    lm = torch.empty((), dtype=torch.float32, device=dev)
    pool = torch.zeros(4096, 4, dtype=torch.float64, device=dev)
    slot = lambda i: (P(pool[i % 4096].data_ptr()), P(pool[i % 4096].data_ptr() + 16))
    PZ, EX = _lib.PREZEROED, _lib.EXACT_F64
    k3, k3p, k4, k14 = lib.so3_frob_fwd_bwd_v2_f32, lib.so3_frob_loss_v2_f32, lib.so3_angle_error_v2, lib.so3_project_angle_error_v2_f32
    timeit("K3 so3_frob_fwd_bwd_v2_f32 (R + dM + loss, atomics)", lambda i: k3(p(x[i % NB]), p(rt[i % NB]), p(r[i % NB]), p(dm[i % NB]), p(ls), None, None, 0, n, st), 144 * n)
    timeit("K3 so3_frob_fwd_bwd_v2_f32 (dM + loss, atomics)", lambda i: k3(p(x[i % NB]), p(rt[i % NB]), None, p(dm[i % NB]), p(ls), None, None, 0, n, st), 108 * n)
    timeit("K3 so3_frob_fwd_bwd_v2_f32 (R + dM + loss + mean, workspace)", lambda i: k3(p(x[i % NB]), p(rt[i % NB]), p(r[i % NB]), p(dm[i % NB]), p(ls), p(lm), p(ws), 0, n, st), 144 * n)
    timeit("K3 so3_frob_fwd_bwd_v2_f32 (dM + loss + mean, workspace)", lambda i: k3(p(x[i % NB]), p(rt[i % NB]), None, p(dm[i % NB]), p(ls), p(lm), p(ws), 0, n, st), 108 * n)
    timeit("K3' so3_frob_loss_v2_f32 (loss + dRpred, atomics)", lambda i: k3p(p(r[i % NB]), p(rt[i % NB]), p(dm[i % NB]), p(ls), None, None, 0, n, st), 108 * n)
    timeit("K3' so3_frob_loss_v2_f32 (loss + dRpred + mean, workspace)", lambda i: k3p(p(r[i % NB]), p(rt[i % NB]), p(dm[i % NB]), p(ls), p(lm), p(ws), 0, n, st), 108 * n)
    timeit("K4 so3_angle_error_v2 (per-row deg)", lambda i: k4(p(r[i % NB]), p(rt[i % NB]), p(deg), None, p(fl), None, 0, n, st), 80 * n)
    timeit("K4 so3_angle_error_v2 (sum,count, zeroed slots)", lambda i: k4(p(r[i % NB]), p(rt[i % NB]), None, slot(i)[0], slot(i)[1], None, PZ, n, st), 72 * n)
    timeit("K4 so3_angle_error_v2 (sum,count, init launch + atomics)", lambda i: k4(p(r[i % NB]), p(rt[i % NB]), None, p(sc), p(fl), None, 0, n, st), 72 * n)
    timeit("K1+K4 so3_project_angle_error_v2_f32 (sum: f32 outside the band, zeroed slots)", lambda i: k14(p(x[i % NB]), p(rt[i % NB]), None, None, slot(i)[0], slot(i)[1], None, PZ, n, st), 72 * n)
    timeit("K1+K4 so3_project_angle_error_v2_f32 (sum: float64 on every row, zeroed slots)", lambda i: k14(p(x[i % NB]), p(rt[i % NB]), None, None, slot(i)[0], slot(i)[1], None, PZ | EX, n, st), 72 * n)
    timeit("K1+K4 so3_project_angle_error_v2_f32 (sum: f32 outside the band, workspace)", lambda i: k14(p(x[i % NB]), p(rt[i % NB]), None, None, p(sc), p(fl), p(ws), 0, n, st), 72 * n)
    timeit("K1+K4 so3_project_angle_error_v2_f32 (per-row deg: float64)", lambda i: k14(p(x[i % NB]), p(rt[i % NB]), None, p(deg), None, p(fl), None, 0, n, st), 80 * n)
    # float64 arguments (the reference's metric casts to double itself; callers that already hold double rotations): one launch with the workspace
    r64 = [t.double() for t in rt[:2]]
    g64 = torch.empty(n, 9, dtype=torch.float64, device=dev)
    lm64 = torch.empty((), dtype=torch.float64, device=dev)
    timeit("K4 f64 so3_angle_error_v2_f64 (sum,count, workspace: one launch)", lambda i: lib.so3_angle_error_v2_f64(p(r64[i % 2]), p(r64[1 - i % 2]), None, p(sc), p(fl), p(ws), 0, n, st), 144 * n)
    timeit("K4 f64 so3_angle_error_v2_f64 (sum,count, no workspace: init + kernel)", lambda i: lib.so3_angle_error_v2_f64(p(r64[i % 2]), p(r64[1 - i % 2]), None, p(sc), p(fl), None, 0, n, st), 144 * n)
    timeit("K4 f64 so3_angle_error_v2_f64 (per-row deg)", lambda i: lib.so3_angle_error_v2_f64(p(r64[i % 2]), p(r64[1 - i % 2]), p(deg), None, p(fl), p(ws), 0, n, st), 152 * n)
    timeit("K3' f64 so3_frob_loss_v2_f64 (loss + dRpred, workspace: one launch)", lambda i: lib.so3_frob_loss_v2_f64(p(r64[i % 2]), p(r64[1 - i % 2]), p(g64), p(ls), p(lm64), p(ws), 0, n, st), 216 * n)
    timeit("K4' geodesic(R1, R2, 'mean') so3_geodesic_eps_f32 (workspace: one launch)", lambda i: lib.so3_geodesic_eps_f32(p(r[i % NB]), p(rt[i % NB]), None, p(ls), p(lm), 1, ctypes.c_float(1e-7), p(ws), n, st), 72 * n)
    timeit("K4' geodesic(R1, R2, 'mean') so3_geodesic_eps_f32 (no workspace: memset + kernel + mean)", lambda i: lib.so3_geodesic_eps_f32(p(r[i % NB]), p(rt[i % NB]), None, p(ls), p(lm), 1, ctypes.c_float(1e-7), None, n, st), 72 * n)
    # K4s / K3s: the metric and the loss up to a symmetry group, single-class tables of K = 1, 4, 24 and ten classes of K = 1 .. 8 (padded to 8)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cls10 = torch.randint(0, 10, (n,), device=dev, dtype=torch.int32)
    sym_tables = [("K=%d" % k, rr.SymmetryTable(rr.cyclic_symmetry(k, "y")), None) for k in (1, 4, 24)]
    sym_tables.append(("10 classes, K=1..8", rr.SymmetryTable([rr.cyclic_symmetry(k, "z") for k in range(1, 9)] + [rr.cyclic_symmetry(2, "x")] * 2), cls10))
    for tag, tab, cl in sym_tables:
        sd, cp, extra = tab._on(dev), (p(cl) if cl is not None else None), (4 * n if cl is not None else 0)
        timeit("K4s so3_sym_angle_error_f32 (%s, deg + index + flags)" % tag,
               lambda i: lib.so3_sym_angle_error_f32(p(r[i % NB]), p(rt[i % NB]), p(sd), cp, tab.num_classes, tab.K, p(deg), p(idx), p(fl), 0, n, st),
               84 * n + extra)
        timeit("K3s so3_sym_frob_loss_f32 (%s, loss + dRpred + dRtrue + mean, workspace)" % tag,
               lambda i: lib.so3_sym_frob_loss_f32(p(r[i % NB]), p(rt[i % NB]), p(sd), cp, tab.num_classes, tab.K, p(dm[i % NB]), p(g[i % NB]), None,
                                                   p(ls), p(lm), p(ws), 0, n, st),
               144 * n + extra)
    del r64, g64
    # K4b: the metrics' backward (round 6): dR1 / dR2 of geodesic(..., 'mean') from a 0-dim upstream gradient, of the per-row form from a
    # per-row one, and angle_error's float64 spelling
    RAD, GS, F64 = _lib.RADIANS, _lib.GRAD_SCALAR, _lib.F64_MATH
    one32, one64 = torch.ones(1, device=dev), torch.ones(1, dtype=torch.float64, device=dev)
    w32, w64 = torch.randn(n, device=dev), torch.randn(n, dtype=torch.float64, device=dev)
    kb = lib.so3_angle_bwd_f32
    D = ctypes.c_double
    timeit("K4b so3_angle_bwd_f32 geodesic mean: dR1 + dR2", lambda i: kb(p(r[i % NB]), p(rt[i % NB]), p(one32), D(n), D(1e-7), RAD | GS, p(dm[i % NB]), p(g[i % NB]), n, st), 144 * n)
    timeit("K4b so3_angle_bwd_f32 geodesic mean: dR1 alone", lambda i: kb(p(r[i % NB]), p(rt[i % NB]), p(one32), D(n), D(1e-7), RAD | GS, p(dm[i % NB]), None, n, st), 108 * n)
    timeit("K4b so3_angle_bwd_f32 per-row upstream gradient: dR1 alone", lambda i: kb(p(r[i % NB]), p(rt[i % NB]), p(w32), D(1), D(0), RAD, p(dm[i % NB]), None, n, st), 112 * n)
    timeit("K4b so3_angle_bwd_f32 angle_error.mean() (float64 math): dR1 alone", lambda i: kb(p(r[i % NB]), p(rt[i % NB]), p(one64), D(n), D(0), GS | F64, p(dm[i % NB]), None, n, st), 108 * n)
    timeit("K4b so3_angle_bwd_f32 angle_error per-row float64 gradient: dR1 + dR2", lambda i: kb(p(r[i % NB]), p(rt[i % NB]), p(w64), D(1), D(0), F64, p(dm[i % NB]), p(g[i % NB]), n, st), 152 * n)
    timeit("K4' so3_geodesic_f32", lambda i: lib.so3_geodesic_f32(p(r[i % NB]), p(rt[i % NB]), p(th), n, st), 76 * n)
    print("--- next rows (f1, f2, f3) at 1M rows ---")
    x6 = [torch.randn(n, 6, device=dev) for _ in range(NB)]
    d6 = torch.empty(n, 6, device=dev)
    timeit("f2 so3_ortho6d_fwd_f32", lambda i: lib.so3_ortho6d_fwd_f32(p(x6[i % NB]), p(r[i % NB]), n, st), 60 * n)
    timeit("f2 so3_ortho6d_bwd_f32", lambda i: lib.so3_ortho6d_bwd_f32(p(x6[i % NB]), p(g[i % NB]), p(d6), n, st), 84 * n)
    del x6, d6
    for name, w in (("quat", 4), ("euler", 3), ("ortho5d", 5), ("expmap", 3)):
        xh = [torch.randn(n, w, device=dev) for _ in range(NB)]
        dh = torch.empty(n, w, device=dev)
        fwd, bwd = getattr(lib, "so3_%s_fwd_f32" % name), getattr(lib, "so3_%s_bwd_f32" % name)
        timeit("f5 so3_%s_fwd_f32" % name, lambda i: fwd(p(xh[i % NB]), p(r[i % NB]), n, st), (4 * w + 36) * n)
        timeit("f5 so3_%s_bwd_f32" % name, lambda i: bwd(p(xh[i % NB]), p(g[i % NB]), p(dh), n, st), (8 * w + 36) * n)
        del xh, dh
    # the inverse maps: rotation -> quaternion / rotation vector / Euler angles, log(R1^T R2), and their tangent-space gradients
    for name, w in (("mat_to_quat", 4), ("logmap", 3), ("mat_to_euler", 3)):
        yh = torch.empty(n, w, device=dev)
        gh = [torch.randn(n, w, device=dev) for _ in range(NB)]
        fwd, bwd = getattr(lib, "so3_%s_fwd_f32" % name), getattr(lib, "so3_%s_bwd_f32" % name)
        timeit("inv so3_%s_fwd_f32" % name, lambda i: fwd(p(rt[i % NB]), p(yh), n, st), (36 + 4 * w) * n)
        timeit("inv so3_%s_bwd_f32" % name, lambda i: bwd(p(rt[i % NB]), p(gh[i % NB]), p(dm[i % NB]), n, st), (72 + 4 * w) * n)
        del yh, gh
    v3 = torch.empty(n, 3, device=dev)
    g3 = [torch.randn(n, 3, device=dev) for _ in range(NB)]
    dm2 = torch.empty(n, 9, device=dev)                # dR2 (the rotation buffers r[] are read again below)
    timeit("inv so3_relative_log_fwd_f32", lambda i: lib.so3_relative_log_fwd_f32(p(rt[i % NB]), p(rt[(i + 1) % NB]), p(v3), n, st), 84 * n)
    timeit("inv so3_relative_log_bwd_f32 (dR1 + dR2)",
           lambda i: lib.so3_relative_log_bwd_f32(p(rt[i % NB]), p(rt[(i + 1) % NB]), p(g3[i % NB]), p(dm[i % NB]), p(dm2), n, st), 156 * n)
    del v3, g3, dm2
    o12 = [torch.randn(n, 12, device=dev) for _ in range(3)]
    ti = [torch.eye(4, device=dev).repeat(n, 1, 1).contiguous() + 0.1 * torch.randn(n, 4, 4, device=dev) for _ in range(3)]
    tp = torch.empty(n, 16, device=dev); g16 = torch.randn(n, 16, device=dev); do12 = torch.empty(n, 12, device=dev)
    fx = ctypes.c_float(444.444)
    timeit("f1 so3_se3_update_f32", lambda i: lib.so3_se3_update_f32(p(o12[i % 3]), p(ti[i % 3]), p(tp), fx, fx, n, st), 176 * n)
    timeit("f1 so3_se3_update_bwd_f32", lambda i: lib.so3_se3_update_bwd_f32(p(o12[i % 3]), p(ti[i % 3]), p(g16), p(do12), fx, fx, n, st), 224 * n)
    del o12, ti, tp, g16, do12
    cls = torch.randint(0, 10, (n,), device=dev, dtype=torch.int32)
    lib.so3_angle_error_v2(p(r[0]), p(rt[0]), p(deg), None, p(fl), None, 0, n, st)
    stats = torch.empty(10, 8, dtype=torch.float64, device=dev)
    work = torch.zeros(lib.so3_angle_stats_workspace_bytes(), dtype=torch.uint8, device=dev)     # zero-filled once
    timeit("f3 so3_angle_stats (10 classes, exact median)", lambda i: lib.so3_angle_stats(p(deg), p(cls), 10, p(stats), p(work), n, st), 12 * n, iters=20)
    timeit("f3 so3_angle_stats (one class: the whole batch's median)", lambda i: lib.so3_angle_stats(p(deg), None, 1, p(stats), p(work), n, st), 8 * n, iters=20)
    del x, xb, g, r, dm, dmb, rt
    torch.cuda.empty_cache()
    print("--- config #3: 65536 clouds x 1024 points ---")
    b, npts = 65536, 1024
    pc = [torch.rand(b, npts, 3, device=dev) - 0.5 for _ in range(2)]
    qc = [torch.rand(b, npts, 3, device=dev) - 0.5 for _ in range(2)]
    rk = torch.empty(b, 9, device=dev)
    timeit("K5 so3_kabsch_f32", lambda i: lib.so3_kabsch_f32(p(pc[i % 2]), p(qc[i % 2]), p(rk), None, b, npts, st), b * (2 * npts * 12 + 36), iters=10, warm=2)
    hk = torch.empty(b, 9, device=dev)
    lib.so3_kabsch_f32(p(pc[0]), p(qc[0]), p(rk), p(hk), b, npts, st)
    gkr, gkh = torch.randn(b, 9, device=dev), torch.randn(b, 9, device=dev)
    dpc, dqc = torch.empty(b, npts, 3, device=dev), torch.empty(b, npts, 3, device=dev)
    timeit("K5b so3_kabsch_bwd_f32 (dP and dQ)", lambda i: lib.so3_kabsch_bwd_f32(p(pc[i % 2]), p(qc[i % 2]), p(hk), p(gkr), p(gkh), p(dpc), p(dqc), b, npts, st),
           b * (48 * npts + 108), iters=10, warm=2)
    timeit("K5b so3_kabsch_bwd_f32 (dQ only)", lambda i: lib.so3_kabsch_bwd_f32(p(pc[i % 2]), p(qc[i % 2]), p(hk), p(gkr), p(gkh), None, p(dqc), b, npts, st),
           b * (24 * npts + 108), iters=10, warm=2)
    # K5c / K5d: rigid_align, the weighted and centred Kabsch giving (R, t) -- K5's bytes unweighted, 4/3 of them weighted
    wk = [torch.rand(b, npts, device=dev) + 0.05 for _ in range(2)]
    tk, sk, dwk = torch.empty(b, 3, device=dev), torch.empty(b, 7, device=dev), torch.empty(b, npts, device=dev)
    ra, rab = lib.so3_rigid_align_f32, lib.so3_rigid_align_bwd_f32
    timeit("K5c so3_rigid_align_f32 (unweighted)", lambda i: ra(p(pc[i % 2]), p(qc[i % 2]), None, p(rk), p(tk), None, None, b, npts, st),
           b * (2 * npts * 12 + 48), iters=10, warm=2)
    timeit("K5c so3_rigid_align_f32 (weighted)", lambda i: ra(p(pc[i % 2]), p(qc[i % 2]), p(wk[i % 2]), p(rk), p(tk), None, None, b, npts, st),
           b * (npts * 28 + 48), iters=10, warm=2)
    ra(p(pc[0]), p(qc[0]), p(wk[0]), p(rk), p(tk), p(hk), p(sk), b, npts, st)
    gtk = torch.randn(b, 3, device=dev)
    timeit("K5d so3_rigid_align_bwd_f32 (dP, dQ and dw)",
           lambda i: rab(p(pc[0]), p(qc[0]), p(wk[0]), p(hk), p(rk), p(sk), p(gkr), p(gtk), p(gkh), p(dpc), p(dqc), p(dwk), b, npts, st),
           b * (56 * npts + 196), iters=10, warm=2)
    del hk, gkr, gkh, dqc, wk, tk, sk, dwk, gtk
    # nearest neighbours between two clouds and ICP on top of them: N * M pairs per cloud (compute bound; the bytes are the clouds')
    bi, ni = 256, 1024
    xi, yi = torch.rand(bi, ni, 3, device=dev), torch.rand(bi, ni, 3, device=dev)
    di, nni = torch.empty(bi, ni, device=dev), torch.empty(bi, ni, dtype=torch.int32, device=dev)
    ri, ti = torch.empty(bi, 9, device=dev), torch.empty(bi, 3, device=dev)
    wsi = torch.empty(lib.so3_icp_workspace_bytes(bi, ni) // 4, device=dev)
    timeit("so3_nearest_f32 (256 x 1024 x 1024)", lambda i: lib.so3_nearest_f32(p(xi), p(yi), 3 * ni, p(di), p(nni), bi, ni, ni, st), bi * ni * 32, iters=10, warm=2)
    for its in (1, 10):
        timeit("so3_icp_f32 (256 x 1024 x 1024, %d iteration%s)" % (its, "" if its == 1 else "s"),
               lambda i: lib.so3_icp_f32(p(xi), p(yi), 3 * ni, None, None, ctypes.c_float(-1.0), its, p(ri), p(ti), None, None, None, None, p(wsi), bi, ni, ni, st),
               its * bi * ni * 24, iters=10, warm=2)
    # point-to-plane ICP at the same shape (profiles/icp_plane_bench.txt): the same search, two gathers per point and 31 sums
    nri = torch.nn.functional.normalize(torch.randn(bi, ni, 3, device=dev), dim=-1)
    wpi = torch.empty(lib.so3_icp_plane_workspace_bytes(bi, ni) // 4, device=dev)
    for its in (1, 10):
        timeit("so3_icp_plane_f32 (256 x 1024 x 1024, %d iteration%s)" % (its, "" if its == 1 else "s"),
               lambda i: lib.so3_icp_plane_f32(p(xi), p(yi), p(nri), 3 * ni, None, None, ctypes.c_float(-1.0), ctypes.c_float(0.0), its, p(ri), p(ti),
                                               None, None, None, None, None, None, p(wpi), bi, ni, ni, st),
               its * bi * ni * 36, iters=10, warm=2)
    # the Chamfer distance at the same shape: both searches in one launch (2 x N * M pairs per cloud), then both gradients in one gather
    dyi, nyi = torch.empty(bi, ni, device=dev), torch.empty(bi, ni, dtype=torch.int32, device=dev)
    rwi, sci = torch.empty(bi, 2, device=dev), torch.full((bi,), 1.0 / ni, device=dev)
    gxi, gyi = torch.empty(bi, ni, 3, device=dev), torch.empty(bi, ni, 3, device=dev)
    wci = torch.empty(lib.so3_chamfer_workspace_bytes(bi, ni, ni) // 4, device=dev)
    timeit("so3_chamfer_fwd_f32 (256 x 1024 x 1024, rows + nearest)",
           lambda i: lib.so3_chamfer_fwd_f32(p(xi), p(yi), None, None, None, p(nni), None, p(nyi), p(rwi), p(wci), 0, bi, ni, ni, st), bi * ni * 32, iters=10, warm=2)
    timeit("so3_chamfer_bwd_f32 (256 x 1024 x 1024, dX + dY)",
           lambda i: lib.so3_chamfer_bwd_f32(p(xi), p(yi), None, None, p(nni), p(nyi), p(sci), p(sci), p(gxi), p(gyi), 0, bi, ni, ni, st), bi * ni * 56, iters=10, warm=2)
    # the same with the normal term (profiles/chamfer_normals_bench.txt): the forward adds two 12-byte loads and the cosine per point behind
    # the search, the backward is the same gather over the normals; then all four entries at the speed condition's shape
    nxi, nni_y = torch.randn(bi, ni, 3, device=dev), torch.randn(bi, ni, 3, device=dev)
    rni, wni = torch.empty(bi, 2, device=dev), torch.empty(lib.so3_chamfer_normals_workspace_bytes(bi, ni, ni) // 4, device=dev)
    timeit("so3_chamfer_normals_fwd_f32 (256 x 1024 x 1024, rows + nearest)",
           lambda i: lib.so3_chamfer_normals_fwd_f32(p(xi), p(yi), p(nxi), p(nni_y), None, None, None, p(nni), None, p(nyi), None, None, p(rwi), p(rni), p(wni),
                                                     0, bi, ni, ni, st), bi * ni * 56, iters=10, warm=2)
    timeit("so3_chamfer_normals_bwd_f32 (256 x 1024 x 1024, dNX + dNY)",
           lambda i: lib.so3_chamfer_normals_bwd_f32(p(nxi), p(nni_y), None, None, p(nni), p(nyi), p(sci), p(sci), p(gxi), p(gyi), 0, bi, ni, ni, st),
           bi * ni * 56, iters=10, warm=2)
    del xi, yi, di, nni, ri, ti, wsi, dyi, nyi, rwi, sci, gxi, gyi, wci, nxi, nni_y, rni, wni
    bs, ns = 16, 2048
    xs, ys = torch.rand(bs, ns, 3, device=dev), torch.rand(bs, ns, 3, device=dev)
    nxs, nys = torch.randn(bs, ns, 3, device=dev), torch.randn(bs, ns, 3, device=dev)
    ixs, iys = torch.empty(bs, ns, dtype=torch.int32, device=dev), torch.empty(bs, ns, dtype=torch.int32, device=dev)
    rws, rns, scs = torch.empty(bs, 2, device=dev), torch.empty(bs, 2, device=dev), torch.full((bs,), 1.0 / ns, device=dev)
    gxs, gys = torch.empty(bs, ns, 3, device=dev), torch.empty(bs, ns, 3, device=dev)
    wss = torch.empty(lib.so3_chamfer_normals_workspace_bytes(bs, ns, ns) // 4, device=dev)
    timeit("so3_chamfer_fwd_f32 (16 x 2048 x 2048, rows + nearest)",
           lambda i: lib.so3_chamfer_fwd_f32(p(xs), p(ys), None, None, None, p(ixs), None, p(iys), p(rws), p(wss), 0, bs, ns, ns, st), bs * ns * 32, iters=10, warm=2)
    timeit("so3_chamfer_normals_fwd_f32 (16 x 2048 x 2048, rows + nearest)",
           lambda i: lib.so3_chamfer_normals_fwd_f32(p(xs), p(ys), p(nxs), p(nys), None, None, None, p(ixs), None, p(iys), None, None, p(rws), p(rns), p(wss),
                                                     0, bs, ns, ns, st), bs * ns * 56, iters=10, warm=2)
    timeit("so3_chamfer_bwd_f32 (16 x 2048 x 2048, dX + dY)",
           lambda i: lib.so3_chamfer_bwd_f32(p(xs), p(ys), None, None, p(ixs), p(iys), p(scs), p(scs), p(gxs), p(gys), 0, bs, ns, ns, st), bs * ns * 56, iters=10, warm=2)
    timeit("so3_chamfer_normals_bwd_f32 (16 x 2048 x 2048, dNX + dNY)",
           lambda i: lib.so3_chamfer_normals_bwd_f32(p(nxs), p(nys), None, None, p(ixs), p(iys), p(scs), p(scs), p(gxs), p(gys), 0, bs, ns, ns, st),
           bs * ns * 56, iters=10, warm=2)
    del xs, ys, nxs, nys, ixs, iys, rws, rns, scs, gxs, gys, wss
    # K nearest neighbours at tools/ubench/knn_paths.hip's shapes: the search, then both gradients in one gather (the bytes are the rows')
    for bk, nk, mk, kk in ((32, 1024, 1024, 16), (32, 512, 128, 8), (8, 4096, 4096, 20)):
        xk, yk = torch.rand(bk, nk, 3, device=dev), torch.rand(bk, mk, 3, device=dev)
        dk, ik = torch.empty(bk, nk, kk, device=dev), torch.empty(bk, nk, kk, dtype=torch.int32, device=dev)
        gk, gxk, gyk = torch.rand(bk, nk, kk, device=dev), torch.empty(bk, nk, 3, device=dev), torch.empty(bk, mk, 3, device=dev)
        timeit("so3_knn_f32 (%d x %d <- %d, K = %d)" % (bk, nk, mk, kk),
               lambda i: lib.so3_knn_f32(p(xk), p(yk), 3 * mk, None, None, p(dk), p(ik), kk, bk, nk, mk, st), bk * nk * kk * 8, iters=10, warm=2)
        timeit("so3_knn_bwd_f32 (%d x %d <- %d, K = %d, dX + dY)" % (bk, nk, mk, kk),
               lambda i: lib.so3_knn_bwd_f32(p(xk), p(yk), None, None, p(ik), p(gk), p(gxk), p(gyk), kk, bk, nk, mk, st),
               bk * (nk * kk * 8 + (nk + mk) * 24), iters=10, warm=2)
    del xk, yk, dk, ik, gk, gxk, gyk
    # local frames: the covariance of every point's K nearest neighbours and its eigen-decomposition, from indices that are given (the
    # bytes are the index rows', one gathered point per slot and the outputs')
    for bl, nl, kl in ((32, 1024, 16), (8, 4096, 20)):
        yl_ = torch.rand(bl, nl, 3, device=dev)
        il = torch.empty(bl, nl, kl, dtype=torch.int32, device=dev)
        _lib.check(lib.so3_knn_f32(p(yl_), p(yl_), 3 * nl, None, None, None, p(il), kl, bl, nl, nl, st), "so3_knn_f32")
        cl, el, ml, fl = (torch.empty(bl, nl, w, device=dev) for w in (6, 3, 3, 9))
        timeit("local_frames: so3_local_frames_f32 (%d x %d, K = %d, all outputs)" % (bl, nl, kl),
               lambda i: lib.so3_local_frames_f32(p(yl_), 3 * nl, p(il), None, None, None, p(cl), p(el), p(ml), p(fl), kl, bl, nl, nl, st),
               bl * nl * (kl * 16 + 84), iters=20, warm=3)
        timeit("local_frames: so3_local_frames_f32 (%d x %d, K = %d, normals only)" % (bl, nl, kl),
               lambda i: lib.so3_local_frames_f32(p(yl_), 3 * nl, p(il), None, None, None, None, None, p(ml), None, kl, bl, nl, nl, st),
               bl * nl * (kl * 16 + 12), iters=20, warm=3)
    del yl_, il, cl, el, ml, fl
    # FPFH beside the local frames: the same index rows, a point and a normal gathered per slot, 33 floats and a count out; then per
    # output element K slots of a broadcast index and point and one float of the neighbour's row (the bytes are the rows', one pass)
    for bh, nh, kh in ((32, 1024, 16), (8, 4096, 32)):
        xh = torch.rand(bh, nh, 3, device=dev)
        nrh = torch.nn.functional.normalize(torch.randn(bh, nh, 3, device=dev), dim=-1)
        ih = torch.empty(bh, nh, kh, dtype=torch.int32, device=dev)
        _lib.check(lib.so3_knn_f32(p(xh), p(xh), 3 * nh, None, None, None, p(ih), kh, bh, nh, nh, st), "so3_knn_f32")
        sh, ph, fh = torch.empty(bh, nh, 33, device=dev), torch.empty(bh, nh, dtype=torch.int32, device=dev), torch.empty(bh, nh, 33, device=dev)
        timeit("fpfh, beside local_frames: so3_spfh_f32 (%d x %d, K = %d, spfh + pairs)" % (bh, nh, kh),
               lambda i: lib.so3_spfh_f32(p(xh), p(nrh), p(ih), None, p(sh), p(ph), kh, bh, nh, st), bh * nh * (kh * 28 + 24 + 136), iters=20, warm=3)
        timeit("fpfh, beside local_frames: so3_fpfh_f32 (%d x %d, K = %d)" % (bh, nh, kh),
               lambda i: lib.so3_fpfh_f32(p(xh), p(ih), None, p(sh), p(ph), p(fh), kh, bh, nh, st), bh * nh * (kh * (4 + 12 + 4 + 132) + 264), iters=20, warm=3)
    del xh, nrh, ih, sh, ph, fh
    # RANSAC over feature matches: every pair valid, the triples drawn by the host; the bytes are what each entry reads and writes once
    for br, nr, hr in ((8, 2048, 4096), (4, 1024, 2048)):
        pr, qr = torch.rand(br, nr, 3, device=dev), torch.rand(br, nr, 3, device=dev)
        cr = torch.randint(0, nr, (br, nr), dtype=torch.int32, device=dev)
        sr = torch.randint(0, nr, (br, hr, 3), dtype=torch.int32, device=dev)
        th, ch, eh = torch.empty(br, hr, 12, device=dev), torch.empty(br, hr, dtype=torch.int32, device=dev), torch.empty(br, hr, device=dev)
        bb, ib = torch.empty(br, dtype=torch.int32, device=dev), torch.empty(br, dtype=torch.int32, device=dev)
        tb, rb, wb, gb = torch.empty(br, 12, device=dev), torch.empty(br, device=dev), torch.empty(br, nr, device=dev), torch.empty(br, nr, 3, device=dev)
        timeit("ransac: so3_ransac_score_f32 (%d x %d points, %d hypotheses)" % (br, nr, hr),
               lambda i: lib.so3_ransac_score_f32(p(pr), p(qr), p(cr), None, None, p(sr), 0.05, 0.0, p(th), p(ch), p(eh), br, nr, nr, hr, st),
               br * (nr * 28 + hr * (12 + 56)), iters=20, warm=3)
        timeit("ransac: so3_ransac_select_f32 (%d x %d points, %d hypotheses)" % (br, nr, hr),
               lambda i: lib.so3_ransac_select_f32(p(pr), p(qr), p(cr), None, None, p(th), p(ch), p(eh), 0.05, p(bb), p(tb), p(ib), p(rb), p(wb), p(gb),
                                                   br, nr, nr, hr, st), br * (nr * (28 + 16) + hr * 8), iters=20, warm=3)
    del pr, qr, cr, sr, th, ch, eh, bb, ib, tb, rb, wb, gb
    # PointNet++ sampling and grouping at the reference model's first level: a chain of 511 dependent argmaxes per cloud (one workgroup
    # each: latency bound, most compute units idle at B = 32), and one wave per centre over the cloud (the bytes are the index rows')
    bf, nf, sf, kf = 32, 1024, 512, 64
    xf = torch.rand(bf, nf, 3, device=dev) - 0.5
    xf = xf / (xf.amax(1) - xf.amin(1)).norm(dim=-1)[:, None, None]                     # pc_normalize's scale
    s0 = torch.zeros(bf, dtype=torch.int32, device=dev)
    of = torch.empty(bf, sf, dtype=torch.int32, device=dev)
    timeit("pointnet: so3_fps_f32 (32 x 1024 -> 512)", lambda i: lib.so3_fps_f32(p(xf), p(s0), p(of), bf, nf, sf, st), bf * (nf * 12 + sf * 4), iters=10, warm=2)
    _lib.check(lib.so3_fps_f32(p(xf), p(s0), p(of), bf, nf, sf, st), "so3_fps_f32")        # the centres, whether or not the line above ran
    cf = torch.gather(xf, 1, of.long()[..., None].expand(-1, -1, 3)).contiguous()
    gi, gc = torch.empty(bf, sf, kf, dtype=torch.int32, device=dev), torch.empty(bf, sf, dtype=torch.int32, device=dev)
    timeit("pointnet: so3_ball_query_f32 (32 x 1024, 512 centres, r=0.2, K=64)", lambda i: lib.so3_ball_query_f32(p(xf), p(cf), ctypes.c_float(0.2), kf, p(gi), None, bf, nf, sf, st),
           bf * sf * kf * 4, iters=10, warm=2)
    timeit("pointnet: so3_ball_query_f32 (the same, with counts)", lambda i: lib.so3_ball_query_f32(p(xf), p(cf), ctypes.c_float(0.2), kf, p(gi), p(gc), bf, nf, sf, st),
           bf * sf * (kf + 1) * 4, iters=10, warm=2)
    del xf, s0, of, cf, gi, gc
    # feature propagation: the reference model's first and second propagation levels, both layouts
    for bt, nt, stn, dt in ((32, 1024, 512, 128), (32, 512, 128, 256)):
        shape = "%d x %d <- %d" % (bt, nt, stn)
        x1, x2 = torch.rand(bt, nt, 3, device=dev) - 0.5, torch.rand(bt, stn, 3, device=dev) - 0.5
        d3, i3, w3 = torch.empty(bt, nt, 3, device=dev), torch.empty(bt, nt, 3, dtype=torch.int32, device=dev), torch.empty(bt, nt, 3, device=dev)
        timeit("three_nn: so3_three_nn_f32 (%s, with weights)" % shape, lambda i: lib.so3_three_nn_f32(p(x1), p(x2), p(d3), p(i3), p(w3), bt, nt, stn, st),
               bt * (nt * 48 + stn * 12), iters=20, warm=3)
        timeit("three_nn: so3_three_nn_f32 (%s, without)" % shape, lambda i: lib.so3_three_nn_f32(p(x1), p(x2), p(d3), p(i3), None, bt, nt, stn, st),
               bt * (nt * 36 + stn * 12), iters=20, warm=3)
        dk3, ik3 = torch.empty_like(d3), torch.empty_like(i3)      # the same rows from the K-neighbour kernel, for the record
        timeit("three_nn: so3_knn_f32 (%s, K = 3)" % shape, lambda i: lib.so3_knn_f32(p(x1), p(x2), 3 * stn, None, None, p(dk3), p(ik3), 3, bt, nt, stn, st),
               bt * (nt * 36 + stn * 12), iters=20, warm=3)
        _lib.check(lib.so3_three_nn_f32(p(x1), p(x2), p(d3), p(i3), p(w3), bt, nt, stn, st), "so3_three_nn_f32")
        ft, gt = torch.randn(bt, stn * dt, device=dev), torch.randn(bt, nt * dt, device=dev)
        ot, gf = torch.empty_like(gt), torch.empty_like(ft)
        moved = bt * ((nt + stn) * dt * 4 + nt * 24)
        for cfl, lay in ((0, "(B,S,D)"), (1, "(B,D,S)")):
            timeit("three_nn: so3_three_interpolate_f32 (%s, D=%d, %s)" % (shape, dt, lay),
                   lambda i: lib.so3_three_interpolate_f32(p(ft), p(i3), p(w3), p(ot), cfl, bt, nt, stn, dt, st), moved, iters=20, warm=3)
            timeit("three_nn: so3_three_interpolate_bwd_f32 (%s, D=%d, %s)" % (shape, dt, lay),
                   lambda i: lib.so3_three_interpolate_bwd_f32(p(gt), p(i3), p(w3), p(gf), cfl, bt, nt, stn, dt, st), moved, iters=20, warm=3)
        del x1, x2, d3, i3, w3, ft, gt, ot, gf
    # set-abstraction grouping: the reference model's first level (one of its three radii) and its second level,
    # both launches in both layouts; then whole Python calls of group_points(channels_first=True) against the torch spelling it replaces
    for bg, ng, sg, kg, dg, rad in ((32, 1024, 512, 64, 3, 0.2), (32, 512, 128, 128, 320, 0.4)):
        shape = "%d x %d, %d centres, K=%d, D=%d" % (bg, ng, sg, kg, dg)
        xg = torch.rand(bg, ng, 3, device=dev) - 0.5
        s0 = torch.zeros(bg, dtype=torch.int32, device=dev)
        og = torch.empty(bg, sg, dtype=torch.int32, device=dev)
        _lib.check(lib.so3_fps_f32(p(xg), p(s0), p(og), bg, ng, sg, st), "so3_fps_f32")
        cg = torch.gather(xg, 1, og.long()[..., None].expand(-1, -1, 3)).contiguous()
        ig = torch.empty(bg, sg, kg, dtype=torch.int32, device=dev)
        _lib.check(lib.so3_ball_query_f32(p(xg), p(cg), ctypes.c_float(rad), kg, p(ig), None, bg, ng, sg, st), "so3_ball_query_f32")
        fg, cot = torch.randn(bg, ng * dg, device=dev), torch.randn(bg, (3 + dg) * kg * sg, device=dev)
        outg, gxg, gcg, gfg = torch.empty_like(cot), torch.empty_like(xg), torch.empty_like(cg), torch.empty_like(fg)
        moved = bg * ((3 + dg) * kg * sg * 4 + sg * kg * 4 + (ng + sg) * 12 + ng * dg * 4)
        for cfl, lay in ((0, "(B,S,K,C)"), (1, "(B,C,K,S)")):
            timeit("grouping: so3_group_points_f32 (%s, %s)" % (shape, lay),
                   lambda i: lib.so3_group_points_f32(p(xg), p(cg), p(fg), p(ig), p(outg), 0, cfl, bg, ng, sg, kg, dg, st), moved, iters=20, warm=3)
            timeit("grouping: so3_group_points_bwd_f32 (%s, %s, all three)" % (shape, lay),
                   lambda i: lib.so3_group_points_bwd_f32(p(cot), p(ig), p(gxg), p(gcg), p(gfg), 0, cfl, bg, ng, sg, kg, dg, st), moved, iters=20, warm=3)
        if not ONLY or ONLY in "grouping: python":
            import numpy as np
            leaves = [t.requires_grad_(True) for t in (xg, cg, fg.view(bg, ng, dg), fg.view(bg, ng, dg).transpose(1, 2).contiguous())]
            il, cot4 = ig.long(), cot.view(bg, 3 + dg, kg, sg)

            def median_ms(fn, warm=3, iters=10 if dg > 64 else 20):
                times = []
                for k in range(warm + iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                return float(np.median(times[warm:]))

            def spelled():
                grouped = rr.index_points(leaves[0], il) - leaves[1][:, :, None, :]
                return torch.cat([grouped, rr.index_points(leaves[2], il)], dim=-1).permute(0, 3, 2, 1).contiguous()

            def both(fn):
                for t in leaves: t.grad = None
                fn().backward(cot4)

            ours = lambda: rr.group_points(leaves[0], leaves[1], leaves[3], il, channels_first=True)
            with torch.no_grad():
                of_, tf_ = median_ms(ours), median_ms(spelled)
            ofb, tfb = median_ms(lambda: both(ours)), median_ms(lambda: both(spelled))
            print("grouping: python calls (%s): forward %.4f ms, torch spelling %.4f ms (x%.1f); forward + backward %.4f ms, torch %.4f ms (x%.1f)"
                  % (shape, of_, tf_, tf_ / of_, ofb, tfb, tfb / ofb))
            del leaves, il, cot4
        del xg, s0, og, cg, ig, fg, cot, outg, gxg, gcg, gfg
        torch.cuda.empty_cache()
    rg = rr.get_sampled_rotation_matrices_by_axisAngle(b, dev).reshape(b, 9).contiguous()
    timeit("f4 so3_kabsch_synth_f32 (sigma=0: P only)", lambda i: lib.so3_kabsch_synth_f32(p(pc[i % 2]), p(rg), ctypes.c_float(0.0), 1, p(rk), None, b, npts, st), b * (npts * 12 + 72), iters=10, warm=2)
    timeit("f4 so3_kabsch_synth_f32 (sigma=0.01, device RNG)", lambda i: lib.so3_kabsch_synth_f32(p(pc[i % 2]), p(rg), ctypes.c_float(0.01), 1, p(rk), None, b, npts, st), b * (npts * 12 + 72), iters=10, warm=2)
    del qc
    tg = torch.eye(4, device=dev).repeat(b, 1, 1).contiguous(); tg[:, :3, :3] = rg.view(b, 3, 3); tg[:, :3, 3] = torch.randn(b, 3, device=dev)
    tq = tg.clone(); tq[:, :3, :3] = rr.get_sampled_rotation_matrices_by_axisAngle(b, dev); tq[:, :3, 3] += 0.1 * torch.randn(b, 3, device=dev)
    dtq = torch.empty(b, 16, device=dev); l3 = torch.empty(3, dtype=torch.float64, device=dev)
    sc = ctypes.c_float(1.0 / b)
    timeit("f6 so3_add_l1_f32 (loss + dTpred)", lambda i: lib.so3_add_l1_f32(p(tg), p(tq), p(pc[i % 2]), None, p(l3), p(dtq), sc, b, npts, st), b * (npts * 12 + 192), iters=10, warm=2)
    timeit("f6 so3_add_l1_disentangled_f32 (loss + dTpred)", lambda i: lib.so3_add_l1_disentangled_f32(p(tq), p(tg), p(pc[i % 2]), p(l3), p(dtq), sc, b, npts, st), b * (npts * 12 + 192), iters=10, warm=2)
    timeit("ADD so3_add_l2_f32 (loss + dTpred)", lambda i: lib.so3_add_l2_f32(p(tg), p(tq), p(pc[i % 2]), None, p(l3), p(dtq), sc, b, npts, st), b * (npts * 12 + 192), iters=10, warm=2)
    qo = torch.empty(b, npts, 3, device=dev)
    timeit("a7 so3_rotate_clouds_f32", lambda i: lib.so3_rotate_clouds_f32(p(pc[i % 2]), p(rg), p(qo), 0, b, npts, st), b * (npts * 24 + 36), iters=10, warm=2)
    timeit("a7 so3_rotate_clouds_f32 (transposed out)", lambda i: lib.so3_rotate_clouds_f32(p(pc[i % 2]), p(rg), p(qo), 1, b, npts, st), b * (npts * 24 + 36), iters=10, warm=2)
    timeit("a7 so3_pc_normalize_f32", lambda i: lib.so3_pc_normalize_f32(p(pc[i % 2]), p(qo), None, None, b, npts, st), b * (npts * 24), iters=10, warm=2)
    drg = torch.empty(b, 9, device=dev)            # qo: the upstream gradient (either layout: same bytes); dpc: dP
    timeit("a7b so3_rotate_clouds_bwd_f32 (dP and dR)", lambda i: lib.so3_rotate_clouds_bwd_f32(p(pc[i % 2]), p(rg), p(qo), p(dpc), p(drg), 0, b, npts, st),
           b * (36 * npts + 72), iters=10, warm=2)
    timeit("a7b so3_rotate_clouds_bwd_f32 (transposed G, dP and dR)",
           lambda i: lib.so3_rotate_clouds_bwd_f32(p(pc[i % 2]), p(rg), p(qo), p(dpc), p(drg), 1, b, npts, st), b * (36 * npts + 72), iters=10, warm=2)
    del pc, tg, tq, dtq, qo, dpc, drg
    torch.cuda.empty_cache()
    print("--- ADD-S / diameter: B = 256 clouds of N = 1024 points (N^2 pairs per cloud: compute bound; GB/s = inputs and outputs only) ---")
    b, npts = 256, 1024
    pa_ = torch.randn(b, npts, 3, device=dev)
    tg = torch.eye(4, device=dev).repeat(b, 1, 1).contiguous(); tg[:, :3, :3] = rr.get_sampled_rotation_matrices_by_axisAngle(b, dev)
    tq = tg.clone(); tq[:, :3, :3] = rr.get_sampled_rotation_matrices_by_axisAngle(b, dev); tq[:, :3, 3] += 0.1 * torch.randn(b, 3, device=dev)
    pd = torch.empty(b, npts, device=dev); nn = torch.empty(b, npts, dtype=torch.int32, device=dev); ds = torch.empty(b, device=dev)
    dtq = torch.empty(b, 16, device=dev); l1 = torch.empty(1, dtype=torch.float64, device=dev)
    timeit("ADD-S so3_add_s_fwd_f32 (rows)", lambda i: lib.so3_add_s_fwd_f32(p(tg), p(tq), p(pa_), p(pd), None, p(ds), None, b, npts, st), b * (npts * 20 + 132))
    timeit("ADD-S so3_add_s_fwd_f32 (rows + nearest + loss_sum)", lambda i: lib.so3_add_s_fwd_f32(p(tg), p(tq), p(pa_), p(pd), p(nn), p(ds), p(l1), b, npts, st), b * (npts * 24 + 132))
    timeit("ADD-S so3_add_s_bwd_f32", lambda i: lib.so3_add_s_bwd_f32(p(tg), p(tq), p(pa_), p(nn), p(ds), ctypes.c_float(1.0), p(dtq), b, npts, st), b * (npts * 28 + 192))
    timeit("diameter so3_cloud_diameter_f32", lambda i: lib.so3_cloud_diameter_f32(p(pa_), p(pd), p(ds), b, npts, st), b * (npts * 20 + 4))
    # ADD up to a symmetry group at the same shape: K = 1 against so3_add_l2_f32 is what the min_k wrapper costs over the plain pass
    kk = 8
    th = 2.0 * math.pi * torch.arange(kk, dtype=torch.float64) / kk
    s8 = torch.zeros(kk, 3, 3, dtype=torch.float64); s8[:, 0, 0] = th.cos(); s8[:, 0, 1] = -th.sin(); s8[:, 1, 0] = th.sin(); s8[:, 1, 1] = th.cos(); s8[:, 2, 2] = 1.0
    s8 = s8.reshape(kk, 9).float().to(dev).contiguous()
    ix = torch.empty(b, dtype=torch.int32, device=dev)
    one = ctypes.c_float(1.0)
    sym = lambda K, rows, idx, tot, dT, mode: lib.so3_sym_add_f32(p(tg), p(tq), p(pa_), p(s8), None, 1, K, rows, idx, tot, dT, one, mode, b, npts, st)
    timeit("ADD so3_add_l2_f32 (B=256, rows)", lambda i: lib.so3_add_l2_f32(p(tg), p(tq), p(pa_), p(ds), None, None, one, b, npts, st), b * (npts * 12 + 132))
    timeit("ADD so3_add_l2_f32 (B=256, rows + dTpred)", lambda i: lib.so3_add_l2_f32(p(tg), p(tq), p(pa_), p(ds), None, p(dtq), one, b, npts, st), b * (npts * 12 + 196))
    timeit("symADD so3_sym_add_f32 (L2, K=1, rows)", lambda i: sym(1, p(ds), None, None, None, _lib.SYM_ADD_L2), b * (npts * 12 + 132))
    timeit("symADD so3_sym_add_f32 (L2, K=1, rows + dTpred)", lambda i: sym(1, p(ds), None, None, p(dtq), _lib.SYM_ADD_L2), b * (npts * 12 + 196))
    timeit("symADD so3_sym_add_f32 (L2, K=8, rows)", lambda i: sym(kk, p(ds), None, None, None, _lib.SYM_ADD_L2), b * (npts * 12 + 132))
    timeit("symADD so3_sym_add_f32 (L2, K=8, rows + index + loss_sum + dTpred)", lambda i: sym(kk, p(ds), p(ix), p(l1), p(dtq), _lib.SYM_ADD_L2), b * (npts * 12 + 200))
    timeit("symADD so3_sym_add_f32 (L1, K=8, rows + dTpred)", lambda i: sym(kk, p(ds), None, None, p(dtq), _lib.SYM_ADD_L1), b * (npts * 12 + 196))
    timeit("symADD so3_sym_add_f32 (MSSD, K=8, rows)", lambda i: sym(kk, p(ds), None, None, None, _lib.SYM_ADD_MAX), b * (npts * 12 + 132))
    del pa_, tg, tq, pd, nn, ds, dtq, s8, ix
    print("--- config #4: B = 512, bf16 storage, fused head + loss + backward ---")
    b = 512
    x4 = torch.randn(b, 9, device=dev).bfloat16(); r4 = torch.empty(b, 9, device=dev); d4 = torch.empty(b, 9, device=dev, dtype=torch.bfloat16)
    t4 = rr.symmetric_orthogonalization(torch.randn(b, 9, device=dev))
    timeit("K3 so3_frob_fwd_bwd_bf16 (B=512)", lambda i: lib.so3_frob_fwd_bwd_v2_bf16(p(x4), p(t4), p(r4), p(d4), p(ls), None, None, 0, b, st), b * (18 + 36 + 36 + 18), iters=300)
    g4 = torch.empty(b, 9, device=dev)
    timeit("K3' so3_frob_loss_f32 (B=512, loss + dRpred: one launch)", lambda i: lib.so3_frob_loss_v2_f32(p(r4), p(t4), p(g4), p(ls), None, None, 0, b, st), b * 108, iters=300)
    x4f = x4.float(); sc4 = torch.empty(2, dtype=torch.float64, device=dev); fl4 = torch.zeros(1, dtype=torch.int32, device=dev)
    timeit("K4 so3_angle_error (B=512, sum,count + flag: one launch)", lambda i: lib.so3_angle_error_v2(p(r4), p(t4), None, p(sc4), p(fl4), None, 0, b, st), b * 72, iters=300)
    timeit("K1+K4 so3_project_angle_error_f32 (B=512, sum,count + flag)", lambda i: lib.so3_project_angle_error_v2_f32(p(x4f), p(t4), None, None, p(sc4), p(fl4), None, 4, b, st), b * 72, iters=300)
    print("--- config #1: B = 256 ---")
    x1 = torch.randn(256, 9, device=dev); r1 = torch.empty(256, 9, device=dev)
    timeit("K1 so3_project_fwd_f32 (B=256)", lambda i: lib.so3_project_fwd_f32(p(x1), p(r1), None, 256, st), 256 * 72, iters=300)


if __name__ == "__main__":
    main()
