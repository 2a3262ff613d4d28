"""k_add_s / k_add_s_rows / k_add_s_bwd (so3_add_s_fwd_f32, so3_add_s_bwd_f32, so3_cloud_diameter_f32) and k_icp_step / k_icp_finish
(so3_nearest_f32, so3_icp_f32) through the raw C ABI on every work split: the geometry ids G1 .. G7 of tests/search_geometry_ref.py,
whose batch sizes are evaluated from the device's compute units, each its own test id.  tests/test_search_geometry_host.py proves the
expectations without a GPU.

  (a) every output lives in a canary-guarded buffer at a 4-byte, not 16-byte aligned offset (test_gpu_cloud_kernels.Out): every slot
      written, every canary intact, indices in range; the ICP workspace 16-byte aligned, NaN-filled, guarded behind its stated size;
  (b) every cloud and every point against float64 on the device in slices (above search_geometry_ref.F64_PAIRS pairs every k-th cloud: G5),
      at test_add_metrics_host's and test_icp_host's bounds, unchanged; the instantiation through so3_last_kernel() on every case;
      and the indices -- so3_nearest_f32's, the first ICP search's (source through pose_point32) and so3_add_s_fwd_f32's (both clouds
      through it) -- EQUAL to the float32 restatement of the defined order (search_geometry_ref.nearest32 over tests/f32_exact.py), on
      the first cloud, the last and every k-th between within search_geometry_ref.F32_PAIRS pairs (k printed; G4 and G5: the last
      cloud is a second-trip one, asserted by f32_sample).  dist keeps its bound: it passes through v_sqrt_f32 (1 ulp);
  (c) the same cloud gives the same bits at U = 1 (batches of <= 64), 2 and 4, in the reversed batch and on the second grid-stride trip;
  (d) the exact lattice families: ties across tiles and in the padding, the last point, identical clouds, the diameter;
  (e) the optional-output spellings at G4;  (f) a NaN and an Inf cloud change no other cloud.

MUTATIONS.  Each applied alone to a scratch copy of the library, rebuilt, this file run once on an MI355X (256 CUs); what failed:
  mutation                                                caught by                                              by how much (bound)
  k_add_s: index t0 + k + kk -> k + kk                    13: every_split[G1 G2 G3 G5 G6-1025 G6-2047 G6-2049],  index excess 0.35 .. 1.33 (1.9e-6); 8 .. 4428 wrong
                                                          all six exact ADD-S families with N > 1024             indices; no single-tile shape fails
  add_s_pair: d2 < best -> d2 <= best                     5: exact ADD-S ties, last_wins 1025 / 2049; exact      12 .. 47 wrong indices; nothing random sees it
                                                          search ties, last_wins 1025
  k_icp_step: the tile filled from t0 + 0                 33: exact search families, every ICP case              search excess 1.2 .. 2.0 (3.9e-7)
     (pads from the tile's FIRST point instead: an equivalent mutant -- a copy of a point already seen never wins under strict <)
  k_icp_finish: c < chunks -> c < chunks - 1              32: every ICP case                                     inliers differ, or rmse 4.1e-5 .. 5.7e-2 (3.7e-5); G5, where the
                                                                                                                 dropped record holds one real point: rmse 8.1e-5 and the inlier count
  k_icp_step: in ? w : 0.f -> w                           28: every ICP case but N = 256 and N = 1024            inliers differ, or rmse 4.5e-4 .. 0.57 (3.7e-5)
  k_add_s_rows: / N -> / (64 ceil(N / 64))                14: every_split but N = 256 and N = 1024               ADD-S off by 2.3e-5 (N = 2047) .. 1.2 (3.6e-7)
  k_add_s: the poses of the workgroup's first item kept   4: every_split[G4 G5], bits[G4 G5]                     point 0.60 and 0.18 (1.9e-6); bitwise exactly the 37 / 5 clouds
     for its later items                                                                                         of the second trip (74 / 10 against the reversed batch)
  k_icp_step: tile 0 not refilled on later items          9: ICP every_split[G4 G5] x own / shared, search       search excess 0.97 .. 1.9 (3.9e-7); bitwise dist of exactly 37 / 5
     (barriers kept)                                      bits[G4 G5] x own / shared, zero_iterations_at_g4      clouds
The last two are what the geometry is for: nothing below G4's and G5's item counts fails under them.
The k_add_s loop these rows name is tile_search's (so3proj.hip), which k_chamfer_fwd shares; k_icp_step and k_three_nn keep theirs.
Two of the mutations applied to the helper; this file, test_gpu_chamfer.py and test_gpu_three_nn.py run once each:
  tile_search: index t0 + k + kk -> k + kk       33: the 13 ADD-S tests above and 20 of test_gpu_chamfer.py (16 work splits,
                                                 2 x G27, four_points_per_lane, a_small_last_hit)
  tile_search: tile 0 not refilled on later      6: ADD-S every_split[G4 G5] and bits[G4 G5] (point 1.2 and 0.80 against 1.9e-6),
     items (barriers kept)                       chamfer batch_above_the_grid_cap and its bit_for_bit
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import add_metrics_ref as aref
import f32_exact as fx
import icp_ref
import search_geometry_ref as geo
from support import ptr, to_device
import test_add_metrics_host as ahost
import test_icp_host as ihost
from test_gpu_cloud_kernels import CANARY, Out
from test_search_geometry_host import split_step_figures

pytestmark = pytest.mark.gpu

GRAD_SCALE = 0.75
WS_GUARD = 64                        # floats around the ICP workspace: 256 bytes, so it keeps its 16-byte alignment
SMALL = 64                           # clouds per batch of the U = 1 re-runs


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    from poseestimation_amd import _lib
    c = Ctx()
    c._lib, c.lib = _lib, _lib.load()
    assert torch.cuda.is_available()
    c.dev = torch.device("cuda:0")
    c.cus = torch.cuda.get_device_properties(c.dev).multi_processor_count
    c.cases = geo.cases(c.cus)
    c.stream = ctypes.c_void_p(torch.cuda.current_stream(c.dev).cuda_stream)
    c.cache = {}
    yield c
    # leave the device and the host as the next file expects them: the batches of G4 and G5 are a few hundred MB each
    c.cache.clear()
    geo.adds_shared.cache_clear()
    geo.icp_shared.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Buf(Out):
    """A guarded Out of float32 or int32 (a slot that still holds CANARY, as an index 0x7FC5A5A5, was not written)."""

    def __init__(self, dev, shape, dtype=torch.float32):
        super().__init__(dev, shape, True)
        if dtype == torch.int32:
            self.t = self.buf[self.lead:self.lead + self.n].view(shape)
            assert self.t.data_ptr() % 4 == 0 and self.t.data_ptr() % 16 != 0

    def checked(self):
        """The output on the device, after Out.get's checks: every slot written, no canary touched."""
        self.get(slice(0, 0))
        return self.t


def _name(ctx):
    return ctx.lib.so3_last_kernel().decode()


def _in_range(idx, n):
    return bool(((idx >= 0) & (idx < n)).all().item())


# ---- ADD-S, its backward and the diameter --------------------------------------------------------------------------------------------
def run_adds(ctx, tg, tp, pts, rows=None, guarded=True, diameter=True):
    """so3_add_s_fwd_f32 (every output), so3_add_s_bwd_f32 through the returned indices, so3_cloud_diameter_f32: device tensors."""
    b, n = pts.shape[:2]
    mk = (lambda shape, dt=torch.float32: Buf(ctx.dev, shape, dt)) if guarded else (lambda shape, dt=torch.float32: Out(ctx.dev, shape, False))
    pd, dists, dT = mk((b, n)), mk((b,)), mk((b, 4, 4))
    nn = mk((b, n), torch.int32) if guarded else None
    nn_t = nn.t if guarded else torch.full((b, n), -1, dtype=torch.int32, device=ctx.dev)
    chk = ctx._lib.check
    chk(ctx.lib.so3_add_s_fwd_f32(ptr(tg), ptr(tp), ptr(pts), pd.ptr, ptr(nn_t), dists.ptr, None, b, n, ctx.stream), "so3_add_s_fwd_f32")
    out = {"name": _name(ctx)}
    chk(ctx.lib.so3_add_s_bwd_f32(ptr(tg), ptr(tp), ptr(pts), ptr(nn_t), ptr(rows), GRAD_SCALE, dT.ptr, b, n, ctx.stream), "so3_add_s_bwd_f32")
    if diameter:
        work, diam = mk((b, n)), mk((b,))
        chk(ctx.lib.so3_cloud_diameter_f32(ptr(pts), work.ptr, diam.ptr, b, n, ctx.stream), "so3_cloud_diameter_f32")
        out["diam_name"] = _name(ctx)
    torch.cuda.synchronize()
    get = (lambda o: o.checked()) if guarded else (lambda o: o.t)
    out.update(point_dist=get(pd), nearest=get(nn) if guarded else nn_t, adds=get(dists), grad=get(dT))
    if diameter:
        out.update(work=get(work), diam=get(diam))
    assert _in_range(out["nearest"], n)
    return out


def adds_inputs(ctx, case_id):
    """(tgt, tpred, pts, grad_rows) of a geometry id on the device; G2, G3 and G5 share G5's batch."""
    c = ctx.cases[case_id]
    b, n = c["b"], c["n_adds"]
    if case_id in ("G2", "G3", "G5"):
        if "adds_shared" not in ctx.cache:
            tg, tp, pts = (t.to(ctx.dev) for t in geo.adds_shared(ctx.cus))
            rows = torch.randn(len(pts), generator=torch.Generator().manual_seed(3)).to(ctx.dev)
            ctx.cache["adds_shared"] = (tg, tp, pts, rows)
        return tuple(t[:b].contiguous() for t in ctx.cache["adds_shared"])
    if ("adds", case_id) not in ctx.cache:
        tg, tp, pts = (t.to(ctx.dev) for t in geo.adds_inputs(b, n, 600 + geo.IDS.index(case_id)))
        ctx.cache["adds", case_id] = (tg, tp, pts, torch.randn(b, generator=torch.Generator().manual_seed(3)).to(ctx.dev))
    return ctx.cache["adds", case_id]


def adds_figures(got, tg, tp, pts, rows, keep):
    """The figures test_gpu_add_metrics.test_shapes_against_float64... bounds, for the clouds `keep`, in float64 on the device in slices:
    every point's distance and index excess, the rows, the diameter, and the gradient against float64 autograd through the returned
    indices (per cloud: relative to max(1, |grad_rows[b]|))."""
    n = pts.shape[1]
    f = {"point": 0.0, "index_excess": 0.0, "adds": 0.0, "diam": 0.0, "adds_grad": 0.0}
    T = lambda t: t.double()
    keep = torch.as_tensor(keep, device=pts.device)
    step = max(1, (1 << 24) // (n * n))
    for lo in range(0, len(keep), step):
        sl = keep[lo:lo + step]
        p64, nn = T(pts[sl]), got["nearest"][sl].long()
        x, y = aref.pose64(T(tg[sl]), p64), aref.pose64(T(tp[sl]), p64)
        d = torch.linalg.vector_norm(x[:, :, None, :] - y[:, None, :, :], dim=-1)
        pd = d.min(-1).values
        sel = torch.gather(d, 2, nn[:, :, None])[:, :, 0]
        f["point"] = max(f["point"], float((got["point_dist"][sl].double() - pd).abs().max()))
        f["index_excess"] = max(f["index_excess"], float((sel - pd).max()))
        f["adds"] = max(f["adds"], float((got["adds"][sl].double() - pd.mean(-1)).abs().max()))
        del d, sel
        dm = torch.linalg.vector_norm(p64[:, :, None, :] - p64[:, None, :, :], dim=-1).flatten(1).amax(1)
        f["diam"] = max(f["diam"], float((got["diam"][sl].double() - dm).abs().max()))
        f["diam"] = max(f["diam"], float((got["work"][sl].double().amax(1) - got["diam"][sl].double()).abs().max()))      # the row IS the maximum
        tp64 = T(tp[sl]).clone().requires_grad_(True)
        ysel = torch.gather(aref.pose64(tp64, p64), 1, nn[:, :, None].expand(-1, -1, 3))
        r64 = T(rows[sl])
        (torch.linalg.vector_norm(x - ysel, dim=-1).mean(-1) * r64).sum().backward()
        err = (got["grad"][sl].double() - GRAD_SCALE * tp64.grad).abs().flatten(1).amax(1) / r64.abs().clamp(min=1.0)
        f["adds_grad"] = max(f["adds_grad"], float(err.max()))
    return f


def hold(label, f, bounds):
    print(label + "  " + "  ".join("%s %.2e" % kv for kv in f.items()))
    for k, v in f.items():
        assert v <= bounds[k], (label, k, v, bounds[k])


@pytest.mark.parametrize("case_id", geo.IDS)
def test_add_s_backward_and_diameter_on_every_split(ctx, case_id):
    c = ctx.cases[case_id]
    b, n = c["b"], c["n_adds"]
    tg, tp, pts, rows = adds_inputs(ctx, case_id)
    got = run_adds(ctx, tg, tp, pts, rows)
    assert got["name"] == "k_add_s<true, false, %d>" % c["u_adds"] and got["diam_name"] == "k_add_s<false, true, %d>" % c["u_adds"], (got["name"], got["diam_name"])
    if case_id in ("G1", "G2", "G3", "G4", "G5"):
        assert c["u_adds"] == {"G1": 1, "G2": 2, "G3": 4, "G4": 4, "G5": 4}[case_id], (case_id, c)        # the device reaches what the id is for
    if case_id in ("G4", "G5"):
        assert c["items_adds"] > c["cap"] and (case_id != "G4" or b > 4 * 16 * ctx.cus)
    keep = geo.f64_sample(b, n * n)
    f = adds_figures(got, tg, tp, pts, rows, keep)
    hold("%s B=%d N=%d U=%d float64 on %d clouds" % (case_id, b, n, c["u_adds"], len(keep)), f, ahost.BOUNDS)
    assert (got["grad"][:, 3] == 0).all()
    # the defined bits: both clouds through pose_point's fmaf order, pair_dist2, the first of equal candidates -- indices EQUAL
    keep32, k32 = geo.f32_sample(b, n * n, c["items_adds"], c["cap"])
    at = torch.as_tensor(keep32, device=ctx.dev)
    p32 = pts[at].cpu().numpy()
    want = geo.nearest32(*(fx.pose_point32(t[at].cpu().numpy().reshape(-1, 16)[:, :12], p32) for t in (tg, tp)))
    wrong = np.argwhere(got["nearest"][at].cpu().numpy() != want)
    print("%s ADD-S nearest against the float32 restatement: %d clouds (every %d, the first and the last), %d differ" % (case_id, len(keep32), k32, len(wrong)))
    assert len(wrong) == 0, (case_id, len(wrong), keep32[wrong[:4, 0]], wrong[:4, 1], want[tuple(wrong[:4].T)])
    if n == 1:
        assert (got["diam"] == 0).all() and (got["nearest"] == 0).all()


def test_add_s_covers_every_work_item_size(ctx):
    assert {c["u_adds"] for c in ctx.cases.values()} == {1, 2, 4} == {c["u"] for c in ctx.cases.values()}, ctx.cus


def small_batches(ctx, fn, b, keys):
    """fn(lo, hi) over the batch in slices of SMALL clouds: the per-cloud results `keys` concatenated, and the kernels' names."""
    parts = [fn(lo, min(b, lo + SMALL)) for lo in range(0, b, SMALL)]
    return {k: torch.cat([p[k] for p in parts]) for k in keys}, {p["name"] for p in parts}


ADDS_ROWS = ("point_dist", "nearest", "adds", "diam", "grad")


@pytest.mark.parametrize("case_id", ["G2", "G3", "G4", "G5"])
def test_add_s_bits_do_not_depend_on_batch_split_or_trip(ctx, case_id):
    """point_dist, nearest, dists, diam and dTpred of a cloud are the same bits at this id's U and trip, in the reversed batch (another
    workgroup, for most clouds the other trip) and in batches of <= 64 clouds (U = 1)."""
    c = ctx.cases[case_id]
    b = c["b"]
    tg, tp, pts, rows = adds_inputs(ctx, case_id)
    got = run_adds(ctx, tg, tp, pts, rows)
    rev = run_adds(ctx, tg.flip(0).contiguous(), tp.flip(0).contiguous(), pts.flip(0).contiguous(), rows.flip(0).contiguous())
    for k in ADDS_ROWS:
        assert torch.equal(rev[k].flip(0), got[k]), (case_id, "reversed", k, int((rev[k].flip(0) != got[k]).flatten(1).any(1).sum()))
    key = ("adds_small", "shared" if case_id != "G4" else "G4")
    if key not in ctx.cache or len(ctx.cache[key][0]["adds"]) < b:
        full = adds_inputs(ctx, "G5" if case_id != "G4" else "G4")
        ctx.cache[key] = small_batches(ctx, lambda lo, hi: run_adds(ctx, *(t[lo:hi].contiguous() for t in full), guarded=False), len(full[2]), ADDS_ROWS)
    ref, names = ctx.cache[key]
    assert names == {"k_add_s<true, false, 1>"}, names
    for k in ADDS_ROWS:
        assert torch.equal(ref[k][:b], got[k]), (case_id, "U = 1", k, int((ref[k][:b] != got[k]).flatten(1).any(1).sum()))


# ---- the exact families ---------------------------------------------------------------------------------------------------------------
def _exact_dist_ok(dist, d2):
    """Exactly 0 where the square is 0; elsewhere within one float32 ulp of the float64 root of the exact square."""
    want = geo.lattice_dist(d2)
    dist = dist.astype(np.float64)
    return bool((dist[d2 == 0] == 0).all() and (np.abs(dist - want) <= geo.ulp32(want)).all())


@pytest.mark.parametrize("name,n,b", geo.EXACT_ADDS + (("identical", 1025, "G2"), ("identical", 1025, "G3")), ids=lambda v: str(v))
def test_exact_add_s_families(ctx, name, n, b):
    u = None
    if isinstance(b, str):
        u, b = ctx.cases[b]["u_adds"], ctx.cases[b]["b"]
    f = geo.exact_adds_family(name, n, b, geo.exact_seed(name, n))
    tg, tp, pts = (to_device(f[k], ctx.dev, None) for k in ("tgt", "tpred", "pts"))
    rows = torch.randn(b, generator=torch.Generator().manual_seed(4)).to(ctx.dev)
    got = run_adds(ctx, tg, tp, pts, rows)
    assert got["name"] == "k_add_s<true, false, %d>" % (u or geo.rule(b, n, ctx.cus)), got["name"]
    nn, pd = got["nearest"].cpu().numpy(), got["point_dist"].cpu().numpy()
    wrong = np.argwhere(nn != f["nearest"])
    assert len(wrong) == 0, (name, n, len(wrong), wrong[:4], nn[tuple(wrong[:4].T)], f["nearest"][tuple(wrong[:4].T)])
    assert _exact_dist_ok(pd, f["d2"]), (name, n)
    if name in ("identical", "ties"):
        assert (pd == 0).all() and (got["adds"] == 0).all() and (got["grad"] == 0).all(), (name, n)
    if name == "identical":
        assert (nn == np.arange(n)).all()
    if name == "ties":
        assert (nn[:, [1023, 1024, 2048]] == 5).all() and (nn[:, 2047] == 1030).all()
    if name == "last_wins":
        sp = f["special"]
        assert (nn[:, sp + [n - 1]] == n - 1).all() and (pd[:, sp] == geo.QUANTUM).all() and (pd[:, n - 1] == 4 * geo.QUANTUM).all(), (name, n, pd[:, sp])
    diam = np.array([math.sqrt(geo.lattice_diameter2(f["ints"][i % len(f["ints"])])) * geo.QUANTUM for i in range(min(b, 4))])
    want = np.resize(diam, b)
    assert (np.abs(got["diam"].cpu().numpy().astype(np.float64) - want) <= geo.ulp32(want)).all(), (name, n)


def run_nearest(ctx, X, Y, stride, b, n, m, want_index=True):
    dist, nn = Buf(ctx.dev, (b, n)), Buf(ctx.dev, (b, n), torch.int32)
    ctx._lib.check(ctx.lib.so3_nearest_f32(ptr(X), ptr(Y), stride, dist.ptr, nn.ptr if want_index else None, b, n, m, ctx.stream), "so3_nearest_f32")
    name = _name(ctx)
    torch.cuda.synchronize()
    out = {"dist": dist.checked(), "name": name}
    if want_index:
        out["nearest"] = nn.checked()
        assert _in_range(out["nearest"], m)
    else:
        assert nn.untouched()
    return out


@pytest.mark.parametrize("name,n", geo.EXACT_SEARCH, ids=lambda v: str(v))
def test_exact_search_families(ctx, name, n):
    f = geo.exact_search_family(name, n, geo.exact_seed(name, n) + 1)
    got = run_nearest(ctx, to_device(f["X"], ctx.dev, None), to_device(f["Y"], ctx.dev, None), 3 * f["m"], 2, n, f["m"])
    assert got["name"] == "k_icp_step<false, false, false, 1>", got["name"]
    nn, dist = got["nearest"].cpu().numpy(), got["dist"].cpu().numpy()
    wrong = np.argwhere(nn != f["nearest"])
    assert len(wrong) == 0, (name, n, len(wrong), wrong[:4], nn[tuple(wrong[:4].T)], f["nearest"][tuple(wrong[:4].T)])
    assert _exact_dist_ok(dist, f["d2"]), (name, n)
    if name == "ties":
        assert (dist == 0).all() and (nn[:, [1023, 1024, 2048]] == 5).all() and (nn[:, 2047] == 1030).all()
    else:
        assert (nn[:, f["special"] + [n - 1]] == n - 1).all() and (dist[:, f["special"]] == geo.QUANTUM).all()
    shared = run_nearest(ctx, to_device(f["X"], ctx.dev, None), to_device(f["Y"][0], ctx.dev, None), 0, 2, n, f["m"])      # one shared target: cloud 0's
    assert torch.equal(shared["nearest"][0], got["nearest"][0]) and torch.equal(shared["dist"][0], got["dist"][0])


# ---- ICP and the search ---------------------------------------------------------------------------------------------------------------
def run_icp(ctx, P, Q, stride, w, T0, md, it, b, n, m, optional=True, guarded=True):
    """so3_icp_f32 with every output guarded (optional=False: R and t alone), the workspace NaN-filled, 16-byte aligned and guarded behind
    so3_icp_workspace_bytes(B, N)."""
    dev = ctx.dev
    mk = (lambda shape, dt=torch.float32: Buf(dev, shape, dt)) if guarded else (lambda shape, dt=torch.float32: Out(dev, shape, False))
    R, t = mk((b, 3, 3)), mk((b, 3))
    nbytes = ctx.lib.so3_icp_workspace_bytes(b, n)
    assert nbytes % 16 == 0 and nbytes >= b * (24 + 20) * 4
    ws = torch.full((nbytes // 4 + 2 * WS_GUARD,), CANARY, dtype=torch.int32, device=dev)
    inner = ws[WS_GUARD:WS_GUARD + nbytes // 4]
    inner.view(torch.float32).fill_(float("nan"))
    assert inner.data_ptr() % 16 == 0
    out = {}
    if optional:
        rmse, dist = mk((max(it, 1), b)), mk((b, n))
        if guarded:
            inl, nn = mk((max(it, 1), b), torch.int32), mk((b, n), torch.int32)
            inl_t, nn_t = inl.t, nn.t
        else:
            inl_t, nn_t = torch.full((max(it, 1), b), -1, dtype=torch.int32, device=dev), torch.full((b, n), -1, dtype=torch.int32, device=dev)
        args = (rmse.ptr if it else None, ptr(inl_t) if it else None, ptr(nn_t), dist.ptr)
    else:
        args = (None, None, None, None)
    ctx._lib.check(ctx.lib.so3_icp_f32(ptr(P), ptr(Q), stride, ptr(w), ptr(T0), -1.0 if md is None else md, it, R.ptr, t.ptr, *args, ptr(inner),
                                       b, n, m, ctx.stream), "so3_icp_f32")
    out["name"] = _name(ctx)
    torch.cuda.synchronize()
    assert bool((ws[:WS_GUARD] == CANARY).all()) and bool((ws[WS_GUARD + nbytes // 4:] == CANARY).all()), "the workspace's guard was overwritten"
    get = (lambda o: o.checked()) if guarded else (lambda o: o.t)
    out.update(R=get(R), t=get(t))
    if optional:
        out.update(dist=get(dist), nearest=get(nn) if guarded else nn_t)
        if it:
            out.update(rmse=get(rmse), inliers=get(inl) if guarded else inl_t)
        assert _in_range(out["nearest"], m)
    return out


def icp_inputs(ctx, case_id):
    """The numpy inputs of a geometry id and their device copies (G2, G3 and G5 share G5's batch)."""
    if ("icp", case_id) not in ctx.cache:
        c = ctx.cases[case_id]
        d = geo.icp_case_inputs(c, ctx.cus)
        R0, t0 = d["R0"], d["t0"]
        d["T0"] = None if R0 is None else np.ascontiguousarray(np.concatenate([R0, t0[:, :, None]], 2).reshape(-1, 12))
        ctx.cache["icp", case_id] = (d, {k: to_device(v, ctx.dev, None) for k, v in d.items()})
    return ctx.cache["icp", case_id]


def icp_figures(ctx, d, keep, shared, md, got, start, it):
    """test_icp_host's search and step figures of iteration `it` for the clouds `keep`, which started from the float64 poses `start`;
    also asserts the condition on the family: at most 5 % of the clouds without a unique float64 step, none at N >= 255."""
    P, Q = (d["Ps"] if shared else d["P"])[keep], d["Qs"] if shared else d["Q"][keep]
    w = None if d["w"] is None else d["w"][keep]
    Ra, ta = start
    X = icp_ref.pose_points(P, Ra, ta)
    dmin, idx = icp_ref.nearest64(X, Q, ctx.dev)
    sub = {k: (v[:, keep] if k in ("rmse", "inliers") else v[keep]) for k, v in got.items()}
    f = ihost.search_figures(X, Q, sub["dist"], sub["nearest"], dmin)
    unique = geo.unique_step(icp_ref.step_from(P, Q, idx, dmin, Ra, ta, w, md))
    n = P.shape[1]
    if n >= 3:
        assert (~unique).sum() <= 0.05 * len(keep) and (unique.all() or n < 255), ((~unique).sum(), len(keep))
    f.update(split_step_figures(P, Q, w, Ra, ta, md, sub, unique, it))
    return f


ICP_ROWS = ("R", "t", "rmse", "inliers")


def _host(got):
    return {k: v.cpu().numpy() for k, v in got.items() if k != "name"}


@pytest.mark.parametrize("target", ["own", "shared"])
@pytest.mark.parametrize("case_id", geo.IDS)
def test_icp_and_search_on_every_split(ctx, case_id, target):
    c = ctx.cases[case_id]
    b, n, m, u = c["b"], c["n"], c["m"], c["u"]
    shared = target == "shared"
    weighted, trimmed, posed, iterations = geo.icp_mode(case_id)
    d, D = icp_inputs(ctx, case_id)
    P, Q, stride = (D["Ps"], D["Qs"], 0) if shared else (D["P"], D["Q"], 3 * m)
    if case_id in ("G1", "G2", "G3", "G4", "G5"):
        assert u == {"G1": 1, "G2": 2, "G3": 4, "G4": 4, "G5": 4}[case_id], (case_id, c)
    if case_id in ("G4", "G5"):
        assert c["items"] > c["cap"] and (case_id != "G4" or b > 4 * 16 * ctx.cus)
    keep = geo.f64_sample(b, n * m)
    start = tuple(a[keep] for a in geo.initial64(d, b))
    md = None
    if trimmed:
        md = geo.max_distance_for((d["Ps"] if shared else d["P"])[keep], d["Qs"] if shared else d["Q"][keep], d["w"][keep], *start, iterations, ctx.dev)
    label = "%s %s B=%d N=%d M=%d U=%d" % (case_id, target, b, n, m, u)
    bnd = ihost.bounds_g4() if case_id == "G4" else ihost.bounds()      # (R and T at G4: 4 x the host model on G4, see test_icp_host)
    # the search alone, on the raw source points
    near = run_nearest(ctx, P, Q, stride, b, n, m)
    assert near["name"] == "k_icp_step<false, false, false, %d>" % u, near["name"]
    assert torch.equal(run_nearest(ctx, P, Q, stride, b, n, m, want_index=False)["dist"], near["dist"])
    hn = _host(near)
    Pk, Qk = (d["Ps"] if shared else d["P"])[keep], d["Qs"] if shared else d["Q"][keep]
    hold(label + " search", ihost.search_figures(Pk, Qk, hn["dist"][keep], hn["nearest"][keep], device=ctx.dev), ihost.bounds())
    # the defined bits (pair_dist2 from coordinate differences, the first of equal candidates): indices EQUAL the float32 restatement;
    # a posed case restates two searches, so each takes half the pairs
    keep32, k32 = geo.f32_sample(b, (2 if posed else 1) * n * m, c["items"], c["cap"])
    P32, Q32 = (d["Ps"] if shared else d["P"])[keep32], d["Qs"] if shared else d["Q"][keep32]

    def same_indices(what, nearest, X):
        wrong = np.argwhere(nearest[keep32] != geo.nearest32(X, Q32))
        print("%s %s against the float32 restatement: %d clouds (every %d, the first and the last), %d differ" % (label, what, len(keep32), k32, len(wrong)))
        assert len(wrong) == 0, (label, what, len(wrong), keep32[wrong[:4, 0]], wrong[:4, 1])

    same_indices("so3_nearest_f32", hn["nearest"], P32)
    # one iteration, then (G4, G5) two: the second is judged from the pose the first one returned
    one = run_icp(ctx, P, Q, stride, D["w"], D["T0"], md, 1, b, n, m)
    want = "k_icp_step<%s, %s, true, %d>" % (str(weighted).lower(), str(trimmed).lower(), u)
    assert one["name"] == want, (one["name"], want)
    h1 = _host(one)
    hold(label + " iteration 1 of 1", icp_figures(ctx, d, keep, shared, md, h1, start, 0), bnd)
    if not posed:                                            # from the identity nothing is multiplied: the search's own bits
        assert torch.equal(one["dist"], near["dist"]) and torch.equal(one["nearest"], near["nearest"])
    else:                                                    # the source through pose_point's fmaf order first
        same_indices("ICP's first search", h1["nearest"], fx.pose_point32(d["T0"][keep32], P32))
    last = one
    if iterations == 2:
        two = run_icp(ctx, P, Q, stride, D["w"], D["T0"], md, 2, b, n, m)
        assert two["name"] == want
        assert torch.equal(two["rmse"][0], one["rmse"][0]) and torch.equal(two["inliers"][0], one["inliers"][0])
        h2 = _host(two)
        hold(label + " iteration 2 of 2", icp_figures(ctx, d, keep, shared, md, h2, (h1["R"][keep].astype(np.float64), h1["t"][keep].astype(np.float64)), 1), bnd)
        if trimmed:
            frac = h2["inliers"].astype(np.float64).mean() / n
            assert 0.5 < frac < 0.95, frac                   # the trimming trims
        last = two
    # (e) every optional output left out: the same pose
    bare = run_icp(ctx, P, Q, stride, D["w"], D["T0"], md, iterations, b, n, m, optional=False)
    assert torch.equal(bare["R"], last["R"]) and torch.equal(bare["t"], last["t"])
    # (c) within the same batch a cloud's results do not depend on the workgroup and the trip it lands on
    flip = lambda t: None if t is None else t.flip(0).contiguous()
    rev = run_icp(ctx, flip(P), Q if shared else flip(Q), stride, flip(D["w"]), flip(D["T0"]), md, iterations, b, n, m)
    for k in ("dist", "nearest", "R", "t"):
        assert torch.equal(rev[k].flip(0), last[k]), (label, "reversed", k, int((rev[k].flip(0) != last[k]).flatten(1).any(1).sum()))
    for k in ("rmse", "inliers"):
        assert torch.equal(rev[k].flip(1), last[k]), (label, "reversed", k, int((rev[k].flip(1) != last[k]).any(0).sum()))
    ctx.cache["icp_one", case_id, target] = (one["dist"], one["nearest"])


@pytest.mark.parametrize("target", ["own", "shared"])
@pytest.mark.parametrize("case_id", ["G2", "G3", "G4", "G5"])
def test_icp_search_bits_do_not_depend_on_the_work_item_size(ctx, case_id, target):
    """dist and nearest of the first iteration are the same bits at this id's U and in batches of <= 64 clouds (U = 1)."""
    c = ctx.cases[case_id]
    b, n, m = c["b"], c["n"], c["m"]
    shared = target == "shared"
    weighted, trimmed, posed, iterations = geo.icp_mode(case_id)
    d, D = icp_inputs(ctx, case_id)
    P, Q, stride = (D["Ps"], D["Qs"], 0) if shared else (D["P"], D["Q"], 3 * m)
    if ("icp_one", case_id, target) in ctx.cache:
        dist, nearest = ctx.cache["icp_one", case_id, target]
    else:
        one = run_icp(ctx, P, Q, stride, D["w"], D["T0"], None, 1, b, n, m)
        dist, nearest = one["dist"], one["nearest"]
    cut = lambda t, lo, hi: None if t is None else t[lo:hi].contiguous()
    ref, names = small_batches(ctx, lambda lo, hi: run_icp(ctx, cut(P, lo, hi), Q if shared else cut(Q, lo, hi), stride, cut(D["w"], lo, hi), cut(D["T0"], lo, hi),
                                                            None, 1, hi - lo, n, m, guarded=False), b, ("dist", "nearest"))
    assert names == {"k_icp_step<%s, false, true, 1>" % str(weighted).lower()}, names
    for k, mine in (("dist", dist), ("nearest", nearest)):
        assert torch.equal(ref[k], mine), (case_id, target, k, int((ref[k] != mine).any(1).sum()))


# ---- the optional outputs at G4 ------------------------------------------------------------------------------------------------------
def test_optional_outputs_at_g4(ctx):
    c = ctx.cases["G4"]
    b, n = c["b"], c["n_adds"]
    tg, tp, pts, rows = adds_inputs(ctx, "G4")
    got = run_adds(ctx, tg, tp, pts, rows, diameter=False)
    pd, nn = Buf(ctx.dev, (b, n)), Buf(ctx.dev, (b, n), torch.int32)
    total = torch.full((3,), float("nan"), dtype=torch.float64, device=ctx.dev)
    # no indices, no rows: one workgroup walks all 64 CUs + 37 rows and leaves their sum
    ctx._lib.check(ctx.lib.so3_add_s_fwd_f32(ptr(tg), ptr(tp), ptr(pts), pd.ptr, None, None, ctypes.c_void_p(total.data_ptr() + 8), b, n, ctx.stream), "so3_add_s_fwd_f32")
    assert _name(ctx) == "k_add_s<false, false, %d>" % c["u_adds"]
    torch.cuda.synchronize()
    assert torch.equal(pd.checked(), got["point_dist"]) and nn.untouched()
    t = total.cpu().numpy()
    want = math.fsum(got["adds"].cpu().numpy().astype(np.float64))
    print("G4 loss_sum %.17g  fsum(rows) %.17g  difference %.3e" % (t[1], want, abs(t[1] - want)))
    assert np.isnan(t[0]) and np.isnan(t[2]) and abs(t[1] - want) <= 1e-12 * b, (t, want)
    # rows and the total: the second, one-workgroup sum over the rows
    dists = Buf(ctx.dev, (b,))
    ctx._lib.check(ctx.lib.so3_add_s_fwd_f32(ptr(tg), ptr(tp), ptr(pts), pd.ptr, None, dists.ptr, ptr(total), b, n, ctx.stream), "so3_add_s_fwd_f32")
    torch.cuda.synchronize()
    assert torch.equal(dists.checked(), got["adds"]) and abs(total[0].item() - want) <= 1e-12 * b
    # grad_rows == NULL is a row of ones
    ones = run_adds(ctx, tg, tp, pts, torch.ones(b, device=ctx.dev), diameter=False)
    none = run_adds(ctx, tg, tp, pts, None, diameter=False)
    assert torch.equal(ones["grad"], none["grad"])


def test_zero_iterations_at_g4(ctx):
    """iterations == 0 with nearest / dist requested: the initial pose comes back and the search is the one the first iteration runs, bit
    for bit; against so3_nearest_f32 on points torch posed it agrees as test_gpu_icp's B = 3 case does."""
    c = ctx.cases["G4"]
    b, n, m = c["b"], c["n"], c["m"]
    d, D = icp_inputs(ctx, "G4")
    zero = run_icp(ctx, D["P"], D["Q"], 3 * m, D["w"], D["T0"], None, 0, b, n, m)
    assert zero["name"] == "k_icp_step<false, false, false, %d>" % c["u"]
    assert torch.equal(zero["R"], D["R0"]) and torch.equal(zero["t"], D["t0"])
    one = run_icp(ctx, D["P"], D["Q"], 3 * m, D["w"], D["T0"], None, 1, b, n, m)
    assert torch.equal(zero["dist"], one["dist"]) and torch.equal(zero["nearest"], one["nearest"])
    X = (torch.einsum("bij,bnj->bni", D["R0"], D["P"]) + D["t0"][:, None]).contiguous()
    near = run_nearest(ctx, X, D["Q"], 3 * m, b, n, m)
    assert (near["dist"] - zero["dist"]).abs().max().item() <= 1e-5
    ident = run_icp(ctx, D["P"], D["Q"], 3 * m, None, None, None, 0, b, n, m)
    assert torch.equal(ident["R"], torch.eye(3, device=ctx.dev).expand(b, 3, 3)) and (ident["t"] == 0).all()
    raw = run_nearest(ctx, D["P"], D["Q"], 3 * m, b, n, m)
    assert torch.equal(ident["dist"], raw["dist"]) and torch.equal(ident["nearest"], raw["nearest"])


# ---- non-finite clouds ------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_cloud_changes_no_other(ctx):
    """A G4-sized batch with a NaN point in one cloud of the first trip and an Inf point in one of the second: every other cloud's outputs
    keep their bits, every index stays in range, the calls return 0.  Nothing is asserted about the two clouds' own values."""
    c = ctx.cases["G4"]
    b, n, m = c["b"], c["n"], c["m"]
    bad = [100, c["cap"] + 20]
    others = torch.ones(b, dtype=torch.bool, device=ctx.dev)
    others[bad] = False
    tg, tp, pts, rows = adds_inputs(ctx, "G4")
    clean = run_adds(ctx, tg, tp, pts, rows)
    dirty_pts = pts.clone()
    dirty_pts[bad[0], 3, 1] = float("nan")
    dirty_pts[bad[1], c["n_adds"] - 1, 0] = float("inf")
    dirty = run_adds(ctx, tg, tp, dirty_pts, rows)
    for k in ADDS_ROWS + ("work",):
        assert torch.equal(dirty[k][others], clean[k][others]), k
    d, D = icp_inputs(ctx, "G4")
    R0, t0 = geo.initial64(d, b)
    md = geo.max_distance_for(d["P"], d["Q"], d["w"], R0, t0, 2, ctx.dev)
    for shared in (False, True):
        P, Q, stride = (D["Ps"], D["Qs"], 0) if shared else (D["P"], D["Q"], 3 * m)
        clean = run_icp(ctx, P, Q, stride, D["w"], D["T0"], md, 2, b, n, m)
        P2, Q2 = P.clone(), Q.clone()
        P2[bad[0], 5, 2] = float("nan")
        P2[bad[1], n - 1, 0] = float("inf")
        if not shared:
            Q2[bad[0], 0, 0] = float("nan")
            Q2[bad[1], m - 1, 1] = -float("inf")
        dirty = run_icp(ctx, P2, Q2, stride, D["w"], D["T0"], md, 2, b, n, m)
        for k in ("dist", "nearest", "R", "t"):
            assert torch.equal(dirty[k][others], clean[k][others]), (shared, k)
        for k in ("rmse", "inliers"):
            assert torch.equal(dirty[k][:, others], clean[k][:, others]), (shared, k)
        near_clean, near_dirty = run_nearest(ctx, P, Q, stride, b, n, m), run_nearest(ctx, P2, Q2, stride, b, n, m)
        for k in ("dist", "nearest"):
            assert torch.equal(near_dirty[k][others], near_clean[k][others]), (shared, k)
