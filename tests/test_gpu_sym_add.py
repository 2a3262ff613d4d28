"""compute_symmetric_ADD_loss, compute_symmetric_ADD_L1_loss and compute_MSSD (so3_sym_add_f32) on the GPU: G26 through the Python
surface and through the raw C ABI at the bounds of tests/test_sym_add_host.py (4 x the float32 host model's error; see its docstring),
the exact cases, every launch geometry the kernel has, class ids, autograd, repeatability and graph replay, and the speed condition
against the torch composition the feature replaces.

The shapes' clouds and poses are of G26's scale (unit radius, two units from the origin), so its bounds apply; at coordinates of 1e3
every quantity but dt_pred's gradient is homogeneous of degree one in (points, translations) and the bounds are scaled by 1e3.
A register sweep is 1024 points (so3::kSymAddSweep), so 1024 / 1025 are the sizes either side of it; 128 / 129 and 512 / 513 are the
thresholds between the three unroll instantiations."""
import functools

import numpy as np
import pytest
import torch

from support import dev  # noqa: F401
import sym_add_ref as ref
import test_sym_add_host as host
import test_gpu_add_metrics as add_gpu

pytestmark = pytest.mark.gpu

MODES = (ref.L2, ref.L1, ref.MAX)


@pytest.fixture(scope="module")
def g26_cases():
    return ref.cases(ref.g26())


def _table(S):
    """The SymmetryTable whose float32 entries are exactly the (C,K,3,3) array S (identity first, padded with the identity)."""
    import poseestimation_amd as pa
    S = np.asarray(S, np.float32)
    t = pa.SymmetryTable([S[c] for c in range(S.shape[0])] if S.shape[0] > 1 else S[0])
    assert (t.num_classes, t.K) == S.shape[:2] and np.array_equal(t._host.numpy().reshape(S.shape), S)
    return t


def abi_run(c, dev, scale=1.0, modes=MODES):
    """One case through the raw C ABI into NaN / -2 pre-filled buffers, results as host.host_run gives them (plus "sum").  Every requested
    element must have been written; a second call with only the rows requested (everything else NULL) gives the same rows."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    b, n = c["b"], c["n"]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    tg, tp, pts, S = (up(c[k], np.float32) for k in ("tgt", "tpred", "pts", "S"))
    cls = None if c["cls"] is None else up(c["cls"], np.int32)
    P = lambda t: None if t is None else t.data_ptr()
    s = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for mode in modes:
        dist = torch.full((b,), float("nan"), dtype=torch.float32, device=dev)
        index = torch.full((b,), -2, dtype=torch.int32, device=dev)
        total = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        grad = None if mode == ref.MAX else torch.full((b, 4, 4), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(lib.so3_sym_add_f32(P(tg), P(tp), P(pts), P(S), P(cls), c["C"], c["K"], P(dist), P(index), P(total), P(grad), scale, mode,
                                       b, n, s), "so3_sym_add_f32")
        only = torch.full((b,), float("nan"), dtype=torch.float32, device=dev)
        _lib.check(lib.so3_sym_add_f32(P(tg), P(tp), P(pts), P(S), P(cls), c["C"], c["K"], P(only), None, None, None, scale, mode, b, n, s),
                   "so3_sym_add_f32")
        alone = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)            # the total alone: one workgroup, its own order
        _lib.check(lib.so3_sym_add_f32(P(tg), P(tp), P(pts), P(S), P(cls), c["C"], c["K"], None, None, P(alone), None, scale, mode, b, n, s),
                   "so3_sym_add_f32")
        torch.cuda.synchronize()
        assert np.array_equal(only.cpu().numpy(), dist.cpu().numpy(), equal_nan=True)
        out[mode] = {"dist": dist.cpu().numpy(), "index": index.cpu().numpy(), "grad": None if grad is None else grad.cpu().numpy(),
                     "sum": total.item(), "sum_alone": alone.item()}
    return out


def surface_run(c, dev, table=None):
    """One case through the Python surface, results as host.host_run gives them."""
    import poseestimation_amd as pa
    table = _table(c["S"]) if table is None else table
    tg, pts = torch.from_numpy(c["tgt"]).to(dev), torch.from_numpy(c["pts"]).to(dev)
    cls = None if c["cls"] is None else torch.from_numpy(np.ascontiguousarray(c["cls"])).to(dev)
    out = {}
    for mode, fn in ((ref.L2, pa.compute_symmetric_ADD_loss), (ref.L1, pa.compute_symmetric_ADD_L1_loss)):
        tp = torch.from_numpy(c["tpred"]).to(dev).requires_grad_(True)
        rows, idx = fn(tg, tp, pts, table, cls, use_batch_mean=False, return_index=True)
        assert rows.shape == (c["b"],) and rows.dtype == torch.float32 and idx.dtype == torch.int32 and not idx.requires_grad
        (g,) = torch.autograd.grad(rows.sum(), tp)
        out[mode] = {"dist": rows.detach().cpu().numpy(), "index": idx.cpu().numpy(), "grad": g.cpu().numpy()}
    rows, idx = pa.compute_MSSD(tg, torch.from_numpy(c["tpred"]).to(dev), pts, table, cls, return_index=True)
    assert not rows.requires_grad
    out[ref.MAX] = {"dist": rows.cpu().numpy(), "index": idx.cpu().numpy(), "grad": None}
    return out


# ---- against G26 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["surface", "abi"])
def test_g26_values_indices_and_gradients(dev, g26_cases, route):
    run = (lambda c: surface_run(c, dev)) if route == "surface" else (lambda c: abi_run(c, dev))
    host.check_against_g26(g26_cases, run, "gpu/" + route)


@pytest.mark.parametrize("route", ["surface", "abi"])
def test_g26_exact_cases(dev, g26_cases, route):
    import poseestimation_amd as pa
    for c in g26_cases:
        if c["family"] not in ("exact_c4", "identical_points") and not (c["family"] == "haar" and c["C"] > 1):
            continue
        table = pa.SymmetryTable(pa.cyclic_symmetry(4, "z")) if c["family"] == "exact_c4" else None
        if table is not None:
            assert np.array_equal(table._host.reshape(1, 4, 3, 3).numpy(), c["S"])               # cyclic_symmetry's exact entries are the fixture's
        got = surface_run(c, dev, table) if route == "surface" else abi_run(c, dev)
        host.exact_case_checks(c, got)
        if c["family"] == "exact_c4" and c["n"] > 1:                                             # plain ADD is large where the symmetric one is 0
            tg, tp, pts = (torch.from_numpy(c[k]).to(dev) for k in ("tgt", "tpred", "pts"))
            assert (pa.compute_ADD_loss(tg, tp, pts, use_batch_mean=False)[1:] > 0.1).all()


def test_trivial_table_is_plain_add(dev, g26_cases):
    """Table {I}: compute_ADD_loss / compute_ADD_L1_loss within the bounds (bit-equality is not required: the sums' orders differ)."""
    import poseestimation_amd as pa
    table = pa.SymmetryTable(torch.eye(3)[None])
    for c in g26_cases:
        tg, tp, pts = (torch.from_numpy(c[k]).to(dev) for k in ("tgt", "tpred", "pts"))
        for sym, plain, tol, gtol in ((pa.compute_symmetric_ADD_loss, pa.compute_ADD_loss, host.L2_TOL, host.L2_GRAD_TOL),
                                      (pa.compute_symmetric_ADD_L1_loss, pa.compute_ADD_L1_loss, host.L1_TOL, host.L1_GRAD_TOL)):
            a, b_ = tp.clone().requires_grad_(True), tp.clone().requires_grad_(True)
            got, idx = sym(tg, a, pts, table, use_batch_mean=False, return_index=True)
            want = plain(tg, b_, pts, use_batch_mean=False)
            assert float((got - want).detach().abs().max()) <= tol and (idx == 0).all()
            got.sum().backward()
            want.sum().backward()
            assert float((a.grad - b_.grad).abs().max()) <= gtol


# ---- every launch geometry -------------------------------------------------------------------------------------------------
def _group(k, axis):
    import poseestimation_amd as pa
    return pa.cyclic_symmetry(k, axis).numpy()


@functools.lru_cache(maxsize=None)
def _shape_case(b, n, k, classes, coord):
    """A case of G26's layout with its float64 answers, computed once per shape: a third of the rows unrelated poses, the others within
    0.05 of T_gt S_j^-1 (the winner is mostly j, not the identity)."""
    if classes == 1:
        groups = [_group(k, "z" if k % 2 else "y")]
    else:
        groups = [_group(k, "z"), _group(7, "x"), np.eye(3)[None], _group(9, [1.0, 2.0, 3.0])][:classes]
    S = np.broadcast_to(np.eye(3), (classes, k, 3, 3)).copy()
    for c, g in enumerate(groups):
        S[c, :len(g)] = g
    S = S.astype(np.float32)
    cpu = torch.device("cpu")
    tg, far = add_gpu._poses(b, cpu, seed=b + n)
    _, near = add_gpu._poses(b, cpu, err=0.05, seed=b + n)
    cls = None if classes == 1 else (np.arange(b) * 7 % classes).astype(np.int32)
    rows = ref.rows_of(S, cls, b)
    j = np.arange(b) % k
    near[:, :3, :3] = near[:, :3, :3] @ torch.from_numpy(rows[np.arange(b), j].astype(np.float32)).transpose(1, 2)
    tp = torch.where((torch.arange(b) % 3 == 0)[:, None, None], far, near)
    pts = add_gpu._cloud(b, n, cpu, seed=n + k)
    tg, tp, pts = tg.numpy().copy(), tp.numpy().copy(), pts.numpy().copy()
    if coord != 1.0:
        pts *= np.float32(coord)
        tg[:, :3, 3] *= np.float32(coord)
        tp[:, :3, 3] *= np.float32(coord)
    c = {"family": "shape", "b": b, "n": n, "C": classes, "K": k, "tgt": tg, "tpred": tp, "pts": pts, "S": S, "cls": cls}
    st = ref.stats(tg, tp, pts, rows)
    c.update(stat_l2=st[ref.L2], stat_l1=st[ref.L1], stat_max=st[ref.MAX])
    return c


SHAPES = [(1, 1, 1, 1), (3, 63, 2, 1), (65, 64, 7, 1), (3, 65, 8, 1), (3, 128, 3, 1), (3, 129, 3, 1), (3, 512, 3, 1), (3, 513, 3, 1),
          (300, 1000, 9, 1), (3, 1024, 64, 1), (65, 1025, 2, 1), (4, 2500, 8, 1), (300, 100, 64, 4), (8200, 5, 2, 1)]


@pytest.mark.parametrize("b,n,k,classes", SHAPES)
def test_shapes_against_float64_and_bitwise_repeatable(dev, b, n, k, classes):
    """N either side of a wave (63 / 64 / 65), of the unroll thresholds and of a register sweep (1000 / 1024 / 1025, 2500: three sweeps);
    K in {1, 2, 7, 8, 9, 64}; one class and 4 x 64 = 256 table entries with mixed ids; B in {1, 3, 65, 300} and 8200, above the grid's
    cap of eight workgroups of four waves per compute unit (8192 rows in flight on 256 CUs).  Through the raw ABI."""
    _check_shape(dev, _shape_case(b, n, k, classes, 1.0), 1.0)


def test_coordinates_at_1e3(dev):
    _check_shape(dev, _shape_case(65, 300, 4, 1, 1e3), 1e3)


def _check_shape(dev, c, coord):
    got, again = abi_run(c, dev), abi_run(c, dev)
    srows = ref.rows_of(c["S"], c["cls"], c["b"])
    for mode in MODES:
        g, tol = got[mode], host.VALUE_TOL[mode] * coord
        assert g["index"].min() >= 0 and g["index"].max() < c["K"]
        err, over = ref.excess(c[host.STAT_KEY[mode]], g["dist"], g["index"])
        print("gpu/shape B=%d N=%d K=%d C=%d mode %d: value %.2e index %.2e (bound %.2e)" % (c["b"], c["n"], c["K"], c["C"], mode, err, over, tol))
        assert err <= tol and over <= tol, (mode, err, over, tol)
        assert np.array_equal(g["dist"], again[mode]["dist"]) and np.array_equal(g["index"], again[mode]["index"])      # two calls: the same bits
        assert g["sum"] == again[mode]["sum"] and g["sum_alone"] == again[mode]["sum_alone"]
        want = g["dist"].astype(np.float64).sum()
        assert abs(g["sum"] - want) <= 1e-12 * max(1.0, abs(want)) and abs(g["sum_alone"] - want) <= 1e-12 * max(1.0, abs(want))
        if mode != ref.MAX:
            assert np.array_equal(g["grad"], again[mode]["grad"])
            ref_grad = ref.grad_autograd(mode, c["tgt"], c["tpred"], c["pts"], srows, g["index"])
            gerr = np.abs(g["grad"] - ref_grad)
            gtol = host.GRAD_TOL[mode]
            print("    gradient dR %.2e dt %.2e (bound %.2e)" % (gerr[:, :3, :3].max(), gerr[:, :3, 3].max(), gtol))
            assert gerr[:, :3, :3].max() <= gtol * coord and gerr[:, :3, 3].max() <= gtol and (g["grad"][:, 3] == 0).all()
    assert (got[ref.MAX]["dist"] >= got[ref.L2]["dist"]).all()
    if c["K"] > 1:
        assert (got[ref.L2]["index"] > 0).any()


def test_every_instantiation_runs(dev):
    """so3_last_kernel names the kernel of the last call: three modes, with and without the gradient, three unrolls."""
    from poseestimation_amd import _lib
    lib = _lib.load()
    seen = set()
    for n, u in ((100, 2), (128, 2), (129, 8), (512, 8), (513, 16), (3000, 16)):
        c = _shape_case(3, n, 3, 1, 1.0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        tg, tp, pts, S = (up(c[k]) for k in ("tgt", "tpred", "pts", "S"))
        rows, dT = torch.empty(3, device=dev), torch.empty(3, 4, 4, device=dev)
        for mode in MODES:
            for grad in ((False,) if mode == ref.MAX else (False, True)):
                _lib.check(lib.so3_sym_add_f32(tg.data_ptr(), tp.data_ptr(), pts.data_ptr(), S.data_ptr(), None, 1, 3, rows.data_ptr(), None, None,
                                               dT.data_ptr() if grad else None, 1.0, mode, 3, n, torch.cuda.current_stream(dev).cuda_stream),
                           "so3_sym_add_f32")
                name = lib.so3_last_kernel().decode()
                assert name == "k_sym_add<%d, %s, %d>" % (mode, "true" if grad else "false", u), (n, mode, grad, name)
                seen.add(name)
    torch.cuda.synchronize()
    assert len(seen) == 15


# ---- class ids and points --------------------------------------------------------------------------------------------------
def test_class_ids_out_of_range_int64_and_shared_model(dev):
    import poseestimation_amd as pa
    c = _shape_case(65, 129, 9, 4, 1.0)
    table = _table(c["S"])
    tg, tp, pts = (torch.from_numpy(c[k]).to(dev) for k in ("tgt", "tpred", "pts"))
    cls = torch.from_numpy(c["cls"]).to(dev)
    bad = cls.clone()
    bad[5], bad[40] = -1, 4
    keep = torch.ones(65, dtype=torch.bool, device=dev)
    keep[[5, 40]] = False
    for fn in (pa.compute_symmetric_ADD_loss, pa.compute_symmetric_ADD_L1_loss):
        a, b_ = tp.clone().requires_grad_(True), tp.clone().requires_grad_(True)
        rows, idx = fn(tg, a, pts, table, bad, use_batch_mean=False, return_index=True)
        clean, cidx = fn(tg, b_, pts, table, cls, use_batch_mean=False, return_index=True)
        assert torch.isnan(rows[~keep]).all() and (idx[~keep] == -1).all()
        assert torch.equal(rows[keep], clean[keep]) and torch.equal(idx[keep], cidx[keep])                   # the other rows untouched
        rows[keep].sum().backward()
        clean[keep].sum().backward()
        assert torch.equal(a.grad[keep], b_.grad[keep]) and (a.grad[:, 3] == 0).all()
        assert torch.isnan(fn(tg, tp, pts, table, bad)) and torch.isfinite(fn(tg, tp, pts, table, cls))      # a NaN loss_sum
        rows64, idx64 = fn(tg, tp, pts, table, bad.long() * 3_000_000_000, use_batch_mean=False, return_index=True)      # int64 ids, far out of int32
        far = bad.long() * 3_000_000_000
        ok = (far >= 0) & (far < 4)
        assert torch.equal(rows64[ok], clean.detach()[ok]) and torch.isnan(rows64[~ok]).all() and (idx64[~ok] == -1).all()
        assert torch.equal(fn(tg, tp, pts, table, cls.long(), use_batch_mean=False), clean.detach())
    # the gradient row of a bad id through the raw ABI: twelve NaN, the bottom row 0
    got = abi_run(dict(c, cls=bad.cpu().numpy()), dev, modes=(ref.L2,))[ref.L2]
    assert np.isnan(got["grad"][[5, 40], :3]).all() and (got["grad"][:, 3] == 0).all() and np.isnan(got["sum"]) and np.isnan(got["sum_alone"])
    assert np.isfinite(got["grad"][keep.cpu().numpy()]).all()
    m, midx = pa.compute_MSSD(tg, tp, pts, table, bad, return_index=True)
    assert torch.isnan(m[~keep]).all() and (midx[~keep] == -1).all() and torch.equal(m[keep], pa.compute_MSSD(tg, tp, pts, table, cls)[keep])
    # one (N,3) model shared by the batch = the expanded call
    one = pts[0].contiguous()
    full = one.unsqueeze(0).expand(65, -1, -1).contiguous()
    for fn in (pa.compute_symmetric_ADD_loss, pa.compute_symmetric_ADD_L1_loss):
        assert torch.equal(fn(tg, tp, one, table, cls, use_batch_mean=False), fn(tg, tp, full, table, cls, use_batch_mean=False))
    assert torch.equal(pa.compute_MSSD(tg, tp, one, table, cls), pa.compute_MSSD(tg, tp, full, table, cls))
    with pytest.raises(ValueError, match="needs class_ids"):
        pa.compute_MSSD(tg, tp, pts, table)
    with pytest.raises(ValueError, match="single-class"):
        pa.compute_MSSD(tg, tp, pts, pa.SymmetryTable(pa.cyclic_symmetry(2)), cls)


# ---- autograd --------------------------------------------------------------------------------------------------------------
def test_autograd_per_sample_batch_mean_and_strided_upstream(dev):
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    c = _shape_case(65, 300, 4, 1, 1.0)
    table = _table(c["S"])
    b = c["b"]
    tg, tp, pts = (torch.from_numpy(c[k]).to(dev) for k in ("tgt", "tpred", "pts"))
    srows = ref.rows_of(c["S"], None, b)
    w2 = torch.randn(b, 2, generator=torch.Generator().manual_seed(9)).to(dev)
    w = w2[:, 0]                                                                     # a non-contiguous upstream gradient
    assert not w.is_contiguous()
    for mode, fn in ((ref.L2, pa.compute_symmetric_ADD_loss), (ref.L1, pa.compute_symmetric_ADD_L1_loss)):
        a = tp.clone().requires_grad_(True)
        rows, idx = fn(tg, a, pts, table, use_batch_mean=False, return_index=True)
        want = ref.grad_autograd(mode, c["tgt"], c["tpred"], c["pts"], srows, idx.cpu().numpy())
        (g,) = torch.autograd.grad(rows, a, grad_outputs=w)
        wmax = float(w.abs().max().clamp(min=1.0))
        assert float((g.double().cpu() - torch.from_numpy(want) * w.double().cpu()[:, None, None]).abs().max()) <= host.GRAD_TOL[mode] * wmax
        a2 = tp.clone().requires_grad_(True)
        mean = fn(tg, a2, pts, table)
        assert mean.dim() == 0 and abs(mean.item() - rows.detach().double().mean().item()) <= 2.0**-23 * max(1.0, abs(mean.item()))
        (2.5 * mean).backward()
        assert float((a2.grad.double().cpu() - torch.from_numpy(want) * (2.5 / b)).abs().max()) <= host.GRAD_TOL[mode] * 2.5 / b + 1e-9
        # T_gt requiring grad: a warning, and no gradient for it
        rr._WARNED.discard(fn.__name__ + "_constants")
        tgg, a3 = tg.clone().requires_grad_(True), tp.clone().requires_grad_(True)
        with pytest.warns(RuntimeWarning, match="TCO_pred only"):
            fn(tgg, a3, pts, table).backward()
        assert tgg.grad is None and a3.grad is not None
        # double backward is refused, never returned wrong: the backward's result is a constant of the graph, and a cotangent that
        # requires grad raises in the node itself (as _SymLossFrobenius)
        a4 = tp.clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="differentiate twice|does not require grad"):
            (g1,) = torch.autograd.grad(fn(tg, a4, pts, table), a4, create_graph=True)
            g1.sum().backward()
        go = torch.ones((), device=dev, requires_grad=True)
        with pytest.raises(RuntimeError, match="differentiate twice"):
            torch.autograd.grad(fn(tg, a4, pts, table), a4, grad_outputs=go, create_graph=True)
        assert not fn(tg, tp, pts, table).requires_grad                                                   # nothing to differentiate: no gradient buffer
    rr._WARNED.discard("compute_MSSD")
    with pytest.warns(RuntimeWarning, match="no gradient"):
        assert not pa.compute_MSSD(tg, tp.clone().requires_grad_(True), pts, table).requires_grad


# ---- repeatability -----------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_eager_bits(dev):
    import poseestimation_amd as pa
    c = _shape_case(65, 1025, 2, 1, 1.0)
    table = _table(c["S"]).to(dev)
    tg, pts = (torch.from_numpy(c[k]).to(dev) for k in ("tgt", "pts"))
    tp = torch.from_numpy(c["tpred"]).to(dev).requires_grad_(True)

    def step():
        loss, idx = pa.compute_symmetric_ADD_loss(tg, tp, pts, table, return_index=True)
        (g,) = torch.autograd.grad(loss, tp)
        l1 = pa.compute_symmetric_ADD_L1_loss(tg, tp.detach(), pts, table, use_batch_mean=False)
        return loss.detach(), idx, g, l1, pa.compute_MSSD(tg, tp.detach(), pts, table)

    eager = [t.clone() for t in step()]
    assert all(torch.equal(a, b_) for a, b_ in zip(eager, step()))                  # two eager calls: equal bits, loss_sum's mean included
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()                                                                      # warm the allocator on the capture stream
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(eager, captured))


# ---- speed, as a condition --------------------------------------------------------------------------------------------------
def test_symmetric_add_is_not_slower_than_the_torch_composition(dev):
    """B = 256, N = 1024, K = 8, HIP events, 5 warm-ups, median of 20: compute_symmetric_ADD_loss(use_batch_mean=False) under no_grad
    against the torch spelling on the same device -- einsum of R_pred @ S, the posed clouds, norm, mean, min."""
    import poseestimation_amd as pa
    from conftest import REPORT_LINES
    b, n, k = 256, 1024, 8
    tg, tp = add_gpu._poses(b, dev, seed=11)
    pts = add_gpu._cloud(b, n, dev, seed=12)
    table = pa.SymmetryTable(pa.cyclic_symmetry(k, "z")).to(dev)
    S = table._host.reshape(k, 3, 3).to(dev)

    def torch_spelling(tg, tp, pts, S):
        a = torch.einsum("bil,klj->bkij", tp[:, :3, :3], S)
        x = torch.einsum("bij,bnj->bni", tg[:, :3, :3], pts) + tg[:, None, :3, 3]
        y = torch.einsum("bkij,bnj->bkni", a, pts) + tp[:, None, None, :3, 3]
        return (x[:, None] - y).norm(dim=-1).mean(-1).min(-1).values

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
        ours = median_ms(lambda: pa.compute_symmetric_ADD_loss(tg, tp, pts, table, use_batch_mean=False))
        theirs = median_ms(lambda: torch_spelling(tg, tp, pts, S))
        got = pa.compute_symmetric_ADD_loss(tg, tp, pts, table, use_batch_mean=False)
        want = torch_spelling(tg.double(), tp.double(), pts.double(), S.double())
    line = "symmetric ADD B=256 N=1024 K=8: compute_symmetric_ADD_loss %.4f ms, torch einsum/norm/mean/min %.4f ms (x%.1f)" % (
        ours, theirs, theirs / ours)
    print(line)
    REPORT_LINES.append(line)
    assert float((got.double() - want).abs().max()) <= host.L2_TOL
    assert theirs / ours >= 1.0, line
