"""K4s / K3s on the device: symmetric_angle_error and symmetric_loss_frobenius against G17 (the reference's angle_error and
loss_frobenius on every candidate R_pred @ S_k), against the float64 oracle of tests/test_symmetry_host.py at batch sizes derived from
the CU count (one workgroup, the ticket finish, the grid-stride loop of the streaming engine, its remainder), and against angle_error /
loss_frobenius for the table {I}."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_symmetry_host import TABLES, g17_case, sym_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import poseestimation_amd
    return poseestimation_amd


def cuda(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def haar(n, gen):
    q = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))[0]
    return q * torch.det(q).sign()[:, None, None]


def engine_sizes():
    """Rows per engine round of the whole grid: CUs workgroups x 16 waves x 64 rows."""
    per = torch.cuda.get_device_properties(0).multi_processor_count * 16 * 64
    return [1, 63, 64, 1023, 1024, 1025, per - 1, per, per + 63, 3 * per + 17]


def ten_class_table(pa):
    """Ten classes with 1 .. 8 elements (C_1 .. C_8 about varied axes; two of them rotate_by_180's set and C_2(z) again)."""
    axes = ["z", "y", "x", [1.0, 1.0, 0.0], [0.3, -0.2, 0.9], "z", "y", [1.0, 2.0, 3.0]]
    flip = torch.stack([torch.eye(3, dtype=torch.float64)] + [torch.diag(torch.tensor(d, dtype=torch.float64))
                                                              for d in ([1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1])])
    groups = [pa.cyclic_symmetry(n, axes[n - 1]) for n in range(1, 9)] + [flip, pa.cyclic_symmetry(2, "z")]
    return pa.SymmetryTable(groups)


def assert_angles(got, want, label=""):
    """1e-9 degrees, widened where acos itself is ill-conditioned: two float64 traces of one product in different orders differ by a
    few ulps (4.5e-16 at cosine 1), which moves an angle of 1e-5 rad by 2e-9 degrees whatever the arithmetic (the kernel's trace goes
    through M = R_pred^T R_true, the oracle's through R_pred @ S_k)."""
    th = np.radians(np.nan_to_num(want, nan=90.0))
    tol = 1e-9 + np.degrees(4.5e-16 / np.sin(np.clip(th, 2e-8, np.pi / 2)) + 4.5e-16 / np.sin(np.clip(np.pi - th, 2e-8, np.pi / 2)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), label
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    assert np.all(err <= tol), (label, err.max(), int(np.argmax(err - tol)))


def table_f32(table):
    return table.matrices.float().numpy()


def trace_margin(p, t, S, cls, loss=False):
    """Best minus second-best candidate trace per row (float64): below 1e-6 the index is not compared (a float32 selection, or
    round-off in the float64 traces, may pick either)."""
    p64, t64 = p.astype(np.float64).reshape(-1, 3, 3), t.astype(np.float64).reshape(-1, 3, 3)
    s = S.astype(np.float64)[np.clip(cls, 0, S.shape[0] - 1)]
    tr = np.einsum("bil,bklj,bij->bk", p64, s, t64)
    if not loss:                                           # the metric compares clamped cosines
        tr = np.clip((tr - 1) / 2, -1, 1) * 2 + 1
    best = tr.max(axis=1)
    # duplicated table entries (padding) tie exactly and agree on the smallest k: only DISTINCT values count
    second = np.where(tr < best[:, None], tr, -np.inf).max(axis=1)
    return best - second


def check_against_oracle(pa, table, p, t, cls, label, grads=True):
    S = table_f32(table)
    o = sym_oracle(p, t, S, cls)
    pd, td = cuda(p), cuda(t)
    cd = None if cls is None else cuda(cls, torch.int32)
    deg, idx = pa.symmetric_angle_error(pd, td, table, cd, return_index=True)
    assert_angles(deg.cpu().numpy(), o["deg"], label)
    sure = trace_margin(p, t, S, o["idx"] * 0 if cls is None else cls) >= 1e-6
    assert np.array_equal(idx.cpu().numpy()[sure], o["idx"][sure]), label
    pg = pd.clone().requires_grad_(grads)
    tg = td.clone().requires_grad_(grads)
    loss, lidx = pa.symmetric_loss_frobenius(pg, tg, table, cd, return_index=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(loss.item() - o["loss"]) <= 1e-6 * abs(o["loss"]), (label, loss.item(), o["loss"])
    sure_l = trace_margin(p, t, S, np.zeros(len(p), np.int64) if cls is None else cls, loss=True) >= 1e-5
    assert np.array_equal(lidx.cpu().numpy()[sure_l], o["loss_idx"][sure_l]), label
    if grads:
        loss.backward()
        # a unit direction (T - P S) / d times 1/B: float32 round-off of T - P S (~1e-7) weighs 1/d in it
        tol = (2e-6 + 4e-7 / o["dist"]) / len(p)
        for got, ref in ((pg.grad, o["dp"]), (tg.grad, o["dt"])):
            err = np.abs(got.cpu().numpy() - ref).max(axis=(1, 2))
            assert np.all((err <= tol)[sure_l]), (label, (err / tol)[sure_l].max())


def test_g17_parity(pa):
    g = load_golden("g17_symmetry.npz")
    for tag in TABLES:
        p, t, S, cls = g17_case(g, tag)
        table = pa.SymmetryTable(list(S.astype(np.float64)) if S.shape[0] > 1 else S[0].astype(np.float64))
        assert np.array_equal(table_f32(table), S)
        cd = None if cls is None else cuda(cls, torch.int32)
        deg, idx = pa.symmetric_angle_error(cuda(p), cuda(t), table, cd, return_index=True)
        np.testing.assert_allclose(deg.cpu().numpy(), g[tag + "_deg"], rtol=0, atol=1e-9, err_msg=tag)
        assert np.array_equal(idx.cpu().numpy(), g[tag + "_idx"]), tag                # exact ties included: the smallest k
        pg, tg = cuda(p).requires_grad_(True), cuda(t).requires_grad_(True)
        loss, lidx = pa.symmetric_loss_frobenius(pg, tg, table, cd, return_index=True)
        ref = float(g[tag + "_loss"])
        assert abs(loss.item() - ref) <= 1e-6 * ref, (tag, loss.item(), ref)
        assert np.array_equal(lidx.cpu().numpy(), g[tag + "_loss_idx"]), tag
        loss.backward()
        for got, key in ((pg.grad, "_dp"), (tg.grad, "_dt")):
            want = g[tag + key]
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5 * np.abs(want).max(), err_msg=tag + key)


@pytest.mark.parametrize("n", [512, 4097])
def test_identity_table_is_angle_error_and_loss_frobenius(pa, n):
    gen = torch.Generator().manual_seed(n)
    t = haar(n, gen).float().cuda()
    p = (haar(n, gen) @ (torch.eye(3, dtype=torch.float64) + 0.01 * torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))).float().cuda()
    table = pa.SymmetryTable(torch.eye(3)[None])
    deg, idx = pa.symmetric_angle_error(p, t, table, return_index=True)
    assert torch.equal(deg, pa.angle_error(p, t))
    assert torch.equal(idx, torch.zeros(n, dtype=torch.int32, device="cuda"))
    p1, t1 = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    p2, t2 = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    l1, i1 = pa.symmetric_loss_frobenius(p1, t1, table, return_index=True)
    l2 = pa.loss_frobenius(p2, t2)
    assert abs(l1.item() - l2.item()) <= 2 ** -23 * abs(l2.item())
    assert not i1.any()
    l1.backward()
    l2.backward()
    for a, b in ((p1.grad, p2.grad), (t1.grad, t2.grad)):
        torch.testing.assert_close(a, b, rtol=2e-7, atol=1e-12)


@pytest.mark.parametrize("which", ["c24", "flip"])
def test_invariance_under_the_group(pa, which):
    gen = torch.Generator().manual_seed(3)
    n = 3000
    if which == "c24":
        g = pa.cyclic_symmetry(24, [0.2, -0.5, 0.8])
    else:
        g = torch.stack([torch.diag(torch.tensor(d, dtype=torch.float64)) for d in ([1.0, 1, 1], [1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1])])
    table = pa.SymmetryTable(g)
    K = g.shape[0]
    j = torch.randint(0, K, (n,), generator=gen)
    t = haar(n, gen).float()
    p = (t.double() @ table.matrices[0, j]).float()                         # R_pred = R_true S_j, rounded to float32
    o = sym_oracle(p.numpy(), t.numpy(), table_f32(table))
    deg, idx = pa.symmetric_angle_error(p.cuda(), t.cuda(), table, return_index=True)
    deg = deg.cpu().numpy()
    assert_angles(deg, o["deg"], which)
    assert deg.max() < 0.05
    inv = (K - j) % K if which == "c24" else j                              # S_j^-1
    assert np.array_equal(idx.cpu().numpy(), inv.numpy().astype(np.int32))
    loss, lidx = pa.symmetric_loss_frobenius(p.cuda(), t.cuda(), table, return_index=True)
    assert loss.item() < 1e-6
    assert np.array_equal(lidx.cpu().numpy(), inv.numpy().astype(np.int32))


def test_ten_classes_at_every_finish(pa):
    table = ten_class_table(pa)
    assert (table.num_classes, table.K) == (10, 8)
    gen = torch.Generator().manual_seed(10)
    for n in engine_sizes():
        t = haar(n, gen)
        cls = torch.randint(0, 10, (n,), generator=gen)
        j = torch.randint(0, 8, (n,), generator=gen)
        a = 0.2 * torch.randn(n, 3, 3, generator=gen, dtype=torch.float64)
        noise = torch.linalg.matrix_exp(a - a.transpose(1, 2))                # rotations about 15 degrees from I
        p = torch.where((torch.arange(n) % 2 == 0)[:, None, None],          # half the rows near a symmetric copy of the target
                        t @ noise @ table.matrices[cls, j].transpose(1, 2), haar(n, gen))
        check_against_oracle(pa, table, p.float().numpy(), t.float().numpy(), cls.numpy().astype(np.int32), "n=%d" % n, grads=n <= 70000)


def test_one_million_rows(pa):
    gen = torch.Generator().manual_seed(6)
    n = 1_000_000
    t, p = haar(n, gen).float(), haar(n, gen).float()
    cls = torch.randint(0, 10, (n,), generator=gen).int()
    check_against_oracle(pa, ten_class_table(pa), p.numpy(), t.numpy(), cls.numpy(), "1M ten classes")
    check_against_oracle(pa, pa.SymmetryTable(pa.cyclic_symmetry(24, "y")), p.numpy(), t.numpy(), None, "1M C24")


def test_bad_class_ids(pa):
    table = ten_class_table(pa)
    gen = torch.Generator().manual_seed(4)
    for n in (100, 5000):
        t, p = haar(n, gen).float().cuda(), haar(n, gen).float().cuda()
        cls = torch.randint(0, 10, (n,), generator=gen)
        bad = torch.zeros(n, dtype=torch.bool)
        bad[[3, n // 2, n - 1]] = True
        cls[3], cls[n // 2], cls[n - 1] = -1, 10, 1 << 20
        for dt in (torch.int32, torch.int64):
            c = cls.to(dt).cuda()
            with pytest.raises(IndexError):
                pa.symmetric_angle_error(p, t, table, c)
            deg, idx = pa.symmetric_angle_error(p, t, table, c, check=False, return_index=True)
            assert torch.isnan(deg.cpu()[bad]).all() and not torch.isnan(deg.cpu()[~bad]).any()
            assert (idx.cpu()[bad] == -1).all() and (idx.cpu()[~bad] >= 0).all()
            loss, lidx = pa.symmetric_loss_frobenius(p, t, table, c, return_index=True)
            assert torch.isnan(loss).item() and (lidx.cpu()[bad] == -1).all()
    c64 = torch.zeros(5, dtype=torch.int64).cuda()
    c64[2] = (1 << 32) + 1                                                  # would wrap to 1 in int32: stays out of range
    r = torch.eye(3).repeat(5, 1, 1).cuda()
    with pytest.raises(IndexError):
        pa.symmetric_angle_error(r, r, table, c64)
    with pytest.raises(ValueError):
        pa.symmetric_angle_error(r, r, table)                               # a multi-class table needs class ids
    with pytest.raises(ValueError):
        pa.symmetric_angle_error(r, r, pa.SymmetryTable(torch.eye(3)[None]), c64)
    with pytest.raises(TypeError):
        pa.symmetric_angle_error(r.double(), r.double(), pa.SymmetryTable(torch.eye(3)[None]))


def test_non_rotations_raise_where_angle_error_raises(pa):
    g = load_golden("g17_symmetry.npz")
    table = pa.SymmetryTable(g["flip_S"][0].astype(np.float64))
    for row in range(len(g["bad_raises"])):
        p, t = cuda(g["bad_p"][row:row + 1]), cuda(g["bad_t"][row:row + 1])
        raised = []
        for fn in (lambda: pa.angle_error(p, t), lambda: pa.symmetric_angle_error(p, t, table)):
            try:
                fn()
                raised.append(False)
            except ValueError as e:
                assert str(e) == "angle out of range, input probably not proper rotation matrices"
                raised.append(True)
        assert raised == [bool(g["bad_raises"][row])] * 2, row
    p, t = cuda(g["bad_p"]), cuda(g["bad_t"])                               # the whole batch, both sides of 64 rows
    with pytest.raises(ValueError):
        pa.symmetric_angle_error(p.repeat(200, 1, 1), t.repeat(200, 1, 1), table)
    assert pa.symmetric_angle_error(p.repeat(200, 1, 1), t.repeat(200, 1, 1), table, check=False).shape == (1200,)


def test_loss_autograd_shapes_sides_and_determinism(pa):
    table = pa.SymmetryTable(pa.cyclic_symmetry(4, "y"))
    gen = torch.Generator().manual_seed(8)
    n = 3000
    t, p = haar(n, gen).float().cuda(), haar(n, gen).float().cuda()
    o = sym_oracle(p.cpu().numpy(), t.cpu().numpy(), table_f32(table))
    sure = trace_margin(p.cpu().numpy(), t.cpu().numpy(), table_f32(table), np.zeros(n, np.int64), loss=True) >= 1e-5
    for layout in ("b9", "b33", "view"):
        for side in ("both", "pred", "true"):
            if layout == "b9":
                pp, tt = p.reshape(n, 9).clone(), t.reshape(n, 9).clone()
            elif layout == "b33":
                pp, tt = p.clone(), t.clone()
            else:                                                           # non-contiguous views of leaves
                pp, tt = torch.stack([p, p], dim=1), torch.stack([t, t], dim=1)
            pp.requires_grad_(side in ("both", "pred"))
            tt.requires_grad_(side in ("both", "true"))
            args = (pp[:, 0], tt[:, 1]) if layout == "view" else (pp, tt)
            if layout == "view":
                assert not args[0].is_contiguous() and not args[1].is_contiguous()
            loss = pa.symmetric_loss_frobenius(*args, table)
            (2.0 * loss).backward()
            for leaf, want, on in ((pp, o["dp"], side in ("both", "pred")), (tt, o["dt"], side in ("both", "true"))):
                if not on:
                    assert leaf.grad is None
                    continue
                assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
                got = leaf.grad
                if layout == "view":
                    used = 0 if leaf is pp else 1
                    assert not got[:, 1 - used].any()
                    got = got[:, used]
                err = np.abs(got.reshape(n, 3, 3).cpu().numpy() - 2.0 * want)[sure].max()
                assert err <= 4e-6 / n, (layout, side, err * n)
    pb = p.bfloat16().requires_grad_(True)                                  # a half-precision argument: its own dtype back
    pa.symmetric_loss_frobenius(pb, t, table).backward()
    assert pb.grad.dtype == torch.bfloat16 and pb.grad.shape == pb.shape
    big = 1_000_000
    tb, pbig = haar(big, gen).float().cuda(), haar(big, gen).float().cuda()
    runs = []
    for _ in range(2):
        pr = pbig.clone().requires_grad_(True)
        tr = tb.clone().requires_grad_(True)
        loss = pa.symmetric_loss_frobenius(pr, tr, table)
        loss.backward()
        runs.append((loss.detach().clone(), pr.grad, tr.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [3, 1091])
@pytest.mark.parametrize("side", ["pred", "true"])
def test_ten_classes_with_one_gradient_alone(pa, n, side):
    """Several classes with the gradient of one argument only (OpSymFrobLoss<true, DP, DT> with one of DP, DT): one workgroup (3 rows),
    and 17 whole units plus 3 rows, where the engine launch, the remainder kernel and the workspace finish all run in one call.
    check_against_oracle's bound."""
    table = ten_class_table(pa)
    gen = torch.Generator().manual_seed(40 + n)
    t, p = haar(n, gen).float(), haar(n, gen).float()
    cls = torch.randint(0, 10, (n,), generator=gen).int()
    S = table_f32(table)
    o = sym_oracle(p.numpy(), t.numpy(), S, cls.numpy())
    pg, tg = cuda(p).requires_grad_(side == "pred"), cuda(t).requires_grad_(side == "true")
    loss = pa.symmetric_loss_frobenius(pg, tg, table, cls.cuda())
    assert abs(loss.item() - o["loss"]) <= 1e-6 * abs(o["loss"]), (loss.item(), o["loss"])
    loss.backward()
    got, ref, other = (pg.grad, o["dp"], tg) if side == "pred" else (tg.grad, o["dt"], pg)
    assert other.grad is None
    sure_l = trace_margin(p.numpy(), t.numpy(), S, cls.numpy(), loss=True) >= 1e-5
    tol = (2e-6 + 4e-7 / o["dist"]) / n
    err = np.abs(got.cpu().numpy() - ref).max(axis=(1, 2))
    assert np.all((err <= tol)[sure_l]), (err / tol)[sure_l].max()


def test_graph_replay_equals_eager(pa):
    table = ten_class_table(pa).to("cuda")
    gen = torch.Generator().manual_seed(12)
    n = 5000
    t, p0 = haar(n, gen).float().cuda(), haar(n, gen).float().cuda()
    cls = torch.randint(0, 10, (n,), generator=gen).int().cuda()
    p = p0.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                                  # warm-up on the side stream, as torch.cuda.graph asks
            p.grad = None
            pa.symmetric_loss_frobenius(p, t, table, cls).backward()
    torch.cuda.current_stream().wait_stream(s)
    p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = pa.symmetric_loss_frobenius(p, t, table, cls)
        loss.backward()
    q = p0.clone().requires_grad_(True)
    ref = pa.symmetric_loss_frobenius(q, t, table, cls)
    ref.backward()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert abs(loss.item() - ref.item()) <= 1e-6 * ref.item()
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-6, atol=1e-12)


def test_first_use_in_a_capture_is_refused(pa, monkeypatch):
    """A table's upload is not capturable: the first use on a device while its stream is captured raises (the capture itself is
    stood in for, so that no graph is left half-captured)."""
    from poseestimation_amd import symmetry                                 # SymmetryTable._on looks _capturing up in its own module
    fresh = pa.SymmetryTable(pa.cyclic_symmetry(2))
    r = torch.eye(3).repeat(4, 1, 1).cuda()
    monkeypatch.setattr(symmetry, "_capturing", lambda dev: True)
    with pytest.raises(RuntimeError, match=r"table\.to\(device\)"):
        pa.symmetric_loss_frobenius(r, r, fresh)
    monkeypatch.undo()
    fresh.to("cuda")
    monkeypatch.setattr(symmetry, "_capturing", lambda dev: True)
    assert fresh._on(r.device) is fresh._dev[r.device.index]                # uploaded: no capture check any more


def test_per_class_statistics(pa):
    table = ten_class_table(pa)
    gen = torch.Generator().manual_seed(21)
    n = 20000
    t, p = haar(n, gen).float(), haar(n, gen).float()
    cls = torch.randint(0, 10, (n,), generator=gen).int()
    deg = pa.symmetric_angle_error(p.cuda(), t.cuda(), table, cls.cuda())
    got = pa.angle_error_statistics(deg, cls.cuda(), 10)
    o = sym_oracle(p.numpy(), t.numpy(), table_f32(table), cls.numpy())["deg"]
    for c in range(10):
        x = o[cls.numpy() == c]
        assert got["count"][c].item() == len(x)
        for name, want in (("mean", x.mean()), ("median", np.median(x)), ("max", x.max()), ("std", x.std()),
                           ("acc30", (x < 30).mean()), ("acc15", (x < 15).mean())):
            assert abs(got[name][c].item() - want) <= 1e-8 * max(1.0, abs(want)), (c, name)


def test_requires_grad_warning_is_emitted_once(pa):
    from poseestimation_amd import rotation_representation as rr
    rr._WARNED.discard("symmetric_angle_error")
    table = pa.SymmetryTable(pa.cyclic_symmetry(2))
    r = torch.eye(3).repeat(4, 1, 1).cuda().requires_grad_(True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = pa.symmetric_angle_error(r, r, table)
        pa.symmetric_angle_error(r, r, table)
    assert not a.requires_grad
    assert sum("symmetric_angle_error is an evaluation call" in str(x.message) for x in w) == 1
