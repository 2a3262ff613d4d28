"""K1 over several buffer pairs in one launch (so3_project_fwd_segments_f32) and the capture-time fusion that uses it
(csrc/so3proj.hip: project_fwd).  Every comparison is torch.equal against the SAME calls run eagerly one by one: a segment's rows
go through the same arithmetic, paired with the same neighbour row, so not a bit may move.  The fused-launch counter
(so3_capture_fused_launches) is asserted in every capture test, so that none can pass without the fusion having happened -- or, in
the cases that must not fuse, with it."""
import ctypes
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
P, I64 = ctypes.c_void_p, ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    from poseestimation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def rr():
    from poseestimation_amd import rotation_representation
    return rotation_representation


@pytest.fixture(scope="module")
def hr():
    spec = importlib.util.spec_from_file_location("k1_hard_rows", os.path.join(ROOT, "tools", "k1_hard_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def k1(lib, x, r, stream, flip=None):
    fn = lib.so3_project_fwd_bf16 if x.dtype is torch.bfloat16 else lib.so3_project_fwd_f32
    assert fn(P(x.data_ptr()), P(r.data_ptr()), P(flip.data_ptr()) if flip is not None else None, x.shape[0], P(stream)) == 0, lib.so3_last_error()


def eager(lib, xs):
    """The reference of every test here: one eager call per buffer (eager calls are never fused)."""
    st = torch.cuda.current_stream().cuda_stream
    outs = [torch.empty(x.shape[0], 9, device=DEV) for x in xs]
    for x, r in zip(xs, outs):
        k1(lib, x, r, st)
    torch.cuda.synchronize()
    return outs


def segments(lib, xs, outs):
    n = len(xs)
    st = torch.cuda.current_stream().cuda_stream
    return lib.so3_project_fwd_segments_f32((P * n)(*[x.data_ptr() for x in xs]), (P * n)(*[r.data_ptr() for r in outs]),
                                            (I64 * n)(*[x.shape[0] for x in xs]), n, P(st))


def randn(rows, seed):
    return torch.randn(rows, 9, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


# ---- the segments entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(64, 128, 192, 64, 4096 + 64), (64,) * 8, (8192, 64, 4096 + 192)])
def test_segments_equal_separate_calls(lib, rr, sizes):
    """Single-unit segments, an odd unit count (192 rows: three units, the second round holds a phantom unit), a segment shorter than
    one wave's deal, and eight segments of one unit each; guard words around every output."""
    xs = [randn(b, 10 + i) for i, b in enumerate(sizes)]
    ref = eager(lib, xs)
    bufs = [torch.full((b * 9 + 16,), 7.0, device=DEV) for b in sizes]
    outs = [buf[8:8 + b * 9].view(b, 9) for buf, b in zip(bufs, sizes)]
    assert segments(lib, xs, outs) == 0, lib.so3_last_error()
    assert lib.so3_last_kernel() == b"so3::k_rows<so3::OpProject<4, false>, 2, 3, 256, false>"
    torch.cuda.synchronize()
    for i, (r, want, buf) in enumerate(zip(outs, ref, bufs)):
        assert torch.equal(r, want), (i, sizes[i], int((r != want).any(dim=1).sum().item()))
        assert (buf[:8] == 7).all() and (buf[8 + sizes[i] * 9:] == 7).all(), i
    got = rr.symmetric_orthogonalization_segments(xs)                       # the Python wrapper: a list of (B_i, 3, 3)
    assert all(torch.equal(g.view(-1, 9), want) and g.shape == (want.shape[0], 3, 3) for g, want in zip(got, ref))


def test_one_segment_is_the_plain_call(lib):
    for rows in (64, 192, 64 * 6201):                                       # one unit, an odd tail, more rounds (3101) than the grid has waves (3072)
        x = randn(rows, 3)
        (ref,) = eager(lib, [x])
        out = torch.empty(rows, 9, device=DEV)
        assert segments(lib, [x], [out]) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, ref), rows


def test_segments_entry_refuses_invalid_arguments(lib):
    xs = [randn(64, i) for i in range(9)]
    outs = [torch.full((64, 9), 7.0, device=DEV) for _ in range(9)]
    st = P(torch.cuda.current_stream().cuda_stream)
    ms, rs = (P * 9)(*[x.data_ptr() for x in xs]), (P * 9)(*[r.data_ptr() for r in outs])
    seg = lib.so3_project_fwd_segments_f32
    assert seg(ms, rs, (I64 * 9)(*[64] * 9), 0, st) == -1
    assert seg(ms, rs, (I64 * 9)(*[64] * 9), 9, st) == -1
    assert seg(ms, rs, (I64 * 2)(64, 65), 2, st) == -1
    assert seg((P * 2)(xs[0].data_ptr(), None), rs, (I64 * 2)(64, 64), 2, st) == -1
    assert seg(ms, (P * 2)(None, outs[1].data_ptr()), (I64 * 2)(64, 64), 2, st) == -1
    assert seg(None, rs, (I64 * 1)(64), 1, st) == -1
    torch.cuda.synchronize()
    assert all((r == 7).all() for r in outs)                                # a refused call launches nothing


# ---- hard rows across segments -------------------------------------------------------------------------------------------------
def sprinkle(hr, x, share, gen, names):
    pick = torch.nonzero(torch.rand(x.shape[0], device=DEV, generator=gen) < share).flatten()
    for f, name in enumerate(names):
        idx = pick[f::len(names)]
        if idx.numel():
            x[idx] = hr.family(name, idx.numel(), torch.device(DEV), gen).reshape(-1, 9)
    return x


def test_hard_rows_keep_their_segment(lib, hr):
    """Parked hard rows are redone behind the loop and written by ROW NUMBER: the number carries its segment.  Zero rows, exact
    reflections, ties and rank-one rows sprinkled over different segments (few per round: parked), one segment made of reflections only
    (dense: the Jacobi path on the spot), one of ties only."""
    gen = torch.Generator(device=DEV).manual_seed(77)
    d = torch.device(DEV)
    xs = [sprinkle(hr, randn(4096 + 64, 1), 0.05, gen, ("all zero", "generic ties")),
          -hr.haar(256, d, gen).reshape(256, 9).contiguous(),                                        # exact reflections, every row
          sprinkle(hr, randn(192, 2), 0.1, gen, ("rank one", "near-reflection")),
          sprinkle(hr, randn(8192, 3), 0.03, gen, ("rank one", "entries in {-1,0,1}", "generic ties", "all zero")),
          hr.family("generic ties", 128, d, gen).reshape(128, 9).contiguous(),
          sprinkle(hr, randn(64, 4), 0.2, gen, ("near-reflection",))]
    exact = sprinkle(hr, randn(1024, 5), 0.05, gen, ("all zero",))
    some = torch.nonzero(torch.rand(1024, device=DEV, generator=gen) < 0.05).flatten()
    exact[some] = -hr.haar(some.numel(), d, gen).reshape(-1, 9)                                      # exact reflections among Gaussian rows
    xs.append(exact)
    hard = torch.empty(8192, dtype=torch.uint8, device=DEV)
    scratch = torch.empty(8192, 9, device=DEV)
    assert lib.so3_project_fwd_diag_f32(P(xs[3].data_ptr()), P(scratch.data_ptr()), P(hard.data_ptr()), 8192, P(torch.cuda.current_stream().cuda_stream)) == 0
    assert 50 < int(hard.sum().item()) < 400                                # the sprinkled rows really are hard, and few per round
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    assert segments(lib, xs, outs) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    for i, (r, want) in enumerate(zip(outs, ref)):
        bad = (r != want).any(dim=1)
        assert not bool(bad.any()), (i, int(bad.sum().item()), torch.nonzero(bad).flatten()[:8].tolist())


def test_more_parked_rows_than_the_list_holds(lib, hr):
    """A workgroup's list holds 512 parked rows.  Five passes of the grid at ~28 hard rows per round (parked: at most 32 of a round's
    128 are) fill it -- 4 waves x 5 rounds x 28 = 560 -- and the rounds it has no room for take the Jacobi path on the spot.  The batch
    is cut into three segments of unequal length, so one list holds rows of several segments when it overflows."""
    gen = torch.Generator(device=DEV).manual_seed(91)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_pass = cus * 4 * 3 * 128                                             # K1: three waves per SIMD, 128 rows per wave and round
    total = 5 * per_pass
    cuts = [0, per_pass + 64 * 37, 3 * per_pass + 64 * 1001, total]           # an odd number of units in the first two segments
    whole = sprinkle(hr, randn(total, 6), 0.22, gen, ("near-reflection", "entries in {-1,0,1}", "generic ties", "rank one", "all zero"))
    xs = [whole[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    assert segments(lib, xs, outs) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    for i, (r, want) in enumerate(zip(outs, ref)):
        bad = (r != want).any(dim=1)
        assert not bool(bad.any()), (i, int(bad.sum().item()), torch.nonzero(bad).flatten()[:8].tolist())


# ---- capture -------------------------------------------------------------------------------------------------------------------
def capture(body):
    """body(raw stream, the capturing torch stream) recorded into a graph on a side stream."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            body(side.cuda_stream, side)
    torch.cuda.synchronize()
    return g


def replay_twice(g, outs, ref, what):
    for rep in range(2):
        for r in outs:
            r.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for i, (r, want) in enumerate(zip(outs, ref)):
            assert torch.equal(r, want), (what, rep, i, int((r != want).any(dim=1).sum().item()))


SIZES = (128, 8192, 192, 4096, 64 * 5, 1024, 64 * 33, 2048, 128)           # 128 .. 8192 rows, odd unit counts among them


@pytest.mark.parametrize("calls, folded", [(2, 1), (8, 7), (9, 7), (17, 14), (18, 15)])
def test_adjacent_calls_are_folded_into_one_node(lib, calls, folded):
    """A node takes up to eight segments: the 9th and the 17th call start nodes of their own, so n calls fold n - ceil(n / 8) times."""
    xs = [randn(SIZES[i % len(SIZES)], 100 + i) for i in range(calls)]
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    before = lib.so3_capture_fused_launches()

    def body(st, _):
        for x, r in zip(xs, outs):
            k1(lib, x, r, st)
            assert lib.so3_last_kernel() == b"so3::k_rows<so3::OpProject<4, false>, 2, 3, 256, false>"

    g = capture(body)
    assert lib.so3_capture_fused_launches() - before == folded
    replay_twice(g, outs, ref, calls)


def test_bfloat16_calls_fold_among_themselves(lib):
    xs = [randn(b, 40 + i).bfloat16() for i, b in enumerate((256, 64, 4096 + 64))]
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    before = lib.so3_capture_fused_launches()
    g = capture(lambda st, _: [k1(lib, x, r, st) for x, r in zip(xs, outs)])
    assert lib.so3_capture_fused_launches() - before == 2
    replay_twice(g, outs, ref, "bf16")


def not_folded(lib, body, outs, ref, what):
    before = lib.so3_capture_fused_launches()
    g = capture(body)
    assert lib.so3_capture_fused_launches() == before, what
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for i, (r, want) in enumerate(zip(outs, ref)):
        assert torch.equal(r, want), (what, i)


def test_hazards_between_calls_are_never_folded(lib):
    st0 = torch.cuda.current_stream().cuda_stream
    a, c = randn(1024, 1), randn(1024, 2)
    # an in-place chain: the output of call k is the input of call k + 1
    b1, b2, b3 = (torch.empty(1024, 9, device=DEV) for _ in range(3))
    k1(lib, a, b1, st0); k1(lib, b1, b2, st0); k1(lib, b2, b3, st0)
    torch.cuda.synchronize()
    ref = [b1.clone(), b2.clone(), b3.clone()]
    for t in (b1, b2, b3):
        t.fill_(7.0)
    not_folded(lib, lambda st, _: (k1(lib, a, b1, st), k1(lib, b1, b2, st), k1(lib, b2, b3, st)), [b1, b2, b3], ref, "chain")
    # the same output twice: the later call's rows must be what is left
    (ra, rc) = eager(lib, [a, c])
    out = torch.empty(1024, 9, device=DEV)
    not_folded(lib, lambda st, _: (k1(lib, a, out, st), k1(lib, c, out, st)), [out], [rc], "same output twice")
    # a call whose output is an earlier call's input
    a2 = a.clone()
    o1 = torch.empty(1024, 9, device=DEV)
    not_folded(lib, lambda st, _: (k1(lib, a2, o1, st), k1(lib, c, a2, st)), [a2], [rc], "write after read")
    assert torch.equal(o1, eager(lib, [rc])[0])                              # (the second replay's first call read the first replay's rotations)


def test_what_is_not_the_same_engine_only_launch_is_not_folded(lib):
    a, c = randn(1024, 3), randn(2048, 4)
    ra, rc = eager(lib, [a, c])
    # a float32 call followed by a bfloat16 one
    cb = c.bfloat16()
    (rcb,) = eager(lib, [cb])
    o1, o2 = torch.empty_like(ra), torch.empty_like(rcb)
    not_folded(lib, lambda st, _: (k1(lib, a, o1, st), k1(lib, cb, o2, st)), [o1, o2], [ra, rcb], "f32 then bf16")
    # a call with flip flags, in either position
    flip = torch.empty(2048, dtype=torch.uint8, device=DEV)
    o1, o2, o3 = torch.empty_like(ra), torch.empty_like(rc), torch.empty_like(ra)
    not_folded(lib, lambda st, _: (k1(lib, a, o1, st), k1(lib, c, o2, st, flip=flip), k1(lib, a, o3, st)), [o1, o2, o3], [ra, rc, ra], "flip")
    det = torch.linalg.det(c.double().view(-1, 3, 3))
    assert torch.equal(flip.bool()[det.abs() > 1e-6], (det < 0)[det.abs() > 1e-6])
    # B = 100: a remainder for the tile kernel
    d = randn(100, 5)
    (rd,) = eager(lib, [d])
    o1, o2, o3 = torch.empty_like(ra), torch.empty_like(rd), torch.empty_like(rc)
    not_folded(lib, lambda st, _: (k1(lib, a, o1, st), k1(lib, d, o2, st), k1(lib, c, o3, st)), [o1, o2, o3], [ra, rd, rc], "remainder")


def test_anything_captured_between_two_calls_keeps_them_apart(lib):
    a, c = randn(1024, 6), randn(2048, 7)
    ra, rc = eager(lib, [a, c])
    # any other torch operation between the two calls
    o1, o2 = torch.empty_like(ra), torch.empty_like(rc)
    t = torch.zeros(16, device=DEV)
    not_folded(lib, lambda st, _: (k1(lib, a, o1, st), t.add_(1.0), k1(lib, c, o2, st)), [o1, o2], [ra, rc], "torch op between")
    # a second stream's work joined by an event wait between the two calls
    o1, o2 = torch.empty_like(ra), torch.empty_like(rc)
    other = torch.cuda.Stream()
    u = torch.zeros(16, device=DEV)

    def body(st, side):
        k1(lib, a, o1, st)
        other.wait_stream(side)
        with torch.cuda.stream(other):
            u.add_(1.0)
        side.wait_stream(other)
        k1(lib, c, o2, st)

    not_folded(lib, body, [o1, o2], [ra, rc], "event wait between")
    assert u[0].item() == 2.0                                                # the joined work is in the graph: it ran with both replays


def test_switched_off_nothing_is_folded(lib):
    xs = [randn(b, 60 + i) for i, b in enumerate((128, 4096, 192))]
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    assert lib.so3_capture_fusion(0) == 1
    try:
        not_folded(lib, lambda st, _: [k1(lib, x, r, st) for x, r in zip(xs, outs)], outs, ref, "switched off")
    finally:
        assert lib.so3_capture_fusion(1) == 0
    before = lib.so3_capture_fused_launches()                                # and on again
    g = capture(lambda st, _: [k1(lib, x, r, st) for x, r in zip(xs, outs)])
    assert lib.so3_capture_fused_launches() - before == 2
    replay_twice(g, outs, ref, "switched on again")


def test_an_eager_call_between_two_captures(lib):
    """The record a capture leaves behind belongs to that capture: an eager call after it is launched as ever, and the next capture
    starts from its own first call."""
    xs = [randn(b, 70 + i) for i, b in enumerate((256, 1024, 64))]
    ref = eager(lib, xs)
    outs = [torch.empty_like(r) for r in ref]
    before = lib.so3_capture_fused_launches()
    g1 = capture(lambda st, _: [k1(lib, x, r, st) for x, r in zip(xs[:2], outs[:2])])
    assert lib.so3_capture_fused_launches() - before == 1
    lone = torch.empty_like(ref[2])
    k1(lib, xs[2], lone, torch.cuda.current_stream().cuda_stream)            # eager, buffers disjoint from the captured ones
    torch.cuda.synchronize()
    assert lib.so3_capture_fused_launches() - before == 1
    assert torch.equal(lone, ref[2])
    g2 = capture(lambda st, _: [k1(lib, x, r, st) for x, r in zip(xs, outs)])
    assert lib.so3_capture_fused_launches() - before == 3                   # the first call of g2 folded into nothing
    replay_twice(g1, outs[:2], ref[:2], "first graph")
    replay_twice(g2, outs, ref, "second graph")
