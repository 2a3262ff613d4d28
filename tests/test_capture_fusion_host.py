"""Capture-time fusion of adjacent K1 calls, the part that needs no device: the decision whether a call may be folded into the
kernel node of the previous one (csrc/so3proj.hip: k1_may_fuse, reached through so3_capture_fusion_would_fuse) is pure logic over
a capture id, the stream's capture dependencies, the segment count and byte ranges; the switch and the counter; and the argument
checks of so3_project_fwd_segments_f32, which refuse before anything is launched."""
import ctypes

import pytest

P, I64 = ctypes.c_void_p, ctypes.c_int64
MAX_SEGMENTS = 8                       # csrc/so3_rows.h: kMaxSegments
MAX_ROUNDS = (1 << 30) - 2048          # csrc/so3proj.hip: kMaxRounds32 (a round = 128 rows)


@pytest.fixture(scope="module")
def lib(built_library):
    from poseestimation_amd import _lib
    return _lib.load()


def in_thread(fn):
    """Run fn on a thread of its own: so3_last_error is thread-local, and a refusal provoked here must not be what a later test of
    this process reads on the main thread."""
    import threading
    box = {}

    def run():
        try:
            fn()
        except BaseException as exc:          # handed to the caller's thread
            box["exc"] = exc

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "exc" in box:
        raise box["exc"]


def would(lib, rec, call, same_capture=1, ndeps=1, dep_is_node=1, rec_eb=4, eb=4):
    """rec: [(M, R, rows), ...] of the recorded node; call: (M, R, rows).  Addresses are plain integers: nothing is dereferenced."""
    n = len(rec)
    ms = (P * max(n, 1))(*[r[0] for r in rec])
    rs = (P * max(n, 1))(*[r[1] for r in rec])
    bs = (I64 * max(n, 1))(*[r[2] for r in rec])
    return lib.so3_capture_fusion_would_fuse(ms, rs, bs, n, rec_eb, same_capture, ndeps, dep_is_node, eb, P(call[0]), P(call[1]), call[2])


A = 1 << 20                            # base address of the recorded segment's input; 64 rows x 36 B = 2304 B per array
ROWS = 64
NB = ROWS * 36
REC = [(A, A + 0x10000, ROWS)]         # input [A, A + 2304), output [A + 0x10000, A + 0x10000 + 2304)


def _expect(cond):
    assert cond


def test_disjoint_buffers_fuse(lib):
    assert would(lib, REC, (A + 0x20000, A + 0x30000, ROWS)) == 1
    assert would(lib, REC, (A + 0x20000, A + 0x30000, 4096)) == 1
    # the same INPUT twice is no hazard: two reads
    assert would(lib, REC, (A, A + 0x30000, ROWS)) == 1


def test_ranges_that_touch_at_a_boundary_fuse(lib):
    rin, rout = REC[0][0], REC[0][1]
    assert would(lib, REC, (rout + NB, A + 0x30000, ROWS)) == 1          # new input starts where the recorded output ends
    assert would(lib, REC, (rout - NB, A + 0x30000, ROWS)) == 1          # ... ends where it starts
    assert would(lib, REC, (A + 0x20000, rout + NB, ROWS)) == 1          # new output against the recorded output, both sides
    assert would(lib, REC, (A + 0x20000, rout - NB, ROWS)) == 1
    assert would(lib, REC, (A + 0x20000, rin + NB, ROWS)) == 1           # new output against the recorded input, both sides
    assert would(lib, REC, (A + 0x20000, rin - NB, ROWS)) == 1


@pytest.mark.parametrize("side", [-1, 1])
def test_one_byte_of_overlap_in_each_hazard_direction_blocks(lib, side):
    rin, rout = REC[0][0], REC[0][1]
    near = lambda base: base + side * (NB - 1)                             # one byte into the range, from below or from above
    assert would(lib, REC, (near(rout), A + 0x30000, ROWS)) == 0          # read after write: the new input is a recorded output
    assert would(lib, REC, (A + 0x20000, near(rout), ROWS)) == 0          # write after write: the same output twice
    assert would(lib, REC, (A + 0x20000, near(rin), ROWS)) == 0           # write after read: the new output is a recorded input


def test_whole_buffer_hazards_block(lib):
    rin, rout = REC[0][0], REC[0][1]
    assert would(lib, REC, (rout, A + 0x30000, ROWS)) == 0                # an in-place chain
    assert would(lib, REC, (A + 0x20000, rout, ROWS)) == 0                # a repeated output buffer
    assert would(lib, REC, (A + 0x20000, rin, ROWS)) == 0                 # overwriting an earlier input
    # hazards are checked against EVERY recorded segment, not the last one only
    rec = [(A + i * 0x100000, A + i * 0x100000 + 0x10000, ROWS) for i in range(5)]
    assert would(lib, rec, (A + 0x900000, A + 0xA00000, ROWS)) == 1
    for i in range(5):
        assert would(lib, rec, (rec[i][1], A + 0xA00000, ROWS)) == 0
        assert would(lib, rec, (A + 0x900000, rec[i][1], ROWS)) == 0
        assert would(lib, rec, (A + 0x900000, rec[i][0], ROWS)) == 0


def test_a_bfloat16_input_is_half_as_long(lib):
    rin = REC[0][0]
    assert would(lib, REC, (A + 0x20000, rin + NB // 2, ROWS), rec_eb=2, eb=2) == 1      # past the recorded bfloat16 input
    assert would(lib, REC, (A + 0x20000, rin + NB // 2 - 1, ROWS), rec_eb=2, eb=2) == 0
    assert would(lib, REC, (A + 0x20000, rin + NB // 2, ROWS)) == 0                      # the same addresses as float32: inside it


def test_capture_and_dependency_conditions(lib):
    call = (A + 0x20000, A + 0x30000, ROWS)
    assert would(lib, REC, call) == 1
    assert would(lib, REC, call, same_capture=0) == 0                     # another capture (or a record left by an earlier one)
    assert would(lib, REC, call, ndeps=0) == 0                            # the stream depends on nothing: a freshly joined stream
    assert would(lib, REC, call, ndeps=2) == 0                            # something else must precede the call
    assert would(lib, REC, call, dep_is_node=0) == 0                      # something was captured on the stream since
    assert would(lib, REC, call, rec_eb=4, eb=2) == 0                     # float32 and bfloat16 inputs are different kernels
    assert would(lib, REC, call, rec_eb=2, eb=4) == 0
    assert would(lib, [], call) == 0                                      # nothing recorded


def test_the_ninth_segment_starts_a_node_of_its_own(lib):
    rec = [(A + i * 0x100000, A + i * 0x100000 + 0x10000, ROWS) for i in range(MAX_SEGMENTS)]
    call = (A + 0x900000, A + 0xA00000, ROWS)
    assert would(lib, rec[:MAX_SEGMENTS - 1], call) == 1
    assert would(lib, rec, call) == 0
    in_thread(lambda: _expect(would(lib, rec + [rec[0]], call) == -1))    # a record no launch can have left


def test_round_numbers_stay_32_bit(lib):
    big = (MAX_ROUNDS - 1) * 128                                           # rows of a segment one round short of the limit
    far = 1 << 50                                                          # (36 * big = 1.5e11 bytes per array: far apart)
    rec = [(far, 2 * far, big)]
    assert would(lib, rec, (3 * far, 4 * far, 128)) == 1                   # exactly the limit
    assert would(lib, rec, (3 * far, 4 * far, 64)) == 1                    # an odd tail still takes a whole round
    assert would(lib, rec, (3 * far, 4 * far, 192)) == 0                   # two rounds: one too many
    assert would(lib, rec, (3 * far, 4 * far, big)) == 0
    # every segment rounds up on its own: seven one-unit segments are seven rounds, not four
    rec = [(far, 2 * far, (MAX_ROUNDS - 7) * 128)] + [(5 * far + i * 0x10000, 6 * far + i * 0x10000, 64) for i in range(6)]
    assert would(lib, rec, (3 * far, 4 * far, 64)) == 1
    assert would(lib, rec, (3 * far, 4 * far, 192)) == 0


def test_switch_returns_the_previous_setting_and_defaults_to_on(lib):
    assert lib.so3_capture_fusion(0) == 1                                  # the default is on
    assert lib.so3_capture_fusion(0) == 0
    assert lib.so3_capture_fusion(5) == 0                                  # any non-zero value switches it on
    assert lib.so3_capture_fusion(1) == 1
    assert lib.so3_capture_fused_launches() >= 0


def test_segments_entry_refuses_bad_arguments_before_it_launches(lib):
    """No device is touched: every refusal happens in front of the launch."""
    in_thread(lambda: _segments_refusals(lib))


def _segments_refusals(lib):
    ok_m, ok_r, ok_b = (P * 9)(*[A] * 9), (P * 9)(*[A + 0x10000] * 9), (I64 * 9)(*[64] * 9)
    seg = lib.so3_project_fwd_segments_f32
    assert seg(ok_m, ok_r, ok_b, 0, None) == -1
    assert seg(ok_m, ok_r, ok_b, 9, None) == -1
    assert seg(ok_m, ok_r, ok_b, -1, None) == -1
    assert seg(None, ok_r, ok_b, 1, None) == -1 and seg(ok_m, None, ok_b, 1, None) == -1 and seg(ok_m, ok_r, None, 1, None) == -1
    for bad_b in (65, 0, -64, 100):
        assert seg(ok_m, ok_r, (I64 * 2)(64, bad_b), 2, None) == -1, bad_b
    assert seg((P * 2)(A, None), ok_r, ok_b, 2, None) == -1                # a null pointer inside the table
    assert seg(ok_m, (P * 2)(A + 0x10000, None), ok_b, 2, None) == -1
    assert seg((P * 2)(A, A + 2), ok_r, ok_b, 2, None) == -1               # not dword aligned
    assert b"so3_project_fwd_segments_f32" in lib.so3_last_error()
    big = (I64 * 2)((MAX_ROUNDS - 1) * 128, 256)
    assert seg(ok_m, ok_r, big, 2, None) == -1                             # the rounds of all segments together do not fit 32 bits
