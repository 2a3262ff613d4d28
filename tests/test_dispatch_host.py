"""The launchers' dispatcher without a GPU (poseestimation_amd/csrc/so3_dispatch.h and so3_device.h's clouds_per_wave / cloud_blocks,
compiled for the host: tests/host_model/dispatch.cpp).

  1  with_flags with one to four flags: every run-time combination reaches the callable exactly once, with constants that equal the
     arguments in argument order;
  2  with_value<1, 2, 4>: a listed value reaches the callable as that constant and returns true, another returns false without a call;
  3  kernel_label: the names so3_last_kernel() reports, from the dispatchers' constants and from plain values alike, the bare name,
     and a buffer that is too short (cut, terminated, nothing written behind it);
  4  the cloud kernels' launch shape against its restatement here."""
import ctypes
import os

import pytest

from conftest import ROOT
from support import build_host_model

SRC = os.path.join(ROOT, "tests", "host_model", "dispatch.cpp")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "dispatch", SRC, fp_contract_off=False)
    lib.model_with_flags.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.model_with_flags.restype = None
    lib.model_with_value.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.model_kernel_label.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.model_kernel_label.restype = None
    lib.model_clouds_per_wave.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.model_clouds_per_wave.restype = ctypes.c_int32
    lib.model_cloud_blocks.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.model_cloud_blocks.restype = ctypes.c_int64
    return lib


def test_with_flags_hands_every_combination_over_once_and_in_order(model):
    for n in (1, 2, 3, 4):
        for bits in range(1 << n):
            calls, seen = ctypes.c_int(-1), ctypes.c_int(-1)
            model.model_with_flags(n, bits, ctypes.byref(calls), ctypes.byref(seen))
            assert calls.value == 1, (n, bits)
            assert seen.value == (1 << (8 + n)) | bits, (n, bits, seen.value)          # n constants; constant i is flag i


def test_with_value_calls_for_a_listed_value_only(model):
    for v in (1, 2, 4):
        calls, got = ctypes.c_int(-1), ctypes.c_int(-1)
        assert model.model_with_value(v, ctypes.byref(calls), ctypes.byref(got)) == 1
        assert (calls.value, got.value) == (1, v)
    for v in (0, 3, 8):
        calls, got = ctypes.c_int(-1), ctypes.c_int(-7)
        assert model.model_with_value(v, ctypes.byref(calls), ctypes.byref(got)) == 0
        assert (calls.value, got.value) == (0, -7)


LABELS = [b"k_icp_step<false, false, false, 4>", b"k_group_bwd<true, 64, 16>", b"k_fps<8, 1024>", b"k_sym_add<2, false, 16>",
          b"k_three_nn<1, true>", b"k_three_interp_bwd_cf"]


def test_kernel_label_spells_the_instantiation(model):
    for which, want in enumerate(LABELS):
        buf = ctypes.create_string_buffer(b"\xaa" * 96, 96)
        model.model_kernel_label(which, buf, 64)
        assert buf.value == want, (which, buf.value)
        assert buf.raw[len(want) + 1:] == b"\xaa" * (96 - len(want) - 1)               # nothing behind the terminator


def test_kernel_label_is_cut_at_the_buffer(model):
    for which, want in enumerate(LABELS):
        for n in (1, 2, 7, len(want) - 1, len(want), len(want) + 1):
            buf = ctypes.create_string_buffer(b"\xaa" * 96, 96)
            model.model_kernel_label(which, buf, n)
            assert buf.raw[:n] == want[:n - 1] + b"\0" + b"\xaa" * (n - 1 - len(want[:n - 1])), (which, n, buf.raw[:n])
            assert buf.raw[n:] == b"\xaa" * (96 - n), (which, n)                      # no overrun


def clouds_per_wave(b, cus):
    """B / (CUs * 16) clouds per wave, clamped to [1, 64]."""
    return min(max(b // (cus * 16), 1), 64)


def cloud_blocks(b, per_wave):
    """Waves of per_wave clouds, four to a block."""
    waves = (b + per_wave - 1) // per_wave
    return (waves + 3) // 4


def test_cloud_launch_shape(model):
    for cus in (256, 32):
        full = 16 * cus
        for b in (1, full - 1, full, full + 1, 2 * full - 1, 64 * full, 64 * full + 1, 2 ** 31):
            pw = model.model_clouds_per_wave(b, cus)
            assert pw == clouds_per_wave(b, cus), (cus, b, pw)
            assert model.model_cloud_blocks(b, pw) == cloud_blocks(b, pw), (cus, b)
            assert model.model_cloud_blocks(b, pw) * 4 * pw >= b                        # every cloud has a slot
    assert [clouds_per_wave(b, 256) for b in (1, 4095, 4096, 8191, 8192, 64 * 4096, 64 * 4096 + 1, 2 ** 31)] == [1, 1, 1, 1, 2, 64, 64, 64]
