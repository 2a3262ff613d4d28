"""The cloud backwards without a GPU: K5b (so3_kabsch_bwd_f32) and a7b (so3_rotate_clouds_bwd_f32) are declared, exported and
bound, their arguments are checked on the host, and G16's reference gradients equal the closed forms the kernels implement."""
import ctypes
import re
import subprocess
import threading

import numpy as np

from conftest import load_golden

NEW = ("so3_kabsch_bwd_f32", "so3_rotate_clouds_bwd_f32")


def test_cloud_backwards_are_declared_exported_and_bound(built_library):
    from poseestimation_amd import _lib
    from test_abi_and_host import header_symbols
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(so3_[a-z0-9_]+)\b", exported))
    for name in NEW:
        assert name in header_symbols()
        assert name in exported
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.so3_version() == 210 == _lib.ABI_VERSION


def test_cloud_backward_arguments_are_checked_on_the_host(built_library):
    """Bad sizes and null required pointers return SO3_ERR_INVALID before any launch; B == 0 is a no-op.  No device is touched.
    On a thread of its own: so3_last_error() is per thread, and other tests expect the main thread's to be empty."""
    errors = []

    def run():
        try:
            check_cloud_backward_arguments()
        except BaseException as e:          # re-raised on the test's thread
            errors.append(e)
    worker = threading.Thread(target=run)
    worker.start()
    worker.join()
    if errors:
        raise errors[0]


def check_cloud_backward_arguments():
    from poseestimation_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: every call below returns before a launch
    kb = lib.so3_kabsch_bwd_f32
    assert kb(None, None, None, None, None, None, None, -1, 8, None) == -1
    assert b"so3_kabsch_bwd_f32" in lib.so3_last_error()
    assert kb(None, None, None, None, None, None, None, 4, -1, None) == -1
    assert kb(None, None, None, None, None, None, None, (1 << 40) + 1, 8, None) == -1
    assert kb(None, None, None, None, None, None, None, 4, 150000001, None) == -1
    assert kb(None, None, None, None, None, None, None, 0, 8, None) == 0
    assert kb(fake, fake, None, fake, None, fake, fake, 4, 8, None) == -1                  # H is required
    assert b"so3_kabsch_bwd_f32: null pointer" in lib.so3_last_error()
    assert kb(None, fake, fake, fake, None, fake, fake, 4, 8, None) == -1                  # P is required when N > 0
    assert kb(fake, None, fake, fake, None, fake, fake, 4, 8, None) == -1                  # Q likewise
    rb = lib.so3_rotate_clouds_bwd_f32
    assert rb(None, None, None, None, None, 0, -1, 8, None) == -1
    assert b"so3_rotate_clouds_bwd_f32" in lib.so3_last_error()
    assert rb(None, None, None, None, None, 0, 4, -1, None) == -1
    assert rb(None, None, None, None, None, 1, (1 << 31) + 1, 8, None) == -1
    assert rb(None, None, None, None, None, 0, 0, 8, None) == 0
    assert rb(fake, None, fake, fake, fake, 0, 4, 8, None) == -1                            # R is required for dP
    assert b"so3_rotate_clouds_bwd_f32: null pointer" in lib.so3_last_error()
    assert rb(fake, fake, None, fake, fake, 1, 4, 8, None) == -1                            # G is required when N > 0
    assert rb(None, fake, fake, fake, fake, 0, 4, 8, None) == -1                            # P is required for dR
    assert rb(None, None, fake, None, None, 0, 4, 8, None) == 0                             # no output asked for: nothing to do
    assert rb(None, None, None, None, None, 0, 4, 0, None) == 0


def kabsch_closed_form(p, q, g_r, g_h):
    """What K5b computes, in float64: dH = K2(H, gR) + gH, dQ_i = dH p_i, dP_i = dH^T q_i."""
    from oracle import so3_oracle as so
    h = np.einsum("bia,bic->bac", q, p)
    dh = so.projection_backward_np(h, g_r)
    if g_h is not None:
        dh = dh + g_h
    return np.einsum("bac,bia->bic", dh, q), np.einsum("bac,bic->bia", dh, p)


def test_g16_kabsch_reference_gradients_are_the_closed_form():
    g = load_golden("g16_cloud_gradients.npz")
    p, q = g["p"].astype(np.float64), g["q"].astype(np.float64)
    h = np.einsum("bia,bic->bac", q, p)
    assert (np.linalg.det(h) < 0).any() and (np.linalg.det(h) > 0).any()          # det-flip rows are among the cases
    assert np.abs(g["kabsch_f64_h"] - h).max() < 1e-12
    for case, g_h in (("r", None), ("rh", g["g_h"].astype(np.float64))):
        dp, dq = kabsch_closed_form(p, q, g["g_r"].astype(np.float64), g_h)
        np.testing.assert_allclose(dp, g["kabsch_%s_f64_dp" % case], rtol=0, atol=1e-10)
        np.testing.assert_allclose(dq, g["kabsch_%s_f64_dq" % case], rtol=0, atol=1e-10)
        # the reference's own float32 autograd is the same function, rounded
        np.testing.assert_allclose(dp, g["kabsch_%s_f32_dp" % case], rtol=0, atol=2e-3 * np.abs(dp).max())


def test_g16_rotation_reference_gradients_are_the_closed_form():
    """dpc_i = R^T g_i and dR = sum_i g_i p_i^T, for the (B,N,3) layout and the transposed one."""
    g = load_golden("g16_cloud_gradients.npz")
    pc, r = g["pc1"].astype(np.float64), g["gt_rmat"].astype(np.float64)
    for layout in ("out", "gg"):
        up = g["u_" + layout].astype(np.float64)
        gi = up if layout == "out" else up.transpose(0, 2, 1)
        np.testing.assert_allclose(np.einsum("bac,bia->bic", r, gi), g["rot_%s_f64_dpc" % layout], rtol=0, atol=1e-10)
        np.testing.assert_allclose(np.einsum("bia,bic->bac", gi, pc), g["rot_%s_f64_dr" % layout], rtol=0, atol=1e-10)
        y = np.einsum("bac,bic->bia", r, pc)
        np.testing.assert_allclose(y if layout == "out" else y.transpose(0, 2, 1), g["rot_%s_f64_y" % layout], rtol=0, atol=1e-12)
