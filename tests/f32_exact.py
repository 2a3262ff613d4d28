"""The exact float32 arithmetic of the fixed-order definitions (include/so3proj.h, poseestimation_amd/csrc/so3_device.h), in numpy.
ARITHMETIC ONLY: no test logic lives here.  tests/three_nn_ref.py, tests/chamfer_ref.py and the GPU search tests build their float32
restatements from these four functions, each of which agrees with a one-line definition in so3_device.h:

    fma32(a, b, c)            fmaf(a, b, c): a * b + c rounded ONCE to float32
    pair_dist2_32(dx, dy, dz) pair_dist2:  fma(dz, dz, fma(dy, dy, dx * dx))
    pose_point32(m, p)        pose_point:  fma(m0, px, fma(m1, py, fma(m2, pz, m3))) per coordinate
    first_argmin32(d2)        add_s_pair's strict < in ascending index: the first index of the smallest value

numpy has no fma, and float32(float64(a) * b + c) rounds twice: to float64, then to float32.  fma32 makes the first rounding harmless by
rounding it TO ODD: the product of two float32 is exact in float64 (48 bits), TwoSum gives the addition's exact error, and where that
error is not zero and the float64 sum's last mantissa bit is even the sum moves one float64 ulp towards the error.  A value rounded to
odd at 53 bits rounds to nearest at 24 bits (or fewer: a subnormal result) exactly as the unrounded value does, because 53 >= 24 + 2.
tests/test_f32_exact_host.py holds fma32 to libm's fmaf bit for bit."""
import numpy as np


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays (broadcast), for finite operands; the result may overflow to inf."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                           # exact: 24 + 24 bits, and the exponents stay inside float64's
        s = p + c
        t = s - p                                           # TwoSum: s + err == p + c exactly
        err = (p - (s - t)) + (c - t)
        odd = (np.atleast_1d(s).view(np.int64) & 1).astype(bool).reshape(np.shape(s))
        fix = np.isfinite(s) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def pair_dist2_32(dx, dy, dz):
    dx, dy, dz = (np.asarray(v, np.float32) for v in (dx, dy, dz))
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def pose_point32(m, p):
    """m (..., 12): the top three rows of a row-major 4x4 pose (m[4c .. 4c+2] = row c of R, m[4c+3] = t_c); p (..., N, 3) -> (..., N, 3)."""
    m, p = np.asarray(m, np.float32)[..., None, :], np.asarray(p, np.float32)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([fma32(m[..., 4 * c], px, fma32(m[..., 4 * c + 1], py, fma32(m[..., 4 * c + 2], pz, m[..., 4 * c + 3]))) for c in range(3)], -1)


def first_argmin32(d2):
    """The index add_s_pair's scan keeps along the last axis: candidates in ascending index, replaced only by a strictly smaller one."""
    return np.argmin(np.asarray(d2, np.float32), axis=-1)
