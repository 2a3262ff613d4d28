#!/usr/bin/env python3
"""The coefficients of Tr<T>::atan_unit (poseestimation_amd/csrc/so3_device.h): atan(z) = z p(s), s = z^2 in [0, 1], p a polynomial of
degree 8 fitted to minimise max_s |p(s) - atan(z) / z| / (atan(z) / z), the RELATIVE error of the angle -- Lawson's iteratively reweighted
least squares in float64, in the Chebyshev basis of [0, 1], converted to monomials for the kernel's Horner chain.  atan2 folds onto this
interval (min / max of |y|, |x|; pi/2 - a; pi - a; the sign of y).  Prints the coefficients highest degree first, as the kernel lists them,
and the largest relative error of the float32 Horner chain over 2^20 arguments.

    python tools/fit_atan_f32.py [degree]        (seconds; tests/test_inverse_maps_host.py sweeps the compiled result against long double)
"""
import sys

import numpy as np
from numpy.polynomial import chebyshev as cheb


def target(s):
    z = np.sqrt(s)
    return np.where(z > 1e-8, np.arctan(z) / np.where(z > 1e-8, z, 1.0), 1.0 - s / 3.0)


def fit(degree, points=4000, iterations=200):
    s = 0.5 * (1.0 - np.cos(np.pi * (np.arange(points) + 0.5) / points))          # Chebyshev points of (0, 1)
    f = target(s)
    basis = cheb.chebvander(2.0 * s - 1.0, degree)
    lam = np.full(points, 1.0 / points)
    best = None
    for _ in range(iterations):
        w = np.sqrt(lam) / f
        a = np.linalg.lstsq(basis * w[:, None], f * w, rcond=None)[0]
        err = np.abs(basis @ a - f) / f
        if best is None or err.max() < best[0]:
            best = (err.max(), a)
        lam = lam * err
        lam /= lam.sum()
    worst, a = best
    mono = cheb.cheb2poly(a)                                                       # in u = 2 s - 1
    shifted = np.polynomial.Polynomial(mono)(np.polynomial.Polynomial([-1.0, 2.0]))
    return worst, shifted.coef


def float32_error(coef, points=1 << 20):
    z = np.linspace(0.0, 1.0, points).astype(np.float32)
    s = z * z
    p = np.full_like(s, np.float32(coef[-1]))
    for c in coef[-2::-1]:
        p = p * s + np.float32(c)              # (rounds the product too: an upper bound for the kernel's fused chain)
    got = (z * p).astype(np.float64)
    want = np.arctan(z.astype(np.float64))
    return np.max(np.abs(got - want)[1:] / want[1:])


if __name__ == "__main__":
    deg = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst, coef = fit(deg)
    print("// degree %d in s = z^2: max relative error %.3e (float64 coefficients), %.3e (float32 Horner chain)" % (deg, worst, float32_error(coef)))
    for c in coef[::-1]:
        print("%.9ef," % c)
