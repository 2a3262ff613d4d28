#!/usr/bin/env python3
"""The coefficients of acos_f64 (poseestimation_amd/csrc/so3_rows.h): asin(x) = x + x z g(z), z = x^2 in [0, 1/4], g a polynomial of degree
9 fitted to minimise max_z z^W |g(z) - p(z)| -- Lawson's iteratively reweighted least squares in 50-digit arithmetic (mpmath), in the
Chebyshev basis of [0, 1/4], converted to monomials for the kernel's Horner chain.  W = 1 bounds the angle's relative error for c > 1/2,
W = 1.5 its absolute error; the kernel uses W = 1.2.  Prints the coefficients highest degree first, as the kernel lists them.

    python tools/fit_acos_f64.py [W] [degree]        (about a minute; tests/test_kernel_model.py checks the result on the host)
"""
import sys

import mpmath as mp


def g(z):
    x = mp.sqrt(z)
    return (mp.asin(x) - x) / (z * x)


def fit(weight_exp, degree, points=600, iterations=60):
    n = degree + 1
    zs = [mp.mpf(1) / 8 * (1 - mp.cos(mp.pi * (i + mp.mpf(1) / 2) / points)) for i in range(points)]   # Chebyshev points of (0, 1/4)
    ws = [z ** weight_exp for z in zs]
    gs = [g(z) for z in zs]
    basis = [[mp.chebyt(k, 8 * z - 1) for k in range(n)] for z in zs]
    lam = [mp.mpf(1) / points] * points
    best = None
    for _ in range(iterations):
        a_mat, rhs = mp.matrix(n, n), mp.matrix(n, 1)
        for i in range(points):
            q = lam[i] * ws[i] ** 2
            for j in range(n):
                rhs[j] += q * basis[i][j] * gs[i]
                for k in range(n):
                    a_mat[j, k] += q * basis[i][j] * basis[i][k]
        a = mp.lu_solve(a_mat, rhs)
        err = [ws[i] * abs(gs[i] - sum(a[k] * basis[i][k] for k in range(n))) for i in range(points)]
        if best is None or max(err) < best[0]:
            best = (max(err), a)
        s = sum(lam[i] * err[i] for i in range(points))
        lam = [lam[i] * err[i] / s for i in range(points)]
    worst, a = best
    mono = [mp.mpf(0)] * n
    for k in range(n):
        tk = mp.taylor(lambda z: mp.chebyt(k, 8 * z - 1), 0, degree)
        for j in range(n):
            mono[j] += a[k] * tk[j]
    return worst, mono


if __name__ == "__main__":
    mp.mp.dps = 50
    w = mp.mpf(sys.argv[1]) if len(sys.argv) > 1 else mp.mpf("1.2")
    deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    worst, mono = fit(w, deg)
    print("// weight z^%s, degree %d: max weighted error %s" % (w, deg, mp.nstr(worst, 5)))
    for c in reversed(mono):
        print("%.17e" % float(c))
