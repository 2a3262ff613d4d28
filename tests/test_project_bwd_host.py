"""The backward of the SVD -> SO(3) projection without a GPU: the host model of the kernels' own templates (oracle/kernel_model.cpp:
project_bwd -- K2's arithmetic, fast path + backward_from_rotation, hard rows through the Jacobi frames; project_bwd_jacobi -- the Jacobi
frames on every row; project_bwd_f64) on every family of tests/project_bwd_ref.py, every row under the judges J and K defined there.

This is where the constants are MEASURED: J32 / K32 / JJAC / KJAC / J64 / K64 hold, per family, the largest figure the shipped host model
reaches here (rounded up in the last digit); the test asserts the model against these figures un-multiplied.  The bound the DEVICE is held
to (tests/test_gpu_project_bwd.py) is 4 x the figure of its family -- DESIGN.md section 7's rule; the factor covers the device's 1-ulp
v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 against libm's correctly rounded ones and its fma contraction.  No bound is taken from the device.

The float64 figures are in units of 2^-53 and measure the AGREEMENT of two float64 computations (the kernel's Jacobi frames and LAPACK's
SVD in the closed form): the reference is no more precise than the kernel there."""
import math

import numpy as np
import pytest
import torch

import project_bwd_ref as ref
from oracle import so3_oracle as so

# family                               float32 model        Jacobi frames alone   float64 model (2^-53)
#                                      J        K           J        K            J        K
MEASURED = {
    "gaussian":                       (5.51,    8.94,       10.05,   11.66,       46.38,   8.46),
    "s=(1,e,-eU) e=1e-01":            (7.65,    9.86,       0.71,    9.70,        8.71,    9.23),
    "s=(1,e,-eU) e=1e-02":            (8.58,    10.57,      0.54,    8.86,        1.59,    9.86),
    "s=(1,e,-eU) e=1e-03":            (7.04,    10.29,      0.45,    10.62,       1.75,    9.33),
    "s=(1,e,-eU) e=1e-04":            (0.39,    10.51,      0.39,    10.51,       2.19,    9.40),
    "s=(1,e,e) e=1e-01":              (2.18,    10.70,      1.30,    11.68,       5.59,    8.98),
    "s=(1,e,e) e=1e-02":              (5.49,    10.99,      0.57,    11.18,       2.44,    9.15),
    "s=(1,e,e) e=1e-03":              (4.28,    8.79,       0.53,    9.66,        2.86,    9.46),
    "s=(1,e,e) e=1e-04":              (1.59,    10.27,      0.55,    10.27,       2.53,    9.47),
    "near-reflection e=1e-01":        (10.48,   10.59,      12.04,   11.48,       71.78,   11.71),
    "near-reflection e=1e-02":        (83.37,   9.60,       83.37,   9.60,        80.57,   10.89),
    "near-reflection e=1e-03":        (117.69,  8.94,       117.69,  8.94,        81.07,   11.58),
    "graded (1,1e-2,1e-4)":           (3.24,    9.07,       0.45,    10.63,       1.63,    10.47),
    "s=(1,10^U(-4,0),0)":             (9.20,    12.07,      2.64,    11.68,       30.17,   9.66),
    "haar + 1e-3 gaussian":           (12.69,   10.63,      109.82,  8.95,        105.36,  9.50),
    "bf16 gaussian":                  (8.18,    9.19,       5.09,    8.96,        51.73,   9.65),
    "entries in -3..3":               (6.24,    10.82,      5.69,    9.57,        51.26,   11.31),
    "gaussian x 1e-5":                (5.73,    10.70,      4.72,    7.23,        56.37,   8.77),
    "gaussian x 1e5":                 (4.75,    10.69,      5.66,    9.04,        57.57,   8.92),
    "gaussian x 2^-40":               (6.58,    8.97,       17.19,   8.37,        51.90,   9.58),
    "gaussian x 2^40":                (6.43,    9.73,       7.17,    9.97,        56.74,   8.07),
    "gaussian x 1e-18":               (6.08,    10.00,      6.49,    8.29,        51.50,   9.03),
    "gaussian x 1e18":                (4.94,    9.88,       29.53,   11.10,       51.26,   9.54),
    # no defined gradient: K alone
    "generic ties":                   (None,    8.42,       None,    8.42,        None,    6.09),
    "rank one":                       (None,    18.55,      None,    18.55,       None,    7.55),
    "entries in {-1,0,1}":            (None,    7.73,       None,    6.96,        None,    10.19),
    "all zero":                       (None,    0.0,        None,    0.0,         None,    0.0),
    "exact reflections":              (None,    8.76,       None,    8.76,        None,    6.64),
}
J32 = {k: v[0] for k, v in MEASURED.items() if v[0] is not None}
K32 = {k: v[1] for k, v in MEASURED.items()}
JJAC = {k: v[2] for k, v in MEASURED.items() if v[2] is not None}
KJAC = {k: v[3] for k, v in MEASURED.items()}
J64 = {k: v[4] for k, v in MEASURED.items() if v[4] is not None}
K64 = {k: v[5] for k, v in MEASURED.items()}
J32_BF16_SMALL_GAP = 6.85                     # float32 model on project_bwd_ref.bf16_small_gap(): the small-gap rows rounded to bfloat16
# K on the families of tests/test_gpu_parity.py's rank-deficiency test, 50 000 rows each (test_k_on_the_rank_deficient_families below)
#                               float32   float64 (2^-53)
RANK_DEFICIENT_K = {
    "small integers":          (15.13,    11.88),
    "outer products":          (44.06,    10.55),
    "integer outer products":  (21.93,    44.06),
    "nine equal entries":      (7.13,     9.23),
    "rank two":                (13.13,    10.30),
    "rank two + 1e-7":         (13.28,    11.72),
    "outer + 1e-7":            (27.95,    11.01),
    "entries in -1..1":        (11.61,    9.54),
    "reflections":             (13.03,    11.97),
    "scaled 1e-5":             (12.68,    12.99),
    "scaled 1e+5":             (12.72,    12.60),
}
DEVICE_FACTOR = 4.0                          # the device's bound is 4 x the host model's figure, per family
# the reference against float64 autograd, in FLOAT32 units of J: a thousandth of the unit every bound above is stated in
REFERENCE_AGREES = 1e-3


@pytest.fixture(scope="module")
def km():
    from oracle import kernel_model
    if kernel_model.clangxx() is None:
        pytest.skip("clang++ (for ext_vector_type) is not available")
    kernel_model.build()
    return kernel_model


MODELS = {"float32": ("project_bwd", "project", np.float32, ref.U32, J32, K32),
          "jacobi": ("project_bwd_jacobi", "project_jacobi", np.float32, ref.U32, JJAC, KJAC),
          "float64": ("project_bwd_f64", "project_f64", np.float64, ref.U64, J64, K64)}


def _run(km, which):
    bwd, fwd, dt, u, jrec, krec = MODELS[which]
    d = ref.data()
    dm = getattr(km, bwd)(d["m"].astype(dt), d["g"].astype(dt)).reshape(-1, 9)
    r = getattr(km, fwd)(d["m"].astype(dt)).reshape(-1, 9)
    return dm, r


@pytest.mark.parametrize("which", list(MODELS))
def test_every_row_of_every_family_and_the_constants_are_the_measured_ones(km, which):
    _, _, _, u, jrec, krec = MODELS[which]
    d = ref.data()
    dm, r = _run(km, which)
    jf, kf = ref.j_figure(dm, u=u), ref.k_figure(dm, r, u=u)
    jm, kmx = ref.per_family(jf), ref.per_family(kf)
    print("%-8s %-26s %9s %9s %9s   %9s %9s %9s" % (which, "family", "J", "recorded", "bound", "K", "recorded", "bound"))
    for name in d["names"]:
        if name in krec:
            print("%-8s %-26s %9s %9s %9s   %9.2f %9.2f %9.2f" % (which, name, "%.2f" % jm[name] if name in jm else "-", "%.2f" % jrec[name] if name in jrec else "-",
                                                                "%.2f" % (DEVICE_FACTOR * jrec[name]) if name in jrec else "-", kmx[name], krec[name], DEVICE_FACTOR * krec[name]))
    # a NaN or Inf row gives a NaN row; every other row is finite, the families without a gradient included
    assert np.isnan(dm[~d["finite"]]).all() and np.isfinite(dm[d["finite"]]).all()
    assert set(jm) == set(jrec) and set(kmx) == set(krec)
    # the recorded constants ARE the measurement (rounded up in the last digit): every row, un-multiplied
    for name, rec in jrec.items():
        assert 0.95 * rec <= jm[name] <= rec, (which, "J", name, jm[name], rec)
    for name, rec in krec.items():
        assert 0.95 * rec <= kmx[name] <= rec, (which, "K", name, kmx[name], rec)
    assert len(ref.over_bound(jf, jrec, factor=1.0)[0]) == 0 and len(ref.over_bound(kf, krec, factor=1.0)[0]) == 0


def test_the_small_gap_rows_rounded_to_bfloat16(km):
    """What the bfloat16 kernels read when a small-gap row comes in bfloat16 storage: every row judged, gaps down to 2.5e-5 s1."""
    b = ref.bf16_small_gap()
    assert np.array_equal(ref._bf16(b["m"]).astype(np.float32), b["m"]) and b["ans"]["jrow"].all()
    assert (b["ans"]["gamma"] / b["ans"]["s1"]).min() < 1e-4
    fig = ref.j_of(km.project_bwd(b["m"], b["g"]), b["ans"])
    print("bf16-rounded small-gap rows: J %.2f, recorded %.2f, bound %.2f" % (fig.max(), J32_BF16_SMALL_GAP, DEVICE_FACTOR * J32_BF16_SMALL_GAP))
    assert 0.95 * J32_BF16_SMALL_GAP <= fig.max() <= J32_BF16_SMALL_GAP


def test_k_on_the_rank_deficient_families(km):
    """The families tests/test_gpu_parity.py's rank-deficiency test draws on the device (500 000 rows each, there; 50 000 here): no
    gradient to compare with, but dM = R [y]x all the same.  K is the defect of R^T R - I in units of u plus a few roundings; the heavy
    tails are the rank-one families, where the rotation is completed from a single direction."""
    rng = np.random.default_rng(9)
    for name, m in ref.rank_deficient(50_000):
        g = rng.standard_normal((len(m), 9)).astype(np.float32)
        k32 = ref.k_figure(km.project_bwd(m, g), km.project(m))
        k64 = ref.k_figure(km.project_bwd_f64(m.astype(np.float64), g.astype(np.float64)), km.project_f64(m.astype(np.float64)), u=ref.U64)
        assert not np.isnan(k32).any() and not np.isnan(k64).any(), name       # floored denominators: every gradient is finite
        rec32, rec64 = RANK_DEFICIENT_K[name]
        print("%-24s K float32 %6.2f (recorded %6.2f, bound %6.2f)   float64 %6.2f (recorded %6.2f, bound %6.2f)" %
              (name, k32.max(), rec32, DEVICE_FACTOR * rec32, k64.max(), rec64, DEVICE_FACTOR * rec64))
        assert 0.95 * rec32 <= k32.max() <= rec32 and 0.95 * rec64 <= k64.max() <= rec64, name


def test_fixture_shape_the_one_per_cent_cap_and_the_tiling():
    d = ref.data()
    n = len(d["m"])
    assert d["m"].dtype == np.float32 and d["g"].dtype == np.float32 and d["d64"].dtype == np.float64
    counts = np.bincount(d["fam"])
    for i, name in enumerate(d["names"]):
        rows = d["fam"] == i
        if d["judged"][i]:
            assert counts[i] == ref.ROWS_JUDGED
            with np.errstate(divide="ignore", invalid="ignore"):
                left_out = (d["gamma"][rows] / d["s1"][rows] <= ref.MIN_GAP).mean()
            assert left_out <= ref.MAX_LEFT_OUT, (name, left_out)
            assert d["jrow"][rows].mean() == 1.0 - left_out
        else:
            assert counts[i] in (ref.ROWS_UNJUDGED, ref.ROWS_NONFINITE) and not d["jrow"][rows].any()
    assert np.isfinite(d["d64"][d["jrow"]]).all()
    # the families are what their names say, on the float32-rounded rows
    fam = lambda name: d["fam"] == d["names"].index(name)
    for e in ref.SMALL_E:
        assert np.abs(d["gamma"][fam("s=(1,e,e) e=%.0e" % e)] / (2 * e) - 1).max() < 1e-2
        g = d["gamma"][fam("s=(1,e,-eU) e=%.0e" % e)] / e
        assert 0.0999 < g.min() and g.max() < 1.0001
    for e in ref.REFLECT_E:
        assert np.abs(d["gamma"][fam("near-reflection e=%.0e" % e)] / e - 1).max() < 1e-3
    for label, sc in ref.SCALES:                                            # both sides of the window |M|^2 in [2^-28, 2^34]
        n2 = (d["m"][fam("gaussian x " + label)].astype(np.float64) ** 2).sum(1)
        assert (np.median(n2) < 2.0**-28) == (sc < 1) and (np.median(n2) > 2.0**34) == (sc > 1)
    assert (d["gamma"][fam("generic ties")] / d["s1"][fam("generic ties")] < 2e-6).all()
    # the tiling: a prime period above the fixture, coprime to one pass of K2's grid (CUs x 4 SIMDs x 2 waves x 2 units x 64 rows)
    period = ref.tile_period(n)
    assert period > n and all(period % q for q in range(2, math.isqrt(period) + 1))
    for cus in (256, 304, 64):
        assert math.gcd(period, cus * 1024) == 1
    idx = ref.tile_index(3 * period, n)
    assert np.array_equal(np.bincount(idx[:period], minlength=n) > 0, np.ones(n, bool))
    assert np.array_equal(idx[period:2 * period], idx[:period])
    for cus in (256, 304, 64):                                              # rows whole passes apart never hold the same fixture row
        p = cus * 1024
        if p < len(idx):
            assert (idx[p:] != idx[:-p]).mean() > 0.99999


def test_the_reference_against_float64_autograd():
    """projection_backward_np is a closed form through LAPACK's SVD.  Once, on the judged rows of three families, against torch's
    float64 autograd through the reference's own call sequence (svd -> det -> scale -> matmul): something that is not the closed form."""
    d = ref.data()
    for name in ("gaussian", "s=(1,e,-eU) e=1e-02", "near-reflection e=1e-02"):
        rows = np.flatnonzero((d["fam"] == d["names"].index(name)) & d["jrow"])
        x = torch.tensor(d["m"][rows].astype(np.float64), requires_grad=True)
        r = so.symmetric_orthogonalization_torch(x)
        (r * torch.tensor(d["g"][rows].astype(np.float64)).reshape(r.shape)).sum().backward()
        fig = ref.j_figure(x.grad.numpy(), idx=rows, u=ref.U32)
        print("%-26s closed form against float64 autograd: %.2e float32 units of J" % (name, fig.max()))
        assert fig.max() <= REFERENCE_AGREES, (name, fig.max())


def test_a_power_of_two_scale_commutes_bit_for_bit_on_the_small_gap_families(km):
    """dM(2^k M) 2^k == dM(M) for k = +-40: the fast path's window prescale, backward_given_rotation's `dm *= factor` and the Jacobi
    path's own prescale are exact.  tests/test_kernel_model.py has this on Gaussian rows; here on every judged family of unit scale --
    settled rows with a small gap, near-reflections (hard rows), graded and rank-two rows."""
    d = ref.data()
    scaled = [d["names"].index("gaussian x " + label) for label, _ in ref.SCALES]
    rows = np.flatnonzero(d["judged"][d["fam"]] & ~np.isin(d["fam"], scaled))
    m, g = d["m"][rows], d["g"][rows]
    base = km.project_bwd(m, g)
    assert np.isfinite(base).all()
    for k in (40, -40):
        c = np.float32(2.0**k)
        got = km.project_bwd(m * c, g) * c                                 # exact products: |M| ~ 1, |dM| < 2^40 on these rows
        bad = (got != base).reshape(len(rows), -1).any(1)
        assert not bad.any(), (k, int(bad.sum()), [d["names"][f] for f in np.unique(d["fam"][rows[bad]])])
