"""The checkers of tests/test_gpu_cloud_gradient_kernels.py (tests/cloud_gradients_ref.py) without a GPU: float32 restatements of the
four entry points pass every one of them at every N of the GPU file's point-count test, and seeded wrong answers fail them.

The restatements: numpy float32 with the kernels' sum order for dR (lane-strided fma, then the xor butterfly) and their fma chains for
the per-point rows; K2 from oracle.kernel_model.project_bwd (the kernels' own template compiled for the host); so3_rigid_align_f32 and
so3_rigid_align_bwd_f32 from tests/host_model/rigid_align.cpp.

TOLERANCES.  The derived bounds (cloud_gradients_ref's docstring) have limit 1.  Where K2 is on the path nothing is proven, so the
project's rule applies: HOST_* is the largest figure the float32 restatement reaches here, over every point of every cloud of
test_the_float32_restatements_pass (B = min(2000, 200 000 // N) clouds at each N of POINTS, weights null and U[0.05, 1]), and the
bound, on the host and on the GPU alike, is 4 x that (the device's v_rcp / v_sqrt are 1-ulp approximations and it contracts
a * b + c).  They are never taken from the GPU's output.  DESIGN.md section 7c quotes them.
The forward's H, centroids, W, rotation property and pose identity keep tests/test_rigid_align_host.py's H_TOL, T_TOL, W_TOL, ROT_TOL;
R is held to 2.5e-6 s1 / gap + 2 |dH|_F / gap with the asserted H bound for dH, and the share of clouds too ill-conditioned for that
(gap < 1e-3 s1), which are left to the properties, is capped: none at N >= 7, 1 % at N = 3; N < 3 has no unique rotation."""
import numpy as np
import pytest

import cloud_gradients_ref as cg
import test_rigid_align_host as host
from test_rigid_align_host import model          # noqa: F401 -- the fixture: tests/host_model/rigid_align.cpp compiled for the host

#                                 measured on the host       bound (4 x)
HOST_KB_DP = 7.86e-7;                KB_DP_TOL = 4 * HOST_KB_DP                     # noqa: E702
HOST_KB_DQ = 7.71e-7;                KB_DQ_TOL = 4 * HOST_KB_DQ                     # noqa: E702
HOST_RA_DP = 7.93e-7;                RA_DP_TOL = 4 * HOST_RA_DP                     # noqa: E702
HOST_RA_DQ = 8.02e-7;                RA_DQ_TOL = 4 * HOST_RA_DQ                     # noqa: E702
HOST_RA_DW = 6.82e-7;                RA_DW_TOL = 4 * HOST_RA_DW                     # noqa: E702
HOST = {"kb_dP": HOST_KB_DP, "kb_dQ": HOST_KB_DQ, "ra_dP": HOST_RA_DP, "ra_dQ": HOST_RA_DQ, "ra_dw": HOST_RA_DW}

FWD_TOL = {"H": host.H_TOL, "centroid": host.T_TOL, "W": host.W_TOL, "rotation": host.ROT_TOL, "pose": host.T_TOL, "finite": 0.0, "R/bound": 1.0}
SEED_SIZES = (3, 65, 513)
LAST_POINT_SIZES = (65, 513, 3001)


def limits():
    """What every figure of the backward checkers may reach."""
    return {"rot_dP": 1.0, "rot_dR": 1.0, "kbH_dP": 1.0, "kbH_dQ": 1.0, "kb_dP": KB_DP_TOL, "kb_dQ": KB_DQ_TOL, "ra_dP": RA_DP_TOL,
            "ra_dQ": RA_DQ_TOL, "ra_dw": RA_DW_TOL}


def forward_limits(n, b):
    """The forward's figures, with the cap on the number of the batch's b clouds whose R is left to the properties: none at N >= 7,
    1 % at N = 3 rounded up to whole clouds (one cloud of a batch of 67 is 1.5 %: a share has no finer grain than 1 / b, and from
    b = 100 on this is the 1 % itself), every cloud at N < 3."""
    return dict(FWD_TOL, unjudged=0.0 if n >= 7 else (float(np.ceil(0.01 * b)) if n >= 3 else float(b)))


def hold(fig, lim, label):
    """Print every figure, then assert each against its limit."""
    print("%-52s " % label + "  ".join("%s %.3e" % kv for kv in fig.items()))
    for k, v in fig.items():
        assert v <= lim[k], (label, k, v, lim[k])


def host_clouds(n):
    return min(2000, 200000 // n)


def _merge(worst, fig):
    for k, v in fig.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.fixture(scope="module")
def restated(model):           # noqa: F811
    """The restatements' figures at every N: computed once, shared by the tests below."""
    worst, rows = {}, []
    for n in cg.POINTS:
        b = host_clouds(n)
        d = cg.bwd_inputs(b, n, 100 + n)
        fig = {}
        rot = cg.rotate_bwd_ref(d["P"], d["R"], d["G"])
        fig.update(cg.check_rotate_bwd(cg.rotate_bwd_model(d["P"], d["R"], d["G"]), rot))
        for g_r, g_h in ((d["gR"], d["gH"]), (d["gR"], None), (None, d["gH"])):
            r = cg.kabsch_bwd_ref(d["P"], d["Q"], d["H"], g_r, g_h)
            _merge(fig, cg.check_kabsch_bwd(cg.kabsch_bwd_model(d["P"], d["Q"], d["H"], g_r, g_h), r))
        for w, st in ((None, d["stats"]), (d["w"], d["stats_w"])):
            for g_r, g_t, g_h in ((d["gR"], d["gt"], d["gH"]), (None, d["gt"], None), (d["gR"], None, None), (None, None, d["gH"])):
                r = cg.rigid_bwd_ref(d["P"], d["Q"], w, d["H"], d["R"], st, g_r, g_t, g_h)
                _merge(fig, cg.check_rigid_bwd(cg.rigid_bwd_model(model, d["P"], d["Q"], w, d["H"], d["R"], st, g_r, g_t, g_h), r))
        rows.append(("N %4d B %4d backward" % (n, b), fig, limits()))
        _merge(worst, fig)
        for offset in (0.0, 10.0):
            f = cg.make_batch(b, n, 200 + n, offset=offset)
            for w in (None, d["w"]):
                fwd = cg.check_rigid_fwd(cg.rigid_fwd_model(model, f["P"], f["Q"], w), f["P"], f["Q"], w, FWD_TOL)
                rows.append(("N %4d B %4d forward offset %g %s" % (n, b, offset, "weighted" if w is not None else "unweighted"), fwd, forward_limits(n, b)))
    return worst, rows


def test_the_float32_restatements_pass(restated):
    worst, rows = restated
    print("worst:", "  ".join("%s %.4e" % kv for kv in worst.items()))
    for label, fig, lim in rows:
        hold(fig, lim, label)
    for k, h in HOST.items():          # the recorded HOST_* constants are this measurement (to the three digits they are written with)
        assert h * 0.995 <= worst[k] <= h * 1.005, (k, worst[k], h)


def _seeded(label, fig, lim, report):
    """A wrong answer must exceed the bound of at least the figure it spoils; returns that worst figure over its bound."""
    over = max(v / lim[k] if lim[k] > 0 else np.inf for k, v in fig.items())
    report.append("%-62s %10.3g x the bound" % (label, over))
    assert over > 1.0, (label, fig)


def test_seeded_wrong_answers_fail(model):          # noqa: F811
    lim, report = limits(), []
    for n in sorted(set(SEED_SIZES + LAST_POINT_SIZES)):
        b = 64 if n < 1000 else 8
        d = cg.bwd_inputs(b, n, 300 + n)
        tag = "N %4d: " % n
        rot = cg.rotate_bwd_ref(d["P"], d["R"], d["G"])
        got = cg.rotate_bwd_model(d["P"], d["R"], d["G"])
        hold(cg.check_rotate_bwd(got, rot), lim, tag + "rotate, as restated")
        if n in LAST_POINT_SIZES:
            less = dict(got, dR=got["dR"] - d["G"][:, -1, :, None] * d["P"][:, -1, None, :])
            _seeded(tag + "the last point is left out of dR", cg.check_rotate_bwd(less, rot, ("dR",)), lim, report)
        if n not in SEED_SIZES:
            continue
        misread = cg.rotate_bwd_model(d["P"], d["R"], d["GT"].reshape(b, n, 3))
        _seeded(tag + "the transposed G is read as (B, N, 3)", cg.check_rotate_bwd(misread, rot), lim, report)

        k_args = (d["P"], d["Q"], d["H"], d["gR"], d["gH"])
        k_ref, k_got = cg.kabsch_bwd_ref(*k_args), cg.kabsch_bwd_model(*k_args)
        hold(cg.check_kabsch_bwd(k_got, k_ref), lim, tag + "kabsch, as restated")
        for mutate, what in (("neighbour", "cloud j takes cloud j + 1's dH (kabsch)"), ("untransposed", "dP from dH instead of dH^T (kabsch)")):
            bad = cg.kabsch_bwd_ref(*k_args, mutate=mutate)
            wrong = {k: k_got[k] + (bad[k] - k_ref[k]) for k in ("dP", "dQ")}
            _seeded(tag + what, cg.check_kabsch_bwd(wrong, k_ref), lim, report)

        r_args = (d["P"], d["Q"], d["w"], d["H"], d["R"], d["stats_w"], d["gR"], d["gt"], d["gH"])
        r_ref, r_got = cg.rigid_bwd_ref(*r_args), cg.rigid_bwd_model(model, *r_args)
        hold(cg.check_rigid_bwd(r_got, r_ref), lim, tag + "rigid, as restated")
        for mutate, what, outs in (("neighbour", "cloud j takes cloud j + 1's constants (rigid)", ("dP", "dQ", "dw")),
                                   ("untransposed", "dP from dH instead of dH^T (rigid)", ("dP",)),
                                   ("no_gt_in_dq", "the (w_i / W) g_t term is dropped from dQ", ("dQ",)),
                                   ("u_untransposed", "u = R g_t instead of R^T g_t", ("dP", "dw")),
                                   ("no_pbar_term", "the -g_t pbar^T term is dropped from gR'", ("dP", "dQ", "dw")),
                                   ("no_inv_w_in_dw", "the 1 / W terms are dropped from dw", ("dw",)),
                                   ("previous_centroid", "the centroid of the previous cloud is used", ("dP", "dQ", "dw"))):
            bad = cg.rigid_bwd_ref(*r_args, mutate=mutate)
            wrong = {k: r_got[k] + (bad[k] - r_ref[k]) for k in ("dP", "dQ", "dw")}
            for k in outs:          # every output the mistake reaches must notice it, not just one of them
                _seeded(tag + what + " [%s]" % k, cg.check_rigid_bwd(wrong, r_ref, (k,)), lim, report)
    print("\n".join(report))
