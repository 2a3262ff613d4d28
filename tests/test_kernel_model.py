"""The kernels' own templates (csrc/so3_device.h) compiled for the host (oracle/kernel_model.cpp) and driven on the CPU:
golden vectors, adversarial families, batch invariance of the packed path, backward, float64 variant.  No GPU needed;
tests/test_gpu_parity.py checks that the device produces the same rows."""
import numpy as np
import pytest

from conftest import load_golden, orth_err

so = pytest.importorskip("oracle.so3_oracle")


@pytest.fixture(scope="module")
def km():
    from oracle import kernel_model
    if kernel_model.clangxx() is None:
        pytest.skip("clang++ (for ext_vector_type) is not available")
    kernel_model.build()
    return kernel_model


def _families(n, rng):
    a = rng.standard_normal((n, 3, 3))
    q1 = so.symmetric_orthogonalization_np(rng.standard_normal((n, 9)))
    q2 = so.symmetric_orthogonalization_np(rng.standard_normal((n, 9)))

    def with_s(s):
        return q1 @ (s[:, :, None] * q2)
    yield "gaussian", a
    for e in (1e-1, 1e-4, 1e-7):
        s = np.ones((n, 3)); s[:, 1] -= e * rng.random(n); s[:, 2] -= 2 * e * rng.random(n)
        yield "clustered %.0e" % e, with_s(s)
    for e in (1e-2, 1e-4, 1e-6):
        yield "graded %.0e" % e, with_s(np.stack((np.ones(n), np.full(n, e), np.full(n, e * e)), 1))
    yield "rotation + noise", q1 + 1e-3 * a
    yield "symmetric", a + a.transpose(0, 2, 1)
    yield "small integers", rng.integers(-3, 4, (n, 3, 3)).astype(np.float64)
    yield "outer products", rng.standard_normal((n, 3, 1)) @ rng.standard_normal((n, 1, 3))
    yield "integer outer products", (rng.integers(-3, 4, (n, 3, 1)) @ rng.integers(-3, 4, (n, 1, 3))).astype(np.float64)
    yield "nine equal entries", np.broadcast_to(rng.standard_normal((n, 1, 1)), (n, 3, 3)).copy()
    yield "rank two", np.concatenate((a[:, :2], a[:, :1] + a[:, 1:2]), 1)
    yield "scaled 1e18", 1e18 * a
    yield "scaled 1e-18", 1e-18 * a
    # families that broke prototypes of the quaternion fast path (docs/history/tools.tar.gz:tools/proto): exact double roots at the top of K's spectrum
    # (entries in -1..1: s2 = s3 with det < 0), reflections (a triple root), near-reflections (the SECOND gap small), and scales
    # at the edges of the window in which the fast path works without a prescale
    yield "entries in -1..1", rng.integers(-1, 2, (n, 3, 3)).astype(np.float64)
    yield "reflections", q1 * np.array([1.0, 1.0, -1.0])
    for e in (1e-3, 1e-1):
        s = np.ones((n, 3)); s[:, 1] -= e * rng.random(n); s[:, 2] = -(1 - e * rng.random(n))
        yield "near-reflections %.0e" % e, with_s(s)
    for sc in (2e-5, 5e-5, 3e4, 1e5):
        yield "scaled %.0e" % sc, sc * a


def test_model_against_golden_vectors(km):
    g = load_golden("g1_gaussian256.npz")
    r, flip = km.project(g["x"], want_flip=True)
    assert np.array_equal(flip, g["det"] < 0)
    assert orth_err(r).max() < 1e-5 and np.abs(r - g["r_f64"]).max() < 2e-5
    g2 = load_golden("g2_adversarial.npz")
    r2 = km.project(g2["x"])
    assert orth_err(r2).max() < 1e-5 and np.abs(np.linalg.det(r2.astype(np.float64)) - 1).max() < 1e-5


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_model_on_adversarial_families(km, dtype):
    rng = np.random.default_rng(2024)
    n = 20000
    for name, m in _families(n, rng):
        m32 = m.astype(np.float32)
        if dtype == "f32":
            r = km.project(m32).astype(np.float64)
            assert np.array_equal(km.project(m32, packed=True).astype(np.float64), r), name      # packed path: same rows
            tol_orth, tol_cond, tol_opt = 1e-5, 1e-5, 2e-6
        else:
            r = km.project_f64(m32.astype(np.float64))
            tol_orth, tol_cond, tol_opt = 1e-12, 1e-11, 1e-12
        assert orth_err(r).max() < tol_orth and np.abs(np.linalg.det(r) - 1).max() < 10 * tol_orth, name
        ref, s, d = so.symmetric_orthogonalization_np(m32, return_parts=True)
        gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / np.maximum(s[:, 0], 1e-300)
        ok = gap > 1e-6
        if ok.any():
            assert (np.abs(r - ref).reshape(n, -1).max(1) * gap)[ok].max() < tol_cond, name
            if dtype == "f32" and name == "scaled 3e+04":
                # entries of 3e4 are inside the fast path's window, but lambda^2 |q|^2 ~ lambda^8 is not inside float32: the residual
                # test once compared against an infinite reference there and kept every first eigenvector, converged or not
                assert (np.abs(r - ref).reshape(n, -1).max(1) * gap)[ok].max() < 2e-6, name
        # optimality (defined even where R is not unique): tr(R^T M) = s1 + s2 +- s3
        best = s[:, 0] + s[:, 1] + np.where(np.linalg.det(m32.astype(np.float64)) < 0, -s[:, 2], s[:, 2])
        got = (r * m32.astype(np.float64)).sum((1, 2))
        # (near-reflections have TWO small gaps, s2 + s3' and s1 + s3': the Jacobi path, which all of them take, stops at a
        #  residual of 0.7e-5 and leaves 4e-6 of the objective there)
        assert ((best - got) / np.maximum(s[:, 0], 1e-300)).max() < (tol_opt if "near-reflections" not in name or dtype == "f64" else 1e-5), name


def test_fast_path_declares_what_it_cannot_do(km):
    """The quaternion fast path alone (`quat_rotation`): on Gaussian input almost every row is settled and every settled row
    is as accurate as its conditioning allows; rank-deficient, tied and badly scaled input is declared hard (and then
    answered by the Jacobi path, which the family test above checks through the product entry point)."""
    rng = np.random.default_rng(5)
    n = 400_000
    m = rng.standard_normal((n, 9)).astype(np.float32)
    r, hard = km.project_quat(m)
    assert hard.mean() < 2e-5                                   # 1.3e-6 measured
    ref, s, d = so.symmetric_orthogonalization_np(m, return_parts=True)
    gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]
    err = np.abs(r.astype(np.float64) - ref).reshape(n, -1).max(1)
    assert (err * gap)[~hard].max() < 2e-6 and np.median(err) < 2e-7 and orth_err(r[~hard]).max() < 3e-6
    # the Jacobi path on the same rows, for the record of what the fast path replaces
    rj = km.project_jacobi(m).astype(np.float64)
    assert (np.abs(rj - ref).reshape(n, -1).max(1) * gap).max() < 5e-6
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    # an all-zero row (a dead head) is answered by the forward itself, in the branch rows outside the scale window take anyway:
    # the identity, exactly what the Jacobi path (and the reference) gives for it -- round 3 sent such rows there
    rz, hz = km.project_quat(np.zeros((4, 9), np.float32))
    assert not hz.any() and np.array_equal(rz.reshape(4, 9), np.tile(eye, (4, 1))) and np.array_equal(km.project_jacobi(np.zeros((4, 9), np.float32)), rz)
    for name, x in (("reflection", np.diag([1.0, 1.0, -1.0]).astype(np.float32).reshape(1, 9)),
                    ("rank one", np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]).astype(np.float32).reshape(1, 9)),
                    ("nan", np.full((2, 9), np.nan, np.float32)), ("inf", np.full((2, 9), np.inf, np.float32)),
                    ("double root", np.array([[0, -1, 1, 1, 0, 1, 1, -1, 0]], np.float32))):
        assert km.project_quat(x)[1].all(), name
    # rows far from unit scale are no longer hard: an exact power-of-two prescale brings them into the fast path's window
    # (round 2 sent them to the Jacobi path: a batch of 1e5 * Gaussian rows took 1.6 x the time of a Gaussian one)
    for scale in (1e18, 1e5, 1e-5, 1e-18, 2.0 ** 40, 2.0 ** -40):
        rs, hs = km.project_quat((scale * m[:4096]).astype(np.float32))
        assert not (hs & ~hard[:4096]).any(), scale
        refs = so.symmetric_orthogonalization_np((scale * m[:4096]).astype(np.float32))
        assert (np.abs(rs - refs).reshape(4096, -1).max(1) * gap[:4096])[~hs].max() < 2e-6, scale
        if np.log2(scale) == round(np.log2(scale)):
            assert np.array_equal(rs[~hs], r[:4096][~hs]), scale          # a power of two: the very same bits
    assert not km.project_quat(eye)[1].any() and np.abs(km.project_quat(eye)[0] - eye.reshape(1, 3, 3)).max() < 1e-6
    # backward: from the rotation alone on settled rows, equal to the Jacobi frames' up to conditioning
    g = rng.standard_normal((n, 9)).astype(np.float32)
    d_new, d_jac = km.project_bwd(m, g).reshape(n, 9), km.project_bwd_jacobi(m, g).reshape(n, 9)
    refg = so.projection_backward_np(m.astype(np.float64).reshape(n, 3, 3), g.astype(np.float64).reshape(n, 3, 3)).reshape(n, 9)
    scaled = lambda dd: (np.abs(dd - refg).max(1) * s[:, 0] * gap * gap)[gap > 1e-4].max()
    assert scaled(d_new) < 1e-5 and scaled(d_jac) < 1e-5
    rel = np.abs(d_new - refg).max(1) / (1e-3 + np.abs(refg).max(1))
    assert np.median(rel) < 5e-7 and np.quantile(rel, 0.99) < 1e-5


def test_model_special_rows(km):
    x = np.zeros((6, 9), np.float32)
    x[1] = np.eye(3).ravel()
    x[2] = np.diag([1.0, 1.0, -1.0]).ravel()                 # reflection -> identity, as the reference
    x[3] = np.diag([2.0, 2.0, 2.0]).ravel()
    x[4] = np.nan
    x[5] = [0, 1, 0, 0, 0, 1, 1, 0, 0]                        # a permutation that is a rotation: returned as is
    r = km.project(x)
    assert np.array_equal(r[0], np.eye(3)) and np.array_equal(r[1], np.eye(3)) and np.abs(r[2] - np.eye(3)).max() < 1e-7
    assert np.abs(r[3] - np.eye(3)).max() < 1e-7 and np.isnan(r[4]).all() and np.abs(r[5] - x[5].reshape(3, 3)).max() < 1e-7


def test_model_backward_against_the_closed_form(km):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((50000, 9)).astype(np.float32)
    g = rng.standard_normal((50000, 9)).astype(np.float32)
    ref = so.projection_backward_np(x, g)
    _, s, d = so.symmetric_orthogonalization_np(x, return_parts=True)
    gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]
    err = np.abs(km.project_bwd(x, g) - ref).reshape(len(x), -1).max(1) * s[:, 0] * gap * gap
    assert np.median(err) < 1e-6 and err.max() < 2e-5
    err64 = np.abs(km.project_bwd_f64(x.astype(np.float64), g.astype(np.float64)) - ref).reshape(len(x), -1).max(1) * s[:, 0] * gap * gap
    assert err64.max() < 1e-11
    # rank-deficient rows: floored denominators, finite gradients
    low = (rng.standard_normal((1000, 3, 1)) @ rng.standard_normal((1000, 1, 3))).astype(np.float32)
    assert np.isfinite(km.project_bwd(low, g[:1000])).all()
    # rows outside the fast path's scale window: the rotation comes from the prescaled matrix, and so must the gradient
    # (S = R^T M, its cofactors and determinant would leave the float32 range): dM(c M) = dM(M) / c, exactly for powers of two
    base = km.project_bwd(x[:4096], g[:4096])
    for scale in (2.0 ** 40, 2.0 ** -40, 1e18, 1e-18):
        xs = (scale * x[:4096]).astype(np.float32)
        d = km.project_bwd(xs, g[:4096])
        assert np.isfinite(d).all(), scale
        refs = so.projection_backward_np(xs, g[:4096])
        rel = np.abs(d - refs).reshape(4096, -1).max(1) / np.abs(refs).reshape(4096, -1).max(1)
        assert np.median(rel) < 5e-7 and rel.max() < 1e-3, scale
        if np.log2(scale) == round(np.log2(scale)):
            assert np.array_equal(d * np.float32(scale), base), scale


def test_model_backward_on_ill_conditioned_settled_rows_is_as_good_as_float32_autograd(km):
    """Rows the fast path SETTLES but whose gap s2 + s3' is small take their gradient from the rotation alone
    (backward_from_rotation).  Its relative error is judged per family against float64 autograd, next to the Jacobi frames'
    and to the reference's own float32 autograd through torch.svd -- not through a gap^2-scaled measure, which hides an
    eps / gap^2 error (round 2 used one triangle of R^T M: 10-300 x the Jacobi frames' error on these families)."""
    import torch
    rng = np.random.default_rng(3)

    def haar(n):
        q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
        q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
        return q * np.linalg.det(q)[:, None, None]

    def with_singular_values(sv):
        u, v = haar(len(sv)), haar(len(sv))
        return ((u * sv[:, None, :]) @ v.transpose(0, 2, 1)).astype(np.float32)

    def torch_f32(m, g):
        x = torch.tensor(m.reshape(-1, 9), dtype=torch.float32, requires_grad=True)
        r = so.symmetric_orthogonalization_torch(x)
        (r * torch.tensor(g, dtype=torch.float32).reshape(r.shape)).sum().backward()
        return x.grad.numpy().reshape(-1, 3, 3)

    n = 20000
    one = np.ones(n)
    families = {
        "s = (1, e, -e'), e = 1e-3": np.stack([one, 1e-3 * one, -1e-3 * rng.uniform(0, 0.9, n)], 1),
        "s = (1, e, e), e = 1e-4": np.stack([one, 1e-4 * one, 1e-4 * one], 1),
        "s = (1, 1e-2, -5e-3)": np.stack([one, 1e-2 * one, -5e-3 * one], 1),
        "s = (1, 0.1, -0.09)": np.stack([one, 0.1 * one, -0.09 * one], 1),
    }
    cases = [(k, with_singular_values(v)) for k, v in families.items()]
    cases += [("Gaussian x %g" % sc, (sc * rng.standard_normal((n, 3, 3))).astype(np.float32)) for sc in (1e-3, 1.0, 1e3)]
    for name, m in cases:
        g = rng.standard_normal((n, 3, 3)).astype(np.float32)
        ref = so.projection_backward_np(m.astype(np.float64), g.astype(np.float64))
        scale = np.abs(ref).reshape(n, -1).max(1)
        q = {}
        for who, d in (("new", km.project_bwd(m, g)), ("jacobi", km.project_bwd_jacobi(m, g)), ("torch32", torch_f32(m, g))):
            rel = np.abs(d - ref).reshape(n, -1).max(1) / scale
            q[who] = (np.median(rel), np.quantile(rel, 0.99))
        bar = [max(q["jacobi"][i], q["torch32"][i]) for i in range(2)]
        assert q["new"][0] <= 4 * bar[0] and q["new"][1] <= 5 * bar[1], (name, q)


@pytest.mark.parametrize("name", ["quat", "euler", "ortho5d", "expmap"])
def test_model_heads_against_golden_and_oracle(km, name):
    """Rows f2 / f5: the head operations of csrc/so3_rows.h on the host, against the reference's own outputs (G10) and
    float64 autograd through the restatement."""
    g = load_golden("g10_heads.npz")
    x, gr = g[name + "_x"], g[name + "_g"]
    assert np.abs(km.head(name, x) - g[name + "_r"]).max() < 5e-6
    ref = so.head_backward_np(name, x.astype(np.float64), gr.astype(np.float64))
    scale = np.maximum(np.abs(ref).max(axis=1), 1.0)
    err = np.abs(km.head_bwd(name, x, gr) - ref).max(axis=1) / scale
    ref_err = np.abs(g[name + "_dx"] - ref).max(axis=1) / scale
    assert np.median(err) < 2e-6 and err.max() < max(2e-5, 2.0 * ref_err.max())
    rng = np.random.default_rng(5)
    xs = rng.standard_normal((20000, km.HEAD_WIDTH[name])) * rng.choice([1e-3, 1.0, 30.0], (20000, 1))
    e = np.abs(km.head(name, xs) - so.head_np(name, xs.astype(np.float32))).reshape(20000, -1).max(1)
    assert np.median(e) < 3e-7 and np.quantile(e, 0.999) < 2e-5


def test_model_ortho6d_and_se3_update(km):
    g7 = load_golden("g7_ortho6d.npz")
    assert np.abs(km.head("ortho6d", g7["p"]) - g7["r"]).max() < 2e-6
    ref = g7["dp_f64"]
    rel = np.abs(km.head_bwd("ortho6d", g7["p"], g7["g"]) - ref).max(1) / (1e-3 + np.abs(ref).max(1))
    assert np.median(rel) < 1e-6 and rel.max() < 2e-4
    rng = np.random.default_rng(8)
    b = 5000
    out = rng.standard_normal((b, 12)).astype(np.float32)
    out[:, 11] = 1 + 0.05 * rng.standard_normal(b)
    t = np.tile(np.eye(4, dtype=np.float32), (b, 1, 1))
    t[:, :3, :3] = so.symmetric_orthogonalization_np(rng.standard_normal((b, 9)))
    t[:, :3, 3] = [0.0, 0.0, 2.0] + 0.2 * rng.standard_normal((b, 3))
    fx = fy = 50 / (36 / 320)
    tp = km.se3_update(out, t, fx, fy)
    ref = so.se3_update_np(out, t, fx, fy)
    _, s, d = so.symmetric_orthogonalization_np(out[:, :9], return_parts=True)
    gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]
    assert (np.abs(tp - ref).reshape(b, -1).max(1) * gap).max() < 5e-6
    gup = rng.standard_normal((b, 4, 4)).astype(np.float32)
    dref = so.se3_update_backward_np(out, t, gup, fx, fy)
    derr = np.abs(km.se3_update_bwd(out, t, gup, fx, fy) - dref).max(1) * np.minimum(1.0, s[:, 0] * gap * gap) / np.maximum(np.abs(dref).max(1), 1.0)
    assert np.median(derr) < 1e-6 and derr.max() < 5e-5


def test_model_property_any_finite_float32_matrix_gives_the_optimal_rotation(km):
    """Property test over arbitrary finite float32 entries (subnormals, 1e38, exact zeros, repeated values ...):
    the result is a rotation and attains max tr(R^T M) = s1 + s2 +- s3."""
    hypothesis = pytest.importorskip("hypothesis")
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st
    from hypothesis.extra import numpy as hnp

    @settings(max_examples=600, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(hnp.arrays(np.float32, (9,), elements=st.floats(width=32, allow_nan=False, allow_infinity=False)))
    def prop(m):
        r = km.project(m.reshape(1, 9))[0].astype(np.float64)
        assert np.isfinite(r).all()
        assert np.linalg.norm(r.T @ r - np.eye(3)) < 1e-5 and abs(np.linalg.det(r) - 1) < 1e-5
        mm = m.reshape(3, 3).astype(np.float64)
        if np.abs(mm).max() > 0:
            mm = mm / np.abs(mm).max()
            s = np.linalg.svd(mm, compute_uv=False)
            best = s[0] + s[1] + (s[2] if np.linalg.det(mm) >= 0 else -s[2])
            assert (best - (r * mm).sum()) / s[0] < 5e-6

    prop()


@pytest.mark.parametrize("scale", [2e-5, 5e-5, 1e-4, 1.0, 3e4, 8e4])
def test_fast_path_accuracy_does_not_depend_on_the_scale_inside_its_window(km, scale):
    """The fast path takes rows with |M|_F^2 in [2^-28, 2^36] as they come.  Its residual test once squared a residual that
    underflows for entries below 1e-4 (zero: every row 'accurate') and compared against lambda^2 |q|^2, which overflows above
    2e4 (infinite: the same) -- rows that needed the second eigenvector kept the first, 3e-6 to 8e-6 instead of 9e-7."""
    rng = np.random.default_rng(5)
    m = (rng.standard_normal((200_000, 9)) * scale).astype(np.float32)
    r, hard = km.project_quat(m)
    ref, s, d = so.symmetric_orthogonalization_np(m, return_parts=True)
    gap = np.where(d < 0, s[:, 1] - s[:, 2], s[:, 1] + s[:, 2]) / s[:, 0]
    err = np.abs(np.asarray(r, np.float64).reshape(-1, 9) - ref.reshape(-1, 9)).max(1) * gap
    ok = ~hard.astype(bool) & (gap > 1e-6)
    assert ok.mean() > 0.3                                       # the window's edges send more rows to the Jacobi path
    assert err[ok].max() < 1.2e-6


def test_park_reservations_tile_the_list_under_interleaving(km):
    """The list of parked hard rows (so3_rows.h: park_reserve_protocol): whatever the waves' interleaving, successful reservations
    tile [start, count) without hole or overlap and a failed one leaves the count alone.  The first case is the advisor's (round 4's
    add-then-subtract protocol gave the third wave base 505 with entries 500..504 unwritten)."""
    count, base = km.park_reserve_interleaved(500, 512, [13, 5, 6])
    assert count == 511 and list(base) == [-1, 500, 505]
    rng = np.random.default_rng(5)
    for trial in range(2000):
        cap = int(rng.choice([256, 512]))
        start = int(rng.integers(max(0, cap - 80), cap + 1))
        n = rng.integers(1, 33, int(rng.integers(1, 5))).astype(np.uint32)
        count, base = km.park_reserve_interleaved(start, cap, n, nested=bool(trial & 1))
        got = sorted((int(b), int(k)) for b, k in zip(base, n) if b >= 0)
        at = start
        for b, k in got:
            assert b == at, (start, cap, n, base)
            at += k
        assert at == count <= cap
        for b, k in zip(base, n):        # a refusal is justified by the count some moment held: at least start, at most the final one
            if b < 0:
                assert count + int(k) > cap or start + int(k) > cap or any(bb >= 0 for bb in base)
                assert int(k) + start > cap or count > start


def test_first_eigenvector_is_final_on_all_but_a_few_gaussian_rows(km):
    """How often the fast path's rare branch is asked for, counted on the host (one "lane" per row): a wave of the device takes the branch
    when ANY of its 128 rows asks, so 1.6e-3 of the rows is one round in five or six -- round 4's residual test asked for one in five.  A
    threshold or a start that drifts shows here before it shows as microseconds."""
    rng = np.random.default_rng(17)
    n = 400_000
    km.fast_path_counters()
    km.project_quat(rng.standard_normal((n, 9)).astype(np.float32))
    rows, adjugates = km.fast_path_counters()
    assert rows / n < 2.0e-3 and adjugates < 1.2 * rows, (rows / n, adjugates)           # 1.6e-3, 1.04 measured


def _acos_sweep_cosines():
    """2e7 cosines over [-1, 1] (a uniform grid, then dense neighbourhoods of +-1/2, where the kernel's acos changes branch, and of +-1,
    where the angle is small or next to pi), in chunks of 2e6."""
    n = 2_000_000
    for k in range(9):
        yield np.linspace(-1.0, 1.0, n) + (k - 4) * (1.0 / (9 * (n - 1)))       # nine interleaved grids, step 1.1e-7 between them
    j = np.arange(-n // 4, n // 4, dtype=np.float64)
    yield np.concatenate((0.5 + j * 2.0**-40, -0.5 + j * 2.0**-40, 0.5 + j * 2.0**-30, -0.5 + j * 2.0**-30))
    k = np.arange(n // 4, dtype=np.float64)
    geo = np.geomspace(2.0**-53, 0.5, n // 4)
    yield np.concatenate((1.0 - k * 2.0**-52, -1.0 + k * 2.0**-53, 1.0 - geo, -1.0 + geo))


def test_acos_f64_against_long_double_on_the_host(km):
    """so3_rows.h's acos_f64 -- every float64 angle the library returns, K4's and the fused K1+K4's degrees on float32 data included --
    against long double acos: <= 1.5e-14 rad absolute everywhere, <= 1e-14 relative for c > 1/2 (small angles stay accurate relative to
    their size), 0 and pi exactly at +-1, NaN for NaN.  tests/test_gpu_float64_metrics.py runs the same function through the device."""
    assert np.finfo(np.longdouble).eps < 1e-18, "needs an extended-precision long double for the reference"
    worst_abs = worst_rel = 0.0
    count = 0
    for c in _acos_sweep_cosines():
        c = np.clip(c, -1.0, 1.0)
        got = km.acos_f64(c)
        ref = np.arccos(c.astype(np.longdouble))
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        worst_abs = max(worst_abs, float(err.max()))
        big = (c > 0.5) & (c < 1.0)
        if big.any():
            worst_rel = max(worst_rel, float((err[big] / ref[big].astype(np.float64)).max()))
        count += c.size
    assert count >= 20_000_000
    assert worst_abs <= 1.5e-14 and worst_rel <= 1e-14, (worst_abs, worst_rel)
    ends = km.acos_f64(np.array([1.0, -1.0, 0.0, -0.0, np.nan]))
    assert ends[0] == 0.0 and ends[1] == np.pi and ends[2] == ends[3] == np.float64(np.pi / 2) and np.isnan(ends[4])


def test_reduction_slot_encoding_round_trips_and_never_reads_as_empty(km):
    """The workspace slots of the reducing kernels (so3_rows.h: slot_encode / slot_decode) hold a partial's bits plus one, 0 meaning
    "not here yet".  Ordinary values come back bit for bit, every NaN comes back a NaN, and no value at all encodes to 0 -- the NaN
    0xFFFF...F, which a float64 row of 0xFF bytes produces, once did (the summing workgroup then polled the slot for 0.1 s)."""
    rng = np.random.default_rng(52)
    bits = rng.integers(0, 2**64, 1_000_000, dtype=np.uint64, endpoint=False)
    special = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.finfo(np.float64).max, -np.finfo(np.float64).max,
                        np.inf, -np.inf, np.pi], np.float64)
    v = np.concatenate((bits.view(np.float64), special))
    ordinary = ~np.isnan(v)
    s = km.slot_encode(v)
    assert not (s == 0).any()
    back = km.slot_decode(s)
    assert np.array_equal(back[ordinary].view(np.uint64), v[ordinary].view(np.uint64))
    # NaN payloads: both signs, quiet and signalling, the extremes of the payload field and random ones in between
    payload = np.concatenate((np.array([1, 2**51 - 1, 2**51, 2**52 - 1], np.uint64), rng.integers(1, 2**52, 100_000, dtype=np.uint64)))
    nan_bits = np.concatenate((np.uint64(0x7FF0000000000000) | payload, np.uint64(0xFFF0000000000000) | payload))
    nans = nan_bits.view(np.float64)
    assert np.isnan(nans).all()
    s = km.slot_encode(nans)
    assert not (s == 0).any()
    assert np.isnan(km.slot_decode(s)).all()
