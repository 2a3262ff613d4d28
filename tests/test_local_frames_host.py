"""local_frames and estimate_normals (so3_local_frames_f32) without a GPU: the boundary (header, binding table, exports, argument
validation, the Python names), the G29 fixture's own consistency under the judges, and the kernel's device functions compiled for the
host (tests/host_model/local_frames.cpp with SO3_HOST_MODEL) on G29 and on the branch cases (sign ties, a viewpoint exactly in the plane).

The covariance is a definition (include/so3proj.h), so it is compared EXACTLY with the numpy restatement (tests/local_frames_ref.py:
cov32).  The eigen stage is judged by bounds whose constants are 4 x what the host model reaches here: the model itself is held to the
UN-multiplied figures (ref.MEASURED), which is what keeps the constants honest.  tests/test_gpu_local_frames.py imports the checks
and runs them on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import local_frames_ref as ref
from support import bits, boundary, build_host_model, lengths_of, np_ptr, on_own_thread

NEW_SYMBOLS = {"so3_local_frames_f32": 15}
SRC = os.path.join(ROOT, "tests", "host_model", "local_frames.cpp")
GRID_CAP, BLOCK = 8192, 256          # so3proj.hip: kThreeMaxGrid, kBlock
SWEEPS = 4                           # so3_device.h: kFramesSweeps


# ---- the boundary ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree(built_library):
    from poseestimation_amd import _lib
    boundary(built_library, NEW_SYMBOLS)
    assert _lib.KNN_MAX_K == ref.MAX_K == 64


def test_argument_validation_without_gpu(built_library):
    on_own_thread(_argument_validation)


def _argument_validation():
    from poseestimation_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    err = lib.so3_last_error

    def call(b, n, m, k=4, Y=p, idx=p, stride=None, cov=p, lam=p, nrm=p, frm=p):
        return lib.so3_local_frames_f32(Y, 3 * max(m, 0) if stride is None else stride, idx, None, None, None, cov, lam, nrm, frm, k, b, n, m, None)

    assert call(0, 8, 8, Y=None, idx=None, cov=None, lam=None, nrm=None, frm=None) == 0          # B == 0: a no-op, whatever the pointers
    big = _lib.ADD_S_MAX_N + 1
    for b, n, m in ((-1, 8, 8), (2**62, 8, 8), (4, 0, 8), (4, 8, 0), (4, -3, 8), (4, big, 8), (4, 8, big)):
        assert call(b, n, m) != 0 and err() == b"so3_local_frames_f32: B/N/M: invalid argument", (b, n, m, err())
    for k in (0, -1, 65, 2**31 - 1):
        assert call(4, 8, 8, k) != 0 and err() == b"so3_local_frames_f32: K: invalid argument", (k, err())
        assert call(0, 8, 8, k) != 0 and err() == b"so3_local_frames_f32: K: invalid argument"    # K is checked before the no-op
    for stride in (1, 23, -24):
        assert call(4, 8, 8, stride=stride) != 0 and err() == b"so3_local_frames_f32: y_stride: invalid argument", (stride, err())
    for kw in ({"Y": None}, {"idx": None}, {"cov": None, "lam": None, "nrm": None, "frm": None}):      # all outputs NULL is an error
        assert call(4, 8, 8, **kw) != 0 and err() == b"so3_local_frames_f32: null pointer: invalid argument", (kw, err())


def test_python_surface_without_gpu():
    import poseestimation_amd as pa
    from poseestimation_amd import rotation_representation as rr
    for name in ("local_frames", "estimate_normals"):
        assert name in pa.__all__ and getattr(pa, name) is getattr(rr, name)
    Y, idx = torch.zeros(2, 7, 3), torch.zeros(2, 5, 4, dtype=torch.long)
    for fn in (lambda: pa.local_frames(Y, idx), lambda: pa.local_frames(Y[0], idx.int(), return_covariance=True),
               lambda: pa.local_frames(Y, idx, torch.tensor([1, 2]), torch.tensor([3, 4]), torch.zeros(2, 3)),
               lambda: pa.estimate_normals(Y), lambda: pa.estimate_normals(Y, 3, torch.tensor([1, 2]), torch.zeros(3), True)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn()
    for k in (0, -1, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="estimate_normals: expected an int 1 <= K <= 64, got"):
            pa.estimate_normals(Y, k)


# ---- the fixture ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g29_cases():
    return ref.cases(ref.g29())


def test_g29_is_self_consistent(g29_cases):
    assert os.path.getsize(ref.GOLDEN) <= 512 * 1024
    by_name = {c["name"]: c for c in g29_cases}
    for fam in ref.SURFACES:
        for n, m, K in ref.SURFACE_SHAPES:
            c = by_name["%s_%dx%dx%d" % (fam, n, m, K)]
            assert (c["n"], c["m"], c["K"]) == (n, m, K) and ref.small_gap_share(c["ref64"][1], c["ref64"][3]) <= ref.SMALL_GAP_SHARE, c["name"]
    assert by_name["sphere_64x64x3"]["K"] == by_name["plane_64x64x3"]["K"] == 3
    assert {c["family"] for c in g29_cases} == set(ref.SURFACES) | {"shifted", "lattice_plane", "collinear", "tied", "flat", "r2", "mixed", "ragged", "view"}
    for c in g29_cases:
        Y, idx, xl, yl = c["Y"], c["idx"], c["x_lengths"], c["y_lengths"]
        C64, lam64, E64, r, piv = c["ref64"]
        assert Y.dtype == np.float32 and np.isfinite(Y).all(), c["name"]
        if c["family"] != "shifted":
            assert np.linalg.norm(Y, axis=-1).max() <= 1 + 1e-6, c["name"]
        assert np.array_equal(bits(ref.cov32(Y, idx, xl, yl)), bits(c["cov32"])), c["name"]
        _, lam, E, r2, _ = ref.frames64(Y, idx, xl, yl)                                          # the recorded eigh is an eigh of C64
        assert np.array_equal(r, r2) and np.abs(lam - lam64).max() <= 1e-14 * max(1.0, np.abs(lam64).max()), c["name"]
        assert np.abs(C64 @ E64 - E64 * lam64[..., None, :]).max() <= 1e-14 and np.abs(np.swapaxes(E64, -1, -2) @ E64 - np.eye(3)).max() <= 1e-14, c["name"]
        ref.judge(c["name"], Y, idx, xl, yl, c["viewpoint"], cov=c["cov32"], ref64=c["ref64"])      # cov32 is an accurate covariance
    c = by_name["shifted_100x150x12"]                                                            # the pivot keeps float32's digits
    assert np.abs(c["Y"]).min() > 98 and ref.judge("shifted", c["Y"], c["idx"], None, None, None, cov=c["cov32"], ref64=c["ref64"])["cov"] <= ref.MEASURED["cov"]
    c = by_name["lattice_plane"]
    assert (c["ref64"][1][..., 0] == 0).all() and np.abs(np.abs(c["ref64"][2][..., :, 0]) - [0, 0, 1]).max() <= 1e-15 and (c["cov32"][..., [2, 4, 5]] == 0).all()
    c = by_name["collinear"]
    assert (c["ref64"][1][..., 1] <= 1e-13).all() and (c["ref64"][1][..., 2] > 1e-4).all()     # collinear up to the points' own rounding
    for name in ("octahedron", "cube"):
        lam = by_name[name]["ref64"][1]
        assert (lam[..., 2] - lam[..., 0] <= 1e-15).all() and (lam > 0.1).all(), name
    for name in ("all_equal", "r1"):
        assert (by_name[name]["ref64"][0] == 0).all() and (by_name[name]["ref64"][3] >= 1).all() and (by_name[name]["cov32"] == 0).all(), name
    assert (by_name["r1"]["ref64"][3] == 1).all() and (by_name["r2"]["ref64"][3] == 2).all() and (by_name["r2"]["ref64"][1][..., 1] <= 1e-15).all()
    c = by_name["mixed"]
    valid = (c["idx"] >= 0) & (c["idx"] < c["m"])
    assert {-1, c["m"], ref.INT32_MIN} <= set(np.unique(c["idx"][~valid])) and not valid[:, :, 0].any() and (np.diff(valid.astype(int), axis=-1) > 0).any()
    assert (c["ref64"][3][:, 0] == 0).all() and (c["ref64"][3][:, 1] == 1).all() and (c["ref64"][3][:, 2] == 2).all()
    c = by_name["ragged"]
    nl, ml = lengths_of(c["x_lengths"], c["b"], c["n"]), lengths_of(c["y_lengths"], c["b"], c["m"])
    assert nl[0] == 0 and ml[1] == 0 and ml[2] == 1 and 1 < ml[3] < c["K"] and (c["ref64"][3][:2] == 0).all() and (c["ref64"][3][2, :nl[2]] == 1).all()
    assert (c["ref64"][3][3, :nl[3]] == ml[3]).all() and (c["ref64"][3][3, nl[3]:] == 0).all()
    assert np.array_equal(by_name["view_inside"]["Y"], by_name["view_outside"]["Y"]) and np.abs(by_name["view_inside"]["viewpoint"]).max() == 0
    assert np.linalg.norm(by_name["view_outside"]["viewpoint"]) > 1


# ---- the checks, shared with tests/test_gpu_local_frames.py ---------------------------------------------------------------
def check_case(label, c, outs, constants=ref.CONSTANTS):
    """outs = (cov, eigenvalues, normals, frames) as numpy arrays or None -> the judges' figures."""
    cov, lam, nrm, frm = outs
    got = ref.judge(label + " " + c["name"], c["Y"], c["idx"], c["x_lengths"], c["y_lengths"], c["viewpoint"], cov, lam, nrm, frm,
                    want_cov=c["cov32"], constants=constants, ref64=c["ref64"])
    if c["name"] == "lattice_plane" and lam is not None:
        assert (lam[..., 0] == 0).all(), label                                                   # lambda_0 == 0 exactly
    if c["name"] == "view_outside" and nrm is not None:                                          # the facing side points outward
        facing = ref.facing_side(c["Y"][:, :c["n"]], c["viewpoint"])
        assert facing.sum() >= 5 and ((nrm.astype(np.float64) * c["Y"][:, :c["n"]]).sum(-1)[facing] > 0).all(), label
    if c["name"] == "view_inside" and nrm is not None:                                           # towards the centre: inward
        assert ((nrm.astype(np.float64) * c["Y"][:, :c["n"]]).sum(-1) < 0).all(), label
    return got


def check_against_g29(cases, run, label, constants=ref.CONSTANTS):
    """`run(case)` -> (cov, eigenvalues, normals, frames).  -> the worst figure of each judge over the fixture."""
    worst = {}
    for c in cases:
        for k, v in check_case(label, c, run(c), constants).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def scaled_case(c, e):
    """The case with its cloud (and viewpoint) multiplied by 2^e."""
    s = np.float32(2.0 ** e)
    d = dict(c)
    d["Y"] = c["Y"] * s
    d["viewpoint"] = None if c["viewpoint"] is None else c["viewpoint"] * s
    return d


def check_power_of_two(label, c, base, run, e=20):
    """Scaling the cloud by 2^+-e scales cov and the eigenvalues by 4^+-e bit for bit and leaves the frames' bits."""
    for ee in (e, -e):
        cov, lam, nrm, frm = run(scaled_case(c, ee))
        f = np.float32(4.0 ** ee)
        assert np.array_equal(bits(cov), bits(base[0] * f)), (label, c["name"], ee, "cov")
        assert np.array_equal(bits(lam), bits(base[1] * f)), (label, c["name"], ee, "eigenvalues")
        assert np.array_equal(bits(nrm), bits(base[2])) and np.array_equal(bits(frm), bits(base[3])), (label, c["name"], ee, "frames")


# ---- where the sign rules branch exactly (tests/local_frames_ref.py: the branch cases) -------------------------------------------------
def flipped(a):
    """The bits of -a."""
    return bits(a) ^ np.uint32(0x80000000)


def check_sign_ties(label, c, outs):
    """The existing judges, and on every row the tied vector (e0 of a plane, e2 of a line): its two tied components bit-equal in
    magnitude (the premise, asserted on the output), the lower-indexed one positive, the other one's sign the patch's, the third
    component a zero.  With a viewpoint e0's own sign is the caller's to judge (check_viewpoint_in_the_plane)."""
    got = check_case(label, c, outs)
    cov, lam, nrm, frm = outs
    what = (label, c["name"])
    E = None if frm is None else frm.reshape(frm.shape[:2] + (3, 3))
    e0, e2 = (None, None) if E is None else (E[..., :, 0], E[..., :, 2])
    for vec, rows, is_e0 in ((nrm, ~c["line"], True), (e0, ~c["line"], True), (e2, c["line"], False)):
        if vec is None or not rows.any():
            continue
        p, q = c["tied"][..., :1], c["tied"][..., 1:]
        vp, vq, vr = (np.take_along_axis(vec, a, -1)[..., 0][rows] for a in (p, q, 3 - p - q))
        assert np.array_equal(bits(np.abs(vp)), bits(np.abs(vq))) and (np.abs(vp) > 0.7).all(), (what, "the tied components are no tie")
        assert (vr == 0).all(), what
        if c["viewpoint"] is None or not is_e0:
            assert (vp > 0).all(), (what, "the lowest index decides")
        assert ((vp > 0) != (vq > 0))[c["opposite"][rows]].all() and ((vp > 0) == (vq > 0))[~c["opposite"][rows]].all(), what
    return got


def check_viewpoint_in_the_plane(label, cases, run):
    """cases: ref.viewpoint_cases(...); run(case) -> (cov, eigenvalues, normals, frames).  A viewpoint exactly in the plane keeps the
    normal the call without one gives, bit for bit; one lattice step off the plane on either side gives the two opposite signs."""
    outs = {k: run(c) for k, c in cases.items()}
    for k, c in cases.items():
        check_sign_ties(label, c, outs[k])
    none = outs["none"]
    for k in ("in", "above"):
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(outs[k], none)), (label, k, "exactly 0 keeps the sign")
    cov, lam, nrm, frm = outs["below"]
    assert np.array_equal(bits(cov), bits(none[0])) and np.array_equal(bits(lam), bits(none[1])), label
    assert np.array_equal(bits(nrm), flipped(none[2])), (label, "below the plane: the other sign")
    f, f0 = frm.reshape(frm.shape[:2] + (3, 3)), none[3].reshape(frm.shape[:2] + (3, 3))
    assert np.array_equal(bits(f[..., :, 0]), flipped(f0[..., :, 0])) and np.array_equal(bits(f[..., :, 2]), bits(f0[..., :, 2])), label
    assert np.array_equal(f[..., :, 1], -f0[..., :, 1]), label                                   # e1 = e2 x e0 turns with e0 (zeros may keep their sign)


def check_left_out_and_shared(label, c, run):
    """run(case, want, shared) -> the outputs.  Each optional output left out once, and the shared cloud once: the same bits."""
    full = run(c, (True, True, True, True), False)
    for drop in range(4):
        want = tuple(k != drop for k in range(4))
        got = run(c, want, False)
        assert all((g is None and not w) or (w and np.array_equal(bits(g), bits(f))) for g, f, w in zip(got, full, want)), (label, drop)
        check_sign_ties(label, c, got)
    assert all(np.array_equal(bits(g), bits(f)) for g, f in zip(run(c, (True, True, True, True), True), full)), (label, "shared")
    return full


# ---- the device functions on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lib = build_host_model(tmp_path_factory, "local_frames", SRC)
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.model_local_frames.argtypes = [P, I64, P, P, P, P, P, P, P, P, I32, I64, I32, I32, I32]
    return lib


def host_run(model, c, sweeps=SWEEPS, want=(True, True, True, True), shared=False):
    """shared: the first cloud alone with y_stride 0."""
    b, n, m, K = c["b"], c["n"], c["m"], c["K"]
    Y, idx = np.ascontiguousarray(c["Y"][0] if shared else c["Y"], np.float32), np.ascontiguousarray(c["idx"], np.int32)
    xl, yl, view = (None if c[k] is None else np.ascontiguousarray(c[k], t) for k, t in (("x_lengths", np.int32), ("y_lengths", np.int32), ("viewpoint", np.float32)))
    outs = [np.full((b, n, w), np.nan, np.float32) if flag else None for flag, w in zip(want, (6, 3, 3, 9))]
    stride = 0 if shared else 3 * m
    assert model.model_local_frames(np_ptr(Y), stride, np_ptr(idx), np_ptr(xl), np_ptr(yl), np_ptr(view), *(np_ptr(o) for o in outs), K, b, n, m, sweeps) == 0
    return tuple(outs)


def test_host_model_against_g29(model, g29_cases):
    """Bit-equal to cov32 and within the UN-multiplied bounds (the judges' constants are 4 x these), twice with the same bits."""
    assert model.model_local_frames_sweeps() == SWEEPS
    worst = check_against_g29(g29_cases, lambda c: host_run(model, c), "host", constants=ref.MEASURED)
    print("host model over G29, in units of u t (orth: u):", {k: round(v, 2) for k, v in sorted(worst.items())})
    assert all(4 * ref.MEASURED[k] == ref.CONSTANTS[k] for k in ref.MEASURED)
    assert all(worst[k] > ref.MEASURED[k] / 2 for k in worst), worst                             # the recorded figures are the measured ones, not slack
    c = next(c for c in g29_cases if c["name"] == "blob_257x300x16")
    a, b_ = host_run(model, c), host_run(model, c)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b_))
    only = host_run(model, c, want=(False, False, True, False))                                  # normals alone
    assert only[0] is None and np.array_equal(bits(only[2]), bits(a[2]))


def test_host_model_sweep_count(model, g29_cases):
    """One sweep fewer misses the un-multiplied residual figure; one sweep more changes nothing the judges see."""
    inf = {k: np.inf for k in ref.CONSTANTS}
    fewer = check_against_g29(g29_cases, lambda c: host_run(model, c, SWEEPS - 1), "host, one sweep fewer", constants=inf)
    more = check_against_g29(g29_cases, lambda c: host_run(model, c, SWEEPS + 1), "host, one sweep more", constants=ref.MEASURED)
    print("one sweep fewer:", {k: round(v, 2) for k, v in sorted(fewer.items())}, " one more:", {k: round(v, 2) for k, v in sorted(more.items())})
    assert fewer["res"] > ref.MEASURED["res"], fewer


def test_host_model_power_of_two(model, g29_cases):
    for c in g29_cases:
        if c["family"] in ("sphere", "plane", "lattice_plane", "tied", "flat", "mixed", "ragged", "view") and c["n"] <= 257:
            check_power_of_two("host", c, host_run(model, c), lambda d: host_run(model, d))


def test_host_model_sign_ties(model):
    c = ref.sign_tie_case()
    assert (np.diff(c["Y"], axis=0) == 0).all() and {-1, c["m"], ref.INT32_MIN} <= set(np.unique(c["idx"]).tolist())
    base = check_left_out_and_shared("host", c, lambda d, want, shared: host_run(model, d, want=want, shared=shared))
    check_sign_ties("host", c, base)
    check_power_of_two("host", c, base, lambda d: host_run(model, d))
    y_eq_z = np.argwhere((c["tied"] == (1, 2)).all(-1) & c["opposite"] & ~c["line"])[0]          # the plane y = z: e0 = (+-0, s, -s), lambda = (0, 4/3, 8/3)
    assert np.array_equal(np.abs(base[2][tuple(y_eq_z)]), np.float32([0, np.sqrt(0.5), np.sqrt(0.5)])) and base[2][tuple(y_eq_z)][2] < 0
    assert np.array_equal(base[1][tuple(y_eq_z)], np.float32([0, 4 / 3, 8 / 3]))


@pytest.mark.parametrize("mirror", [False, True])
def test_host_model_viewpoint_in_the_plane(model, mirror):
    cases = ref.viewpoint_cases(mirror)
    check_viewpoint_in_the_plane("host", cases, lambda c: host_run(model, c))
    for k in ("in", "below"):
        check_power_of_two("host", cases[k], host_run(model, cases[k]), lambda d: host_run(model, d))
