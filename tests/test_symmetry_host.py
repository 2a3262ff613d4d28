"""The symmetry-aware metric and loss without a GPU: K4s (so3_sym_angle_error_f32) and K3s (so3_sym_frob_loss_f32) are declared,
exported and bound, their arguments are checked on the host, SymmetryTable and cyclic_symmetry validate and lay out their groups,
and the numpy float64 oracle below (what tests/test_gpu_symmetry.py compares the kernels with) reproduces G17, the reference's
angle_error and loss_frobenius run on every candidate R_pred @ S_k."""
import ctypes
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import load_golden

NEW = ("so3_sym_angle_error_f32", "so3_sym_frob_loss_f32")
TABLES = ("flip", "c4y", "multi")


def sym_oracle(p, t, S, cls=None):
    """float64 oracle of both functions.  p, t: (B,3,3) float32 data; S: (C,K,3,3) the table's float32 entries; cls: (B,) ints or None.
    Every candidate R_pred @ S_k is formed in float64 from the float32 values.  Returns a dict: deg_all (B,K), deg, idx (-1 and NaN for a
    class id out of range), dist_all, loss_idx, loss (the mean), dp, dt (the selected branch's gradients of the mean), range (B,) bool:
    the identity cosine outside [-1.1, 1.1]."""
    p64, t64 = np.asarray(p, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3, 3)
    S = np.asarray(S, np.float64)
    b = p64.shape[0]
    cls = np.zeros(b, np.int64) if cls is None else np.asarray(cls, np.int64)
    bad = (cls < 0) | (cls >= S.shape[0])
    s = S[np.where(bad, 0, cls)]                                                    # (B, K, 3, 3)
    cand = np.einsum("bil,bklj->bkij", p64, s)
    c = (np.einsum("bkij,bij->bk", cand, t64) - 1.0) / 2.0
    with np.errstate(invalid="ignore"):
        deg_all = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    idx = np.argmin(deg_all, axis=1)
    diff = t64[:, None] - cand
    dist_all = np.sqrt((diff * diff).sum(axis=(2, 3)))
    loss_idx = np.argmin(dist_all, axis=1)
    rows = np.arange(b)
    d = dist_all[rows, loss_idx]
    dsel, ssel = diff[rows, loss_idx], s[rows, loss_idx]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(d > 0, 1.0 / (b * d), 0.0)[:, None, None]
    dt = dsel * w
    dp = -np.einsum("bil,bjl->bij", dsel, ssel) * w
    deg = deg_all[rows, idx].copy()
    deg[bad], d = np.nan, np.where(bad, np.nan, d)
    dp[bad], dt[bad] = np.nan, np.nan
    c0 = (np.einsum("bij,bij->b", p64, t64) - 1.0) / 2.0
    return dict(deg_all=deg_all, deg=deg, idx=np.where(bad, -1, idx), dist_all=dist_all, loss_idx=np.where(bad, -1, loss_idx),
                loss=d.mean() if b else np.nan, dist=d, dp=dp, dt=dt, range=(c0 < -1.1) | (c0 > 1.1), bad=bad)


def g17_case(g, tag):
    S = g[tag + "_S"]
    return g[tag + "_p"], g[tag + "_t"], S, (g[tag + "_cls"] if S.shape[0] > 1 else None)


def test_g17_oracle_reproduces_the_reference():
    g = load_golden("g17_symmetry.npz")
    for tag in TABLES:
        p, t, S, cls = g17_case(g, tag)
        o = sym_oracle(p, t, S, cls)
        np.testing.assert_allclose(o["deg_all"], g[tag + "_deg_all"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(o["deg"], g[tag + "_deg"], rtol=0, atol=1e-9)
        assert np.array_equal(o["idx"], g[tag + "_idx"]), tag
        assert np.array_equal(o["loss_idx"], g[tag + "_loss_idx"]), tag
        np.testing.assert_allclose(o["dist_all"], g[tag + "_dist_all"], rtol=1e-12, atol=1e-14)
        assert abs(o["loss"] - float(g[tag + "_loss"])) < 1e-12
        np.testing.assert_allclose(o["dp"], g[tag + "_dp"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(o["dt"], g[tag + "_dt"], rtol=0, atol=1e-12)
        # the fixture covers what it claims: exact ties (resolved to the smallest k), a winner other than the identity
        assert np.any((g[tag + "_deg_all"] == g[tag + "_deg"][:, None]).sum(axis=1) > 1), tag
        assert np.any(g[tag + "_idx"] > 0), tag
    flip_tie = g["flip_deg_all"][1]
    assert flip_tie[1] == flip_tie[2] == flip_tie.min() and g["flip_idx"][1] == 1       # a tie between k = 1 and 2 picks 1
    p, t = g["bad_p"], g["bad_t"]
    S = g["flip_S"]
    assert np.array_equal(sym_oracle(p, t, S)["range"], g["bad_raises"])


def test_cyclic_symmetry_is_a_group():
    from poseestimation_amd import cyclic_symmetry
    for n, axis in ((1, "z"), (2, "z"), (4, "y"), (6, "x"), (24, "z"), (7, [1.0, 2.0, -0.5]), (64, torch.tensor([0.0, 3.0, 4.0]))):
        g = cyclic_symmetry(n, axis).numpy()
        assert g.shape == (n, 3, 3) and g.dtype == np.float64
        assert np.array_equal(g[0], np.eye(3))
        for i in range(n):
            for j in range(n):
                np.testing.assert_allclose(g[i] @ g[j], g[(i + j) % n], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.linalg.det(g), 1.0, rtol=0, atol=1e-12)
    c4 = cyclic_symmetry(4, "y").numpy()                                          # quarter turns are exact
    assert set(np.unique(c4)) <= {-1.0, 0.0, 1.0}
    np.testing.assert_array_equal(c4[1], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]])      # Ry(pi/2)
    for bad in ((0, "z"), (-1, "z"), (2.5, "z"), (3, "w"), (3, [0.0, 0.0, 0.0]), (3, [1.0, 2.0])):
        with pytest.raises(ValueError):
            cyclic_symmetry(*bad)


def test_symmetry_table_validates_and_lays_out():
    from poseestimation_amd import SymmetryTable, cyclic_symmetry
    t = SymmetryTable(cyclic_symmetry(4, "y"))
    assert (t.num_classes, t.K) == (1, 4) and tuple(t.matrices.shape) == (1, 4, 3, 3)
    assert torch.equal(t.matrices[0], cyclic_symmetry(4, "y"))
    rx = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64))
    t = SymmetryTable([torch.eye(3)[None], [rx.numpy()], cyclic_symmetry(3, "z")])     # {I}, a group without I, C_3
    assert (t.num_classes, t.K) == (3, 3)
    eye = torch.eye(3, dtype=torch.float64)
    for c in range(3):
        assert torch.equal(t.matrices[c, 0], eye)                                       # the identity at slot 0 ...
    assert torch.equal(t.matrices[0, 1], eye) and torch.equal(t.matrices[0, 2], eye)      # ... and as padding
    assert torch.equal(t.matrices[1, 1], rx) and torch.equal(t.matrices[1, 2], eye)
    assert torch.equal(t.matrices[2], cyclic_symmetry(3, "z"))
    ry_first = torch.stack([cyclic_symmetry(2, "y")[1], eye])                          # the identity moves to slot 0
    assert torch.equal(SymmetryTable(ry_first).matrices[0], torch.stack([eye, cyclic_symmetry(2, "y")[1]]))
    assert SymmetryTable(np.eye(3)).K == 1                                              # one (3,3) matrix
    assert tuple(SymmetryTable(cyclic_symmetry(64)).matrices.shape) == (1, 64, 3, 3)
    assert SymmetryTable([cyclic_symmetry(4)] * 64).K == 4                               # 64 x 4 = 256 entries
    bad = [
        1.01 * cyclic_symmetry(4),                                                      # not orthogonal
        torch.diag(torch.tensor([1.0, 1.0, -1.0]))[None],                               # a reflection
        -torch.eye(3)[None],                                                            # det -1
        torch.zeros(2, 3, 3),
        torch.eye(3).repeat(2, 1)[None],                                                # (1, 6, 3)
        torch.eye(4)[None],
        torch.zeros(0, 3, 3),
        torch.full((1, 3, 3), float("nan")),
        cyclic_symmetry(65),                                                            # K > 64
        [cyclic_symmetry(4)] * 65,                                                      # 65 x 4 > 256
        [],
    ]
    for g in bad:
        with pytest.raises(ValueError):
            SymmetryTable(g)
    ok = cyclic_symmetry(4).clone()
    ok[1] += 5e-7                                                                       # within 1e-5: accepted
    SymmetryTable(ok)


def test_cpu_tensors_and_bad_arguments_raise():
    import poseestimation_amd as pa
    t = pa.SymmetryTable(pa.cyclic_symmetry(2))
    r = torch.eye(3).repeat(4, 1, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        pa.symmetric_angle_error(r, r, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        pa.symmetric_loss_frobenius(r, r, t)
    with pytest.raises(TypeError):
        pa.symmetric_angle_error(r, r, pa.cyclic_symmetry(2))                         # not a SymmetryTable


def test_symmetric_entries_are_declared_exported_and_bound(built_library):
    from poseestimation_amd import _lib
    from test_abi_and_host import header_symbols
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(so3_[a-z0-9_]+)\b", exported))
    for name in NEW:
        assert name in header_symbols()
        assert name in exported
        assert name in _lib.SYMBOLS
    assert _lib.load().so3_version() == 210 == _lib.ABI_VERSION


def test_symmetric_arguments_are_checked_on_the_host(built_library):
    """Each bad argument returns SO3_ERR_INVALID with a so3_last_error text before any launch; B == 0 is a no-op.  No device is
    touched.  On a thread of its own: so3_last_error() is per thread, and other tests expect the main thread's to be empty."""
    errors = []

    def run():
        try:
            check_symmetric_arguments()
        except BaseException as e:          # re-raised on the test's thread
            errors.append(e)
    worker = threading.Thread(target=run)
    worker.start()
    worker.join()
    if errors:
        raise errors[0]


def check_symmetric_arguments():
    from poseestimation_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)             # never dereferenced: every call below returns before a launch
    ang, loss = lib.so3_sym_angle_error_f32, lib.so3_sym_frob_loss_f32

    def a(S=f, cls=None, C=1, K=4, P=f, T=f, deg=f, flags=0, B=8):
        return ang(P, T, S, cls, C, K, deg, None, None, flags, B, None)

    def lo(S=f, cls=None, C=1, K=4, P=f, T=f, ls=f, flags=0, B=8):
        return loss(P, T, S, cls, C, K, None, None, None, ls, None, None, flags, B, None)

    for call, name in ((a, b"so3_sym_angle_error_f32"), (lo, b"so3_sym_frob_loss_f32")):
        for kw, text in (({"K": 0}, b"K must be in [1, 64]"), ({"K": 65}, b"K must be in [1, 64]"),
                         ({"C": 0}, b"num_classes must be >= 1"), ({"C": -3}, b"num_classes must be >= 1"),
                         ({"C": 5, "K": 64, "cls": f}, b"num_classes * K must be <= 256"),
                         ({"C": 2, "cls": None}, b"class_id must be given"), ({"C": 1, "cls": f}, b"class_id must be given"),
                         ({"S": None}, b"S is null"), ({"B": -1}, b": B"), ({"B": 1 << 50}, b": B"),
                         ({"flags": 0x100}, b"unknown flag"), ({"P": None}, b"null pointer"), ({"T": None}, b"null pointer")):
            assert call(**kw) == -1, (name, kw)
            err = lib.so3_last_error()
            assert name in err and text in err, (kw, err)
        assert call(B=0) == 0                                               # a no-op, nothing checked past the limits
        assert call(C=64, K=4, cls=f, B=0) == 0                             # 256 entries: accepted
    assert a(deg=None) == -1 and b"null pointer" in lib.so3_last_error()
    assert lo(ls=None) == -1 and b"null pointer" in lib.so3_last_error()
    assert a(flags=_lib.RADIANS, B=0) == 0                                   # SO3_RADIANS is the metric's one flag
    assert lo(flags=_lib.RADIANS) == -1                                      # the loss has none
