"""match_features on CPU tensors against its float64 definition (tests/match_ref.py): every family at every shape, full and ragged,
B in {1, 3}, mutual on and off; the dtypes; independence of B; the existing brute-force loop against the reference; and the rank map
of ransac_align's sampler with torch.rand replaced by chosen values.  Indices are compared exactly on the rows the reference calls
judged (at most 1 % of a case's live rows are not: the builders assert it).  No GPU."""
import numpy as np
import pytest
import torch

import match_ref as ref
from test_fpfh_host import match_loop

TORCH = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16}


def tensor(a, fmt, dev="cpu"):
    return torch.tensor(np.asarray(a), device=dev).to(TORCH[fmt])


def lengths_tensor(lengths, itype, dev="cpu"):
    return None if lengths is None else torch.tensor(np.asarray(lengths, itype), device=dev)


def run_on(dev):
    import poseestimation_amd as pa

    def run(fx, fy, xl, yl, itype, mutual, fmt="float32", fmt_y="float32"):
        got = pa.match_features(tensor(fx, fmt, dev), tensor(fy, fmt_y, dev), lengths_tensor(xl, itype, dev), lengths_tensor(yl, itype, dev), mutual=mutual)
        assert got.dtype == torch.int64 and got.shape == fx.shape[:2] and got.device.type == torch.device(dev).type
        return got.cpu().numpy()
    return run


def check_case(case, run, fmt="float32", fmt_y=None, alone=("full", "ragged64"), other=None):
    """Every (B, lengths, mutual) of a case through `run`: judged rows equal match_ref exactly; under the labels of `alone`, cloud b by
    itself gives row b of the batched call on every row.  other: a second runner (the GPU file's CPU call) held to the same and, on the
    judged rows, to the first one's answer."""
    fmt_y = fmt_y or fmt
    wrong = []
    for b, label, mutual in ref.variants_of(case):
        want, judged, xl, yl, itype = ref.expected(case, b, label, mutual)
        fx, fy = case["fx"][:b], case["fy"][:b]
        got = run(fx, fy, xl, yl, itype, mutual, fmt, fmt_y)
        bad = judged & (got != want)
        if bad.any():
            wrong.append((b, label, mutual, int(bad.sum()), int(judged.sum())))
        if other is not None:
            theirs = other(fx, fy, xl, yl, itype, mutual, fmt, fmt_y)
            assert np.array_equal(theirs[judged], got[judged]), (case["name"], b, label, mutual)
        if b > 1 and label in alone:
            for c in range(b):
                one = run(fx[c:c + 1], fy[c:c + 1], None if xl is None else xl[c:c + 1], None if yl is None else yl[c:c + 1], itype, mutual, fmt, fmt_y)
                assert np.array_equal(one[0], got[c]), (case["name"], label, mutual, c)
    assert not wrong, (case["name"], "(B, lengths, mutual, wrong rows, judged rows)", wrong)


# ---- the families at every shape ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_families_and_shapes(family, shape):
    check_case(ref.build(family, *shape), run_on("cpu"))


@pytest.mark.parametrize("family,d", [("small_integer", 1), ("small_integer", 352), ("fpfh_like", 352)])
def test_other_descriptor_lengths(family, d):
    for shape in ((26, 9), (64, 64)):
        check_case(ref.build(family, *shape, d=d), run_on("cpu"))


# ---- the dtypes ---------------------------------------------------------------------------------------------------------------
DTYPE_SHAPES = [(13, 9), (26, 9), (64, 64), (257, 300)]


@pytest.mark.parametrize("fmt,fmt_y", [("float64", "float64"), ("float32", "float64"), ("float64", "float32")])
def test_float64_and_mixed_inputs(fmt, fmt_y):
    """float64 and mixed inputs are computed in float64: the band is float64's, so the decoys 1e-3 apart in d2 and closer are judged."""
    for family in ref.FAMILIES:
        for shape in DTYPE_SHAPES:
            check_case(ref.build(family, *shape, fmt=fmt, fmt_y=fmt_y), run_on("cpu"), fmt, fmt_y)


@pytest.mark.parametrize("fmt,fmt_y", [("bfloat16", "bfloat16"), ("float16", "float16"), ("bfloat16", "float32"), ("float16", "bfloat16")])
def test_half_precision_inputs_are_computed_in_float32(fmt, fmt_y):
    """The inputs are rounded to the half format first; the reference reads those values and judges with float32's band.  half_exact
    is exact in float32 and ambiguous in an 8- or 11-bit significand: its decoy comes BEFORE the true row."""
    for family in ("half_exact", "small_integer", "fpfh_like", "duplicates"):
        for shape in DTYPE_SHAPES:
            check_case(ref.build(family, *shape, fmt=fmt, fmt_y=fmt_y), run_on("cpu"), fmt, fmt_y)
    c = ref.build("half_exact", 64, 64, fmt=fmt, fmt_y=fmt_y)
    want = ref.expected(c, 3, "full", False)[0]
    assert (want[:, :32] % 2 == 1).all()                                           # the first M / 2 queries: the true row is odd, behind its decoy


# ---- the older statement of the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (13, 9), (26, 9), (9, 26), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_match_loop_agrees_with_match_ref(shape):
    """tests/test_fpfh_host.py's loop and match_ref say the same on the family the loop was written for (every row is judged there)."""
    c = ref.build("small_integer", *shape)
    assert c["fx"].shape[2] == ref.SMALL_INTEGER_D and "D=5" in c["name"]
    for b, label, mutual in ref.variants_of(c):
        want, judged, xl, yl, _ = ref.expected(c, b, label, mutual)
        assert judged.all()
        loop = match_loop(c["fx"][:b], c["fy"][:b], ref.lengths_of(xl, b, shape[0]), ref.lengths_of(yl, b, shape[1]), mutual)
        assert np.array_equal(loop, want), (shape, b, label, mutual)


def test_the_reference_on_hand_made_rows():
    """match_ref itself, where the answer can be read off: ties, dead rows, the band."""
    fy = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [np.nan, 0.0], [5.0, 5.0]]])
    fx = np.array([[[0.1, 0.0], [0.9, 0.0], [np.inf, 0.0], [5.0, 5.0], [0.5, 0.0]]])
    want, judged = ref.match_ref(fx, fy, mutual=False)
    assert want.tolist() == [[0, 1, -1, 4, 0]] and judged.tolist() == [[True, True, True, True, False]]     # row 4 is equally far from rows 0 and 1
    want, judged = ref.match_ref(fx, fy, mutual=True)
    assert want.tolist() == [[0, 1, -1, 4, -1]] and judged.tolist() == [[True, True, True, True, False]]
    want, judged = ref.match_ref(fx, fy, [4], [1], mutual=False)
    assert want.tolist() == [[0, 0, -1, 0, -1]] and judged.all()
    assert (ref.match_ref(fx, fy, None, [0])[0] == -1).all() and (ref.match_ref(fx, fy[:, 3:4])[0] == -1).all()
    near = np.array([[[1.0, 0.0], [1.0 + 2.0 ** -20, 0.0]]])                       # d2 to (0, 0): a relative gap of 2^-19, above float32's band 20 * 2^-24
    assert ref.band(2, ref.EPS32) < 2.0 ** -19 and ref.match_ref(np.zeros((1, 1, 2)), near)[1].all()
    near[0, 1, 0] = 1.0 + 2.0 ** -23                                              # relative gap 2^-22: inside float32's band, outside float64's
    assert not ref.match_ref(np.zeros((1, 1, 2)), near)[1].any() and ref.match_ref(np.zeros((1, 1, 2)), near, eps=ref.EPS64)[1].all()


def check_overflow(dev):
    """float32: (3e38 - -3e38)^2 is +inf, the value a dead entry carries; the live row is matched all the same, and in float64 too."""
    import poseestimation_amd as pa
    fx, fy = np.array([[[3e38, 0.0]]]), np.array([[[np.nan, 0.0], [-3e38, 0.0], [-3e38, 0.0], [1.0, 1.0]]])
    for mutual in (True, False):
        want, judged = ref.match_ref(fx, fy, None, [3], mutual=mutual)
        assert want.tolist() == [[1]] and judged.all()
        for fmt in ("float32", "float64"):
            got = pa.match_features(tensor(fx, fmt, dev), tensor(fy, fmt, dev), y_lengths=torch.tensor([3], device=dev), mutual=mutual)
            assert got.tolist() == [[1]], (fmt, mutual)


def test_a_distance_that_overflows_still_beats_a_dead_row():
    check_overflow("cpu")


# ---- the sampler's rank map -----------------------------------------------------------------------------------------------------
class _TorchWithRand:
    """The torch module with rand replaced: what neighbors._ransac_samples sees as `torch`."""

    def __init__(self, u):
        self._u = u

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, shape, dtype=None, device=None, generator=None):
        assert tuple(shape) == tuple(self._u.shape) and dtype == torch.float32
        return self._u.to(device)


ONE_BELOW = 1.0 - 2.0 ** -24                                                      # the largest value torch.rand returns in float32


def chosen_u(c):
    """float32 values in [0, 1): the ends, the neighbours of k / c, values well inside a rank's interval ((k + 0.5) / c, a few seeded
    draws), and 1.0 itself (never drawn: it shows the clamp)."""
    ks = np.array([1, 2, 3, c // 3, c // 2, c - 2, c - 1], np.float64).clip(0, c)
    mid = (ks / c).astype(np.float32)
    u = np.concatenate([[0.0, 2.0 ** -149, 2.0 ** -24, 0.5, ONE_BELOW, 1.0 - 2.0 ** -23], mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1)),
                        (np.minimum(ks, c - 1) + 0.5) / c, np.random.default_rng(c).random(8)])
    u = np.clip(u.astype(np.float32), 0, np.float32(ONE_BELOW))
    u = np.concatenate([u, [np.float32(1.0)]])
    return np.concatenate([u, np.zeros(-len(u) % 3, np.float32)]).astype(np.float32)


def check_rank_map(monkeypatch, dev):
    """The sampler's rank for chosen u at chosen c, read back through the index it names.  The intended index is floor(u c) in real
    arithmetic; the sampler forms u c in float32, so where the real product lies within one float32 ulp of an integer the rank may be
    that integer's either side (asserted: the float32 product's floor, at most 1 off) and everywhere else it must be the exact floor."""
    from poseestimation_amd import neighbors
    for c in (3, 4, 50, 257, 2 ** 20 - 1, 2 ** 20):
        u = chosen_u(c)
        for stride in (1, 2) if c <= 257 else (1,):                               # stride 2: every other row is valid, rank r is index 2 r
            valid = torch.zeros(2, c * stride, dtype=torch.bool, device=dev)
            valid[0, ::stride] = True
            valid[1, :2 * stride:stride] = True                                   # the second cloud has 2 valid pairs: -1 throughout
            monkeypatch.setattr(neighbors, "torch", _TorchWithRand(torch.from_numpy(np.stack([u, u]))))
            got = neighbors._ransac_samples(valid, len(u) // 3, None)
            monkeypatch.undo()
            assert got.dtype == torch.int32 and got.shape == (2, len(u) // 3, 3)
            got = got.cpu().numpy().reshape(2, -1).astype(np.int64)
            rank = np.minimum(np.floor(u * np.float32(c)).astype(np.int64), c - 1)  # the float32 product, as the sampler forms it
            real = u.astype(np.float64) * c                                         # exact: 24 x 21 bits
            exact = np.minimum(np.floor(real).astype(np.int64), c - 1)
            clear = np.abs(real - np.round(real)) > np.spacing(real.astype(np.float32)).astype(np.float64)
            assert clear.sum() >= 6 and np.array_equal(got[0][clear], exact[clear] * stride), c
            assert (got[1] == -1).all() and np.array_equal(got[0], rank * stride), c
            assert ((rank >= 0) & (rank < c)).all() and (np.abs(rank - exact) <= 1).all() and rank[u == 0].max() == 0
            assert rank[u == np.float32(ONE_BELOW)].min() == c - 1 and rank[-3:].max() == c - 1     # u = 1 would name c: the clamp holds it


def test_rank_map_with_chosen_u(monkeypatch):
    check_rank_map(monkeypatch, "cpu")
