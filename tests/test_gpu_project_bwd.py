"""The backward of the SVD -> SO(3) projection on the GPU (K2: so3_project_bwd_f32 / _bf16 / _f64; K3: the fused dM of
so3_frob_fwd_bwd_v2_f32) through the raw C ABI, on every way its rows are sent -- the tile kernel alone (B < 64), K2's persistent engine
with and without a remainder, one pass of its whole grid -1, +0, +1, +64, three passes + 5 -- with every row judged against float64.

The input is tests/project_bwd_ref.py's families tiled with a prime period coprime to a pass; the float64 answers are GATHERED with the
same index, never recomputed.  Every judged row must meet J <= 4 x what the host model of the same templates reaches on its family,
every finite row K <= 4 x (tests/test_project_bwd_host.py: MEASURED; the figures J and K are defined in project_bwd_ref).  No quantile.
A row computed from another round's M or G is another family's row: it misses J by orders of magnitude.

WHAT THESE TESTS CATCH.  Each mutation below was applied alone to a copy of the sources; the host model was rebuilt and judged
(mutations 1-3, which live in so3_device.h), and the library was rebuilt and this file run once on an MI355X (all six).  Worst figure
against its bound (4 x the shipped host model's figure); "rows" counts the rows of the largest call that missed.

  mutation                                          what failed                                  worst figure against its bound
  1 backward_from_rotation: s01 from one triangle   (a) at every size >= pass - 1, the tile-     s=(1,e,-eU) e=1e-3  231.6 / 28.16 (K3: 301.1)
    (a third of round 2's defect)                   kernel route, (e) odd offset, (g) all sizes  s=(1,10^U(-4,0),0)  372.3 / 36.80 on the host
                                                    8 292 rows of 786 437                        s=(1,e,e) e=1e-4    300.5 /  6.36 on the host,
                                                                                                 e=1e-3 43.5 / 17.12, graded 15.9 / 12.96,
                                                                                                 bf16 small-gap rows 163.4 / 27.40
                                                    Gaussian and every scaled Gaussian pass, as the issue measured.  s=(1,e,-eU) e=1e-2 reaches
                                                    its bound only in K3 (37.2 / 34.32); in K2 its 2 048 rows stay below 34.32 (the issue's
                                                    108.6 was the worst of 50 000).  Sizes 1 .. 65 hold too few small-gap rows to see it.
  2 backward_given_rotation: the prescale branch's  (a) from 63 rows on, the tile-kernel route,  gaussian x 1e18  6.2e25 / 19.76, x 1e5 8.6e12 / 19.00,
    final dm *= factor dropped                      (f), (g) all sizes; 194 320 rows of 786 437  x 1e-5 2.1e7 / 22.92, x 1e-18 2.5e7 / 24.32;
                                                                                                 (f): all 2 048 rows of k = -40 differ in bits
  3 Consts<float>::bwd_rel 1e-12 -> 1e-3            (a) from 63 rows on, the tile-kernel route,  s=(1,e,-eU) e=1e-4 1447.5 / 1.56, e=1e-3 3790.6 / 28.16,
                                                    (e) odd offset, (g); 62 293 rows             s=(1,e,e) e=1e-4 2970.1 / 6.36, s=(1,10^U,0) 3517.3 / 36.80,
                                                                                                 bf16 small-gap rows 3008.7 / 27.40
                                                    The near-reflections pass: their hard rows have s1 + s3' and s2 + s3' >= 1e-3 s1, at or above
                                                    the mutated floor.  The hard rows WITH a real gap below it are the e = 1e-4 families.
  4 OpProjectBwd::compute parks G's words before    (a) from 64 rows on (63: no engine, passes): s=(1,10^U(-4,0),0) 4.2e7 / 36.80, near-reflection
    late_in1 has read them                          J, and non-finite rows from pass - 1 on;     e=1e-2 1.1e5 / 333.48; (b) the bits; (c) 57 564 rows;
                                                    (c), (e) every case, (i)                     (e) 38 642 rows; (i) 19 263 rows
  5 the engine's loads of round k >= 1 issued for   (a) at pass + 64 and 3 passes + 5 ONLY;      bf16 gaussian 1.4e10 / 32.72, gaussian 3.6e6 / 22.04:
    round k - 1                                     (c); (e) pass + 64 against the tile route;   61 of the 64 rows of the second round (the other
                                                    (g) at pass + 81                             three are unjudged families); (c) 1 048 768 rows
  6 overwrite_row<2, 9>: a parked row's bfloat16    (e) every case: 38 452 rows of 262 208,      (bits)
    store truncates instead of rounding             115 313 of 786 437; the odd-offset call
                                                    against the aligned one: 65 rows
No mutation went uncaught."""
import math
import re

import numpy as np
import pytest
import torch

import conftest
import project_bwd_ref as ref
from test_gpu_float64_metrics import _p, _st
from test_project_bwd_host import DEVICE_FACTOR, J32, J32_BF16_SMALL_GAP, J64, K32, K64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -777.0
ROWS_PER_CU = 1024                          # K2: CUs x 4 SIMDs x 2 waves x 2 units x 64 rows (launch_rows<2, SO3_WPS_K2, 256>)
SIZE_IDS = ["1", "63", "64", "65", "pass-1", "pass", "pass+1", "pass+64", "3pass+5"]
WINDOW_K = (-40, -15, -14, 16, 17, 40)
ENTRY = {"f32": ("so3_project_bwd_f32", torch.float32), "bf16": ("so3_project_bwd_bf16", torch.bfloat16), "f64": ("so3_project_bwd_f64", torch.float64)}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def rr():
    from poseestimation_amd import rotation_representation
    return rotation_representation


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def launch(lib, m, g, kind="f32"):
    """One call of K2 into a sentinel-filled output with one guard row behind it; the guard intact."""
    name, dtype = ENTRY[kind]
    b = m.shape[0]
    assert m.dtype == dtype and g.dtype == (torch.float64 if kind == "f64" else torch.float32)
    out = torch.full((b + 1, 9), SENTINEL, dtype=dtype, device=DEV)
    code = getattr(lib, name)(_p(m), _p(g), _p(out), b, _st())
    assert code == 0, (name, code, lib.so3_last_error())
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all(), name
    return out[:b]


def forward(lib, m):
    """The same kernel family's forward rotation of the rows (K1), for the structural judge K."""
    b = m.shape[0]
    out = torch.full((b + 1, 9), SENTINEL, dtype=torch.float64 if m.dtype == torch.float64 else torch.float32, device=DEV)
    name = {torch.float32: "so3_project_fwd_f32", torch.bfloat16: "so3_project_fwd_bf16", torch.float64: "so3_project_fwd_f64"}[m.dtype]
    assert getattr(lib, name)(_p(m), _p(out), None, b, _st()) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all(), name
    return out[:b]


def in_small_calls(lib, m, g, kind="f32"):
    """The rows through the one-row-per-thread tile kernel alone: calls of at most 63 rows (no unit for the engine)."""
    name, dtype = ENTRY[kind]
    b = m.shape[0]
    out = torch.full((b + 1, 9), SENTINEL, dtype=dtype, device=DEV)
    fn, st = getattr(lib, name), _st()
    assert m.is_contiguous() and g.is_contiguous()
    pm, pg, po, em, eg = _p(m), _p(g), _p(out), 9 * m.element_size(), 9 * g.element_size()
    for lo in range(0, b, 63):
        assert fn(pm + lo * em, pg + lo * eg, po + lo * em, min(63, b - lo), st) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (out[b] == SENTINEL).all()
    return out[:b]


def same_bits(a, b):
    """Bit for bit, a NaN equal to a NaN: the rows that differ."""
    a, b = a.float() if a.dtype == torch.bfloat16 else a, b.float() if b.dtype == torch.bfloat16 else b
    return torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b))).all(dim=1)).flatten()


_PASS = []


def _pass(lib):
    """Rows in one pass of the grid K2 launches: a 64-row call goes to the engine alone, and NPL, WPS and the block size are read from
    the instantiation's name, so3::k_rows<so3::OpProjectBwd<4>, NPL, WPS, BLOCK, false> (launch_rows caps the grid at CUs x 4 x WPS /
    waves workgroups of `waves` persistent waves, each taking NPL units of 64 rows per round)."""
    if not _PASS:
        d = ref.data()
        launch(lib, _dev(d["m"][:64]), _dev(d["g"][:64]))
        name = lib.so3_last_kernel().decode()
        m = re.fullmatch(r"so3::k_rows<so3::OpProjectBwd<4>, (\d+), (\d+), (\d+), false>", name)
        assert m, name
        npl, wps, block = (int(v) for v in m.groups())
        waves = block // 64
        workgroups = torch.cuda.get_device_properties(0).multi_processor_count * 4 * wps // waves
        _PASS.append(workgroups * waves * npl * 64)
    return _PASS[0]


def _sizes(lib):
    p = _pass(lib)
    return [1, 63, 64, 65, p - 1, p, p + 1, p + 64, 3 * p + 5]


_TILED = {}


def tiled(lib):
    """The fixture tiled to 3 passes + 5 rows, on the device, with the index it was gathered by (built once)."""
    if not _TILED:
        d = ref.data()
        n_fix = len(d["m"])
        period = ref.tile_period(n_fix)
        assert math.gcd(period, _pass(lib)) == 1, (period, _pass(lib))     # rows whole passes apart: never the same fixture row
        idx = ref.tile_index(max(_sizes(lib)), n_fix)
        gi = torch.as_tensor(idx, device=DEV)
        _TILED.update(idx=idx, gi=gi, period=period, m=_dev(d["m"])[gi], g=_dev(d["g"])[gi], t=_dev(d["t"])[gi])
    return _TILED


_ROUTE = {}


def fixture_through_the_tile_kernel(lib, kind="f32"):
    """The fixture itself, one period, through the tile kernel in calls of at most 63 rows: the reference route (bits) of every other."""
    if kind not in _ROUTE:
        d = ref.data()
        m, g = _dev(d["m"]), _dev(d["g"])
        if kind == "bf16":
            m = m.bfloat16()
        _ROUTE[kind] = in_small_calls(lib, m, g, kind)
    return _ROUTE[kind]


_DEVICE_J, _DEVICE_K = {}, {}


def _worst(bad, fig, lim, idx):
    """For a failure's message: per family that missed, its worst row, figure and bound."""
    d = ref.data()
    out = {}
    for row, f, b in zip(bad, fig, lim):
        name = d["names"][d["fam"][idx[row]]]
        if name not in out or f / b > out[name][1] / out[name][2]:
            out[name] = (int(row), float(f), float(b))
    return out


def judge(lib, got, m, idx, jrec=J32, krec=K32, u=ref.U32, label="", record=True):
    """Every judged row under J, every finite row under K, unjudged rows finite, NaN / Inf rows NaN: asserts, and returns the worst."""
    d = ref.data()
    host = got.double().cpu().numpy()
    assert not (host == SENTINEL).all(1).any(), label                       # a row left unwritten
    fin = d["finite"][idx]
    assert np.isfinite(host[fin]).all(), (label, np.flatnonzero(~np.isfinite(host).all(1) & fin)[:8])
    assert np.isnan(host[~fin]).all(), label                                # a NaN or Inf row gives a NaN row
    jf = ref.j_figure(host, idx, u=u)
    kf = ref.k_figure(host, forward(lib, m).double().cpu().numpy(), u=u)
    jm, kmx = ref.per_family(jf, idx), ref.per_family(kf, idx)
    if record:
        for store, figs in ((_DEVICE_J, jm), (_DEVICE_K, kmx)):
            for name, v in figs.items():
                store[(label.split()[0], name)] = max(v, store.get((label.split()[0], name), 0.0))
    worst = max(jm, key=lambda k: jm[k] / jrec[k]) if jm else None
    if worst is not None:
        print("%s B = %d: worst J %.2f of bound %.2f (host %.2f) in family %s; worst K %.2f" %
              (label, len(idx), jm[worst], DEVICE_FACTOR * jrec[worst], jrec[worst], worst, max(kmx.values()) if kmx else 0.0))
    bad, fig, lim = ref.over_bound(jf, jrec, idx, DEVICE_FACTOR)
    assert len(bad) == 0, (label, "J", len(bad), _worst(bad, fig, lim, idx))
    bad, fig, lim = ref.over_bound(kf, krec, idx, DEVICE_FACTOR)
    assert len(bad) == 0, (label, "K", len(bad), _worst(bad, fig, lim, idx))
    return jm, kmx


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The device's J and K per family (the largest over every size of test (a) and over the float64 calls) go to the run's record."""
    yield
    d = ref.data()
    for kind, jrec, krec in (("K2-f32", J32, K32), ("K2-f64", J64, K64), ("K3-f32", J32, K32)):
        for name in d["names"]:
            if (kind, name) in _DEVICE_K or (kind, name) in _DEVICE_J:
                j = _DEVICE_J.get((kind, name))
                line = "project_bwd %s %-26s device J %s (host %s, bound %s)  K %s (host %.2f, bound %.2f)" % (
                    kind, name, "%7.2f" % j if j is not None else "      -", "%.2f" % jrec[name] if name in jrec else "-",
                    "%.2f" % (DEVICE_FACTOR * jrec[name]) if name in jrec else "-",
                    "%6.2f" % _DEVICE_K[(kind, name)] if (kind, name) in _DEVICE_K else "     -", krec[name], DEVICE_FACTOR * krec[name])
                conftest.REPORT_LINES.append(line)


# ---- the pass --------------------------------------------------------------------------------------------------------------------
def test_a_pass_is_what_the_library_launches(lib):
    """`pass` comes from the launched instantiation's NPL, WPS and BLOCK; the table says CUs x 1024.  If K2's launch template changes,
    this test says so while the size tests go on straddling the real pass."""
    assert _pass(lib) == torch.cuda.get_device_properties(0).multi_processor_count * ROWS_PER_CU


# ---- a, b: every route, every row; bit for bit across routes ------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(SIZE_IDS)), ids=SIZE_IDS)
def test_k2_f32_every_row_within_its_bound_on_every_route(lib, which):
    b = _sizes(lib)[which]
    t = tiled(lib)
    got = launch(lib, t["m"][:b], t["g"][:b])
    judge(lib, got, t["m"][:b], t["idx"][:b], label="K2-f32 %s" % SIZE_IDS[which])
    # (b) the same bits as the fixture row it was tiled from gives in the tile kernel alone, whichever round, wave, slot or park-list
    # entry computed it: the stride puts hard families into every wave
    want = fixture_through_the_tile_kernel(lib)[t["gi"][:b]]
    differ = same_bits(got, want)
    d = ref.data()
    assert differ.numel() == 0, (b, differ.numel(), differ[:8].tolist(), [d["names"][f] for f in d["fam"][t["idx"][differ[:8].cpu().numpy()]]])


def test_the_fixture_through_the_tile_kernel_alone(lib):
    """Every fixture row through the one-row-per-thread kernel, 63 at a time: J and K there too (the sizes above send only the last
    B mod 64 rows that way)."""
    d = ref.data()
    got = fixture_through_the_tile_kernel(lib)
    judge(lib, got, _dev(d["m"]), np.arange(len(d["m"])), label="K2-f32 tile-kernel")


# ---- c: hard rows over a wave's rounds -------------------------------------------------------------------------------------------
def test_hard_rows_over_the_rounds_of_a_wave(lib):
    """K2 parks the hard rows of a round that holds few of them (M, G and the row number: 18 + 1 words in the workgroup's LDS list) and
    redoes them behind the loop; a round it has no room for, or a dense one, takes the Jacobi frames on the spot.  What a wave does
    depends on what it met before.  Five passes of the grid, each of its own kind -- sparse, crowded, all near-reflections, all ties,
    mixed -- then an odd tail of units and a remainder; G distinct in every row, so a parked G of the wrong round or slot cannot
    coincide.  Every row bit for bit against the tile kernel alone."""
    d = ref.data()
    p = _pass(lib)
    plan = ("sparse", "crowded", "reflection", "ties", "mixed")
    n = p * len(plan) + 64 * 3 + 11
    rng = np.random.default_rng(5)
    fam = lambda *names: np.flatnonzero(np.isin(d["fam"], [d["names"].index(k) for k in names]))
    gauss = fam("gaussian", "bf16 gaussian", "gaussian x 1e5")
    hard = {"reflection": fam("near-reflection e=1e-02", "near-reflection e=1e-03"), "ties": fam("generic ties"),
            "any": fam("near-reflection e=1e-03", "exact reflections", "generic ties", "rank one", "all zero", "s=(1,e,-eU) e=1e-04")}
    rows = gauss[rng.integers(0, len(gauss), n)]
    for k, kind in enumerate(plan + ("mixed",)):
        lo, hi = k * p, min((k + 1) * p, n)
        if kind in ("reflection", "ties"):
            rows[lo:hi] = hard[kind][rng.integers(0, len(hard[kind]), hi - lo)]
        else:
            pick = lo + np.flatnonzero(rng.random(hi - lo) < {"sparse": 0.05, "crowded": 0.22, "mixed": 0.5}[kind])
            rows[pick] = hard["any"][rng.integers(0, len(hard["any"]), len(pick))]
    m = _dev(d["m"])[torch.as_tensor(rows, device=DEV)]
    g = torch.randn(n, 9, device=DEV, generator=torch.Generator(device=DEV).manual_seed(17))
    # the passes are what they are meant to be: K1's diagnostic entry says which rows the fast path hands to the Jacobi path
    r_, is_hard = torch.empty(n, 9, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    assert lib.so3_project_fwd_diag_f32(_p(m), _p(r_), _p(is_hard), n, _st()) == 0
    share = [is_hard[k * p:(k + 1) * p].float().mean().item() for k in range(len(plan))]
    print("share of hard rows per pass:", dict(zip(plan, share)))
    # (an all-zero row is answered by K1's forward itself: hard for K2 alone, so the diagnostic sees 11/12 of the picks -- the zero
    #  family is 512 of the 6 144 rows they are drawn from)
    assert 0.04 < share[0] < 0.05 and 0.18 < share[1] < 0.22 and share[2] == 1.0 and share[3] == 1.0 and 0.42 < share[4] < 0.5, share
    got = launch(lib, m, g)
    want = in_small_calls(lib, m, g)
    differ = same_bits(got, want)
    assert differ.numel() == 0, (differ.numel(), differ[:8].tolist(), [k // p for k in differ[:8].tolist()])
    assert torch.isfinite(got).all()


# ---- d: alignment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["3units+11", "pass+64"])
def test_four_byte_but_not_sixteen_byte_aligned(lib, size):
    """M, G and dM one element into their buffers: 4-byte alignment only.  Still the engine for the whole units, and the tile kernel's
    VEC = false on the remainder.  The same bits, and nothing written outside dM."""
    b = 64 * 3 + 11 if size == "3units+11" else _pass(lib) + 64
    t = tiled(lib)
    want = launch(lib, t["m"][:b], t["g"][:b])

    def shifted(v, fill=None):
        base = torch.full((b * 9 + 1 + 9,), SENTINEL, dtype=torch.float32, device=DEV)
        view = base[1:1 + b * 9].view(b, 9)
        if v is not None:
            view.copy_(v)
        assert view.data_ptr() % 16 == 4
        return base, view

    (_, ms), (_, gs), (obase, out) = shifted(t["m"][:b]), shifted(t["g"][:b]), shifted(None)
    assert lib.so3_project_bwd_f32(_p(ms), _p(gs), _p(out), b, _st()) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert obase[0].item() == SENTINEL and (obase[1 + b * 9:] == SENTINEL).all()
    assert same_bits(out, want).numel() == 0
    # one shifted at a time: each operand's alignment is tested by the launcher on its own
    for which in range(3):
        args = [t["m"][:b], t["g"][:b], torch.full((b + 1, 9), SENTINEL, device=DEV)]
        guard = None
        if which == 2:
            guard, args[2] = shifted(None)
        else:
            args[which] = shifted(args[which])[1]
        assert lib.so3_project_bwd_f32(_p(args[0]), _p(args[1]), _p(args[2]), b, _st()) == 0, lib.so3_last_error()
        torch.cuda.synchronize()
        assert same_bits(args[2][:b], want).numel() == 0, which
        if guard is not None:
            assert guard[0].item() == SENTINEL and (guard[1 + b * 9:] == SENTINEL).all()
        else:
            assert (args[2][b] == SENTINEL).all()


# ---- e: bfloat16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 2])
@pytest.mark.parametrize("size", ["pass+64", "3pass+5"])
def test_bf16_is_the_float32_result_rounded_to_nearest_even(lib, size, off):
    """so3_project_bwd_bf16 on even element offsets (dword aligned: the engine, its bfloat16 stores and OpProjectBwd<2>'s park list over
    several rounds): dM equals torch's round-to-nearest-even of the float32 call's dM on the bfloat16-rounded input, bit for bit."""
    b = _pass(lib) + 64 if size == "pass+64" else 3 * _pass(lib) + 5
    t = tiled(lib)
    base = torch.full((b * 9 + off + 9,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    mb = base[off:off + b * 9].view(b, 9)
    mb.copy_(t["m"][:b])
    obase = torch.full((b * 9 + off + 9,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = obase[off:off + b * 9].view(b, 9)
    assert mb.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    assert lib.so3_project_bwd_bf16(_p(mb), _p(t["g"][:b]), _p(out), b, _st()) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (obase[:off] == SENTINEL).all() and (obase[off + b * 9:] == SENTINEL).all()
    want = launch(lib, mb.float(), t["g"][:b]).to(torch.bfloat16)             # torch: round to nearest even
    differ = same_bits(out, want)
    assert differ.numel() == 0, (b, off, differ.numel(), differ[:8].tolist())
    # and the tile kernel alone gives those bits too
    if size == "pass+64" and off == 0:
        route = fixture_through_the_tile_kernel(lib, "bf16")[t["gi"][:b]]
        assert same_bits(out, route).numel() == 0


def test_bf16_at_an_odd_offset_on_the_small_gap_rows(lib):
    """A bfloat16 view at an odd element offset is not dword aligned: the tile kernels alone, 1 025 rows (more than one workgroup).  The
    small-gap rows rounded to bfloat16, against float64 on exactly those numbers: J, with one bfloat16 ulp of the answer allowed for the
    store (2^-8 |dM64|, the spacing of bfloat16 at the answer's size), within 4 x the host model's figure on these rows."""
    s = ref.bf16_small_gap()
    b = len(s["m"])
    base = torch.full((b * 9 + 1 + 9,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    mb = base[1:1 + b * 9].view(b, 9)
    mb.copy_(_dev(s["m"]))
    assert torch.equal(mb.float(), _dev(s["m"])) and mb.data_ptr() % 4 == 2
    obase = torch.full((b * 9 + 1 + 9,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = obase[1:1 + b * 9].view(b, 9)
    assert lib.so3_project_bwd_bf16(_p(mb), _p(_dev(s["g"])), _p(out), b, _st()) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (obase[:1] == SENTINEL).all() and (obase[1 + b * 9:] == SENTINEL).all()      # (the sentinel as bfloat16 holds it)
    got = out.float().cpu().numpy()
    assert np.isfinite(got).all()
    fig = ref.j_of(got, s["ans"], extra=2.0**-8 * np.abs(s["ans"]["d64"]))
    print("bf16, odd offset, small-gap rows: worst J %.2f beyond one bfloat16 ulp (bound %.2f)" % (fig.max(), DEVICE_FACTOR * J32_BF16_SMALL_GAP))
    assert (fig <= DEVICE_FACTOR * J32_BF16_SMALL_GAP).all(), (fig.max(), int(np.argmax(fig)))
    # the same rows on the aligned route: the same bits
    aligned = launch(lib, _dev(s["m"]).bfloat16(), _dev(s["g"]), "bf16")
    assert same_bits(out, aligned).numel() == 0


# ---- f: the prescale window --------------------------------------------------------------------------------------------------------
def test_the_prescale_window_row_by_row(lib):
    """Gaussian rows times 2^k, interleaved row by row with the unscaled rows, so that `prescale.any` is true for waves whose rows differ:
    some inside the fast path's window |M|_F^2 in [2^-28, 2^34], some outside.  For unit-variance rows (|M|^2 = 1 .. 30) the edges
    run THROUGH k = -15 (|M|^2 >= 4 is inside: 91 % of the rows) and k = 16 (|M|^2 <= 4: 9 %); k = -14 is inside, k = 17 outside.
    dM(2^k M) 2^k == dM(M) bit for bit, and J on every row."""
    d = ref.data()
    rows = np.flatnonzero(d["fam"] == d["names"].index("gaussian"))
    m0, g0 = d["m"][rows], d["g"][rows]
    ks = (0,) + WINDOW_K
    m = np.stack([m0 * np.float32(2.0**k) for k in ks], 1).reshape(-1, 9)     # row 9 j + i: 2^ks[i] M_j
    g = np.repeat(g0, len(ks), 0)
    n2 = (m.astype(np.float64) ** 2).sum(1).reshape(-1, len(ks))
    inside = (n2 >= 2.0**-28) & (n2 <= 2.0**34)
    for i, k in enumerate(ks):                                                # the set straddles both edges, row by row
        assert inside[:, i].all() == (k in (0, -14)) and (not inside[:, i].any()) == (k in (-40, 17, 40)), (k, inside[:, i].mean())
    assert 0.05 < inside[:, ks.index(16)].mean() < 0.5 < inside[:, ks.index(-15)].mean() < 0.95
    md, gd = _dev(m), _dev(g)
    got = launch(lib, md, gd)
    assert torch.isfinite(got).all()
    per = got.view(len(rows), len(ks), 9)
    for i, k in enumerate(ks[1:], 1):
        differ = same_bits(per[:, i] * float(2.0**k), per[:, 0])
        assert differ.numel() == 0, (k, differ.numel(), differ[:8].tolist())
    idx = np.repeat(rows, len(ks))
    ans = {key: (np.repeat(d[key][rows], len(ks), 0) if key != "d64" else None) for key in ("d64", "s1", "gamma", "gnorm", "jrow")}
    scale = np.tile(np.array([2.0**k for k in ks]), len(rows))
    ans["d64"] = np.repeat(d["d64"][rows], len(ks), 0) / scale[:, None]       # dM(c M) = dM(M) / c: exact for a power of two
    ans["s1"], ans["gamma"] = ans["s1"] * scale, ans["gamma"] * scale
    fig = ref.j_of(got.double().cpu().numpy(), ans)
    print("prescale window: worst J %.2f (bound %.2f)" % (np.nanmax(fig), DEVICE_FACTOR * J32["gaussian"]))
    assert (fig[ans["jrow"]] <= DEVICE_FACTOR * J32["gaussian"]).all(), (np.nanmax(fig), idx[int(np.nanargmax(fig))])
    # the unscaled rows keep the bits they have in a call where no row is outside the window
    alone = launch(lib, _dev(m0), _dev(g0))
    assert same_bits(per[:, 0].contiguous(), alone).numel() == 0


# ---- g: K3's dM --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1024", "1025", "pass+81"])
def test_k3_dm_every_judged_row_on_the_families(lib, size):
    """so3_frob_fwd_bwd_v2_f32 on the tiled fixture against Haar targets: the one-workgroup kernel (1 024), the engine + remainder
    (1 025) and more than one pass of its grid.  dM against projection_backward_np(M, G64) with G64 = (R - T) / (B |R - T|) formed in
    float64 from the call's own R; |G|_F = 1 / B.  Every judged row under J; no sample, no quantile."""
    b = {"1024": 1024, "1025": 1025}.get(size) or _pass(lib) + 81
    t = tiled(lib)
    d = ref.data()
    idx = t["idx"][:b]
    r = torch.full((b + 1, 9), SENTINEL, device=DEV)
    dm = torch.full((b + 1, 9), SENTINEL, device=DEV)
    ls = torch.full((1,), 777.0, dtype=torch.float64, device=DEV)
    assert lib.so3_frob_fwd_bwd_v2_f32(_p(t["m"][:b]), _p(t["t"][:b]), _p(r), _p(dm), _p(ls), None, None, 0, b, _st()) == 0, lib.so3_last_error()
    torch.cuda.synchronize()
    assert (r[b] == SENTINEL).all() and (dm[b] == SENTINEL).all()
    fin = d["finite"][idx]
    rk, got = r[:b].double().cpu().numpy(), dm[:b].double().cpu().numpy()
    assert np.isfinite(got[fin]).all() and np.isnan(got[~fin]).all()
    diff = np.where(fin[:, None], rk - d["t"][idx].astype(np.float64), 1.0)
    g64 = diff / (b * np.linalg.norm(diff, axis=1, keepdims=True))
    with np.errstate(invalid="ignore"):
        d64 = ref.so.projection_backward_np(np.where(fin[:, None], d["m"][idx].astype(np.float64), 0.0), g64).reshape(b, 9)
    jf = ref.j_figure(got, idx, d64=d64, gnorm=np.full(b, 1.0 / b))
    jm = ref.per_family(jf, idx)
    for name, v in jm.items():
        _DEVICE_J[("K3-f32", name)] = max(v, _DEVICE_J.get(("K3-f32", name), 0.0))
    worst = max(jm, key=lambda k: jm[k] / J32[k])
    print("K3 B = %d: worst J %.2f of bound %.2f in family %s" % (b, jm[worst], DEVICE_FACTOR * J32[worst], worst))
    bad, fig, lim = ref.over_bound(jf, J32, idx, DEVICE_FACTOR)
    assert len(bad) == 0, (b, "J", len(bad), _worst(bad, fig, lim, idx))
    kf = ref.k_figure(got, rk)
    kmx = ref.per_family(kf, idx)
    for name, v in kmx.items():
        _DEVICE_K[("K3-f32", name)] = max(v, _DEVICE_K.get(("K3-f32", name), 0.0))
    bad, fig, lim = ref.over_bound(kf, K32, idx, DEVICE_FACTOR)
    assert len(bad) == 0, (b, "K", len(bad), _worst(bad, fig, lim, idx))


# ---- h: float64 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["fixture", "257"])
def test_f64_every_row_in_units_of_2_to_the_minus_53(lib, size):
    """so3_project_bwd_f64 on the fixture at its own length, and at B = 257 (one live lane in the last workgroup).  The figures are an
    agreement measure between two float64 computations; the bound is 4 x what the float64 host model reaches."""
    d = ref.data()
    n = len(d["m"])
    idx = np.arange(n) if size == "fixture" else ref.tile_index(257, n)
    m, g = _dev(d["m"][idx]).double(), _dev(d["g"][idx]).double()
    got = launch(lib, m, g, "f64")
    judge(lib, got, m, idx, jrec=J64, krec=K64, u=ref.U64, label="K2-f64 %s" % size)


# ---- i: the Python spelling --------------------------------------------------------------------------------------------------------
def test_the_python_spelling_gives_the_c_calls_bits(lib, rr):
    """symmetric_orthogonalization(x).backward(g) at 3 passes + 5 with g a non-contiguous view, and with the expanded gradient of
    .sum(): the bits of the C call on the contiguous G."""
    t = tiled(lib)
    b = 3 * _pass(lib) + 5
    wide = torch.empty(b, 3, 5, device=DEV)
    wide[:, :, 1:4] = t["g"][:b].view(b, 3, 3)
    g = wide[:, :, 1:4]
    assert not g.is_contiguous()
    x = t["m"][:b].clone().requires_grad_(True)
    rr.symmetric_orthogonalization(x).backward(g)
    assert same_bits(x.grad, launch(lib, t["m"][:b], t["g"][:b])).numel() == 0
    x = t["m"][:b].clone().requires_grad_(True)
    rr.symmetric_orthogonalization(x).sum().backward()
    assert same_bits(x.grad, launch(lib, t["m"][:b], torch.ones(b, 9, device=DEV))).numel() == 0
