"""What the tests of so3_angle_stats (angle_error_statistics) must know about the kernels, restated in numpy from include/so3proj.h and
the comments of csrc/so3proj.hip ("next row f3") -- never from the kernels' answers -- and the list of inputs that reach every
branch of the exact median by construction.  The reference for every statistic is oracle.so3_oracle.angle_statistics_np (numpy,
float64).  No GPU here: tests/test_angle_stats_host.py holds every case to what its name promises, tests/test_gpu_angle_stats.py
runs the list on the device.

The contract the cases rely on (include/so3proj.h): an empty class reports count 0 and NaN elsewhere; -0.0 counts as +0.0; a class
holding +inf has mean = max = +inf and std = NaN; a class holding a NaN reports NaN for mean / std / max / median; negative angles
are outside the contract; ids outside [0, ncls) are ignored."""
import numpy as np

# ---- constants of the kernels (csrc/so3proj.hip, "next row f3") -------------------------------------------------------------------
STAT_BLOCK = 1024            # threads per workgroup; a workgroup takes PAIRS of rows in blocks of 1024 pairs, dealt round-robin
STAT_REGION = 4096           # candidates one collecting workgroup can stage (more: bit 0 of StatWork::overflow)
STAT_LDS_KEYS = 16384        # candidates of one class the finishing workgroup keeps in LDS from the start
CAND_CAP = 1 << 20           # the candidate buffer
STAT_MAX_WGS = 1024
FINE_CLASSES = 4             # at most this many classes: bins of 1/64 octave (the top 18 bits), else 1/16 (the top 16)
LDS_CLASSES = 16             # at most this many classes: the small LDS histograms
SEL_CHUNK = 32               # the selection handles this many classes at a time
MAX_CLASSES = 64
FIELDS = ("count", "mean", "std", "max", "median", "acc30", "acc15", "acc7.5")
EXACT = ("count", "max", "median", "acc30", "acc15", "acc7.5")
U = 2.0 ** -53


# ---- restatements -----------------------------------------------------------------------------------------------------------------
def key(a):
    """The unsigned 64-bit pattern the kernels order angles by: non-negative doubles order like their bits; -0.0 (and whatever is
    below zero) counts as +0.0."""
    a = np.array(a, np.float64, ndmin=1)
    return np.where(a <= 0, 0.0, a).view(np.uint64)


def is_fine(ncls):
    return ncls <= FINE_CLASSES


def n_bins(fine):
    """Bins of the window's histogram: one below 2^-23, 16 (fine: 64) per octave up to 2^9 degrees, one above (and +inf)."""
    return (2048 if fine else 512) + 2


def window_bin(a, fine):
    shift = 46 if fine else 48
    base = 0x3E80 << 2 if fine else 0x3E80                  # (bits >> shift) of 2^-23
    inner = n_bins(fine) - 2
    top = (key(a) >> np.uint64(shift)).astype(np.int64)
    return np.where(top < base, 0, np.where(top >= base + inner, inner + 1, top - base + 1))


def grid(B, cus):
    """Workgroups of both launches: one per 1024 pairs of rows, at most one per compute unit (and 1024), at least one."""
    want = (B // 2 + STAT_BLOCK - 1) // STAT_BLOCK
    return int(max(1, min(want, cus, STAT_MAX_WGS)))


def workgroup_of_rows(B, cus, mode=0):
    """Which workgroup reads row r: pairs (head + 2i, head + 2i + 1) in blocks of 1024 dealt round-robin; a peeled first row (mode 1:
    head = 1) and an odd last row go to workgroup 0."""
    head = 1 if mode == 1 else 0
    g = grid(B, cus)
    r = np.arange(B, dtype=np.int64)
    pairs = max(B - head, 0) // 2
    i = (r - head) // 2
    wg = (i // STAT_BLOCK) % g
    wg[(r < head) | (i >= pairs)] = 0
    return wg


def selected_bins(ang, cls, ncls):
    """Per class the window bins of the lower and the upper middle element, (-1, -1) for a class without a non-NaN row."""
    ang = np.asarray(ang, np.float64)
    c = np.zeros(len(ang), np.int64) if cls is None else np.asarray(cls, np.int64)
    fine = is_fine(ncls)
    out = np.full((ncls, 2), -1, np.int64)
    for k in range(ncls):
        x = ang[c == k]
        ks = np.sort(key(x[~np.isnan(x)]))
        if len(ks):
            mid = ks[[(len(ks) - 1) // 2, len(ks) // 2]].view(np.float64)
            out[k] = window_bin(mid, fine)
    return out


def staged_mask(ang, cls, ncls):
    """The rows k_stats_collect stages: not NaN, of a class in [0, ncls), inside one of their class's two selected bins."""
    ang = np.asarray(ang, np.float64)
    c = np.zeros(len(ang), np.int64) if cls is None else np.asarray(cls, np.int64)
    sel = selected_bins(ang, cls, ncls)
    ok = (c >= 0) & (c < ncls) & ~np.isnan(ang)
    cc = np.where(ok, c, 0)
    b = window_bin(ang, is_fine(ncls))
    return ok & ((b == sel[cc, 0]) | (b == sel[cc, 1]))


def candidate_totals(ang, cls, ncls):
    c = np.zeros(len(ang), np.int64) if cls is None else np.asarray(cls, np.int64)
    m = staged_mask(ang, cls, ncls)
    return np.bincount(c[m], minlength=ncls)[:ncls]


def rows_staged_per_workgroup(B, cus, mode=0, staged=None):
    """How many rows each workgroup of k_stats_collect stages: of all its rows (staged=None: what it stages when every row is a
    candidate), or of those in the mask."""
    wg = workgroup_of_rows(B, cus, mode)
    if staged is not None:
        wg = wg[np.asarray(staged, bool)]
    return np.bincount(wg, minlength=grid(B, cus))


def depth(B, cus):
    """A generous count of the float64 additions one row's value passes on its way into a class's sum: the LDS slot it is added to
    (a workgroup's rows over at least 8 slots), the slots (at most 32), the workgroups' atomics into a replica (at most the
    grid), the replicas (at most 16)."""
    g = grid(B, cus)
    return -(-max(B, 1) // g) // 8 + 1 + 32 + g + 16


STD_C = 0.13         # see std_bound


def std_bound(x, B, cus):
    """Bound on |std_got^2 - var_ref| for the kernels' one-pass formula S2/m - (S1/m)^2 on the non-negative rows x of one class,
    c D u (mean(x^2) + mean(x)^2) with D = depth(B, cus) and u = 2^-53.  Its form: S1 carries a relative error of at most D u, S2 of
    (D + 1) u (the products' rounding), so (S1/m)^2 is off by (2D + 3) u mean(x)^2 and S2/m by (D + 2) u mean(x^2), and the
    subtraction adds u |var| <= u mean(x^2) -- never more than c = 2 and a little, every rounding against the result.  Roundings do
    not conspire: a numpy model of the formula that sums as deep as D counts, every level in sequence, in shuffled orders
    (tests/test_angle_stats_host.py) needs c = 0.032 at the most over every case of the list, and c = STD_C is four times that."""
    x = np.asarray(x, np.float64)
    return STD_C * depth(B, cus) * U * (np.mean(x * x) + np.mean(x) ** 2)


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def _half_normal(rng, n):
    return np.minimum(np.abs(rng.standard_normal(n)) * 25.0, 180.0)


def _sizes(n, ncls):
    return [n // ncls + (1 if k < n % ncls else 0) for k in range(ncls)]


def _assemble(rng, per_class, ncls=None, to_class=None):
    """Rows of per_class[j] get id to_class[j] (default j), shuffled together."""
    ncls = len(per_class) if ncls is None else ncls
    to_class = list(range(len(per_class))) if to_class is None else to_class
    ang = np.concatenate([np.asarray(x, np.float64) for x in per_class]) if per_class else np.zeros(0)
    cls = np.concatenate([np.full(len(x), k, np.int32) for x, k in zip(per_class, to_class)]) if per_class else np.zeros(0, np.int32)
    p = rng.permutation(len(ang))
    return ang[p], cls[p].astype(np.int32), ncls


def _case(name, ang, cls, ncls, **props):
    d = dict(name=name, ang=np.ascontiguousarray(ang, np.float64), cls=None if cls is None else np.ascontiguousarray(cls, np.int32), ncls=int(ncls))
    d.update(props)
    return d


def _mix(rng, m, share, special):
    """m rows: ceil(share * m) of them from special(count), the rest half-normal and positive."""
    k = min(m, int(np.ceil(share * m)))
    rest = np.maximum(_half_normal(rng, m - k), 1e-3)
    return np.concatenate((special(k), rest))


def _edge_cases(rng):
    out = []
    tiny = lambda k: np.resize(np.array([0.0, 5e-324, 1e-310, 2.0 ** -1030, 2.0 ** -40, 2.0 ** -24, np.nextafter(2.0 ** -23, 0.0)]), k)
    above = lambda k: rng.uniform(512.0001, 20000.0, k)

    def above_inf(k):
        x = above(k)
        x[:max(1, k // 10)] = np.inf
        return x
    for ncls in (1, 3, 5, 17):
        for n in (3001, 70001):
            per = [_mix(rng, m, 0.6, np.zeros) for m in _sizes(n, ncls)]
            out.append(_case("edge zeros 60%% n=%d ncls=%d" % (n, ncls), *_assemble(rng, per), median_bins="low"))
        n = 3001
        per = [_mix(rng, m, 0.6, tiny) for m in _sizes(n, ncls)]
        out.append(_case("edge denormals 60%% ncls=%d" % ncls, *_assemble(rng, per), median_bins="low"))
        per = [np.concatenate((np.zeros(m // 2), np.full(m // 2, 5.0))) for m in _sizes(n, ncls)]
        out.append(_case("edge half zeros half 5.0 ncls=%d" % ncls, *_assemble(rng, per), median_bins="low+inner"))
        per = [_mix(rng, m, 0.6, above) for m in _sizes(n, ncls)]
        out.append(_case("edge above 512 ncls=%d" % ncls, *_assemble(rng, per), median_bins="high"))
        per = [_mix(rng, m, 0.6, above_inf) for m in _sizes(n, ncls)]
        out.append(_case("edge above 512 with +inf ncls=%d" % ncls, *_assemble(rng, per), median_bins="high", has_inf=True))
        k = ncls // 2
        out.append(_case("edge [0, 180] n=2 ncls=%d" % ncls, [0.0, 180.0], [k, k], ncls, median_bins="low+inner",
                         empty=[c for c in range(ncls) if c != k]))
        for share, word in ((0.1, "minority"), (0.6, "majority")):
            per = [_mix(rng, m, share, lambda q: np.full(q, -0.0)) for m in _sizes(n, ncls)]
            out.append(_case("edge -0.0 %s ncls=%d" % (word, ncls), *_assemble(rng, per), median_bins="low" if share > 0.5 else "inner",
                             neg_zero=True))
    return out


_SPLIT_EDGES = (20.0, 7.5, 15.0, 30.0, 40.0, 60.0, 3.75, 1.875, 120.0, 10.0)        # few mantissa bits: bin edges at both widths


def _split_cases(rng):
    out = []
    for ncls in (3, 10):
        for kind in ("adjacent bins", "an octave apart", "same bin, last byte"):
            per, mids = [], []
            for k in range(ncls):
                e = _SPLIT_EDGES[k]
                if kind == "adjacent bins":
                    lo, hi = np.nextafter(e, 0.0), e
                elif kind == "an octave apart":
                    lo, hi = 0.45 * e, 2.0 * (0.45 * e)
                else:
                    bits = np.array([1.1 * e]).view(np.uint64)[0] & ~np.uint64(0xFF)
                    lo, hi = np.array([bits | np.uint64(0x10), bits | np.uint64(0x90)], np.uint64).view(np.float64)
                h = 50 + 7 * k
                per.append(np.concatenate((rng.uniform(0.0, 0.9 * lo, h - 1), [lo, hi], rng.uniform(1.1 * hi, 179.0, h - 1))))
                mids.append((float(lo), float(hi)))
            out.append(_case("split middles, %s, ncls=%d" % (kind, ncls), *_assemble(rng, per), middles=mids, split=kind))
    return out


def _threshold_class(rng, v, m=301):
    return _mix(rng, m, 0.6, lambda k: np.full(k, v))


def _threshold_cases(rng):
    out = []
    per, vals = [], []
    for t in (7.5, 15.0, 30.0):
        for v in (np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)):
            per.append(_threshold_class(rng, v))
            vals.append(float(v))
    per.append(np.full(200, 30.0))
    vals.append(30.0)
    out.append(_case("thresholds, coarse window, ncls=10", *_assemble(rng, per), majority=vals, only30=9))
    for t in (7.5, 15.0, 30.0):
        vs = [float(np.nextafter(t, 0.0)), t, float(np.nextafter(t, np.inf)), 30.0]
        per = [_threshold_class(rng, v) for v in vs[:3]] + [np.full(200, 30.0)]
        out.append(_case("thresholds at %g, fine window, ncls=4" % t, *_assemble(rng, per), majority=vs, only30=3))
    return out


def _shape_cases(rng):
    out = []
    for ncls in (1, 4, 5, 16, 17, 32, 33, 64):
        per = [_half_normal(rng, m) for m in _sizes(2000 + 3 * ncls + 1, ncls)]
        for x in per:
            x[::17] = 0.0
        out.append(_case("class shape ncls=%d" % ncls, *_assemble(rng, per), empty=[]))
    for ncls in (3, 4, 5, 33):
        per = [_half_normal(rng, 150 + k) for k in range(ncls - 2)]
        out.append(_case("first and last class empty ncls=%d" % ncls, *_assemble(rng, per, ncls, list(range(1, ncls - 1))), empty=[0, ncls - 1]))
    for ncls in (4, 5):
        n = 70000
        big = n * 99 // 100
        per = [_half_normal(rng, 1), _half_normal(rng, 2), _half_normal(rng, big)] + [_half_normal(rng, m) for m in _sizes(n - big - 3, ncls - 3)]
        out.append(_case("one row, two rows and 99%% of 70 000 ncls=%d" % ncls, *_assemble(rng, per), empty=[], counts=[1, 2, big]))
    for ncls in (3, 5):
        per = [_half_normal(rng, 300), np.full(40, np.nan), _half_normal(rng, 200)] + [_half_normal(rng, 50) for _ in range(ncls - 3)]
        out.append(_case("a class of NaNs ncls=%d" % ncls, *_assemble(rng, per), empty=[], nan_classes=[1]))
        per = [_half_normal(rng, 300), np.full(1, np.nan), _half_normal(rng, 200)] + [_half_normal(rng, 50) for _ in range(ncls - 3)]
        out.append(_case("a NaN in a one-row class ncls=%d" % ncls, *_assemble(rng, per), empty=[], nan_classes=[1]))
    for ncls in (1, 5, 17):
        ang, cls, _ = _assemble(rng, [_half_normal(rng, m) for m in _sizes(3000, ncls)])
        bad = np.array([-1, ncls, 2 ** 31 - 1, -2 ** 31], np.int64)
        at = rng.choice(len(ang), 400, replace=False)
        cls = cls.astype(np.int64)
        cls[at] = bad[np.arange(400) % 4]
        out.append(_case("ids outside [0, ncls) ncls=%d" % ncls, ang, cls.astype(np.int32), ncls, empty=[], ignored=400))
    for ncls in (1, 5):
        out.append(_case("B = 0 ncls=%d" % ncls, np.zeros(0), None if ncls == 1 else np.zeros(0, np.int32), ncls, empty=list(range(ncls))))
    return out


def _grid_cases(rng):
    out = []
    for n in (2, 1000, 4097, 4098, 10_000, 40_000):            # grids of 1, 1, 2, 3, 5 and 20 workgroups against 64 classes
        ang = _half_normal(rng, n)
        cls = rng.permutation(n).astype(np.int32) % 64          # every class as full as n allows
        out.append(_case("grid against 64 classes n=%d" % n, ang, cls, 64, empty=list(range(n, 64)) if n < 64 else []))
    return out


def _tie_cases(rng):
    out = []
    for n in (3000, 20_000):
        for ncls in (1, 5):
            per = []
            for k, m in enumerate(_sizes(n, ncls)):
                v = 17.3 + k
                third = m // 3
                per.append(np.concatenate((np.full(m - 2 * third, v), rng.uniform(0.0, 0.99 * v, third), rng.uniform(1.01 * v, 180.0, third))))
            ang, cls, _ = _assemble(rng, per)
            out.append(_case("ties at the median n=%d ncls=%d" % (n, ncls), ang, None if ncls == 1 else cls, ncls, tie_values=[17.3 + k for k in range(ncls)]))
    return out


def _lds_boundary_cases():
    """K rows inside the median's bin (20.0 opens a bin at both widths, 20.2 is inside it at both), spread evenly through 70 000."""
    out = []
    n = 70_000
    for ncls in (1, 5):
        for K in (STAT_LDS_KEYS, STAT_LDS_KEYS + 1):
            rng = np.random.default_rng(K + ncls)
            ang = np.empty(n)
            inside = np.zeros(n, bool)
            inside[np.arange(K) * n // K] = True
            ang[inside] = rng.uniform(20.0, 20.2, K)
            rest = n - K
            other = np.concatenate((rng.uniform(0.0, 19.0, rest // 2), rng.uniform(21.0, 180.0, rest - rest // 2)))
            ang[~inside] = rng.permutation(other)
            cls = None if ncls == 1 else np.full(n, 2, np.int32)
            out.append(_case("LDS boundary: %d rows in the median's bin ncls=%d" % (K, ncls), ang, cls, ncls, in_bin=K, the_class=0 if ncls == 1 else 2,
                             empty=[] if ncls == 1 else [0, 1, 3, 4]))
    return out


def _staging_cases(cus):
    out = []
    full = np.full
    out.append(_case("staging: 4096 x CUs equal rows", full(STAT_REGION * cus, 12.5), None, 1, staging=True, overflows=False, max_staged=STAT_REGION))
    out.append(_case("staging: 4096 x CUs + 2 equal rows", full(STAT_REGION * cus + 2, 12.5), None, 1, staging=True, overflows=True, max_staged=STAT_REGION + 2))
    n = 2 * STAT_REGION * cus + 3
    out.append(_case("staging: 8192 x CUs + 3 equal rows", full(n, 12.5), None, 1, staging=True, overflows=True, every_wg=True))
    ang = full(n, 12.5)
    ang[1 + 3 * 1000] = np.nan                                  # (a row of class 1)
    out.append(_case("staging: 8192 x CUs + 3 equal rows, three classes, a NaN", ang, (np.arange(n) % 3).astype(np.int32), 3, staging=True, overflows=True,
                     every_wg=True, nan_classes=[1]))
    return out


_CACHE = {}


def cases(cus):
    """The list (dicts with name, ang, cls, ncls and what the case promises).  Built once per `cus`; nobody writes into the arrays."""
    if cus not in _CACHE:
        rng = np.random.default_rng(20250)
        lst = (_edge_cases(rng) + _split_cases(rng) + _threshold_cases(rng) + _shape_cases(rng) + _grid_cases(rng) + _tie_cases(rng) +
               _lds_boundary_cases() + _staging_cases(cus))
        for d in lst:
            d["ang"].setflags(write=False)
            if d["cls"] is not None:
                d["cls"].setflags(write=False)
        assert len({d["name"] for d in lst}) == len(lst)
        _CACHE[cus] = lst
    return _CACHE[cus]


_REFS = {}


def reference(case):
    """oracle.so3_oracle.angle_statistics_np of a case, computed once (numpy warns about inf - inf and empty slices: expected here)."""
    from oracle import so3_oracle as so
    import warnings
    k = (id(case["ang"]), id(case["cls"]), case["ncls"])
    if k not in _REFS:
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _REFS[k] = (case["ang"], case["cls"], so.angle_statistics_np(case["ang"], case["cls"], case["ncls"]))      # (the arrays are held: their ids stay theirs)
    return _REFS[k][-1]


def check_against_reference(got, case, cus, label=""):
    """got: (ncls, 8) float64 array.  The exact fields bit for bit (NaN = NaN); mean within the project's 1e-10 where the class is
    finite and within [0, 180], numpy's inf / nan elsewhere; std by std_bound (on the variance), numpy's nan where it gives one.
    Returns the worst ratio |std^2 - var| / bound met."""
    ref = reference(case)
    got = np.asarray(got, np.float64)
    for k in EXACT:
        assert np.array_equal(got[:, FIELDS.index(k)], ref[k], equal_nan=True), (label, case["name"], k, got[:, FIELDS.index(k)], ref[k])
    ang = case["ang"]
    c = np.zeros(len(ang), np.int64) if case["cls"] is None else case["cls"].astype(np.int64)
    worst = 0.0
    for k in range(case["ncls"]):
        x = ang[c == k]
        mean, std = got[k, 1], got[k, 2]
        tame = len(x) > 0 and bool(np.all(np.isfinite(x))) and float(x.max()) <= 180.0
        if tame:
            assert abs(mean - ref["mean"][k]) < 1e-10, (label, case["name"], k, mean, ref["mean"][k])
        elif np.isfinite(ref["mean"][k]):
            # (finite angles above 180 degrees: the same sum, D additions deep, at the rows' own scale)
            assert abs(mean - ref["mean"][k]) <= depth(len(ang), cus) * U * np.mean(np.abs(x)) + 1e-10, (label, case["name"], k, mean, ref["mean"][k])
        else:
            assert np.array_equal(mean, ref["mean"][k], equal_nan=True), (label, case["name"], k, mean, ref["mean"][k])
        if np.isfinite(ref["std"][k]):
            bound = std_bound(np.where(x <= 0, 0.0, x), len(ang), cus)
            err = abs(std * std - ref["std"][k] ** 2)
            assert err <= bound, (label, case["name"], k, std, ref["std"][k], err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
        else:
            assert np.array_equal(std, ref["std"][k], equal_nan=True), (label, case["name"], k, std, ref["std"][k])
    return worst
