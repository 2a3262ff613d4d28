"""so3_angle_stats (angle_error_statistics) on every route of its exact median and at its edges: every input of
angle_stats_ref.cases() -- each built to reach one branch of csrc/so3proj.hip's "next row f3" by construction, which
tests/test_angle_stats_host.py asserts without a GPU -- against oracle.so3_oracle.angle_statistics_np (numpy, float64):
count, max, median and the three accuracies bit for bit, mean within 1e-10, std within angle_stats_ref.std_bound.  Through the raw
C ABI on ONE workspace (forwards and backwards through the list, the counted part of the workspace zero after every call, the
flag words StatWork::overflow and ticket read after every call), through the Python surface with int32 and int64 ids, through
the test build whose finishing workgroups never wait (every class selected over the rows themselves), and under graph capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

import angle_stats_ref as ar
from test_gpu_parity import _STAT_ACC_BYTES, _STAT_HIST_AT, DEV, dev

pytestmark = pytest.mark.gpu

CANARY = -12345.678


@pytest.fixture(scope="module")
def rr():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from poseestimation_amd import _lib, rotation_representation
    _lib.load()                                   # fail loudly if the HIP extension is missing
    return rotation_representation


class _Env:
    def __init__(self):
        from poseestimation_amd import _lib
        self.lib = _lib.load()
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.cases = ar.cases(self.cus)
        self.small = [d for d in self.cases if not d.get("staging")]
        self.total = self.lib.so3_angle_stats_workspace_bytes()
        self.counted = self.total - 9 * (1 << 20)          # tag (1 B) and cand (8 B) of 2^20 candidates close the layout
        assert 0 < _STAT_HIST_AT < self.counted < self.total
        self.work = torch.zeros(self.total, dtype=torch.uint8, device=DEV)       # ONE workspace for every raw call of this module
        self.st = torch.cuda.current_stream().cuda_stream
        self._dev = {}
        self.worst_std = 0.0

    def on_device(self, case):
        k = case["name"]
        if k not in self._dev:
            # (copies: the list's arrays are read-only, and torch takes no read-only array)
            self._dev[k] = (dev(case["ang"].copy(), torch.float64), None if case["cls"] is None else dev(case["cls"].copy(), torch.int32))
        return self._dev[k]

    def raw(self, lib, case, a=None, c=None):
        """One call through the C ABI into a canary-filled result; the workspace's counted part must be zero afterwards.  Returns
        ((ncls, 8) array, overflow word, ticket word)."""
        if a is None:
            a, c = self.on_device(case)
        ncls = case["ncls"]
        stats = torch.full((ncls, 8), CANARY, dtype=torch.float64, device=DEV)
        assert lib.so3_angle_stats(a.data_ptr() if a.numel() else None, None if c is None else c.data_ptr(), ncls, stats.data_ptr(), self.work.data_ptr(),
                                   a.numel(), self.st) == 0, case["name"]
        torch.cuda.synchronize()
        assert int(torch.count_nonzero(self.work[:_STAT_ACC_BYTES]).item()) == 0, case["name"]
        assert int(torch.count_nonzero(self.work[_STAT_HIST_AT:self.counted]).item()) == 0, case["name"]
        flags = self.work[_STAT_ACC_BYTES:_STAT_ACC_BYTES + 8].cpu().numpy().view(np.uint32)
        got = stats.cpu().numpy()
        assert not (got == CANARY).any(), case["name"]                  # every class's row is written, empty classes included
        return got, int(flags[0]), int(flags[1])

    def check(self, got, case, label):
        self.worst_std = max(self.worst_std, ar.check_against_reference(got, case, self.cus, label))


@pytest.fixture(scope="module")
def env(rr):
    return _Env()


def _exact(got):
    return got[:, [ar.FIELDS.index(k) for k in ar.EXACT]]


def test_every_case_through_the_c_abi_on_one_workspace(env):
    """Forwards, then backwards through the list: the answers do not depend on what ran before on the workspace.  The flag words:
    every workgroup draws its ticket; bit 0 of `overflow` (a collecting workgroup staged more than 4096 rows) is set exactly where
    the case is built to overflow -- 4096 x CUs + 2 and 8192 x CUs + 3 equal rows -- and clear at 4096 x CUs, where every workgroup's
    staging area (and, with 256 CUs, the candidate buffer) is exactly full; bit 2 (a wait timed out) may be either."""
    from conftest import REPORT_LINES
    first = {}
    for order in (env.cases, env.cases[::-1]):
        for case in order:
            got, overflow, ticket = env.raw(env.lib, case)
            env.check(got, case, "C ABI")
            assert ticket == ar.grid(len(case["ang"]), env.cus), (case["name"], ticket)
            assert (overflow & 1) == (1 if case.get("overflows") else 0), (case["name"], overflow)
            assert overflow & ~5 == 0, (case["name"], overflow)
            if case["name"] in first:
                assert np.array_equal(_exact(got), _exact(first[case["name"]]), equal_nan=True), case["name"]
            first[case["name"]] = got
    assert sum(1 for d in env.cases if d.get("overflows")) == 3
    REPORT_LINES.append("so3_angle_stats: worst |std^2 - var_ref| / bound over %d cases = %.3g (%d CUs)" % (len(env.cases), env.worst_std, env.cus))


@pytest.mark.parametrize("ids", [torch.int32, torch.int64])
def test_every_case_through_angle_error_statistics(rr, env, ids):
    for case in env.cases:
        a, c = env.on_device(case)
        got = rr.angle_error_statistics(a, None if c is None else c.to(ids), case["ncls"])
        assert set(got) == set(ar.FIELDS)
        env.check(torch.stack([got[k] for k in ar.FIELDS], 1).cpu().numpy(), case, "python, %s ids" % ids)


def test_int64_ids_beyond_int32_are_ignored(rr, env):
    """An int64 id of 2^32 + 1 narrows to 1, -2^33 to 0 and 2^31 to INT32_MIN's neighbour: include/so3proj.h ignores rows whose id
    is outside [0, ncls), and the Python surface keeps such ids outside before it narrows them -- the same answers as the C ABI
    gives with ids out of range."""
    case = next(d for d in env.small if d["name"] == "class shape ncls=5")
    rng = np.random.default_rng(9)
    cls = case["cls"].astype(np.int64)
    at = rng.choice(len(cls), 300, replace=False)
    far = np.array([2 ** 32 + 1, -2 ** 33, 2 ** 31, 2 ** 32, -2 ** 32 + 3, 2 ** 63 - 1], np.int64)
    cls[at] = far[np.arange(300) % len(far)]
    c32 = case["cls"].copy()
    c32[at] = np.array([-1, 5, 2 ** 31 - 1, -2 ** 31], np.int64)[np.arange(300) % 4].astype(np.int32)
    as_abi = dict(case, name="int64 ids beyond int32", cls=c32)
    a = env.on_device(case)[0]
    want, _, _ = env.raw(env.lib, as_abi, a, dev(c32, torch.int32))
    env.check(want, dict(as_abi, cls=cls), "C ABI, ids out of range")                 # (the oracle ignores them by itself)
    got = rr.angle_error_statistics(a, dev(cls, torch.int64), 5)
    got = torch.stack([got[k] for k in ar.FIELDS], 1).cpu().numpy()
    assert np.array_equal(_exact(got), _exact(want), equal_nan=True)
    env.check(got, dict(as_abi, cls=cls), "python, int64 ids beyond int32")
    assert got[:, 0].sum() == len(cls) - 300


def test_small_cases_when_no_finishing_workgroup_waits(env):
    """The test build with SO3_STAT_SPINS=0 (tests/test_gpu_parity.py::test_angle_stats_survives_timed_out_waits): a finishing
    workgroup that does not find every ticket drawn at once selects over the rows of its class themselves -- every edge input
    through that selection too, on the workspace the shipped library uses before and after."""
    from poseestimation_amd import _lib, build
    path = os.path.join(os.path.dirname(build.LIB), "libso3proj_spins0.so")
    if not os.path.exists(path):
        build.build_test_variant("spins0", build.TEST_VARIANTS["spins0"])
    slow = ctypes.CDLL(path)
    slow.so3_angle_stats.restype = ctypes.c_int
    slow.so3_angle_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert slow.so3_version() == _lib.ABI_VERSION
    timed_out = 0
    for i, case in enumerate(env.small):
        got, overflow, ticket = env.raw(slow, case)
        env.check(got, case, "spins0")
        assert ticket == ar.grid(len(case["ang"]), env.cus) and (overflow & 1) == 0 and overflow & ~5 == 0, (case["name"], overflow, ticket)
        timed_out += overflow >> 2 & 1
        if i % 16 == 0:                                                 # the shipped library in between, on the same workspace
            got, overflow, _ = env.raw(env.lib, case)
            env.check(got, case, "shipped after spins0")
            assert (overflow & 1) == 0
    print("spins0: %d of %d small cases had a wait time out" % (timed_out, len(env.small)))


def test_a_class_does_not_see_the_other_classes(env):
    """Class k's row of the result with the other classes' rows dealt anew among the other ids and their angles shuffled: the exact
    fields bit for bit."""
    rng = np.random.default_rng(4)
    picked = [d for d in env.small if 3 <= d["ncls"] <= 17 and d["cls"] is not None and 1000 <= len(d["ang"]) <= 3100]
    assert len(picked) >= 20
    for case in picked:
        ncls = case["ncls"]
        k = 1
        base, _, _ = env.raw(env.lib, case)
        cls, ang = case["cls"].copy(), case["ang"].copy()
        others = np.nonzero((cls != k) & (cls >= 0) & (cls < ncls))[0]
        ids = np.array([c for c in range(ncls) if c != k], np.int32)
        cls[others] = ids[rng.integers(0, len(ids), len(others))]
        ang[others] = ang[others][rng.permutation(len(others))]
        moved = dict(case, name=case["name"] + " (others replaced)", ang=ang, cls=cls)
        got, _, _ = env.raw(env.lib, moved, dev(ang, torch.float64), dev(cls, torch.int32))
        assert np.array_equal(_exact(got)[k], _exact(base)[k], equal_nan=True), case["name"]
        env.check(got, moved, "others replaced")


def test_graph_capture_gives_the_eager_answers(rr, env):
    case = next(d for d in env.small if d["name"] == "edge zeros 60% n=3001 ncls=5")
    a, c = env.on_device(case)

    def step():
        got = rr.angle_error_statistics(a, c, 5)
        return torch.stack([got[k] for k in ar.FIELDS], 1)
    eager = step().cpu().numpy()
    env.check(eager, case, "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                          # warm up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        captured.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        got = captured.cpu().numpy()
        assert np.array_equal(_exact(got), _exact(eager), equal_nan=True)
        env.check(got, case, "replay")
