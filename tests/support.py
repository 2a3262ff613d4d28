"""What the per-family test files share, said once: the device fixture and the tensor/pointer helpers of tests/test_gpu_<family>.py,
and the numpy pointer, the thread wrapper, the boundary check and the host-model build of tests/test_<family>_host.py.  Imported like
the *_ref.py modules (`from support import ...`); a new family's test files start from here, not from a copy of a neighbour's."""
import ctypes
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT

ABI_VERSION = 210                    # include/so3proj.h: SO3PROJ_VERSION, the one place the tests spell it
GUARD = 64                           # elements in front of and behind a guarded buffer


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from poseestimation_amd import _lib
    _lib.load()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def to_device(a, dev, dtype=np.float32):
    """numpy -> a contiguous tensor of `dtype` on `dev` (dtype=None keeps the array's own); None stays None."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def last_kernel():
    from poseestimation_amd import _lib
    return _lib.load().so3_last_kernel().decode()


def median_ms(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def guarded(shape, fill, dtype, dev):
    """A buffer of `shape` filled with `fill` between two guard bands; returns (the whole allocation, the view the call gets)."""
    count = int(np.prod(shape))
    whole = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + count].view(shape)


def guards_intact(whole, fill):
    edge = torch.cat([whole[:GUARD], whole[-GUARD:]])
    return bool(torch.isnan(edge).all()) if isinstance(fill, float) and np.isnan(fill) else bool((edge == fill).all())


# ---- the host side --------------------------------------------------------------------------------------------------------
def np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lengths_of(lengths, b, full):
    return np.full(b, full, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, full)


def on_own_thread(fn):
    """Run fn() on a thread of its own and re-raise its first exception here.  so3_last_error is per thread and never cleared, and
    other tests read the main thread's: a test that provokes errors does so where nobody else looks."""
    failure = []

    def body():
        try:
            fn()
        except BaseException as exc:               # noqa: BLE001 -- re-raised on the caller's thread
            failure.append(exc)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failure:
        raise failure[0]


def boundary(built_library, new_symbols):
    """The header's prototypes, the binding table and the library's export list name the same functions; every name of `new_symbols`
    is among them with the same argument count in the header and the table (and, for a mapping, the count it gives); the library
    reports the ABI version the table was written for.  -> (the header's text, the library), for the family's own assertions."""
    from poseestimation_amd import _lib
    raw = open(os.path.join(ROOT, "include", "so3proj.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(so3_[a-z0-9_]+)\s*\(", text))
    exported = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(so3_[a-z0-9_]+)\b", exported))
    assert declared == set(_lib.SYMBOLS) == exported
    lib = ctypes.CDLL(built_library)
    for name in new_symbols:
        assert name in declared and name in _lib.SYMBOLS and name in exported and hasattr(lib, name), name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",")
        nargs = new_symbols[name] if isinstance(new_symbols, dict) else len(args)
        assert len(args) == len(_lib.SYMBOLS[name][1]) == nargs, (name, args)
    assert lib.so3_version() == _lib.ABI_VERSION == ABI_VERSION
    return raw, lib


def build_host_model(tmp_path_factory, name, src, fp_contract_off=True):
    """tests/host_model/<src> compiled for the host as lib<name>.so -> ctypes.CDLL; the caller declares argtypes and restype."""
    from oracle import kernel_model
    cxx = kernel_model.clangxx()
    if cxx is None:
        pytest.skip("clang++ is not available (ext_vector_type)")
    out = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    flags = ["-ffp-contract=off"] if fp_contract_off else []
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", *flags, "-fPIC", "-shared", "-o", out, src], check=True)
    return ctypes.CDLL(out)
