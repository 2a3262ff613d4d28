"""tests/support.py itself, without a GPU: the thread wrapper re-raises, the guard bands notice a write on either side, the boundary
check fails when the binding table and the header stop agreeing, and the pointer helpers pass None through."""
import numpy as np
import pytest
import torch

from support import GUARD, bits, boundary, guarded, guards_intact, np_ptr, on_own_thread, ptr

REAL = "so3_project_fwd_f32"         # an entry of every ABI version: five arguments


def test_on_own_thread_reraises_here():
    def fails():
        assert False, "from the other thread"

    with pytest.raises(AssertionError, match="from the other thread"):
        on_own_thread(fails)
    seen = []
    assert on_own_thread(lambda: seen.append(1)) is None and seen == [1]


@pytest.mark.parametrize("shape", [(1,), (3, 5, 3)])
@pytest.mark.parametrize("fill, dtype", [(float("nan"), torch.float32), (-2, torch.int32)])
def test_guard_bands_notice_a_write_on_either_side(shape, fill, dtype):
    cpu, count = torch.device("cpu"), int(np.prod(shape))
    whole, view = guarded(shape, fill, dtype, cpu)
    assert view.shape == shape and whole.numel() == count + 2 * GUARD and guards_intact(whole, fill)
    view[...] = 7                                                       # the whole view, and nothing else
    assert guards_intact(whole, fill) and (whole[GUARD:GUARD + count] == 7).all()
    for at in (GUARD - 1, GUARD + count):
        hit = whole.clone()
        hit[at] = 7
        assert not guards_intact(hit, fill), at


def test_boundary_passes_on_the_tree(built_library):
    from poseestimation_amd import _lib
    raw, lib = boundary(built_library, {REAL: 5})
    assert "SO3PROJ_VERSION" in raw and lib.so3_version() == _lib.ABI_VERSION
    boundary(built_library, [REAL])


def test_boundary_fails_when_the_three_lists_disagree(built_library, monkeypatch):
    from poseestimation_amd import _lib
    with monkeypatch.context() as m:                                    # a name the header declares and the table lacks
        m.delitem(_lib.SYMBOLS, REAL)
        with pytest.raises(AssertionError):
            boundary(built_library, [])
    with monkeypatch.context() as m:                                    # a name in the table that the header does not declare
        m.setitem(_lib.SYMBOLS, "so3_not_in_the_header_f32", _lib.SYMBOLS[REAL])
        with pytest.raises(AssertionError):
            boundary(built_library, [])
    with pytest.raises(AssertionError):                                 # a wrong count for a real entry
        boundary(built_library, {REAL: 6})
    with pytest.raises(AssertionError):                                 # a new symbol that is nowhere
        boundary(built_library, ["so3_not_in_the_header_f32"])
    boundary(built_library, {REAL: 5})                                  # and everything is back as it was


def test_pointers_and_bits():
    assert np_ptr(None) is None and ptr(None) is None
    a, t = np.arange(4, dtype=np.float32), torch.arange(4.0)
    assert np_ptr(a).value == a.ctypes.data and ptr(t).value == t.data_ptr()
    assert bits(np.float32(-0.0)) != bits(np.float32(0.0)) and bits(np.float32(0.0)) == 0
