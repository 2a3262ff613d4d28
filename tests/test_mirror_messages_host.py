"""The argument checks of the pair operations -- nearest_neighbors, icp_align, icp_align_plane, chamfer_distance, knn_points -- on the
host: exception type and FULL text of what a malformed call raises, against literals recorded from the package as it stood before the
mirror was split into modules.  These are the messages the shared pair validator and the ICPs' shared argument handling rebuild.

No GPU and no library: every case raises before the first C-ABI call.  _require_device, which would refuse a CPU tensor first, is
stood in for in the modules that look it up, so the shape checks themselves are reached with CPU tensors."""
import pytest
import torch

import poseestimation_amd as pa
from poseestimation_amd import _lib, _runtime, neighbors

BIG = _lib.ADD_S_MAX_N + 1


def _cloud(*shape):
    return torch.zeros(shape)


def _huge(b, width=3):
    """(b, ADD_S_MAX_N + 1, width) without the memory: one element, expanded."""
    return torch.empty((1, 1, 1)).expand(b, BIG, width)


def _cases():
    """(id, function name, args, kwargs)"""
    P, Q = _cloud(2, 5, 3), _cloud(2, 7, 3)
    out = []
    for op, more in (("nearest_neighbors", ()), ("icp_align", ()), ("icp_align_plane", ()), ("chamfer_distance", ()), ("knn_points", (3,))):
        for tag, x, y in (("source_rank", _cloud(5, 3), Q), ("target_rank", P, _cloud(7)), ("source_width", _cloud(2, 5, 4), Q),
                          ("target_width", P, _cloud(2, 7, 4)), ("n_zero", _cloud(2, 0, 3), Q), ("m_zero", P, _cloud(2, 0, 3)),
                          ("n_too_large", _huge(2), Q), ("m_too_large", P, _huge(2)), ("batch_mismatch", P, _cloud(3, 7, 3)),
                          ("shared_m_zero", P, _cloud(0, 3))):
            out.append(("%s-%s" % (op, tag), op, (x, y) + more, {}))
    out.append(("chamfer_distance-shared_target", "chamfer_distance", (P, _cloud(7, 3)), {}))          # the one op without "or (M, 3)"
    for op in ("icp_align", "icp_align_plane"):
        out += [("%s-R_init_shape" % op, op, (P, Q), {"R_init": _cloud(3, 3)}),
                ("%s-t_init_shape" % op, op, (P, Q), {"t_init": _cloud(2, 4)}),
                ("%s-weights_shape" % op, op, (P, Q), {"weights": _cloud(2, 6)}),
                ("%s-all_three_shapes" % op, op, (P, Q), {"R_init": _cloud(2, 9), "t_init": _cloud(3), "weights": _cloud(5)}),
                ("%s-shared_target_weights_shape" % op, op, (P, _cloud(7, 3)), {"weights": _cloud(2, 7)}),
                ("%s-iterations_negative" % op, op, (P, Q), {"iterations": -1})]
    out += [("icp_align_plane-damping_negative", "icp_align_plane", (P, Q), {"damping": -0.5}),
            ("icp_align_plane-damping_nan", "icp_align_plane", (P, Q), {"damping": float("nan")}),
            ("icp_align_plane-normals_shape", "icp_align_plane", (P, Q), {"normals": _cloud(2, 5, 3)})]
    for op, more in (("chamfer_distance", ()), ("knn_points", (3,))):
        out += [("%s-x_lengths_shape" % op, op, (P, Q) + more, {"x_lengths": torch.zeros(3, dtype=torch.int64)}),
                ("%s-x_lengths_dtype" % op, op, (P, Q) + more, {"x_lengths": torch.zeros(2, dtype=torch.float32)}),
                ("%s-y_lengths_shape" % op, op, (P, Q) + more, {"y_lengths": torch.zeros((2, 1), dtype=torch.int32)}),
                ("%s-y_lengths_dtype" % op, op, (P, Q) + more, {"y_lengths": torch.zeros(2, dtype=torch.int16)})]
    return out


EXPECTED = {
    'nearest_neighbors-source_rank':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (5, 3) and (2, 7, 3)'),
    'nearest_neighbors-target_rank':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7,)'),
    'nearest_neighbors-source_width':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 4) and (2, 7, 3)'),
    'nearest_neighbors-target_width':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 7, 4)'),
    'nearest_neighbors-n_zero':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 0, 3) and (2, 7, 3)'),
    'nearest_neighbors-m_zero':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 0, 3)'),
    'nearest_neighbors-n_too_large':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 1048577, 3) and (2, 7, 3)'),
    'nearest_neighbors-m_too_large':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 1048577, 3)'),
    'nearest_neighbors-batch_mismatch':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (3, 7, 3)'),
    'nearest_neighbors-shared_m_zero':
        (RuntimeError, 'nearest_neighbors: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (0, 3)'),
    'icp_align-source_rank':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (5, 3) and (2, 7, 3)'),
    'icp_align-target_rank':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7,)'),
    'icp_align-source_width':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 4) and (2, 7, 3)'),
    'icp_align-target_width':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 7, 4)'),
    'icp_align-n_zero':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 0, 3) and (2, 7, 3)'),
    'icp_align-m_zero':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 0, 3)'),
    'icp_align-n_too_large':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 1048577, 3) and (2, 7, 3)'),
    'icp_align-m_too_large':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 1048577, 3)'),
    'icp_align-batch_mismatch':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (3, 7, 3)'),
    'icp_align-shared_m_zero':
        (RuntimeError, 'icp_align: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (0, 3)'),
    'icp_align_plane-source_rank':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (5, 3) and (2, 7, 3)'),
    'icp_align_plane-target_rank':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7,)'),
    'icp_align_plane-source_width':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 4) and (2, 7, 3)'),
    'icp_align_plane-target_width':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 7, 4)'),
    'icp_align_plane-n_zero':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 0, 3) and (2, 7, 3)'),
    'icp_align_plane-m_zero':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 0, 3)'),
    'icp_align_plane-n_too_large':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 1048577, 3) and (2, 7, 3)'),
    'icp_align_plane-m_too_large':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 1048577, 3)'),
    'icp_align_plane-batch_mismatch':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (3, 7, 3)'),
    'icp_align_plane-shared_m_zero':
        (RuntimeError, 'icp_align_plane: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (0, 3)'),
    'chamfer_distance-source_rank':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (5, 3) and (2, 7, 3)'),
    'chamfer_distance-target_rank':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7,)'),
    'chamfer_distance-source_width':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 4) and (2, 7, 3)'),
    'chamfer_distance-target_width':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 7, 4)'),
    'chamfer_distance-n_zero':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 0, 3) and (2, 7, 3)'),
    'chamfer_distance-m_zero':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 0, 3)'),
    'chamfer_distance-n_too_large':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 1048577, 3) and (2, 7, 3)'),
    'chamfer_distance-m_too_large':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 1048577, 3)'),
    'chamfer_distance-batch_mismatch':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (3, 7, 3)'),
    'chamfer_distance-shared_m_zero':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (0, 3)'),
    'knn_points-source_rank':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (5, 3) and (2, 7, 3)'),
    'knn_points-target_rank':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7,)'),
    'knn_points-source_width':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 4) and (2, 7, 3)'),
    'knn_points-target_width':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 7, 4)'),
    'knn_points-n_zero':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 0, 3) and (2, 7, 3)'),
    'knn_points-m_zero':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 0, 3)'),
    'knn_points-n_too_large':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 1048577, 3) and (2, 7, 3)'),
    'knn_points-m_too_large':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (2, 1048577, 3)'),
    'knn_points-batch_mismatch':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (3, 7, 3)'),
    'knn_points-shared_m_zero':
        (ValueError, 'knn_points: expected a source (B, N, 3) and a target (B, M, 3) or (M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (0, 3)'),
    'chamfer_distance-shared_target':
        (RuntimeError, 'chamfer_distance: expected a source (B, N, 3) and a target (B, M, 3) with 1 <= N, M <= 1048576, got (2, 5, 3) and (7, 3)'),
    'icp_align-R_init_shape':
        (RuntimeError, 'icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [(3, 3), None, None]'),
    'icp_align-t_init_shape':
        (RuntimeError, 'icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, (2, 4), None]'),
    'icp_align-weights_shape':
        (RuntimeError, 'icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, None, (2, 6)]'),
    'icp_align-all_three_shapes':
        (RuntimeError, 'icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [(2, 9), (3,), (5,)]'),
    'icp_align-shared_target_weights_shape':
        (RuntimeError, 'icp_align: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, None, (2, 7)]'),
    'icp_align-iterations_negative':
        (RuntimeError, 'icp_align: iterations must be >= 0, got -1'),
    'icp_align_plane-R_init_shape':
        (RuntimeError, 'icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [(3, 3), None, None]'),
    'icp_align_plane-t_init_shape':
        (RuntimeError, 'icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, (2, 4), None]'),
    'icp_align_plane-weights_shape':
        (RuntimeError, 'icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, None, (2, 6)]'),
    'icp_align_plane-all_three_shapes':
        (RuntimeError, 'icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [(2, 9), (3,), (5,)]'),
    'icp_align_plane-shared_target_weights_shape':
        (RuntimeError, 'icp_align_plane: expected R_init (B, 3, 3), t_init (B, 3) and weights (B, N) for B = 2, N = 5, got [None, None, (2, 7)]'),
    'icp_align_plane-iterations_negative':
        (RuntimeError, 'icp_align_plane: iterations must be >= 0, got -1'),
    'icp_align_plane-damping_negative':
        (RuntimeError, 'icp_align_plane: damping must be >= 0, got -0.5'),
    'icp_align_plane-damping_nan':
        (RuntimeError, 'icp_align_plane: damping must be >= 0, got nan'),
    'icp_align_plane-normals_shape':
        (RuntimeError, "icp_align_plane: expected normals of the target's shape (2, 7, 3), got (2, 5, 3)"),
    'chamfer_distance-x_lengths_shape':
        (RuntimeError, 'chamfer_distance: expected x_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (3,) torch.int64 on cpu'),
    'chamfer_distance-x_lengths_dtype':
        (RuntimeError, 'chamfer_distance: expected x_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2,) torch.float32 on cpu'),
    'chamfer_distance-y_lengths_shape':
        (RuntimeError, 'chamfer_distance: expected y_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2, 1) torch.int32 on cpu'),
    'chamfer_distance-y_lengths_dtype':
        (RuntimeError, 'chamfer_distance: expected y_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2,) torch.int16 on cpu'),
    'knn_points-x_lengths_shape':
        (ValueError, 'knn_points: expected x_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (3,) torch.int64 on cpu'),
    'knn_points-x_lengths_dtype':
        (ValueError, 'knn_points: expected x_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2,) torch.float32 on cpu'),
    'knn_points-y_lengths_shape':
        (ValueError, 'knn_points: expected y_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2, 1) torch.int32 on cpu'),
    'knn_points-y_lengths_dtype':
        (ValueError, 'knn_points: expected y_lengths as a (B,) int32 or int64 tensor on cpu for B = 2, got (2,) torch.int16 on cpu'),
}


@pytest.fixture
def on_host(monkeypatch):
    for module in (neighbors, _runtime):               # _cloud_pair's lookup, and _cloud_lengths'
        monkeypatch.setattr(module, "_require_device", lambda *tensors: torch.device("cpu"))


def test_every_case_has_its_literal():
    assert sorted(EXPECTED) == sorted(c[0] for c in _cases()) and len(EXPECTED) == len(_cases())


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_malformed_arguments_raise_the_recorded_type_and_text(case, on_host):
    key, op, args, kwargs = case
    kind, text = EXPECTED[key]
    with pytest.raises(Exception) as info:
        getattr(pa, op)(*args, **kwargs)
    assert type(info.value) is kind and str(info.value) == text
