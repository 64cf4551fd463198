"""What tests/test_gpu_layered_adaptive.py relies on, asserted on the NumPy reference alone (layered_ref.stable_dt and
layered_ref.ssprk33 through layered_adaptive_cases.defining_sequence): no GPU, no HIP library."""
import numpy as np
import pytest

import layered_adaptive_cases as A
import layered_ref as R

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(A.FLAG_CASES))
def test_flag_cases_keep_their_margin(name, dtype):
    """bound / step of the state every chunk ends on stays MARGIN away from 1, on the side the case claims: the
    Float32 accumulation of the device bound (2e-4 at most) cannot flip the flag"""
    lay, hold, courant, cap, expect = A.flag_case(name, dtype)
    dts, starts, ends, y = A.defining_sequence(lay, courant, cap * R.stable_dt(lay, courant), A.NCHUNKS, hold)
    ratios = [e / d for e, d in zip(ends, dts)]
    print(name, np.dtype(dtype).name, "dt", dts, "bound / dt at the chunk ends", ratios)
    assert np.all(np.isfinite(y)) and np.any(y != lay.case.vl) and all(d > 0 for d in dts)
    assert all(abs(r - 1.0) >= A.MARGIN for r in ratios)
    assert any(r < 1.0 for r in ratios) == expect
    if not expect:
        assert all(r >= 1.0 + A.MARGIN for r in ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_cap_is_below_every_chunk_bound(dtype):
    lay = A.capped_case(dtype)
    for hold in (1, 3, 16):
        dt_max = A.CAP_FRACTION * R.stable_dt(lay, A.COURANT)
        dts, starts, ends, _ = A.defining_sequence(lay, A.COURANT, dt_max, A.NCHUNKS, hold)
        assert all(d == float(np.dtype(dtype).type(dt_max)) for d in dts)
        assert all(dt_max <= 0.5 * b for b in starts + ends), (hold, dt_max, starts, ends)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_dirichlet_half_cell_term_binds_where_claimed(dtype):
    lay = A.dirichlet_binding_case(dtype)
    cell, face, inner = A.bound_terms(lay)
    assert A.dirichlet_face_binds(lay) and face.max() >= 2.0 * max(cell.max(), inner.max())
    # ... and the three kinds of terms together are layered_ref.stable_dt
    dz = (lay.case.om.zmax - lay.case.om.zmin) / lay.case.om.nlev
    D = max(cell.max(), face.max(), inner.max())
    assert abs(2.0 * A.COURANT * dz * dz / D - R.stable_dt(lay, A.COURANT)) <= 1e-5 * R.stable_dt(lay, A.COURANT)


def test_the_numpy_bound_of_the_dry_clay_case_is_finite():
    lay = A.dry_clay_case()
    b = R.stable_dt(lay, A.COURANT)
    assert np.isfinite(b) and b > 0
    # the dry column has no positive finite diffusivity of its own: K is 0 where the slope is not finite
    cell, face, inner = A.bound_terms(lay)
    dry = np.array([cell[A.DRY_COLUMN], face[A.DRY_COLUMN], inner[A.DRY_COLUMN]])
    assert not np.any(np.isfinite(dry) & (dry > 0))
    assert np.any(lay.class_map == A.CLAY_CLASS) and lay.classes[A.CLAY_CLASS, 0] < 1.07


def test_the_alternating_map_joins_unlike_classes_at_every_face():
    m = A.alternating_map(7, 127)
    cls = R.texture_classes()
    K, n = cls[:, 3][m], cls[:, 0][m]
    assert np.all(np.maximum(K[:, 1:] / K[:, :-1], K[:, :-1] / K[:, 1:]) >= 100) and np.all(n[:, 1:] != n[:, :-1])
