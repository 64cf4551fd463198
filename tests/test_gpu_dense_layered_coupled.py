"""lh_integrate_layered_coupled_dense: the adaptive TR-BDF2 of the coupled model with soil classes with output
interpolated inside the launch.  tests/test_gpu_dense_heat.py's checks on the family of
tests/test_gpu_layered_coupled_series.py: sand over clay with thermal supplements, the interface at a level that differs
from column to column; both vartheta_l and rhoe_int of a snapshot are written."""
import ctypes as C
import functools

import numpy as np
import pytest

import case_model as M
import layered_coupled_implicit_ref as LC
import parity_cases as pc
from test_gpu_bc_series import KNOTS, NCOLS, NLEV, SHAPE_H, SHIFT_E, T0, T1, _dptr, _step_buffer
from test_gpu_dense import SAVES
from test_gpu_dense_heat import (DTYPES, IDS, TOP_IDS, TOPS, call_dense, check_a_failing_column,
                                 check_accuracy_against_the_clipped_chain, check_columns_alone, check_dense_refusals,
                                 check_invisible_with_a_series, check_invisible_without_a_series, check_nested_save_sets, handles,
                                 refused as _refused, stats_of, truth_of)
from test_gpu_heat_series import _stats, make_series
from test_gpu_layered_coupled_series import family, uniform_values

pytestmark = pytest.mark.gpu
NAME = "lh_integrate_layered_coupled_dense"
NO_CLASS_MAP = NAME + ": the context has no class map (lh_set_soil_class_map); lh_integrate_dense steps a model without soil classes"


# ------------------------------------------------------------------ 1. the integration does not see the output

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
def test_output_is_invisible_with_a_series(top, dtype):
    fam, sd = family(dtype, top)
    got = check_invisible_with_a_series(fam, sd, uniform_values(fam, top))
    assert got["stats"]["newton_iterations"] > 0


# ------------------------------------------------------------------ 2. ... nor without a series

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_output_is_invisible_without_a_series(dtype):
    """theta_i in Ya is not zero: the !NOICE instantiation"""
    fam, sd = family(dtype, M.BC_FLUX, ice=True)
    assert np.any(fam.case.ti != 0)
    check_invisible_without_a_series(fam, sd)


# ------------------------------------------------------------------ 3. nested save sets

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nested_save_sets(dtype):
    fam, sd = family(dtype, M.BC_DIRICHLET)
    check_nested_save_sets(fam, sd, uniform_values(fam, M.BC_DIRICHLET))


# ------------------------------------------------------------------ 6. accuracy and the payoff, against the clipped chain

SPACING = 1.0       # stable steps between two save times, as tests/test_gpu_dense.py's
# E_dense / max(E_chain, 1) as measured on the MI355X, per (top, dtype); the assertion allows
# twice the largest.
RECORDED_RATIO = {("flux", "f64"): 1.251, ("flux", "f32"): 1.251, ("dirichlet", "f64"): 2.173, ("dirichlet", "f32"): 2.173}
RATIO_ALLOWED = 2.0 * max(RECORDED_RATIO.values())


@functools.lru_cache(maxsize=None)
def _truth(top):
    fam64, sd = family(np.float64, top)
    return truth_of(fam64, sd, SPACING), sd


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
def test_accuracy_and_step_counts_against_the_clipped_chain(top, dtype):
    truth, sd = _truth(top)          # (the Float64 case's stable step: the save times are the truth's)
    fam, _ = family(dtype, top)
    label = "layered-coupled %s %s" % (TOP_IDS[TOPS.index(top)], np.dtype(dtype).name)
    got, clipped = check_accuracy_against_the_clipped_chain(label, fam, sd, SPACING, RATIO_ALLOWED, truth)
    assert got["stats"]["newton_iterations"] <= clipped["stats"]["newton_iterations"], (got["stats"], clipped["stats"])


# ------------------------------------------------------------------ 7. column independence

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_columns_snapshots_are_its_own(dtype):
    fam, sd = family(dtype, M.BC_FLUX)
    check_columns_alone(fam, sd, uniform_values(fam, M.BC_FLUX))


# ------------------------------------------------------------------ 8. a failing column

def test_a_failing_column_fills_its_snapshots_with_its_kept_state():
    fam, sd = family(np.float32, M.BC_FLUX, ncols=64)
    check_a_failing_column(fam, sd, uniform_values(fam, M.BC_FLUX), 64)


# ------------------------------------------------------------------ 9. refusals

def refused(gm, rc, code, *words):
    _refused(gm, rc, code, *words, name=NAME)


def test_refusals_leave_everything_untouched():
    fam, sd = family(np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    vals = uniform_values(fam, M.BC_FLUX)
    t0, t1 = T0 * sd, T1 * sd
    with fam.open() as gm, fam.open() as other:
        F, L = gm.F, gm.L
        EINVAL, EMODEL = F.LH_EINVAL, F.LH_EMODEL
        VL, RE = F.LH_VAR_VARTHETA_L, F.LH_VAR_RHOE_INT
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)
        marks = [np.full((67, NLEV), 0.1 * (k + 1)) for k in range(3)]
        snaps = [gm.state(0) for _ in range(3)]
        for sn, a in zip(snaps, marks):
            gm.upload(sn, VL, a)
            gm.upload(sn, RE, 1.0e8 * a)
        water_only = gm.state((1 << VL) | (1 << F.LH_VAR_THETA_I))
        good = np.array([3.0, 9.0, 20.0]) * sd
        cols = _step_buffer(fam.case, np.full(67, 0.5 * sd))
        cols_before = cols.cpu().numpy().copy()

        def call(times=good, states=snaps, nsave=None, series_h=h, dt=sd, t0=t0, t1=t1, null_times=False, null_states=False,
                 flags=0, abstol=0.0, with_cols=True):
            s = np.ascontiguousarray(times, dtype=np.float64)
            return call_dense(fam, gm, Y, Ya, series_h, t0, t1, dt, C.c_void_p(cols.data_ptr()) if with_cols else None,
                              len(s) if nsave is None else nsave, None if null_times else _dptr(s),
                              None if null_states else handles(states), flags=flags, abstol=abstol)

        # a run first, so that the statistics are not zero before the refusals (into states of its own, no step buffer)
        F.check(call(states=[gm.state(0) for _ in range(3)], with_cols=False), gm.ctx)
        assert _stats(gm)["accepted"] >= 67
        before = gm.download(Y, VL), gm.download(Y, RE)
        # ---- the wrapped series call's refusals come first, in its words, with a bad nsave in the same call
        refused(gm, call(t0=2.0 * sd, t1=1.0 * sd, nsave=-1), EINVAL, ": need finite t0 <= t1")
        refused(gm, call(dt=0.0, nsave=-1), EINVAL, ": need a finite dt > 0")
        refused(gm, call(abstol=-1e-6, nsave=-1), EINVAL, ": tolerances must be finite and >= 0")
        refused(gm, call(flags=1, nsave=-1), EINVAL, ": unknown flags 0x1")
        refused(gm, call(series_h=make_series(other, T, vals), nsave=-1), EINVAL, "not a series of this context")
        refused(gm, call(t1=T[-1] + 0.5 * sd, nsave=-1), EINVAL, "no extrapolation")
        v0 = np.ascontiguousarray(vals[(M.FACE_TOP, M.COMP_HYDROLOGY)])
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)   # free drainage
        refused(gm, call(nsave=-1), EMODEL, "bottom hydrology", "reads no value")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        # (series == NULL is no refusal here: the series' checks apply only with a series)
        refused(gm, call(series_h=None, nsave=-1), EINVAL, "nsave = -1")
        assert getattr(L, NAME)(None, Y, Ya, h, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None, 0, None, None) == EINVAL
        # ---- then dense_refusals; a snapshot must hold both written planes
        check_dense_refusals(fam, gm, other, call, snaps, water_only, Y, Ya, sd)
        # ---- Y, the snapshots and dt_cols are as they were
        np.testing.assert_array_equal(gm.download(Y, VL), before[0])
        np.testing.assert_array_equal(gm.download(Y, RE), before[1])
        for sn, a in zip(snaps, marks):
            np.testing.assert_array_equal(gm.download(sn, VL), a)
            np.testing.assert_array_equal(gm.download(sn, RE), 1.0e8 * a)
        np.testing.assert_array_equal(cols.cpu().numpy(), cols_before)
        # ---- and the call goes on working: only vartheta_l and rhoe_int of a snapshot are written; t0 == t1 writes Y
        ti_mark = np.full((67, NLEV), 0.0125)
        gm.upload(snaps[0], F.LH_VAR_THETA_I, ti_mark)
        F.check(call(), gm.ctx)
        assert np.max(np.abs(gm.download(snaps[0], VL) - marks[0])) > 0 and np.max(np.abs(gm.download(snaps[0], RE) - 1e8 * marks[0])) > 0
        np.testing.assert_array_equal(gm.download(snaps[0], F.LH_VAR_THETA_I), ti_mark)
        now = gm.download(Y, VL), gm.download(Y, RE)
        F.check(call(times=[3.0 * sd], states=snaps[:1], t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(snaps[0], VL), now[0])
        np.testing.assert_array_equal(gm.download(snaps[0], RE), now[1])
        np.testing.assert_array_equal(gm.download(Y, VL), now[0])
        assert all(v == 0 for v in _stats(gm).values())
        # ---- lh_integrate_dense still refuses this context
        rc = L.lh_integrate_dense(gm.ctx, Y, Ya, None, t0, t1, sd, 0.0, 0.0, 0.0, 0, None, 0, None, None)
        assert rc == EMODEL and "soil classes" in L.lh_last_error(gm.ctx).decode()
    # ---- and a coupled context without a map, which lh_integrate_dense serves, is pointed there
    with pc.GpuModel(fam.case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        rc = getattr(gm.L, NAME)(gm.ctx, Y, Ya, None, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None, -1, None, None)
        refused(gm, rc, gm.F.LH_EMODEL)
        assert gm.L.lh_last_error(gm.ctx).decode() == NO_CLASS_MAP
        gm.F.check(gm.L.lh_integrate_dense(gm.ctx, Y, Ya, None, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None, 0, None, None), gm.ctx)
        assert gm.status() == 0


# ------------------------------------------------------------------ 10. the host mirror

def test_host_mirror():
    """integrate_layered_coupled_dense with and without a series: the statistics and the snapshots are the C call's."""
    from test_gpu_layered_coupled_trbdf2 import horizon_model
    lh = pc._pkg()
    N = 5
    lay = LC.layered_case(np.float64, N, NLEV, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    case = lay.case
    fw = -2e-9
    model, dom, bc = horizon_model(lh, lay, lambda t: 287.0, 281.0, fw)
    ic = lambda z, m: {"ϑ_l": 0.2 + 0.0 * z, "θ_i": 0.0 * z, "ρe_int": 1e7 + 0.0 * z}
    states = [lh.initialize_states(model, ic, 0.0) for _ in range(4)]
    for Y, _ in states:
        Y.soil.ϑ_l, Y.soil.ρe_int = case.vl, case.rhoe
    (Y1, Ya), (Y2, _), (Y3, _), (Y4, _) = states
    sd = LC.stable_dt(lay)
    T = KNOTS * sd
    u = pc.uhash(np.arange(N), 3, 1)
    fs = lh.BoundarySeries(T, {("top", "hydrology"): fw * SHAPE_H[M.BC_FLUX][:, None] * (0.8 + 0.4 * u)[None, :],
                               ("top", "energy"): 287.0 + SHIFT_E})
    s = np.ascontiguousarray(SAVES * sd)
    F = lh._ffi
    L, be = F.lib(), model._backend()
    for series_, Ym, Yc in ((fs, Y1, Y2), (None, Y3, Y4)):
        st, snaps = lh.integrate_layered_coupled_dense(model, Ym, Ya, T0 * sd, T1 * sd, sd, s, series=series_, reltol=1e-4)
        assert st["failed"] == 0 and st["accepted"] >= N and len(snaps) == len(s), st
        mine = [Yc.similar() for _ in s]
        arr = (C.c_void_p * len(s))(*[x.handle.value for x in mine])
        F.check(getattr(L, NAME)(be.ctx, Yc.handle, getattr(Ya, "handle", None), None if series_ is None else fs._device(model),
                                 T0 * sd, T1 * sd, sd, 1e-6, 0.0, 1e-4, 0, None, len(s), _dptr(s), arr), be.ctx)
        assert stats_of(lh, be) == st
        for name in ("ϑ_l", "ρe_int"):
            np.testing.assert_array_equal(Yc.get(name), Ym.get(name))
            np.testing.assert_array_equal(snaps[-1].get(name), Ym.get(name))
            for a, b in zip(snaps, mine):
                np.testing.assert_array_equal(a.get(name), b.get(name))
    assert np.max(np.abs(Y1.get("ρe_int") - Y3.get("ρe_int"))) > 0      # (the series is read)
    with pytest.raises(ValueError, match="integrate_layered_coupled_dense: save time 0"):
        lh.integrate_layered_coupled_dense(model, Y1, Ya, T0 * sd, T1 * sd, sd, [T1 * sd + 1.0], series=fs)
    # a model without classes is pointed to the call that serves it
    plain = lh.SoilModel(np.float64, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(np.float64),
                         boundary_conditions=bc, domain=dom, earth_param_set=lh.EarthParameterSet())
    with pytest.raises(NotImplementedError, match="lh_integrate_dense steps a model without soil classes"):
        lh.integrate_layered_coupled_dense(plain, object(), None, T[0], T[1], sd, [T[1]], series=fs)
    model.close()
