"""The persistent column stepper of layered soils (layered_column_stepper_wave_kernel): a
Richards context with a class map under `persist=2` steps in one launch per call, bitwise the three fused-stage
launches per step it takes under `persist=0`.

Every comparison is array_equal on vartheta_l plus equality of lh_status, between the two tunings, from the same
start, with dt = 0.5 lh_stable_dt(courant 0.5); every test also asserts that the state moved."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import case_model as M
import layered_heat_ref as H
import layered_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
FUSED, STEPPER = b"persist=0", b"persist=2"
STEP_BOUND = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 3e-6}    # DESIGN.md section 2, of the field scale
DP = C.POINTER(C.c_double)


def layered_gpu(lay):
    g = pc.GpuModel(lay.case)
    g.set_soil_classes(lay.classes, lay.class_map)
    return g


def stable_dt(g, Y, Ya, courant=0.5):
    out = C.c_double()
    g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, courant, C.byref(out)), g.ctx)
    return out.value


def fresh_state(g, zero_ti_plane=False):
    """(Y, Ya) of the case; zero_ti_plane: the all-zero theta_i goes up as a plane, not as a fill"""
    Y, Ya = g.prognostic_and_aux()
    if zero_ti_plane:
        assert not np.any(g.case.ti)
        z = np.zeros_like(g.case.vl)
        g.F.check(g.L.lh_upload(g.ctx, Y, g.F.LH_VAR_THETA_I, z.ctypes.data, 1, g.case.om.nlev), g.ctx)
    return Y, Ya


def step(g, tuning, dt, nsteps, calls=1, bcv=None, zero_ti_plane=False, engine=None):
    """`calls` calls of lh_step_ssprk33 with nsteps steps each from the case's start under `tuning`;
    bcv: [calls * nsteps][3][2][2].  -> (vartheta_l, status)"""
    F, L = g.F, g.L
    F.check(L.lh_set_tuning(g.ctx, tuning), g.ctx)
    if engine is not None:
        assert L.lh_step_engine(g.ctx, nsteps, int(bcv is not None)) == engine
    Y, Ya = fresh_state(g, zero_ti_plane)
    for k in range(calls):
        b = None
        if bcv is not None:
            b = np.ascontiguousarray(bcv[k * nsteps:(k + 1) * nsteps], dtype=np.float64)
            assert b.shape == (nsteps, 3, 2, 2)
            b = b.ctypes.data_as(DP)
        F.check(L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, dt, nsteps, b), g.ctx)
    return g.download(Y, F.LH_VAR_VARTHETA_L), g.status()


def both_engines(lay, nsteps=5, bcv=None, one_by_one=False, zero_ti_plane=False):
    """The fused stages and the stepper from the same start in one context, compared bitwise.
    -> (the stepper's vartheta_l, status, dt)"""
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
        assert np.isfinite(dt) and dt > 0
        want, st_want = step(g, FUSED, dt, nsteps, bcv=bcv, engine=F.LH_ENGINE_FUSED_STAGES)
        got, st_got = step(g, STEPPER, dt, nsteps, bcv=bcv, zero_ti_plane=zero_ti_plane, engine=F.LH_ENGINE_COLUMN_STEPPER)
        np.testing.assert_array_equal(got, want)
        assert st_got == st_want
        if one_by_one:
            got1, st1 = step(g, STEPPER, dt, 1, calls=nsteps, bcv=bcv, engine=F.LH_ENGINE_COLUMN_STEPPER)
            np.testing.assert_array_equal(got1, want)
            assert st1 == st_want
    assert np.any(got != lay.case.vl), "the state did not move"
    return got, st_got, dt


def alternating_map(ncols, nlev, ncls=16):
    """class(c, i) = (i + c) mod ncls: every face of every column joins two classes"""
    return ((np.arange(nlev)[None, :] + np.arange(ncols)[:, None]) % ncls).astype(np.uint8)


# ------------------------------------------------------------ 1. the engine report

def _engine(g, tuning, nsteps=5):
    if tuning is not None:
        g.F.check(g.L.lh_set_tuning(g.ctx, tuning), g.ctx)
    return g.L.lh_step_engine(g.ctx, nsteps, 0)


def test_engine_report():
    F = pc._pkg()._ffi
    for nlev, want in ((64, F.LH_ENGINE_COLUMN_STEPPER), (128, F.LH_ENGINE_COLUMN_STEPPER), (130, F.LH_ENGINE_FUSED_STAGES)):
        lay = R.make_layered(np.float64, 5, nlev, R.horizon_map(5, nlev))
        with layered_gpu(lay) as g:
            assert _engine(g, None) == F.LH_ENGINE_FUSED_STAGES, "the default tuning keeps the fused stages"
            assert _engine(g, STEPPER) == want, nlev
            assert _engine(g, FUSED) == F.LH_ENGINE_FUSED_STAGES
            assert _engine(g, b"") == F.LH_ENGINE_FUSED_STAGES
            # ... and lh_step_ssprk33 does what the report says: the 130-level column steps by fused stages
            Y, Ya = g.prognostic_and_aux()
            dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
            got, st = step(g, STEPPER, dt, 2, engine=want)
            ref, st_ref = step(g, FUSED, dt, 2)
            np.testing.assert_array_equal(got, ref)
            assert st == st_ref == 0 and np.any(got != lay.case.vl)
    layh = H.make_layered_heat(np.float64, 5, 64, R.horizon_map(5, 64), model=M.MODEL_COUPLED)
    g = pc.GpuModel(layh.case)
    with g:
        g.set_soil_classes(layh.classes, layh.class_map, thermal=layh.thermal)
        assert _engine(g, STEPPER) == F.LH_ENGINE_FUSED_STAGES, "a layered coupled context has no stepper"


# ------------------------------------------------------------ 2. bitwise the fused stages over shapes

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 64, 65, 97, 128])
def test_bitwise_the_fused_stages_over_shapes(dtype, nlev):
    """ncols in {1, 67, 130} x nclasses in {1, 3, 16}, horizon maps: 5 steps in one call and as five 1-step calls.
    (Dirichlet faces: the diffusive step bound then bounds the boundary terms too, so columns of one to three
    cells stay finite at the step the comparisons take.)"""
    for ncols in (1, 67, 130):
        for ncls in (1, 3, 16):
            lay = R.make_layered(dtype, ncols, nlev, R.horizon_map(ncols, nlev, ncls), classes=R.texture_classes()[:ncls],
                                 bc="dirichlet")
            got, st, _ = both_engines(lay, one_by_one=True)
            assert st == 0 and np.all(np.isfinite(got)), (ncols, ncls)


# ------------------------------------------------------------ 3. every face a class interface

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [64, 127, 128])
def test_every_face_a_class_interface(dtype, nlev):
    """class(c, i) = (i + c) mod 16: the in-lane faces (two cells per lane) and the lane-to-lane faces all join
    classes whose Ksat differ by a factor >= 100"""
    ncols = 7
    m = alternating_map(ncols, nlev)
    K = R.texture_classes()[:, 3][m]
    jump = np.maximum(K[:, 1:] / K[:, :-1], K[:, :-1] / K[:, 1:])
    assert np.all(jump >= 100)
    got, st, _ = both_engines(R.make_layered(dtype, ncols, nlev, m))
    assert st == 0 and np.all(np.isfinite(got))


# ------------------------------------------------------------ 4. boundary kinds, factors and ice

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
@pytest.mark.parametrize("factors,ice", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "ice", "factors", "factors_ice"])
def test_boundary_kinds_factors_and_ice(dtype, bc, factors, ice):
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc=bc, factors=factors, ice=ice)
    got, st, _ = both_engines(lay)
    assert st == 0 and np.all(np.isfinite(got))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_uploaded_zero_theta_i_plane_gives_the_known_zero_bits(dtype):
    """the kernel that reads theta_i, given an ice-free state, against the one that knows the plane to be zero"""
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet")
    known, st0, _ = both_engines(lay)
    plane, st1, _ = both_engines(lay, zero_ti_plane=True)
    np.testing.assert_array_equal(plane, known)
    assert st0 == st1 == 0


# ------------------------------------------------------------ 5. per-stage boundary values

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["dirichlet", "flux_drain"])
def test_per_stage_boundary_values(dtype, bc):
    """[5][3][2][2] values (step, stage, face, component) whose top hydrology entry changes every stage"""
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc=bc)
    H_, top, bot = M.COMP_HYDROLOGY, M.FACE_TOP, M.FACE_BOTTOM
    bcv = np.zeros((5, 3, 2, 2))
    bcv[:, :, bot, H_] = lay.case.om.bc[(bot, H_)][1]
    k = np.arange(15, dtype=np.float64).reshape(5, 3)
    v0 = lay.case.om.bc[(top, H_)][1]
    bcv[:, :, top, H_] = v0 + 0.002 * k if bc == "dirichlet" else v0 * (1.0 + 0.25 * k)
    got, st, dt = both_engines(lay, bcv=bcv, one_by_one=True)
    assert st == 0
    with layered_gpu(lay) as g:     # ... and the values are read: constant ones end elsewhere
        const, _ = step(g, STEPPER, dt, 5)
    assert np.any(const != got)


# ------------------------------------------------------------ 6. columns are independent

def _column(lay, k):
    case = lay.case
    one = dataclasses.replace(case, ncols=1, vl=case.vl[k:k + 1], ti=case.ti[k:k + 1],
                              T_aux=None if case.T_aux is None else case.T_aux[k:k + 1])
    return R.Layered(one, lay.classes, np.ascontiguousarray(lay.class_map[k:k + 1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_columns_are_independent(dtype):
    """67 columns: 4 per workgroup, so the last workgroup has one spare slot that shadows column 66"""
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet")
    got, st, dt = both_engines(lay)
    assert st == 0
    for k in (0, 63, 66):
        with layered_gpu(_column(lay, k)) as g:
            alone, st1 = step(g, STEPPER, dt, 5, engine=g.F.LH_ENGINE_COLUMN_STEPPER)
        np.testing.assert_array_equal(alone, got[k:k + 1])
        assert st1 == 0


# ------------------------------------------------------------ 7. against the NumPy reference

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stepper_matches_the_numpy_reference_at_128_levels(dtype):
    lay = R.make_layered(dtype, 130, 128, R.horizon_map(130, 128))
    got, st, dt = both_engines(lay, nsteps=20)
    assert st == 0
    want = R.ssprk33(lay, dt, 20).astype(np.float64)
    err = float(np.max(np.abs(got.astype(np.float64) - want)) / np.max(np.abs(want)))
    moved = float(np.max(np.abs(want - lay.case.vl)))
    print("theta(z, t) after 20 steps of %.3g s at 130 x 128: %.3g of the field scale (the state moved by %.3g)" % (dt, err, moved))
    assert moved > 1e-6
    assert err <= STEP_BOUND[np.dtype(dtype)], err


# ------------------------------------------------------------ 8. status

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_poisoned_column_sets_the_status_and_stays_alone(dtype):
    """the top cell of column 40 is of a class with nu <= theta_r: a non-finite tendency, flagged by both engines"""
    classes = R.texture_classes()[:4].copy()
    sound = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64, 3), classes=classes)
    classes[3, 2], classes[3, 4] = 0.06, 0.05    # theta_r, nu
    m = sound.class_map.copy()
    bad = 40
    m[bad, -1] = 3
    lay = R.Layered(sound.case, classes, m)
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
        assert np.isfinite(dt) and dt > 0
        want, st_want = step(g, FUSED, dt, 5, engine=F.LH_ENGINE_FUSED_STAGES)
        got, st_got = step(g, STEPPER, dt, 5, engine=F.LH_ENGINE_COLUMN_STEPPER)
    assert st_want & 1 and st_got & 1 and st_got == st_want
    others = np.arange(67) != bad
    np.testing.assert_array_equal(got[others], want[others])
    assert np.all(np.isfinite(got[others]))
    assert not np.all(np.isfinite(got[bad])) and not np.all(np.isfinite(want[bad]))
    assert np.any(got[others] != lay.case.vl[others])


# ------------------------------------------------------------ 9. clay-like classes

def test_clay_like_classes_take_the_ldexp_form():
    """one class with m = 1 - 1/n < 0.07: the host chooses the v_ldexp form of the closures for the whole table"""
    classes = R.texture_classes().copy()
    classes[5, 0] = 1.06
    lay = R.make_layered(np.float64, 67, 64, R.horizon_map(67, 64), classes=classes)
    assert np.any(lay.class_map == 5)
    with layered_gpu(lay) as g:
        for tuning in (FUSED, STEPPER):
            g.F.check(g.L.lh_set_tuning(g.ctx, tuning), g.ctx)
            assert g.L.lh_closure_form(g.ctx) == g.F.LH_CLOSURE_LDEXP
    got, st, _ = both_engines(lay)
    assert st == 0 and np.all(np.isfinite(got))


# ------------------------------------------------------------ 10. the host mirror

def test_python_set_tuning_and_step_engine():
    lh = pc._pkg()
    FT = np.float64
    n, N = 48, 70
    classes = R.texture_classes()[[0, 5, 2]]
    horizons = np.zeros(n, dtype=np.int64)
    horizons[15:] = 1
    horizons[33:] = 2
    lay = R.make_layered(FT, N, n, np.repeat(horizons[None, :], N, axis=0), classes=classes, bc="flux_drain")
    om = lay.case.om
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3]), ν=k[4], S_s=k[5])
                         for k in classes], horizons)
    nsteps, ends = 6, {}
    for spec, engine in (("persist=0", lh._ffi.LH_ENGINE_FUSED_STAGES), ("persist=2", lh._ffi.LH_ENGINE_COLUMN_STEPPER)):
        dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-2e-8)),
                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage()))
        model = lh.SoilModel(FT, domain=dom, energy_model=lh.PrescribedTemperatureModel(),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT)),
                             boundary_conditions=bc, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet(),
                             soil_classes=sc)
        assert lh.step_engine(model, nsteps) == lh._ffi.LH_ENGINE_FUSED_STAGES      # the default tuning
        lh.set_tuning(model, spec)
        assert lh.step_engine(model, nsteps) == engine
        assert lh.step_engine(model, 1, per_stage_boundary_values=True) == engine
        Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z}, 0.0)
        Y.soil.ϑ_l = lay.case.vl
        dt = 0.5 * lh.stable_dt(model, Y, Ya)
        sim = lh.Simulation(model, lh.SSPRK33(), Y_init=Y, dt=dt, tspan=(0.0, nsteps * dt), Ya_init=Ya)
        lh.run(sim)
        assert lh.step_engine(model, nsteps) == engine
        ends[spec] = np.array(sim.integrator.u.soil.ϑ_l)
        model.close()
    np.testing.assert_array_equal(ends["persist=2"], ends["persist=0"])
    assert np.any(ends["persist=2"] != lay.case.vl)


# ------------------------------------------------------------ 11. nothing moved for others

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_context_without_a_map_is_untouched(dtype):
    """under persist=2 a context without a map takes the scalar stepper, before and after a map was set and removed"""
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet")
    with layered_gpu(lay) as g:     # (a step both parameter sets are stable with)
        dt_layered = stable_dt(g, *g.prognostic_and_aux(), 0.5)
    with pc.GpuModel(lay.case) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        dt = 0.5 * min(stable_dt(g, Y, Ya, 0.5), dt_layered)
        before, st0 = step(g, STEPPER, dt, 5, engine=F.LH_ENGINE_COLUMN_STEPPER)
        g.set_soil_classes(lay.classes, lay.class_map)
        layered, st1 = step(g, STEPPER, dt, 5, engine=F.LH_ENGINE_COLUMN_STEPPER)
        g.set_soil_class_map(None)
        after, st2 = step(g, STEPPER, dt, 5, engine=F.LH_ENGINE_COLUMN_STEPPER)
    np.testing.assert_array_equal(after, before)
    assert st0 == st1 == st2 == 0
    assert np.any(before != lay.case.vl) and np.any(layered != before)
