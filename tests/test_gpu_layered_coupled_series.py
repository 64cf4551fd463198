"""lh_integrate_layered_coupled_series / LayeredCoupledSeriesTRBDF2: the adaptive TR-BDF2 of the coupled model with soil
classes under a per-column boundary-value time series -- one launch for the chain of
lh_integrate_layered_coupled_trbdf2 calls, pinned BITWISE against that chain with tests/test_gpu_heat_series.py's
construction: sand over clay with thermal supplements, the interface at a level that differs from column to column,
series on the top hydrology value (a flux, a Dirichlet state), the top temperature and, in one case, both energy fluxes.

No case relies on failing columns: every chain asserts status bits 3 and 4 clear, so the comparisons cover all 130
columns."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc
from test_gpu_bc_series import KNOTS, NCOLS, NLEV, SAND_OVER_CLAY, SHAPE_H, SHIFT_E, T0, T1, _dptr, spread_steps
from test_gpu_heat_series import (BOTTOM_E, SHAPE_FLUX, TOP_E, TOP_H, _stats, assert_is_the_chain, assert_same_state, chain,
                                  check_per_column_arrays, make_series, percol_values, refused as _refused, series)
from test_gpu_layered_coupled_implicit import ATMOS, COUPLED_ONLY, FACTORS, LAYERED_OTHER_MODEL, PERCOL

pytestmark = pytest.mark.gpu
NAME, WRAPPED = "lh_integrate_layered_coupled_series", "lh_integrate_layered_coupled_trbdf2"
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TOPS = [M.BC_FLUX, M.BC_DIRICHLET]
TOP_IDS = ["flux", "dirichlet"]
BOTTOM_H = (M.FACE_BOTTOM, M.COMP_HYDROLOGY)
NO_CLASS_MAP = NAME + ": the context has no class map (lh_set_soil_class_map); lh_integrate_series steps a model without soil classes"


class LayeredCoupled:
    """test_gpu_heat_series.Heat for a layered coupled case (a layered_heat_ref.LayeredHeat)"""

    def __init__(self, lay):
        self.obj, self.case = lay, lay.case

    def open(self):
        gm = pc.GpuModel(self.case)
        gm.set_soil_classes(self.obj.classes, self.obj.class_map, thermal=self.obj.thermal)
        return gm

    def column(self, k):
        case1 = dataclasses.replace(pc._w.reorder_columns(self.case, np.array([k])), ncols=1)
        return LayeredCoupled(LH.LayeredHeat(case1, self.obj.classes, self.obj.thermal,
                                             np.ascontiguousarray(self.obj.class_map[k:k + 1])))

    def call_wrapped(self, gm, Y, Ya, a, b, dt, cols_ptr, bcv, abstol=0.0, abstol_e=0.0, reltol=0.0):
        return getattr(gm.L, WRAPPED)(gm.ctx, Y, Ya, a, b, dt, abstol, abstol_e, reltol, 0, cols_ptr, _dptr(bcv))

    def call_series(self, gm, Y, Ya, h, t0, t1, dt, cols_ptr, abstol=0.0, abstol_e=0.0, reltol=0.0):
        return getattr(gm.L, NAME)(gm.ctx, Y, Ya, h, t0, t1, dt, abstol, abstol_e, reltol, 0, cols_ptr)

    def state(self, gm, Y):
        return dict(vl=gm.download(Y, gm.F.LH_VAR_VARTHETA_L), rhoe=gm.download(Y, gm.F.LH_VAR_RHOE_INT))


@functools.lru_cache(maxsize=None)
def family(dtype, top, ncols=NCOLS, energy="dirichlet", ice=False, nlev=NLEV):
    """(LayeredCoupled, its stable step): sand over clay, the interface at a level that differs from column to column;
    `top`: the kind of the top hydrology boundary condition over a free-draining bottom; energy: "dirichlet" or "flux",
    both faces.  nlev 1 and 2 (no room for two horizons): layered_coupled_implicit_ref's "cells" case, a class per cell
    of five, with the same faces."""
    if nlev != NLEV:
        lay = LC.layered_case(dtype, ncols, nlev, kind="cells", hyd=(top, M.BC_FREE_DRAINAGE), energy=energy, ice=ice)
        return LayeredCoupled(lay), LC.stable_dt(lay)
    cut = 4 + (np.arange(ncols) % 5)
    cmap = (np.arange(NLEV)[None, :] < cut[:, None]).astype(np.uint8)     # bottom first: clay (1) below, sand (0) above
    lay = LH.make_layered_heat(dtype, ncols, NLEV, cmap, model=M.MODEL_COUPLED, classes=SAND_OVER_CLAY,
                               thermal=LH.thermal_classes()[:2], bc="flux" if energy == "flux" else "dirichlet", ice=ice,
                               name="layered_coupled_series")
    om = lay.case.om
    om.bc[TOP_H] = (top, 0.30 if top == M.BC_DIRICHLET else -2e-9)     # (layered_coupled_implicit_ref.layered_case's values)
    om.bc[BOTTOM_H] = (M.BC_FREE_DRAINAGE, 0.0)
    om.consistent_bottom_sign = False
    om.percol_bc = {}
    return LayeredCoupled(lay), LC.stable_dt(lay)


def uniform_values(fam, top):
    """{(face, component): [nknots]}: the top hydrology value and the top energy value (K on a Dirichlet top, multiples
    of the case's flux on a flux top)"""
    om = fam.case.om
    assert om.bc[TOP_H][0] == top
    vals = {TOP_H: om.bc[TOP_H][1] * SHAPE_H[top]}
    kind, v = om.bc[TOP_E]
    vals[TOP_E] = v + SHIFT_E if kind == M.BC_DIRICHLET else v * SHAPE_FLUX
    return vals


# ------------------------------------------------------------------ 1. a uniform series is the chain, bitwise

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
def test_uniform_series_is_the_chain_bitwise(top, dtype):
    fam, sd = family(dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(fam, top)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert len(want["per_call"]) == 4
    got = series(fam, T, values, t0, t1, sd, h0=h0)
    print(top, np.dtype(dtype).name, got["stats"], [p["max_steps"] for p in want["per_call"]])
    assert_is_the_chain(got, want, NCOLS)
    assert got["stats"]["newton_iterations"] > 0 and got["stats"]["unconverged"] == 0      # (slot 6 stays 0)
    # the series is read: the values at t0 held through the call give another state
    flat = {k: np.full_like(v, np.interp(t0, T, v)) for k, v in values.items()}
    other = series(fam, T, flat, t0, t1, sd, h0=h0)
    assert np.max(np.abs(other["vl"].astype(np.float64) - got["vl"])) > 0
    assert np.max(np.abs(other["rhoe"].astype(np.float64) - got["rhoe"])) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_knot_to_knot_inside_one_interval_and_an_empty_series(dtype):
    fam, sd = family(dtype, M.BC_DIRICHLET)
    T = KNOTS * sd
    values = uniform_values(fam, M.BC_DIRICHLET)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, T[1], T[3], sd, h0=h0)
    assert len(want["per_call"]) == 2
    assert_is_the_chain(series(fam, T, values, T[1], T[3], sd, h0=h0), want, NCOLS)
    want = chain(fam, T, values, 14.0 * sd, 22.5 * sd, sd, h0=h0)
    assert len(want["per_call"]) == 1
    got = series(fam, T, values, 14.0 * sd, 22.5 * sd, sd, h0=h0)
    assert_same_state(got, want)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    # an empty series over one knot interval: the single wrapped call with lh_set_bc's values at both ends
    want = chain(fam, T, {}, T[1], T[2], sd, h0=h0)
    got = series(fam, T, {}, T[1], T[2], sd, h0=h0)
    assert_same_state(got, want)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_null_dt_cols_is_a_chain_from_a_zeroed_buffer(dtype):
    fam, sd = family(dtype, M.BC_FLUX)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(fam, M.BC_FLUX)
    want = chain(fam, T, values, t0, t1, 0.5 * sd)
    got = series(fam, T, values, t0, t1, 0.5 * sd, null_cols=True, repeat=2)
    assert_is_the_chain(got, want, NCOLS, cols=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_flux_energy_faces_with_a_bottom_series(dtype):
    """both energy faces a flux, each with a series, beside the top hydrology flux: three series"""
    fam, sd = family(dtype, M.BC_FLUX, energy="flux")
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(fam, M.BC_FLUX)
    kind, v = fam.case.om.bc[BOTTOM_E]
    assert kind == M.BC_FLUX and fam.case.om.bc[TOP_E][0] == M.BC_FLUX
    values[BOTTOM_E] = v * SHAPE_FLUX[::-1]
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(series(fam, T, values, t0, t1, sd, h0=h0), want, NCOLS)


def test_ice_is_the_chain_bitwise():
    """theta_i in Ya is not zero: the !NOICE instantiation"""
    fam, sd = family(np.float64, M.BC_FLUX, ice=True)
    assert np.any(fam.case.ti != 0)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(fam, M.BC_FLUX)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(series(fam, T, values, t0, t1, sd, h0=h0), want, NCOLS)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2])
def test_one_and_two_levels(nlev, dtype):
    """both faces on one cell; no interior cell"""
    fam, sd = family(dtype, M.BC_FLUX, nlev=nlev)
    assert fam.case.om.nlev == nlev and fam.obj.class_map.shape == (NCOLS, nlev) and len(set(fam.obj.class_map.ravel())) > 1
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(fam, M.BC_FLUX)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert len(want["per_call"]) == 4
    got = series(fam, T, values, t0, t1, sd, h0=h0)
    print(nlev, np.dtype(dtype).name, got["stats"], [p["max_steps"] for p in want["per_call"]])
    assert_is_the_chain(got, want, NCOLS)
    assert np.max(np.abs(got["rhoe"].astype(np.float64) - fam.case.rhoe)) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_series_ignores_the_per_column_array_of_its_face_and_keeps_the_others(dtype):
    """Dirichlet top water and temperatures, each with an lh_set_bc per-column array; series on the two top faces"""
    fam, sd = family(dtype, M.BC_DIRICHLET)
    assert fam.case.om.bc[BOTTOM_E][0] == M.BC_DIRICHLET
    check_per_column_arrays(fam, sd, uniform_values(fam, M.BC_DIRICHLET), [BOTTOM_E])


# ------------------------------------------------------------------ 2. a per-column table

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
def test_per_column_table_against_one_column_contexts(top, dtype):
    fam, sd = family(dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = percol_values(uniform_values(fam, top), NCOLS)
    h0 = spread_steps(NCOLS, sd)
    got = series(fam, T, values, t0, t1, sd, h0=h0, layout="strided")
    assert got["stats"]["failed"] == 0 and got["status"] == 0
    for c in (0, 70, NCOLS - 1):      # the first column, one of the middle wave, the last
        mine = {k: v[:, c] for k, v in values.items()}
        one = fam.column(c)
        want = chain(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        alone = series(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        assert_same_state(alone, want)
        for key in ("vl", "rhoe"):
            np.testing.assert_array_equal(got[key][c], alone[key][0])
        assert got["cols"][c] == alone["cols"][0]
        steps = want["stats"]["accepted"] + want["stats"]["rejected"]
        assert alone["stats"]["max_steps"] == steps and alone["stats"]["wave_steps"] == 64 * steps, (alone["stats"], steps)
    # the same values through a uniform and a per-column table
    uniform = uniform_values(fam, top)
    table = {k: np.repeat(v[:, None], NCOLS, axis=1) for k, v in uniform.items()}
    a, b = series(fam, T, uniform, t0, t1, sd, h0=h0), series(fam, T, table, t0, t1, sd, h0=h0, layout="transposed")
    assert_same_state(b, a)
    assert a["stats"] == b["stats"]


# ------------------------------------------------------------------ 3. refusals and the contract

def refused(gm, rc, code, *words):
    _refused(gm, rc, code, *words, name=NAME)


def test_refusals_and_the_contract():
    fam, sd = family(np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    vals = uniform_values(fam, M.BC_FLUX)
    nan = float("nan")
    with fam.open() as gm, fam.open() as other:
        F, L = gm.F, gm.L
        EINVAL, EMODEL = F.LH_EINVAL, F.LH_EMODEL
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)

        def call(series_h=h, t0=T0 * sd, t1=T1 * sd, dt=sd, abstol=0.0, abstol_e=0.0, reltol=0.0, flags=0, Y=Y, Ya=Ya):
            return getattr(L, NAME)(gm.ctx, Y, Ya, series_h, t0, t1, dt, abstol, abstol_e, reltol, flags, None)

        def ran():   # a run first, so that the statistics are not zero before a refusal
            F.check(call(), gm.ctx)
            assert _stats(gm)["accepted"] >= 67

        ran()
        # ---- the wrapped call's argument checks, in its words
        refused(gm, call(t0=2.0 * sd, t1=1.0 * sd), EINVAL, ": need finite t0 <= t1")
        refused(gm, call(dt=0.0), EINVAL, ": need a finite dt > 0")
        for kw in (dict(abstol=-1e-6), dict(abstol_e=nan), dict(reltol=-1.0)):
            refused(gm, call(**kw), EINVAL, ": tolerances must be finite and >= 0")
        refused(gm, call(flags=1), EINVAL, ": unknown flags 0x1")
        assert getattr(L, NAME)(None, Y, Ya, h, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None) == EINVAL
        ran()
        assert call(Y=None, series_h=None) == F.LH_ESTATE and all(v == 0 for v in _stats(gm).values())   # the states before the series
        # ---- the series' own checks
        ran()
        refused(gm, call(series_h=None), EINVAL, "the series is NULL")
        refused(gm, call(series_h=make_series(other, T, vals)), EINVAL, "not a series of this context")
        refused(gm, call(t0=-0.5 * sd), EINVAL, "no extrapolation")
        refused(gm, call(t1=T[-1] + 0.5 * sd), EINVAL, "no extrapolation")
        ran()
        v0 = np.ascontiguousarray(vals[TOP_H])
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)   # free drainage
        refused(gm, call(), EMODEL, "bottom hydrology", "reads no value")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        # ---- t0 == t1 does nothing and reports zeros
        ran()
        before = gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT)
        F.check(call(t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), before[0])
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before[1])
        assert all(v == 0 for v in _stats(gm).values()) and gm.status() == 0
        # ---- what lh_integrate_layered_coupled_trbdf2 refuses, in its order and words: a prescribed atmosphere, per-column
        # parameter arrays, conductivity factors -- each before the series is looked at
        a = M.AtmosForcing()
        f = F.lh_atmos_forcing(a.u_atm, a.theta_atm, a.z_atm, a.theta_scale, a.rho_a_sfc, a.q_atm, 0.001, 0.001, a.R_v, a.R_d,
                               a.grav, a.cp_d, a.cp_v, a.LH_v0, a.T_triple, a.press_triple, a.von_karman)
        nu = np.full(67, 0.45)
        cf = M.default_cf(impedance=True)
        F.check(L.lh_set_atmos_forcing(gm.ctx, C.byref(f), None), gm.ctx)
        F.check(L.lh_set_percol_param(gm.ctx, F.LH_PC["nu"], _dptr(nu)), gm.ctx)
        F.check(L.lh_set_conductivity_factors(gm.ctx, cf.viscosity_kind, cf.gamma, cf.T_ref, cf.impedance_kind, cf.Omega), gm.ctx)
        refused(gm, call(series_h=None), EMODEL)
        assert L.lh_last_error(gm.ctx).decode() == NAME + ATMOS
        F.check(L.lh_set_atmos_forcing(gm.ctx, None, None), gm.ctx)
        refused(gm, call(series_h=None), EMODEL)
        assert L.lh_last_error(gm.ctx).decode() == NAME + PERCOL
        F.check(L.lh_set_percol_param(gm.ctx, F.LH_PC["nu"], None), gm.ctx)
        refused(gm, call(series_h=None), EMODEL)
        assert L.lh_last_error(gm.ctx).decode() == NAME + FACTORS
    # ---- a coupled context without a map is lh_integrate_series'
    with pc.GpuModel(fam.case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)
        rc = getattr(gm.L, NAME)(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None)
        refused(gm, rc, gm.F.LH_EMODEL)
        assert gm.L.lh_last_error(gm.ctx).decode() == NO_CLASS_MAP
        gm.F.check(gm.L.lh_integrate_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None), gm.ctx)   # ... which integrates it
        assert gm.status() == 0
    # ---- and a context WITH one stays refused there
    with fam.open() as gm:
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)
        assert gm.L.lh_integrate_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None) == gm.F.LH_EMODEL
        assert "soil classes" in gm.L.lh_last_error(gm.ctx).decode()
    # ---- a Richards context, with and without a map
    rich = R.make_layered(np.float64, 5, 6, R.uniform_map(5, 6, 2), classes=R.texture_classes()[:2])
    for with_map, words in ((True, LAYERED_OTHER_MODEL), (False, COUPLED_ONLY)):
        with pc.GpuModel(rich.case) as gm:
            if with_map:
                gm.set_soil_classes(rich.classes, rich.class_map)
            Y, Ya = gm.prognostic_and_aux()
            h = make_series(gm, T, {})
            refused(gm, getattr(gm.L, NAME)(gm.ctx, Y, Ya, h, T[0], T[1], 0.0, 0.0, 0.0, 0.0, 0, None), gm.F.LH_EINVAL, "dt > 0")
            refused(gm, getattr(gm.L, NAME)(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None), gm.F.LH_EMODEL)
            assert gm.L.lh_last_error(gm.ctx).decode() == NAME + words


# ------------------------------------------------------------------ 4. the host mirror

def test_host_mirror():
    """Simulation(model, LayeredCoupledSeriesTRBDF2(forcing=fs)) over the whole series is one
    integrate_layered_coupled_series call, in state and statistics; that call is the ctypes call."""
    from test_gpu_layered_coupled_trbdf2 import horizon_model
    lh = pc._pkg()
    N = 5
    lay = LC.layered_case(np.float64, N, NLEV, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    case = lay.case
    fw = -2e-9
    model, dom, bc = horizon_model(lh, lay, lambda t: 287.0, 281.0, fw)
    ic = lambda z, m: {"ϑ_l": 0.2 + 0.0 * z, "θ_i": 0.0 * z, "ρe_int": 1e7 + 0.0 * z}
    states = [lh.initialize_states(model, ic, 0.0) for _ in range(3)]
    for Y, _ in states:
        Y.soil.ϑ_l, Y.soil.ρe_int = case.vl, case.rhoe
    (Y1, Ya), (Y2, _), (Y3, _) = states
    sd = LC.stable_dt(lay)
    T = KNOTS * sd
    u = pc.uhash(np.arange(N), 3, 1)
    fs = lh.BoundarySeries(T, {("top", "hydrology"): fw * SHAPE_H[M.BC_FLUX][:, None] * (0.8 + 0.4 * u)[None, :],
                               ("top", "energy"): 287.0 + SHIFT_E})
    sim = lh.Simulation(model, lh.LayeredCoupledSeriesTRBDF2(forcing=fs, reltol=1e-4), Y_init=Y1, dt=sd, tspan=(T[0], T[-1]),
                        Ya_init=Ya)
    lh.run(sim)
    want = lh.integrate_layered_coupled_series(model, Y2, Ya, fs, T[0], T[-1], sd, reltol=1e-4)
    for name in ("ϑ_l", "ρe_int"):
        np.testing.assert_array_equal(Y1.get(name), Y2.get(name))
    assert sim.integrator.trbdf2_stats == want, (sim.integrator.trbdf2_stats, want)
    assert sim.integrator.t == T[-1] and want["failed"] == 0 and want["accepted"] >= 4 * N
    assert np.max(np.abs(Y2.get("ρe_int") - case.rhoe)) > 0 and np.max(np.abs(Y2.get("ϑ_l") - case.vl)) > 0
    # the ctypes call on the same context, a series of its own
    F = lh._ffi
    L, be = F.lib(), model._backend()
    h = C.c_void_p()
    Tc = np.ascontiguousarray(T)
    a, e = np.ascontiguousarray(fs.values[(M.FACE_TOP, M.COMP_HYDROLOGY)]), np.ascontiguousarray(fs.values[(M.FACE_TOP, M.COMP_ENERGY)])
    F.check(L.lh_bc_series_create(be.ctx, 5, _dptr(Tc), C.byref(h)), be.ctx)
    F.check(L.lh_bc_series_set(be.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(a), N, 1), be.ctx)
    F.check(L.lh_bc_series_set(be.ctx, h, M.FACE_TOP, M.COMP_ENERGY, _dptr(e), 1, 0), be.ctx)
    F.check(getattr(L, NAME)(be.ctx, Y3.handle, getattr(Ya, "handle", None), h, T[0], T[-1], sd, 1e-6, 0.0, 1e-4, 0, None), be.ctx)
    for name in ("ϑ_l", "ρe_int"):
        np.testing.assert_array_equal(Y3.get(name), Y2.get(name))
    with pytest.raises(ValueError):
        lh.integrate_layered_coupled_series(model, Y1, Ya, fs, T[0] - 1.0, T[1], sd)
    # the marker refuses a model without classes when the Simulation is built, pointing to lh_integrate_coupled_trbdf2 as
    # its parent does; the function names the call that serves such a model
    plain = lh.SoilModel(np.float64, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(np.float64),
                         boundary_conditions=bc, domain=dom, earth_param_set=lh.EarthParameterSet())
    with pytest.raises(NotImplementedError, match="LayeredCoupledSeriesTRBDF2: the context has no class map"):
        lh.Simulation(plain, lh.LayeredCoupledSeriesTRBDF2(forcing=fs), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
    with pytest.raises(NotImplementedError, match="lh_integrate_series steps a model without soil classes"):
        lh.integrate_layered_coupled_series(plain, object(), None, fs, T[0], T[1], sd)
    model.close()
