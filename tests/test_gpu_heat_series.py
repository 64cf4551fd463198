"""lh_integrate_heat_series / HeatSeriesTRBDF2 / LayeredHeatSeriesTRBDF2: the adaptive TR-BDF2 of the heat-only model,
without and with a class map, under a per-column boundary-value time series -- one launch for the chain of
lh_integrate_heat_trbdf2 / lh_integrate_layered_heat_trbdf2 calls the host would make, pinned BITWISE against that
chain (tests/test_gpu_bc_series.py's construction), on its energy budget, its refusals and its host mirror.

No case relies on failing columns: every chain asserts status bits 3 and 4 clear, so the bitwise comparisons cover all
130 columns.

One refusal the series' own checks hold cannot be reached on a heat-only context: a series on a face whose kind reads
no value.  A heat-only context has two energy faces, each must be a flux or a Dirichlet face (the model's validation,
which every stepping call runs first), and its hydrology series are refused as such.  That check is exercised where it
can fire, in tests/test_gpu_layered_coupled_series.py (a free-draining bottom); here the call on such a context is
held to LH_EMODEL and zeroed statistics."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import heat_implicit_ref as H
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc
from test_gpu_bc_series import (KEYS, KNOTS, NCOLS, NLEV, SHIFT_E, T0, T1, _dptr, _step_buffer, assert_counters,
                                breakpoints, series_value, spread_steps)

pytestmark = pytest.mark.gpu
NAME = "lh_integrate_heat_series"
STATUS_UNCONVERGED, STATUS_FAILED = 8, 16
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
KINDS = ["scalar", "layered"]
TOPS = [M.BC_FLUX, M.BC_DIRICHLET]
TOP_IDS = ["flux", "dirichlet"]
TOP_E, BOTTOM_E = (M.FACE_TOP, M.COMP_ENERGY), (M.FACE_BOTTOM, M.COMP_ENERGY)
TOP_H = (M.FACE_TOP, M.COMP_HYDROLOGY)
SHAPE_FLUX = np.array([1.0, 3.0, 0.5, 2.0, 1.5])     # multiples of the case's own flux at the five knots


# ------------------------------------------------------------------ the two families

class Heat:
    """What the chain and the series call need of a heat-only case: `obj` is a parity_cases.Case (no class map) or a
    layered_heat_ref.LayeredHeat (with one)."""
    series_name = NAME

    def __init__(self, obj, math_mode=None):
        self.obj, self.math_mode = obj, math_mode
        self.layered = isinstance(obj, LH.LayeredHeat)
        self.case = obj.case if self.layered else obj
        self.wrapped = "lh_integrate_layered_heat_trbdf2" if self.layered else "lh_integrate_heat_trbdf2"

    def open(self):
        gm = pc.GpuModel(self.case, self.math_mode)
        if self.layered:
            gm.set_soil_classes(self.obj.classes, self.obj.class_map, thermal=self.obj.thermal)
        return gm

    def column(self, k):
        case1 = dataclasses.replace(pc._w.reorder_columns(self.case, np.array([k])), ncols=1)
        if not self.layered:
            return Heat(case1, self.math_mode)
        return Heat(LH.LayeredHeat(case1, self.obj.classes, self.obj.thermal, np.ascontiguousarray(self.obj.class_map[k:k + 1])))

    def call_wrapped(self, gm, Y, Ya, a, b, dt, cols_ptr, bcv, abstol_e=0.0, reltol=0.0):
        return getattr(gm.L, self.wrapped)(gm.ctx, Y, Ya, a, b, dt, abstol_e, reltol, 0, cols_ptr, _dptr(bcv))

    def call_series(self, gm, Y, Ya, h, t0, t1, dt, cols_ptr, abstol_e=0.0, reltol=0.0):
        return gm.L.lh_integrate_heat_series(gm.ctx, Y, Ya, h, t0, t1, dt, abstol_e, reltol, 0, cols_ptr)

    def state(self, gm, Y):
        return dict(rhoe=gm.download(Y, gm.F.LH_VAR_RHOE_INT))

    def stable_dt(self):
        return LI.stable_dt(self.obj) if self.layered else H.stable_dt(self.case)


def horizon_map(ncols, nlev):
    """three horizons, both interfaces at a level that differs from column to column"""
    c, lev = np.arange(ncols)[:, None], np.arange(nlev)[None, :]
    return ((lev >= nlev * 5 // 16 + c % 3).astype(np.uint8) + (lev >= nlev * 11 // 16 + c % 4).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def family(kind, dtype, top, ncols=NCOLS, nlev=NLEV, bottom=M.BC_DIRICHLET, ice=False, variant=None):
    """(Heat, its stable step).  variant: None, "percol" (a porosity per column) or "libm"; scalar cases only."""
    if kind == "layered":
        lay = LH.make_layered_heat(dtype, ncols, nlev, horizon_map(ncols, nlev), model=M.MODEL_HEAT,
                                   classes=R.texture_classes()[[0, 5, 2]], thermal=LH.thermal_classes()[[0, 4, 2]],
                                   bc="flux" if bottom == M.BC_FLUX else "dirichlet", ice=ice, name="heat_series")
        if top == M.BC_FLUX:
            lay.case.om.bc[TOP_E] = LI.FLUX_TOP
        elif bottom == M.BC_FLUX:
            lay.case.om.bc[TOP_E] = LH.ENERGY_BC["dirichlet"][1]
        fam = Heat(lay)
    else:
        case = H.heat_case(ncols, nlev, dtype, bottom=bottom, top=top, ice=ice)
        if variant == "percol":
            nu = case.om.soil.nu * (1.0 + 0.1 * pc.uhash(np.arange(ncols), 31, 1))
            case = dataclasses.replace(case, om=dataclasses.replace(case.om, percol={"nu": nu.astype(dtype).astype(np.float64)}))
        fam = Heat(case, math_mode=1 if variant == "libm" else None)
    return fam, fam.stable_dt()


def top_values(fam, top):
    """{(face, component): [nknots]}: multiples of the case's top flux, or its Dirichlet top temperature shifted by K"""
    kind, v = fam.case.om.bc[TOP_E]
    assert kind == top
    return {TOP_E: v * SHAPE_FLUX if top == M.BC_FLUX else v + SHIFT_E}


# ------------------------------------------------------------------ the two ways to integrate

def _stats(gm):
    st = (C.c_int64 * gm.F.LH_TRBDF2_NSTATS)(*([7] * gm.F.LH_TRBDF2_NSTATS))
    gm.F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    return dict(zip(KEYS, list(st)))


def _result(fam, gm, Y, cols, stats, **more):
    return dict(stats=stats, status=gm.status(), cols=None if cols is None else cols.cpu().numpy().astype(np.float64),
                **fam.state(gm, Y), **more)


def chain(fam, T, values, t0, t1, dt, h0=None, ends=None, **tols):
    """The chain of calls the host makes today: the wrapped entry point once per sub-interval, dt_cols carried, bcv =
    lh_set_bc's values with the series' own at both ends (`values`: {(face, comp): [nknots]}, one column's).  No
    column may fail: the comparisons against it cover every column."""
    with fam.open() as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        cols = _step_buffer(fam.case, h0)
        base = np.zeros((2, 2, 2))
        for (f, k), (_, v) in fam.case.om.bc.items():
            base[:, f, k] = v
        total = dict.fromkeys(KEYS, 0)
        per_call = []
        bp = breakpoints(T, t0, t1) if ends is None else ends
        for a, b in zip(bp, bp[1:]):
            bcv = base.copy()
            for (f, k), v in values.items():
                bcv[0, f, k] = series_value(T, v, a)
                bcv[1, f, k] = series_value(T, v, b)
            F.check(fam.call_wrapped(gm, Y, Ya, a, b, dt, C.c_void_p(cols.data_ptr()), bcv, **tols), gm.ctx)
            st = _stats(gm)
            per_call.append(st)
            for key in KEYS:
                total[key] += st[key]
        out = _result(fam, gm, Y, cols, total, per_call=per_call)
    assert out["stats"]["failed"] == 0 and not out["status"] & (STATUS_UNCONVERGED | STATUS_FAILED), (out["status"], out["stats"])
    assert np.all(out["cols"] > 0)
    return out


def make_series(gm, T, values, layout="plain"):
    """An lh_bc_series of the context: [nknots] values are uniform, [nknots, ncols] per-column.  layout: "plain"
    (C order), "transposed" (stored [ncols, nknots]) or "strided" (a view into a larger array: a column stride of 2
    and a knot stride of 2 ncols + 3, both non-trivial)."""
    F = gm.F
    T = np.ascontiguousarray(T, dtype=np.float64)
    h = C.c_void_p()
    F.check(gm.L.lh_bc_series_create(gm.ctx, len(T), _dptr(T), C.byref(h)), gm.ctx)
    for (f, k), v in values.items():
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 1:
            a, ks, cs = np.ascontiguousarray(v), 1, 0
        elif layout == "transposed":
            a, ks, cs = np.ascontiguousarray(v.T), 1, v.shape[0]
        elif layout == "strided":
            ks, cs = 2 * v.shape[1] + 3, 2
            a = np.full(v.shape[0] * ks, np.nan)        # (a value read from a gap would show)
            for j in range(v.shape[0]):
                a[j * ks:j * ks + cs * v.shape[1]:cs] = v[j]
        else:
            a, ks, cs = np.ascontiguousarray(v), v.shape[1], 1
        F.check(gm.L.lh_bc_series_set(gm.ctx, h, f, k, _dptr(a), ks, cs), gm.ctx)   # (the call copies the values)
    return h


def series(fam, T, values, t0, t1, dt, h0=None, null_cols=False, layout="plain", repeat=1, **tols):
    """One series call (repeat > 1: again on the same context from the same state, which must give the same bits)."""
    with fam.open() as gm:
        F = gm.F
        h = make_series(gm, T, values, layout)
        out = None
        for _ in range(repeat):
            Y, Ya = gm.prognostic_and_aux()
            cols = None if null_cols else _step_buffer(fam.case, h0)
            F.check(fam.call_series(gm, Y, Ya, h, t0, t1, dt, None if cols is None else C.c_void_p(cols.data_ptr()), **tols), gm.ctx)
            got = _result(fam, gm, Y, cols, _stats(gm))
            if out is not None:
                assert_same_state(got, out, cols=not null_cols)
                assert got["stats"] == out["stats"]
            out = got
        F.check(gm.L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        return out


def assert_same_state(got, want, cols=True):
    for key in ("rhoe", "vl"):
        if key in want:
            np.testing.assert_array_equal(got[key], want[key])
    if cols:
        np.testing.assert_array_equal(got["cols"], want["cols"])
    assert got["status"] == want["status"], (got["status"], want["status"])


def assert_is_the_chain(got, want, ncols, cols=True):
    assert_same_state(got, want, cols)
    assert_counters(got, want, ncols)      # accepted, rejected, failed (and the zeros) summed; max_steps, wave_steps bounded
    assert got["stats"]["newton_iterations"] == want["stats"]["newton_iterations"]


# ------------------------------------------------------------------ 1. a uniform series is the chain, bitwise

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_uniform_series_is_the_chain_bitwise(kind, top, dtype):
    """t0 inside the first knot interval, t1 inside the last: four sub-intervals, initial steps spread over a factor of
    100 within each wave."""
    fam, sd = family(kind, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, top)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert len(want["per_call"]) == 4
    got = series(fam, T, values, t0, t1, sd, h0=h0)
    print(kind, top, np.dtype(dtype).name, got["stats"], [p["max_steps"] for p in want["per_call"]])
    assert_is_the_chain(got, want, NCOLS)
    assert got["stats"]["newton_iterations"] == 0 and got["stats"]["unconverged"] == 0      # slots 2 and 6
    # the series is read: the value at t0 held through the call gives another state
    flat = {k: np.full_like(v, series_value(T, v, t0)) for k, v in values.items()}
    other = series(fam, T, flat, t0, t1, sd, h0=h0)
    assert np.max(np.abs(other["rhoe"].astype(np.float64) - got["rhoe"])) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_knot_to_knot_and_inside_one_interval(kind, dtype):
    fam, sd = family(kind, dtype, M.BC_DIRICHLET)
    T = KNOTS * sd
    values = top_values(fam, M.BC_DIRICHLET)
    h0 = spread_steps(NCOLS, sd)
    # from a knot to a knot: two sub-intervals, every boundary value a knot's own
    want = chain(fam, T, values, T[1], T[3], sd, h0=h0)
    assert len(want["per_call"]) == 2
    assert_is_the_chain(series(fam, T, values, T[1], T[3], sd, h0=h0), want, NCOLS)
    # inside one knot interval: one sub-interval, the single wrapped call with the interpolated values at its ends
    want = chain(fam, T, values, 14.0 * sd, 22.5 * sd, sd, h0=h0)
    assert len(want["per_call"]) == 1
    got = series(fam, T, values, 14.0 * sd, 22.5 * sd, sd, h0=h0)
    assert_same_state(got, want)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_series_is_the_single_wrapped_call(kind, dtype):
    """No (face, component) has a series: over one knot interval the call is bitwise the wrapped call with bcv = NULL."""
    fam, sd = family(kind, dtype, M.BC_FLUX)
    T = KNOTS * sd
    h0 = spread_steps(NCOLS, sd)
    got = series(fam, T, {}, T[1], T[2], sd, h0=h0)
    with fam.open() as gm:
        Y, Ya = gm.prognostic_and_aux()
        cols = _step_buffer(fam.case, h0)
        gm.F.check(fam.call_wrapped(gm, Y, Ya, T[1], T[2], sd, C.c_void_p(cols.data_ptr()), None), gm.ctx)
        want = _result(fam, gm, Y, cols, _stats(gm))
    assert want["stats"]["failed"] == 0 and want["status"] == 0
    assert_same_state(got, want)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_null_dt_cols_is_a_chain_from_a_zeroed_buffer(kind, dtype):
    fam, sd = family(kind, dtype, M.BC_FLUX)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, M.BC_FLUX)
    want = chain(fam, T, values, t0, t1, 0.5 * sd)
    # ... twice in one context: the library's buffer is zeroed for every call
    got = series(fam, T, values, t0, t1, 0.5 * sd, null_cols=True, repeat=2)
    assert_is_the_chain(got, want, NCOLS, cols=False)


@pytest.mark.parametrize("nlev", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_one_and_two_levels(kind, nlev):
    """both faces on one cell; no interior cell"""
    fam, sd = family(kind, np.float64, M.BC_FLUX, nlev=nlev)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, M.BC_FLUX)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(series(fam, T, values, t0, t1, sd, h0=h0), want, NCOLS)


# ------------------------------------------------------------------ 2. per-column tables

def percol_values(values, ncols):
    """[nknots, ncols]: every column its own multiple (a flux) or shift (a temperature) of the uniform series, per knot"""
    c = np.arange(ncols)
    out = {}
    for (f, k), v in values.items():
        u = np.stack([pc.uhash(c, 200 + 10 * j + f, 1) for j in range(len(v))])          # [nknots, ncols] in [0, 1)
        out[(f, k)] = v[:, None] * (0.8 + 0.4 * u) if np.max(np.abs(v)) < 100.0 else v[:, None] + 4.0 * (u - 0.5)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_per_column_table_against_one_column_contexts(kind, top, dtype):
    """A [nknots, ncols] table with both strides non-trivial: three columns are bitwise their one-column contexts under
    a uniform series of that column's values (and those the one-column chain, whose attempted steps are exact)."""
    fam, sd = family(kind, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = percol_values(top_values(fam, top), NCOLS)
    h0 = spread_steps(NCOLS, sd)
    got = series(fam, T, values, t0, t1, sd, h0=h0, layout="strided")
    assert got["stats"]["failed"] == 0 and got["status"] == 0
    most = 0
    for c in (0, 70, NCOLS - 1):      # the first column, one of the middle wave, the last
        mine = {k: v[:, c] for k, v in values.items()}
        one = fam.column(c)
        alone = series(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        np.testing.assert_array_equal(got["rhoe"][c], alone["rhoe"][0])
        assert got["cols"][c] == alone["cols"][0]
        want = chain(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        assert_same_state(alone, want)
        steps = want["stats"]["accepted"] + want["stats"]["rejected"]
        assert alone["stats"]["max_steps"] == steps and alone["stats"]["wave_steps"] == 64 * steps, (alone["stats"], steps)
        most = max(most, steps)
    assert got["stats"]["max_steps"] >= most


@pytest.mark.parametrize("layout", ["plain", "transposed", "strided"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_same_values_through_a_uniform_and_a_per_column_table(kind, layout):
    fam, sd = family(kind, np.float64, M.BC_DIRICHLET)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, M.BC_DIRICHLET)
    h0 = spread_steps(NCOLS, sd)
    want = series(fam, T, values, t0, t1, sd, h0=h0)
    table = {k: np.repeat(v[:, None], NCOLS, axis=1) for k, v in values.items()}
    got = series(fam, T, table, t0, t1, sd, h0=h0, layout=layout)
    assert_same_state(got, want)
    assert got["stats"] == want["stats"]


# ------------------------------------------------------------------ 2b. lh_set_bc's per-column arrays

def with_arrays(fam, keys, spread=None):
    """`fam` with an lh_set_bc per-column array on the faces `keys` (every Dirichlet (face, component) of the case:
    its value shifted per column, rounded to the working type)"""
    om, c = fam.case.om, np.arange(fam.case.ncols)
    spread = spread or {M.COMP_ENERGY: 2.0, M.COMP_HYDROLOGY: 0.02}
    arrays = {}
    for k in keys:
        kind, v = om.bc[k]
        assert kind == M.BC_DIRICHLET
        arrays[k] = (v + spread[k[1]] * (pc.uhash(c, 77 + 2 * k[0] + k[1], 1) - 0.5)).astype(fam.case.dtype).astype(np.float64)
    case = dataclasses.replace(fam.case, om=dataclasses.replace(om, percol_bc=arrays))
    if isinstance(fam, Heat):
        return Heat(LH.LayeredHeat(case, fam.obj.classes, fam.obj.thermal, fam.obj.class_map) if fam.layered else case, fam.math_mode)
    return type(fam)(LH.LayeredHeat(case, fam.obj.classes, fam.obj.thermal, fam.obj.class_map))


def check_per_column_arrays(fam, sd, values, kept):
    """Arrays on the series' faces AND on the faces `kept`, which have no series: a series ignores lh_set_bc's array on
    its own face, a face without a series keeps its array.  So the call is bitwise the chain on a context that holds
    the arrays of `kept` alone (where the wrapped call's bcv cannot be overridden on the series' faces), and differs
    from the call on a context without any array."""
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    h0 = spread_steps(NCOLS, sd)
    want = chain(with_arrays(fam, kept), T, values, t0, t1, sd, h0=h0)
    got = series(with_arrays(fam, list(values) + list(kept)), T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(got, want, NCOLS)
    plain = series(fam, T, values, t0, t1, sd, h0=h0)
    assert np.max(np.abs(plain["rhoe"].astype(np.float64) - got["rhoe"])) > 0      # (the kept arrays are in force)
    # ... and without the series the array on its face is in force again: another state
    none = series(with_arrays(fam, list(values) + list(kept)), T, {}, t0, t1, sd, h0=h0)
    assert np.max(np.abs(none["rhoe"].astype(np.float64) - got["rhoe"])) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_series_ignores_the_per_column_array_of_its_face_and_keeps_the_others(kind, dtype):
    fam, sd = family(kind, dtype, M.BC_DIRICHLET)
    assert fam.case.om.bc[BOTTOM_E][0] == M.BC_DIRICHLET
    check_per_column_arrays(fam, sd, top_values(fam, M.BC_DIRICHLET), [BOTTOM_E])


# ------------------------------------------------------------------ 3. the scalar kernel's variants

@pytest.mark.parametrize("variant", ["ice", "percol", "libm"])
def test_scalar_variants_are_the_chain_bitwise(variant):
    """static ice in every other column; a porosity per column (the PERCOL instantiation); libm math"""
    fam, sd = family("scalar", np.float64, M.BC_DIRICHLET, ice=True, variant=None if variant == "ice" else variant)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, M.BC_DIRICHLET)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(series(fam, T, values, t0, t1, sd, h0=h0), want, NCOLS)


def test_layered_ice_is_the_chain_bitwise():
    fam, sd = family("layered", np.float64, M.BC_FLUX, ice=True)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = top_values(fam, M.BC_FLUX)
    h0 = spread_steps(NCOLS, sd)
    want = chain(fam, T, values, t0, t1, sd, h0=h0)
    assert_is_the_chain(series(fam, T, values, t0, t1, sd, h0=h0), want, NCOLS)


# ------------------------------------------------------------------ 4. the energy budget

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_energy_budget_under_two_flux_series(kind, dtype):
    """Flux faces top and bottom, each with a per-column series: sum_i rhoe_int changes by the trapezoid integral over
    the breakpoints of (F_bottom - F_top) / dz, however a column chose its steps -- tests/test_heat_series_cpu.py's
    identity with its bound, nlev 4 eps sum |rhoe_int| (tests/test_gpu_heat_trbdf2.py::test_conservation_with_flux_faces)."""
    fam, sd = family(kind, dtype, M.BC_FLUX, bottom=M.BC_FLUX, ice=True)
    om = fam.case.om
    assert om.bc[TOP_E][0] == M.BC_FLUX and om.bc[BOTTOM_E][0] == M.BC_FLUX
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = percol_values({TOP_E: om.bc[TOP_E][1] * SHAPE_FLUX, BOTTOM_E: om.bc[BOTTOM_E][1] * SHAPE_FLUX[::-1]}, NCOLS)
    got = series(fam, T, values, t0, t1, sd, h0=spread_steps(NCOLS, sd))
    assert got["status"] == 0 and got["stats"]["failed"] == 0
    bp = breakpoints(T, t0, t1)
    net = lambda t: (np.array([series_value(T, values[BOTTOM_E][:, c], t) for c in range(NCOLS)])
                     - np.array([series_value(T, values[TOP_E][:, c], t) for c in range(NCOLS)]))
    integral = sum(0.5 * (b - a) * (net(a) + net(b)) for a, b in zip(bp, bp[1:]))
    dz = (om.zmax - om.zmin) / om.nlev
    re = fam.case.rhoe.astype(np.float64)
    change = got["rhoe"].astype(np.float64).sum(axis=1) - re.sum(axis=1)
    want = integral / dz
    allowed = om.nlev * 4 * float(np.finfo(dtype).eps) * np.abs(re).sum(axis=1)
    print(f"series budget {kind} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, "
          f"expected change {np.min(want):.3g} .. {np.max(want):.3g}, steps per column {got['stats']['accepted'] / NCOLS:.1f}")
    assert np.all(np.abs(want) > 0)
    assert np.all(np.abs(change - want) <= allowed), float(np.max(np.abs(change - want) / allowed))


# ------------------------------------------------------------------ 5. refusals and the contract

def refused(gm, rc, code, *words, name=NAME):
    msg = gm.L.lh_last_error(gm.ctx).decode()
    assert rc == code, (rc, code, msg)
    for w in (name,) + words:
        assert w in msg, (w, msg)
    assert all(v == 0 for v in _stats(gm).values()), "statistics after a refused call"


HEAT_ONLY = NAME + ": heat-only models (SoilEnergyModel + PrescribedHydrologyModel)"


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_the_contract(kind):
    fam, sd = family(kind, np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    vals = top_values(fam, M.BC_FLUX)
    nan, inf = float("nan"), float("inf")
    with fam.open() as gm, fam.open() as other:
        F, L = gm.F, gm.L
        EINVAL, EMODEL = F.LH_EINVAL, F.LH_EMODEL
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)

        def call(series_h=h, t0=T0 * sd, t1=T1 * sd, dt=sd, abstol_e=0.0, reltol=0.0, flags=0, Y=Y, Ya=Ya):
            return L.lh_integrate_heat_series(gm.ctx, Y, Ya, series_h, t0, t1, dt, abstol_e, reltol, flags, None)

        def ran():   # a run first, so that the statistics are not zero before a refusal
            F.check(call(), gm.ctx)
            assert _stats(gm)["accepted"] >= 67

        ran()
        first = gm.download(Y, F.LH_VAR_RHOE_INT)
        # ---- the wrapped call's argument checks, in its words
        refused(gm, call(t0=2.0 * sd, t1=1.0 * sd), EINVAL, ": need finite t0 <= t1")
        ran()
        refused(gm, call(t1=nan), EINVAL, ": need finite t0 <= t1")
        for dt in (0.0, -1.0, nan, inf):
            refused(gm, call(dt=dt), EINVAL, ": need a finite dt > 0")
        for bad in (-1e-6, nan, inf):
            refused(gm, call(abstol_e=bad), EINVAL, ": tolerances must be finite and >= 0")
            refused(gm, call(reltol=bad), EINVAL, ": tolerances must be finite and >= 0")
        ran()
        refused(gm, call(flags=1), EINVAL, ": unknown flags 0x1")
        assert L.lh_integrate_heat_series(None, Y, Ya, h, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None) == EINVAL
        # ... and its states, before the series is looked at
        assert call(Ya=None, series_h=None) == F.LH_ESTATE
        assert all(v == 0 for v in _stats(gm).values())
        # ---- the series' own checks
        ran()
        refused(gm, call(series_h=None), EINVAL, "the series is NULL")
        foreign = make_series(other, T, vals)
        refused(gm, call(series_h=foreign), EINVAL, "not a series of this context")
        ran()
        refused(gm, call(t0=-0.5 * sd), EINVAL, "no extrapolation")
        refused(gm, call(t1=T[-1] + 0.5 * sd), EINVAL, "no extrapolation")
        refused(gm, call(dt=0.0, t1=T[-1] + 0.5 * sd), EINVAL, ": need a finite dt > 0")      # (the arguments come first)
        v0 = np.ascontiguousarray(vals[TOP_E])
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)
        refused(gm, call(), EMODEL, "top hydrology values", "a heat-only model has no hydrology component")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)
        refused(gm, call(), EMODEL, "bottom hydrology values", "a heat-only model has no hydrology component")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        # ---- the call goes on working; t0 == t1 does nothing and reports zeros
        F.check(call(), gm.ctx)
        before = gm.download(Y, F.LH_VAR_RHOE_INT)
        assert np.max(np.abs(before - first)) > 0 and gm.status() == 0
        F.check(call(t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before)
        assert all(v == 0 for v in _stats(gm).values())
        # ---- a face whose kind reads no value: not a state a heat-only context can step in (see the module's text)
        ran()
        F.check(L.lh_set_bc(gm.ctx, M.FACE_TOP, M.COMP_ENERGY, M.BC_NONE, 0.0, None), gm.ctx)
        assert call() == EMODEL and all(v == 0 for v in _stats(gm).values())
        F.check(L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        # (`foreign` is left to lh_destroy)
    # ---- the wrong model: a Richards context and a coupled context, arguments first
    for name in ("c2_richards_f64", "coupled_f64_small"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            h = make_series(gm, T, {})
            L = gm.L
            refused(gm, L.lh_integrate_heat_series(gm.ctx, Y, Ya, h, T[0], T[1], 0.0, 0.0, 0.0, 0, None), gm.F.LH_EINVAL, "dt > 0")
            rc = L.lh_integrate_heat_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0, None)
            refused(gm, rc, gm.F.LH_EMODEL)
            assert L.lh_last_error(gm.ctx).decode() == HEAT_ONLY
            # (the model comes before the series: a NULL series on the wrong model is the model's refusal)
            rc = L.lh_integrate_heat_series(gm.ctx, Y, Ya, None, T[0], T[1], sd, 0.0, 0.0, 0, None)
            assert rc == gm.F.LH_EMODEL and L.lh_last_error(gm.ctx).decode() == HEAT_ONLY


def test_lh_integrate_series_keeps_refusing_a_heat_only_context():
    fam, sd = family("scalar", np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    with fam.open() as gm:
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, top_values(fam, M.BC_FLUX))
        rc = gm.L.lh_integrate_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None)
        refused(gm, rc, gm.F.LH_EMODEL, name="lh_integrate_series")


def test_layered_refusals_in_the_wrapped_calls_words():
    """A heat-only context with a class map and per-column parameter arrays, or LH_MATH_LIBM: what every layered call refuses."""
    fam, sd = family("layered", np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    with fam.open() as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, top_values(fam, M.BC_FLUX))
        call = lambda: L.lh_integrate_heat_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0, None)
        F.check(call(), gm.ctx)
        nu = np.full(67, 0.45)
        F.check(L.lh_set_percol_param(gm.ctx, F.LH_PC["nu"], _dptr(nu)), gm.ctx)
        refused(gm, call(), F.LH_EMODEL, "per-column parameter arrays")
        F.check(L.lh_set_percol_param(gm.ctx, F.LH_PC["nu"], None), gm.ctx)
        F.check(L.lh_set_math_mode(gm.ctx, F.LH_MATH_LIBM), gm.ctx)
        refused(gm, call(), F.LH_EMODEL, "LH_MATH_LIBM")
        F.check(L.lh_set_math_mode(gm.ctx, F.LH_MATH_FAST), gm.ctx)
        F.check(call(), gm.ctx)
        assert gm.status() == 0


# ------------------------------------------------------------------ 6. the host mirror

def _host_model(lh, lay=None, n=NLEV, N=5):
    """a heat-only SoilModel with a flux top and a Dirichlet bottom; lay: with its classes and (first column's) map"""
    FT = np.float64
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(-2.0)),
                         bottom=lh.SoilComponentBC(energy=lh.Dirichlet(lambda t: 284.0)))
    kw = dict(boundary_conditions=bc, earth_param_set=lh.EarthParameterSet())
    if lay is None:
        return lh.SoilModel(FT, domain=lh.Column(FT, zlim=(0.0, 0.2), nelements=n, ncolumns=N), energy_model=lh.SoilEnergyModel(),
                            hydrology_model=lh.PrescribedHydrologyModel(),
                            soil_param_set=lh.SoilParams(FT, ν=0.495, ν_ss_gravel=0.1, ν_ss_om=0.1, ν_ss_quartz=0.1,
                                                         ρc_ds=2.0e6, κ_solid=8.0, κ_sat_unfrozen=0.57, κ_sat_frozen=2.29), **kw)
    om = lay.case.om
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(LH.THERMAL_FIELDS, t))))
                         for k, t in zip(lay.classes, lay.thermal)], lay.class_map[0].astype(np.int64))
    vl_row = np.ascontiguousarray(lay.case.vl[0]).astype(np.float64)
    return lh.SoilModel(FT, domain=lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N), energy_model=lh.SoilEnergyModel(),
                        hydrology_model=lh.PrescribedHydrologyModel(vartheta_l_profile=lambda z, t: vl_row + 0.0 * z),
                        soil_param_set=lh.SoilParams(FT), soil_classes=sc, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_host_mirror(kind):
    """Simulation(model, HeatSeriesTRBDF2(forcing=fs)) / LayeredHeatSeriesTRBDF2 over the whole series is one
    integrate_heat_series call, in state and statistics; that call is the ctypes call."""
    lh = g.load_package()
    N = 5
    lay = family("layered", np.float64, M.BC_FLUX, ncols=N)[0].obj if kind == "layered" else None
    marker = lh.LayeredHeatSeriesTRBDF2 if kind == "layered" else lh.HeatSeriesTRBDF2
    ic = lambda z, m: {"ρe_int": 2.5e7 + 4.0e6 * np.sin(9.0 * z)}
    model = _host_model(lh, lay, N=N)
    (Y1, Ya), (Y2, _), (Y3, _) = [lh.initialize_states(model, ic, 0.0) for _ in range(3)]
    sd = lh.stable_dt(model, Y1, Ya, 0.5)
    T = KNOTS * sd
    vals = -2.0 * SHAPE_FLUX[:, None] * (0.8 + 0.4 * pc.uhash(np.arange(N), 3, 1))[None, :]
    fs = lh.BoundarySeries(T, {("top", "energy"): vals})
    sim = lh.Simulation(model, marker(forcing=fs, reltol=1e-4), Y_init=Y1, dt=sd, tspan=(T[0], T[-1]), Ya_init=Ya)
    lh.run(sim)
    want = lh.integrate_heat_series(model, Y2, Ya, fs, T[0], T[-1], sd, reltol=1e-4)
    np.testing.assert_array_equal(Y1.get("ρe_int"), Y2.get("ρe_int"))
    assert sim.integrator.trbdf2_stats == want, (sim.integrator.trbdf2_stats, want)
    assert sim.integrator.t == T[-1] and want["failed"] == 0 and want["accepted"] >= 4 * N
    # the ctypes call on the same context, a series of its own
    F = lh._ffi
    L, be = F.lib(), model._backend()
    h = C.c_void_p()
    Tc, a = np.ascontiguousarray(T), np.ascontiguousarray(vals)
    F.check(L.lh_bc_series_create(be.ctx, 5, _dptr(Tc), C.byref(h)), be.ctx)
    F.check(L.lh_bc_series_set(be.ctx, h, M.FACE_TOP, M.COMP_ENERGY, _dptr(a), N, 1), be.ctx)
    F.check(L.lh_integrate_heat_series(be.ctx, Y3.handle, Ya.handle, h, T[0], T[-1], sd, 0.0, 1e-4, 0, None), be.ctx)
    np.testing.assert_array_equal(Y3.get("ρe_int"), Y2.get("ρe_int"))
    with pytest.raises(ValueError):
        lh.integrate_heat_series(model, Y1, Ya, fs, T[0] - 1.0, T[1], sd)
    with pytest.raises(TypeError):
        lh.integrate_heat_series(model, Y1, Ya, None, T[0], T[1], sd)
    # the markers refuse what their parents refuse, when the Simulation is built
    other = lh.LayeredHeatSeriesTRBDF2 if kind == "scalar" else lh.HeatSeriesTRBDF2
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.Simulation(model, other(forcing=fs), Y_init=Y1, dt=sd, tspan=(T[0], T[-1]), Ya_init=Ya)
    model.close()
