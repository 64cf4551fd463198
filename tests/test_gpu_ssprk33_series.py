"""lh_step_ssprk33_series: fixed-step SSPRK33 under a per-column boundary-value series, pinned BITWISE -- a uniform
series against lh_step_ssprk33 given bc_stage_values sampled by the tests' own sampler (test_ssprk33_series_cpu), a
per-column series column by column against uniform runs, the wave stepper against the fused stages, a call against
its pieces -- and on what it leaves alone, its refusals and its host mirror.

The issue asks for the marker as SSPRK33(forcing=...).  tests/test_host_mirror_contract_cpu.py pins SSPRK33's
constructor without parameters (signature "()", no attributes), so the marker is SeriesSSPRK33(forcing), a subclass;
test_host_mirror uses that name."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import coupled_implicit_ref as CR
import heat_implicit_ref as HR
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import layered_ref as LR
import parity_cases as pc
import test_ssprk33_series_cpu as S
from test_ssprk33_series_cpu import BOT_E, BOT_H, NSTEPS, TOP_E, TOP_H

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
STEPPER, FUSED = "persist=2", "persist=0,seg=-1"
NCOLS = (1, 67, 130)           # 67 and 130 leave a partial wave and shadowed spare slots
NLEVS = (1, 2, 3, 64, 65, 128, 129)   # 65 and 128 take two cells per lane; 129 is the first fused-only column


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _case_of(obj):
    return obj if isinstance(obj, pc.Case) else obj.case


def _open(obj):
    if isinstance(obj, pc.Case):
        return pc.GpuModel(obj)
    gm = pc.GpuModel(obj.case)
    gm.set_soil_classes(obj.classes, obj.class_map, thermal=getattr(obj, "thermal", None))
    return gm


def _state(gm, Y):
    F, m = gm.F, gm.case.om.model
    out = {}
    if m != F.LH_MODEL_HEAT:
        out["vl"] = gm.download(Y, F.LH_VAR_VARTHETA_L)
        out["ti"] = gm.download(Y, F.LH_VAR_THETA_I)
    if m != F.LH_MODEL_RICHARDS:
        out["rhoe"] = gm.download(Y, F.LH_VAR_RHOE_INT)
    out["status"] = gm.status()
    return out


def assert_same(got, want, cols=None):
    """every prognostic plane and lh_status (cols: on these columns only)"""
    assert set(got) == set(want)
    for k in want:
        if k == "status":
            assert got[k] == want[k], (got[k], want[k])
        else:
            sel = slice(None) if cols is None else cols
            np.testing.assert_array_equal(got[k][sel], want[k][sel], err_msg=k)


def make_series(gm, T, values):
    """An lh_bc_series of the context: [nknots] values are uniform (col_stride 0), [nknots, ncols] per column"""
    F = gm.F
    T = np.ascontiguousarray(T, dtype=np.float64)
    h = C.c_void_p()
    F.check(gm.L.lh_bc_series_create(gm.ctx, len(T), _dptr(T), C.byref(h)), gm.ctx)
    for (f, k), v in values.items():
        a = np.ascontiguousarray(v, dtype=np.float64)
        F.check(gm.L.lh_bc_series_set(gm.ctx, h, f, k, _dptr(a), 1 if a.ndim == 1 else a.shape[1], 0 if a.ndim == 1 else 1), gm.ctx)
    return h


def run(obj, tune, action, engine=None, nsteps=NSTEPS):
    """A fresh context under `tune`, the case's states, action(gm, Y, Ya); the state and status it leaves"""
    with _open(obj) as gm:
        gm.F.check(gm.L.lh_set_tuning(gm.ctx, tune.encode()), gm.ctx)
        if engine is not None:
            assert gm.L.lh_step_series_engine(gm.ctx, nsteps) == engine
        Y, Ya = gm.prognostic_and_aux()
        action(gm, Y, Ya)
        return _state(gm, Y)


def existing(bcv, t, dt, nsteps=NSTEPS):
    def action(gm, Y, Ya):
        gm.F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, t, dt, nsteps, _dptr(np.ascontiguousarray(bcv))), gm.ctx)
    return action


def series(T, values, t, dt, pieces=(NSTEPS,)):
    """lh_step_ssprk33_series, the call cut into `pieces` steps each (piece j starts at t + dt * steps before it)"""
    def action(gm, Y, Ya):
        h = make_series(gm, T, values)
        done = 0
        for n in pieces:
            gm.F.check(gm.L.lh_step_ssprk33_series(gm.ctx, Y, Ya, h, t + dt * float(done), dt, n), gm.ctx)
            done += n
    return action


@functools.lru_cache(maxsize=None)
def half_stable_step(key):
    """half the stable step (courant 1/2) of the start state of CASES[key]"""
    with _open(CASES[key]()) as gm:
        Y, Ya = gm.prognostic_and_aux()
        out = C.c_double()
        gm.F.check(gm.L.lh_stable_dt(gm.ctx, Y, Ya, 0.5, C.byref(out)), gm.ctx)
    return 0.5 * out.value


def base_values(om):
    return {k: v for k, (_, v) in om.bc.items()}


# ------------------------------------------------------------------ cases

def richards(ncols, nlev, dtype=F64, top=M.BC_FLUX, bottom=M.BC_FLUX, **kw):
    return CR.coupled_case(top, bottom, dtype=dtype, ncols=ncols, nlev=nlev, model=M.MODEL_RICHARDS, **kw)


def coupled(ncols, nlev, dtype=F64):
    return CR.coupled_case(M.BC_FLUX, M.BC_FREE_DRAINAGE, dtype=dtype, ncols=ncols, nlev=nlev, ice=True)


def layered_richards(ncols=67, nlev=12):
    cut = 4 + (np.arange(ncols) % 5)
    cmap = (np.arange(nlev)[None, :] < cut[:, None]).astype(np.uint8)
    return LR.make_layered(F64, ncols, nlev, cmap, bc="flux_drain")


def layered_coupled(ncols=67, nlev=12):
    return LC.layered_case(F64, ncols, nlev, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")


def atmos(ncols=67):
    from test_gpu_atmos_bc import _atmos_case
    case = _atmos_case(F64, N=ncols, n=24, percol=True)
    om = dataclasses.replace(case.om, bc={BOT_E: (M.BC_FLUX, 0.03), BOT_H: (M.BC_FLUX, -1e-9)})
    return dataclasses.replace(case, om=om)


# name -> (constructor, the (face, component)s that get a series)
CASES, KEYS = {}, {}


def _case(name, make, keys):
    CASES[name], KEYS[name] = make, keys


for _n in NCOLS:
    for _l in NLEVS:
        _case("richards/%dx%d" % (_n, _l), functools.partial(richards, _n, _l), (TOP_H,))
for _dt, _id in ((F64, "f64"), (F32, "f32")):
    _case("richards-dirichlet-drain/" + _id, functools.partial(richards, 67, 65, _dt, M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), (TOP_H,))
    _case("richards-flux/" + _id, functools.partial(richards, 130, 64, _dt), (TOP_H,))
    _case("heat/" + _id, functools.partial(HR.heat_case, 67, 60, _dt, M.BC_FLUX, M.BC_DIRICHLET), (TOP_E, BOT_E))
    _case("coupled/" + _id, functools.partial(coupled, 67, 65, _dt), (TOP_E, TOP_H))
    _case("coupled-factors-ice/" + _id, functools.partial(pc.make_case, "mixed_smooth_" + _id, 67), (TOP_E, TOP_H))
_case("richards-viscosity", functools.partial(pc.make_case, "richards_viscosity_f64", 67), (TOP_H,))
_case("richards-percol", functools.partial(richards, 67, 64, F64, M.BC_FLUX, M.BC_FREE_DRAINAGE, percol=True), (TOP_H,))
_case("layered-richards", layered_richards, (TOP_H,))
_case("layered-coupled", layered_coupled, (TOP_E, TOP_H))
_case("atmos", atmos, (BOT_E, BOT_H))
_case("richards-bottom-array", functools.partial(richards, 67, 64, F64, M.BC_FLUX, M.BC_DIRICHLET), (TOP_H,))


def setup(key):
    """(obj, dt, t, T, uniform values) of a case"""
    obj = CASES[key]()
    dt = half_stable_step(key)
    return obj, dt, S.start_time(dt), S.knots(dt), S.uniform_values(_case_of(obj).om, KEYS[key])


def engines_of(key):
    """(tuning, the engine lh_step_series_engine must report) for both tunings"""
    obj = CASES[key]()
    om = _case_of(obj).om
    stepper = isinstance(obj, pc.Case) and om.nlev <= 128 and om.atmos is None
    return ((STEPPER, g.load_package()._ffi.LH_ENGINE_COLUMN_STEPPER if stepper else 0), (FUSED, 0))


@functools.lru_cache(maxsize=None)
def reference(key, tune=STEPPER):
    """lh_step_ssprk33 given bc_stage_values sampled by the test's sampler from the uniform series"""
    obj, dt, t, T, values = setup(key)
    bcv = S.sample_bcv(T, values, base_values(_case_of(obj).om), t, dt, NSTEPS)
    return run(obj, tune, existing(bcv, t, dt))


# ------------------------------------------------------------------ 1. a uniform series is the existing call

UNIFORM = [k for k in CASES if k not in ("atmos", "richards-bottom-array") and not k.startswith("layered")]


@pytest.mark.parametrize("key", UNIFORM)
def test_uniform_series_is_the_existing_call(key):
    obj, dt, t, T, values = setup(key)
    ncols = _case_of(obj).ncols
    for tune, engine in engines_of(key):
        want = reference(key, tune)
        assert want["status"] == 0
        assert_same(run(obj, tune, series(T, values, t, dt), engine), want)
    # a per-column table whose columns are all equal (the full grid of shapes: at the stepper's path only)
    equal = {k: np.repeat(v[:, None], ncols, axis=1) for k, v in values.items()}
    for tune, engine in engines_of(key)[:1 if key.startswith("richards/") else 2]:
        assert_same(run(obj, tune, series(T, equal, t, dt), engine), reference(key, tune))


def test_uniform_series_with_the_ldexp_closures():
    key = "richards-flux/f64"
    obj, dt, t, T, values = setup(key)
    tune = STEPPER + ",vgfast=0"

    def checked(action):
        def wrapped(gm, Y, Ya):
            assert gm.L.lh_closure_form(gm.ctx) == gm.F.LH_CLOSURE_LDEXP
            action(gm, Y, Ya)
        return wrapped
    bcv = S.sample_bcv(T, values, base_values(obj.om), t, dt, NSTEPS)
    want = run(obj, tune, checked(existing(bcv, t, dt)))
    assert_same(run(obj, tune, checked(series(T, values, t, dt)), 1), want)


@pytest.mark.parametrize("key", ["richards/130x64", "richards/67x128", "coupled/f32"])
def test_a_table_of_300_knots(key):
    """More than 65 knots: the wave's search bisects down to a window of 64 knots before its lanes count
    (series_knot_interval_wave); many_knots puts stage times into the first interval, intervals far above index 64, the
    last interval, and on a knot above index 64.  Uniform against the existing call, then per column against uniform
    runs, on both engines."""
    obj, dt, t, _, _ = setup(key)
    case = _case_of(obj)
    T = S.many_knots(dt)
    values = {k: S.many_knot_values(case.om.bc[k][1]) if case.om.bc[k][0] == M.BC_FLUX
              else np.interp(T, S.knots(dt), S.uniform_table(k, *case.om.bc[k])) for k in KEYS[key]}
    bcv = S.sample_bcv(T, values, base_values(case.om), t, dt, NSTEPS)
    scale = 0.6 + 0.05 * ((np.arange(case.ncols) * 7) % 13)
    percol = {k: v[:, None] * scale[None, :] if case.om.bc[k][0] == M.BC_FLUX else np.repeat(v[:, None], case.ncols, axis=1)
              for k, v in values.items()}
    for tune, engine in engines_of(key):
        want = run(obj, tune, existing(bcv, t, dt))
        assert want["status"] == 0
        assert_same(run(obj, tune, series(T, values, t, dt), engine), want)
        got = run(obj, tune, series(T, percol, t, dt), engine)
        for c in sorted({0, 64, case.ncols - 1}):
            own = {k: np.ascontiguousarray(v[:, c]) for k, v in percol.items()}
            bcv_c = S.sample_bcv(T, own, base_values(case.om), t, dt, NSTEPS)
            assert_same(got, run(obj, tune, existing(bcv_c, t, dt)), cols=[c])


def test_large_ensembles_take_the_fused_stages_unless_told_otherwise():
    """lh_step_series_engine's rule for more than 2^20 threads (no launch: the query alone)"""
    big = dataclasses.replace(richards(1, 64), ncols=16385)          # 16385 x 64 threads: one column past 2^20
    small = dataclasses.replace(richards(1, 64), ncols=16384)
    with pc.GpuModel(big) as gm, pc.GpuModel(small) as gs:
        F, L = gm.F, gm.L
        for n in (1, 4, 30):
            assert L.lh_step_series_engine(gm.ctx, n) == F.LH_ENGINE_FUSED_STAGES
            assert L.lh_step_series_engine(gs.ctx, n) == F.LH_ENGINE_COLUMN_STEPPER
        F.check(L.lh_set_tuning(gm.ctx, b"persist=2"), gm.ctx)
        assert L.lh_step_series_engine(gm.ctx, 4) == F.LH_ENGINE_COLUMN_STEPPER
        F.check(L.lh_set_tuning(gm.ctx, b"persist=0"), gm.ctx)
        assert L.lh_step_series_engine(gm.ctx, 4) == F.LH_ENGINE_FUSED_STAGES


# ------------------------------------------------------------------ 2. / 3. a per-column series, column by column; the engines

PERCOL = ["richards/%dx%d" % (n, l) for n in (67, 130) for l in NLEVS] + ["coupled/f64", "heat/f32", "richards-dirichlet-drain/f64"]


@functools.lru_cache(maxsize=None)
def percol_run(key, tune):
    obj, dt, t, T, _ = setup(key)
    case = _case_of(obj)
    values = S.percol_values(T, case.om, KEYS[key], case.ncols)
    engine = dict(engines_of(key))[tune]
    return run(obj, tune, series(T, values, t, dt), engine), values


@pytest.mark.parametrize("key", PERCOL)
def test_per_column_series_column_by_column(key):
    obj, dt, t, T, _ = setup(key)
    ncols = _case_of(obj).ncols
    got = {tune: percol_run(key, tune) for tune in (STEPPER, FUSED)}
    for c in sorted({0, 63, 64, ncols - 1}):
        own = {k: np.ascontiguousarray(v[:, c]) for k, v in got[STEPPER][1].items()}
        want = run(obj, STEPPER, series(T, own, t, dt))
        for tune in (STEPPER, FUSED):
            assert_same(got[tune][0], want, cols=[c])


@pytest.mark.parametrize("key", [k for k in PERCOL if not k.endswith("x129")])   # (all shapes with nlev <= 128)
def test_engines_agree(key):
    assert_same(percol_run(key, STEPPER)[0], percol_run(key, FUSED)[0])
    assert percol_run(key, STEPPER)[0]["status"] == 0


# ------------------------------------------------------------------ 4. splitting a call

@pytest.mark.parametrize("key", ["richards/130x65", "richards/67x129", "coupled/f32"])
@pytest.mark.parametrize("pieces", [(1, 1, 1, 1, 1), (2, 3)])
def test_a_call_is_its_pieces(key, pieces):
    obj, dt, t, T, _ = setup(key)
    whole, values = percol_run(key, STEPPER)
    assert_same(run(obj, STEPPER, series(T, values, t, dt, pieces)), whole)


# ------------------------------------------------------------------ 5. what a series leaves alone and what it overrides

@pytest.mark.parametrize("tune", [STEPPER, FUSED])
def test_other_components_keep_their_arrays(tune):
    key = "richards-bottom-array"
    obj, dt, t, T, values = setup(key)
    ncols = obj.ncols
    om = dataclasses.replace(obj.om, percol_bc={BOT_H: 0.2 * (1.0 + 0.05 * (pc.uhash(np.arange(ncols), 5, 1) - 0.5))})
    with_array = dataclasses.replace(obj, om=om)
    bcv = S.sample_bcv(T, values, base_values(om), t, dt, NSTEPS)
    want = run(with_array, tune, existing(bcv, t, dt))
    assert_same(run(with_array, tune, series(T, values, t, dt)), want)
    assert not np.array_equal(want["vl"], reference(key)["vl"])           # (the array is read)
    # an array and a series on the same component: the series wins
    om2 = dataclasses.replace(obj.om, percol_bc={TOP_H: -1e-8 * (1.0 + pc.uhash(np.arange(ncols), 6, 1))})
    assert_same(run(dataclasses.replace(obj, om=om2), tune, series(T, values, t, dt)), reference(key, tune))


@pytest.mark.parametrize("tune", [STEPPER, FUSED])
def test_the_boundary_state_of_the_context_is_not_modified(tune):
    key = "richards-bottom-array"
    obj, dt, t, T, _ = setup(key)
    values = S.percol_values(T, obj.om, KEYS[key], obj.ncols)
    want = pc.run_gpu_rhs(obj)

    def action(gm, Y, Ya):
        series(T, values, t, dt)(gm, Y, Ya)
        Y2, Ya2 = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y2, Ya2, dY)
        for k, v in gm.tendencies(dY).items():
            np.testing.assert_array_equal(v, want[k])
    run(obj, tune, action)


# ------------------------------------------------------------------ 6. layered contexts, 7. a prescribed atmosphere

@pytest.mark.parametrize("key", ["layered-richards", "layered-coupled", "atmos"])
def test_fused_only_contexts(key):
    obj, dt, t, T, values = setup(key)
    case = _case_of(obj)
    for tune in (STEPPER, FUSED):    # (persist=2: lh_step_ssprk33 takes the layered stepper for Richards; the series call does not)
        want = reference(key, tune)
        assert want["status"] == 0
        assert_same(run(obj, tune, series(T, values, t, dt), 0), want)
    pv = S.percol_values(T, case.om, KEYS[key], case.ncols)
    got = run(obj, STEPPER, series(T, pv, t, dt), 0)
    for c in (0, 63, 64, case.ncols - 1):
        own = {k: np.ascontiguousarray(v[:, c]) for k, v in pv.items()}
        assert_same(got, run(obj, STEPPER, series(T, own, t, dt)), cols=[c])


def test_a_top_series_under_a_prescribed_atmosphere_is_refused():
    obj, dt, t, T, _ = setup("atmos")
    with _open(obj) as gm:
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, {TOP_H: -1e-9 * S.SHAPE["flux"]})
        # (the top components of such a context have no lh_set_bc kind that reads a value: series_kind_refusals' LH_EMODEL)
        assert gm.L.lh_step_ssprk33_series(gm.ctx, Y, Ya, h, t, dt, NSTEPS) == gm.F.LH_EMODEL
        assert b"reads no value" in gm.L.lh_last_error(gm.ctx)


# ------------------------------------------------------------------ 8. refusals and their order

def test_refusals_and_their_order():
    key = "richards-dirichlet-drain/f64"
    obj, dt, t, T, values = setup(key)
    with _open(obj) as gm, pc.GpuModel(obj) as other:
        F, L, ctx = gm.F, gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        before = _state(gm, Y)
        h = make_series(gm, T, values)
        foreign = make_series(other, T, values)
        bad = C.c_void_p()       # a state without the prognostic planes
        F.check(L.lh_state_create(ctx, 0b1000, C.byref(bad)), ctx)

        def refused(code, words, Y_=Y, h_=h, t_=t, dt_=dt, n=NSTEPS):
            assert L.lh_step_ssprk33_series(ctx, Y_, Ya, h_, t_, dt_, n) == code
            assert words in L.lh_last_error(ctx).decode(), L.lh_last_error(ctx)

        own = "lh_step_ssprk33_series: need nsteps >= 0 and dt > 0"    # lh_step_ssprk33's words under the new name
        refused(F.LH_EINVAL, own, n=-1, h_=None, t_=float("nan"))       # (before everything else)
        refused(F.LH_EINVAL, own, dt_=0.0, h_=None)
        refused(F.LH_EINVAL, own, dt_=float("nan"))
        assert L.lh_step_ssprk33(ctx, Y, Ya, t, 0.0, 1, None) == F.LH_EINVAL
        assert L.lh_last_error(ctx).decode() == own.replace("_series", "")
        assert L.lh_step_ssprk33_series(ctx, bad, Ya, None, float("inf"), dt, 1) == L.lh_step_ssprk33(ctx, bad, Ya, t, dt, 1, None) != 0
        refused(F.LH_EINVAL, "t is not finite", t_=float("inf"), h_=None)
        refused(F.LH_EINVAL, "the series is NULL", h_=None, t_=T[0] - dt)
        refused(F.LH_EINVAL, "not a series of this context", h_=foreign, t_=T[0] - dt)
        hk = make_series(gm, T, {BOT_H: values[TOP_H]})                      # free drainage
        refused(F.LH_EMODEL, "bottom hydrology values, and the boundary condition there (lh_set_bc) reads no value", h_=hk,
                t_=T[0] - dt)                                                # (before the span)
        # NoBC on a component the model has is lh_step_ssprk33's own refusal, in its words (the one NoBC component a
        # series can meet is the top under a prescribed atmosphere: test_a_top_series_under_a_prescribed_atmosphere_is_refused)
        F.check(L.lh_set_bc(ctx, TOP_H[0], TOP_H[1], F.LH_BC_NONE, 0.0, None), ctx)
        assert L.lh_step_ssprk33(ctx, Y, Ya, t, dt, 1, None) == F.LH_EMODEL
        refused(F.LH_EMODEL, L.lh_last_error(ctx).decode(), h_=None, t_=float("nan"))
        gm.set_bcs(obj.om)
        he = make_series(gm, T, {TOP_E: values[TOP_H]})
        refused(F.LH_EMODEL, "a Richards model has no energy component", h_=he)
        # the span: a first stage time below T_0, a last one above T_last by one ulp; T_last itself is accepted
        below = np.nextafter(T[0], -np.inf)
        refused(F.LH_EINVAL, "%.17g" % below, t_=below, n=1)
        st = S.stage_times(t, dt, NSTEPS)
        assert st[-1, 1] == T[-1]
        T_short = np.append(T[:-1], np.nextafter(T[-1], -np.inf))
        short = make_series(gm, T_short, values)
        refused(F.LH_EINVAL, "%.17g" % st[-1, 1], h_=short)
        assert L.lh_step_ssprk33_series(ctx, Y, Ya, short, t, dt, NSTEPS - 1) == 0      # (its last stage time is inside)
        assert_same(_state(gm, Y), run(obj, "", series(T_short, values, t, dt, (NSTEPS - 1,))))
        # nsteps == 0 leaves Y untouched (after the checks)
        gm.upload(Y, F.LH_VAR_VARTHETA_L, obj.vl)
        assert L.lh_step_ssprk33_series(ctx, Y, Ya, h, T[0] - 10 * dt, dt, 0) == 0
        assert_same(_state(gm, Y), before)
        assert L.lh_step_series_engine(None, 1) == F.LH_EINVAL and L.lh_step_series_engine(ctx, -1) == F.LH_EINVAL


@pytest.mark.parametrize("tune", [STEPPER, FUSED])
def test_a_poisoned_column_leaves_the_others_alone(tune):
    key = "richards/130x64"
    obj, dt, t, T, _ = setup(key)
    values = S.percol_values(T, obj.om, KEYS[key], obj.ncols)
    poisoned = {TOP_H: values[TOP_H].copy()}
    poisoned[TOP_H][2, 70] = np.nan
    got, want = run(obj, tune, series(T, poisoned, t, dt)), percol_run(key, tune)[0]
    assert got["status"] == 1 and want["status"] == 0
    others = [c for c in range(obj.ncols) if c != 70]
    np.testing.assert_array_equal(got["vl"][others], want["vl"][others])
    assert np.isnan(got["vl"][70]).any()


# ------------------------------------------------------------------ 9. the host mirror

def test_host_mirror():
    lh = g.load_package()
    FT, ncols, nlev = np.float64, 67, 12
    sp, vg = pc.coupled_soil()
    flux0 = -2e-9

    def model_and_states(n=3):
        model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-0.24, 0.0), nelements=nlev, ncolumns=ncols),
                             energy_model=lh.PrescribedTemperatureModel(),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(
                                 FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)),
                             boundary_conditions=lh.SoilColumnBC(
                                 top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(flux0)),
                                 bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                             soil_param_set=lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s), earth_param_set=lh.EarthParameterSet())
        init = lambda z, m: {"ϑ_l": 0.2 + 0.1 * np.exp(4.0 * z), "θ_i": 0.0 * z}
        return model, [lh.initialize_states(model, init, 0.0) for _ in range(n)]

    model, ((Y1, Ya), (Y2, _), (Y3, _)) = model_and_states()
    dt = 0.5 * lh.stable_dt(model, Y1, Ya, 0.5)
    t, T = S.start_time(dt), S.knots(dt, 6)
    vals = S.percol_table(T, TOP_H, M.BC_FLUX, flux0, ncols)
    fs = lh.BoundarySeries(T, {("top", "hydrology"): vals})
    F = lh._ffi
    L, be = F.lib(), model._backend()
    assert lh.step_series_engine(model, 6) == L.lh_step_series_engine(be.ctx, 6) == F.LH_ENGINE_COLUMN_STEPPER
    # step_series is the C call
    assert lh.step_series(model, Y1, Ya, fs, t, dt, 6) == t + 6 * dt
    F.check(L.lh_step_ssprk33_series(be.ctx, Y2.handle, None, fs._device(model), t, dt, 6), be.ctx)
    np.testing.assert_array_equal(Y1.get("ϑ_l"), Y2.get("ϑ_l"))
    assert not np.array_equal(Y1.get("ϑ_l"), Y3.get("ϑ_l"))
    # a Simulation over two saveat chunks is two step_series calls
    sim = lh.Simulation(model, lh.SeriesSSPRK33(forcing=fs), Y_init=Y3, dt=dt, tspan=(t, t + 6 * dt), Ya_init=Ya, saveat=3 * dt)
    lh.run(sim)
    model_b, ((Z1, Za),) = model_and_states(1)
    t3 = lh.step_series(model_b, Z1, Za, fs, t, dt, 3)
    lh.step_series(model_b, Z1, Za, fs, t3, dt, 3)
    np.testing.assert_array_equal(Y3.get("ϑ_l"), Z1.get("ϑ_l"))
    assert len(sim.integrator.sol.t) == 3
    with pytest.raises(ValueError):
        lh.step_series(model, Y1, Ya, fs, T[0] - dt, dt, 1)
    with pytest.raises(TypeError):
        lh.SeriesSSPRK33(forcing={("top", "hydrology"): vals})
    # SSPRK33() without a forcing makes the call it made before
    model_c, ((A1, Aa), (A2, _)) = model_and_states(2)
    sim0 = lh.Simulation(model_c, lh.SSPRK33(), Y_init=A1, dt=dt, tspan=(t, t + 3 * dt), Ya_init=Aa)
    lh.run(sim0)
    bc = model_c._backend()
    bc.set_bcs(model_c, t)
    F.check(L.lh_step_ssprk33(bc.ctx, A2.handle, None, t, dt, 3, None), bc.ctx)
    np.testing.assert_array_equal(A1.get("ϑ_l"), A2.get("ϑ_l"))


def test_time_varying_prescribed_profiles_refuse_a_forcing():
    lh = g.load_package()
    FT, ncols, nlev = np.float64, 3, 8
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-0.16, 0.0), nelements=nlev, ncolumns=ncols),
                         energy_model=lh.PrescribedTemperatureModel(T_profile=lambda z, t: 280.0 + 0.0 * z + 100.0 * t),
                         hydrology_model=lh.SoilHydrologyModel(FT, viscosity_factor=lh.TemperatureDependentViscosity(FT)),
                         boundary_conditions=lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-1e-9)),
                                                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                         earth_param_set=lh.EarthParameterSet())
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.2 + 0.0 * z, "θ_i": 0.0 * z}, 0.0)
    dt = 0.5 * lh.stable_dt(model, Y, Ya, 0.5)
    fs = lh.BoundarySeries([0.0, 10 * dt], {("top", "hydrology"): [-1e-9, -2e-9]})
    sim = lh.Simulation(model, lh.SeriesSSPRK33(fs), Y_init=Y, dt=dt, tspan=(0.0, 2 * dt), Ya_init=Ya)
    with pytest.raises(ValueError, match="SeriesSSPRK33.*_advance_refreshing_aux"):
        lh.run(sim)
