"""lh_bc_series / lh_integrate_series: the TR-BDF2 integrators under a per-column boundary-value time series,
one launch for the chain of calls the host would make -- pinned BITWISE against that chain through the
existing entry points (scalar Richards, layered Richards, the coupled model), against the NumPy reference in
fixed-step mode, and on its refusals and its host mirror."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import coupled_implicit_ref as CR
import layered_ref as LR
import parity_cases as pc
import trbdf2_ref as R
from test_gpu_implicit import bonan_case, richards_case, stable_dt
from test_gpu_layered import layered_gpu

pytestmark = pytest.mark.gpu
STATUS_FAILED = 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
SUMMED = ("accepted", "rejected", "newton_iterations", "failed", "unconverged")
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NCOLS, NLEV = 130, 12          # two full waves and a partial one
TOP_H = (M.FACE_TOP, M.COMP_HYDROLOGY)
TOP_E = (M.FACE_TOP, M.COMP_ENERGY)
# 5 knots at uneven spacing in units of the case's stable step; t0 inside the first knot interval, t1 inside the last
KNOTS = np.array([0.0, 7.0, 12.0, 25.0, 31.0])
T0, T1 = 2.5, 28.0
SHAPE_H = {M.BC_FLUX: np.array([1.0, 3.0, 0.5, 2.0, 1.5]), M.BC_DIRICHLET: np.array([1.0, 0.9, 1.05, 0.95, 1.0])}
SHIFT_E = np.array([0.0, 2.0, -1.0, 3.0, 1.0])   # K on the coupled model's Dirichlet top temperature


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def series_value(T, v, t):
    """The issue's formula: v_k + (v_k+1 - v_k) ((t - T_k) / (T_k+1 - T_k)) in double, exactly v_k on a knot."""
    k = min(int(np.searchsorted(T, t, side="right")) - 1, len(T) - 2)
    if t == T[k]:
        return v[k]
    if t == T[k + 1]:
        return v[k + 1]
    return v[k] + (v[k + 1] - v[k]) * ((t - T[k]) / (T[k + 1] - T[k]))


def breakpoints(T, t0, t1):
    return [t0] + [float(x) for x in T if t0 < x < t1] + [t1]


# ------------------------------------------------------------------ the three families

SAND_OVER_CLAY = np.array([[3.0, 4.0, 0.03, 3e-5, 0.40, 1e-3],     # (n, alpha, theta_r, Ksat, nu, S_s)
                           [1.3, 1.0, 0.08, 1e-7, 0.48, 1e-3]])


def _case_of(obj):
    return obj.case if isinstance(obj, LR.Layered) else obj


def _open(obj):
    return layered_gpu(obj) if isinstance(obj, LR.Layered) else pc.GpuModel(obj)


def _family_of(obj):
    if isinstance(obj, LR.Layered):
        return "layered"
    return "coupled" if obj.om.model == M.MODEL_COUPLED else "richards"


@functools.lru_cache(maxsize=None)
def family_case(family, dtype, top, ncols=NCOLS):
    """(case or Layered, its stable step): `top` is the kind of the top hydrology boundary condition."""
    if family == "layered":
        # sand over clay, the interface at a level that differs from column to column
        cut = 4 + (np.arange(ncols) % 5)
        cmap = (np.arange(NLEV)[None, :] < cut[:, None]).astype(np.uint8)     # bottom first: clay (1) below, sand (0) above
        obj = LR.make_layered(dtype, ncols, NLEV, cmap, classes=SAND_OVER_CLAY,
                              bc="flux_drain" if top == M.BC_FLUX else "dirichlet")
    else:
        obj = CR.coupled_case(top, M.BC_FREE_DRAINAGE, dtype=dtype, ncols=ncols, nlev=NLEV,
                              model=M.MODEL_COUPLED if family == "coupled" else M.MODEL_RICHARDS)
    with _open(obj) as gm:
        Y, Ya = gm.prognostic_and_aux()
        out = C.c_double()
        gm.F.check(gm.L.lh_stable_dt(gm.ctx, Y, Ya, 0.5, C.byref(out)), gm.ctx)
    return obj, out.value


def uniform_values(obj, top):
    """{(face, component): [nknots]}: the top hydrology value, and for the coupled model the top energy value"""
    om = _case_of(obj).om
    vals = {TOP_H: om.bc[TOP_H][1] * SHAPE_H[top]}
    if om.model == M.MODEL_COUPLED:
        assert om.bc[TOP_E][0] == M.BC_DIRICHLET
        vals[TOP_E] = om.bc[TOP_E][1] + SHIFT_E
    return vals


def spread_steps(ncols, sd):
    """initial steps over a factor of 100 across the lanes of each wave: lanes of one wave need different numbers
    of steps per sub-interval"""
    lane = (np.arange(ncols) * 37) % 64
    return 0.1 * sd * 100.0 ** (lane / 63.0)


def one_column(obj, c):
    case = _case_of(obj)
    take = lambda a: None if a is None else np.ascontiguousarray(a[c:c + 1])
    case1 = dataclasses.replace(case, ncols=1, vl=take(case.vl), ti=take(case.ti), rhoe=take(case.rhoe))
    if isinstance(obj, LR.Layered):
        return LR.Layered(case1, obj.classes, np.ascontiguousarray(obj.class_map[c:c + 1]))
    return case1


# ------------------------------------------------------------------ the two ways to integrate

def _entry(gm, family, Y, Ya, a, b, dt, abstol, reltol, flags, cols_ptr, bcv):
    L = gm.L
    if family == "coupled":
        return L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, a, b, dt, abstol, 0.0, reltol, flags, cols_ptr, _dptr(bcv))
    call = L.lh_integrate_layered_trbdf2 if family == "layered" else L.lh_integrate_trbdf2
    return call(gm.ctx, Y, Ya, a, b, dt, abstol, reltol, flags, cols_ptr, _dptr(bcv))


def _stats(gm):
    st = (C.c_int64 * gm.F.LH_TRBDF2_NSTATS)()
    gm.F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    return dict(zip(KEYS, list(st)))


def _result(gm, Y, cols, stats, **more):
    F = gm.F
    out = dict(vl=gm.download(Y, F.LH_VAR_VARTHETA_L), stats=stats, status=gm.status(),
               cols=None if cols is None else cols.cpu().numpy().astype(np.float64), **more)
    if gm.case.om.model == M.MODEL_COUPLED:
        out["rhoe"] = gm.download(Y, F.LH_VAR_RHOE_INT)
    return out


def _step_buffer(case, h0):
    import torch
    ft = torch.float64 if case.dtype == np.float64 else torch.float32
    cols = torch.zeros(case.ncols, dtype=ft, device="cuda")
    if h0 is not None:
        cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
    torch.cuda.synchronize()
    return cols


def chain(obj, T, values, t0, t1, dt, h0=None, fixed=False, abstol=0.0, reltol=0.0, ends=None):
    """The chain of calls the host makes today: the existing entry point once per sub-interval, dt_cols carried,
    bcv = lh_set_bc's values with the series' own at both ends (`values`: {(face, comp): [nknots]}, one column's)."""
    case, family = _case_of(obj), _family_of(obj)
    with _open(obj) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        cols = _step_buffer(case, h0)
        base = np.zeros((2, 2, 2))
        for (f, k), (_, v) in case.om.bc.items():
            base[:, f, k] = v
        total = dict.fromkeys(KEYS, 0)
        per_call = []
        bp = breakpoints(T, t0, t1) if ends is None else ends
        for a, b in zip(bp, bp[1:]):
            bcv = base.copy()
            for (f, k), v in values.items():
                bcv[0, f, k] = series_value(T, v, a)
                bcv[1, f, k] = series_value(T, v, b)
            F.check(_entry(gm, family, Y, Ya, a, b, dt, abstol, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                           C.c_void_p(cols.data_ptr()), bcv), gm.ctx)
            st = _stats(gm)
            per_call.append(st)
            for key in KEYS:
                total[key] += st[key]
        return _result(gm, Y, cols, total, per_call=per_call)


def make_series(gm, T, values, transposed=False):
    """An lh_bc_series of the context: [nknots] values are uniform, [nknots, ncols] per-column (transposed: stored
    [ncols, nknots], i.e. a column stride of nknots and a knot stride of 1)."""
    F = gm.F
    T = np.ascontiguousarray(T, dtype=np.float64)
    h = C.c_void_p()
    F.check(gm.L.lh_bc_series_create(gm.ctx, len(T), _dptr(T), C.byref(h)), gm.ctx)
    keep = []
    for (f, k), v in values.items():
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 1:
            a, ks, cs = np.ascontiguousarray(v), 1, 0
        elif transposed:
            a, ks, cs = np.ascontiguousarray(v.T), 1, v.shape[0]
        else:
            a, ks, cs = np.ascontiguousarray(v), v.shape[1], 1
        keep.append(a)
        F.check(gm.L.lh_bc_series_set(gm.ctx, h, f, k, _dptr(a), ks, cs), gm.ctx)
    return h


def series(obj, T, values, t0, t1, dt, h0=None, fixed=False, abstol=0.0, reltol=0.0, null_cols=False, transposed=False):
    """One lh_integrate_series call."""
    case = _case_of(obj)
    with _open(obj) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        cols = None if null_cols else _step_buffer(case, h0)
        h = make_series(gm, T, values, transposed)
        F.check(gm.L.lh_integrate_series(gm.ctx, Y, Ya, h, t0, t1, dt, abstol, 0.0, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                                         None if cols is None else C.c_void_p(cols.data_ptr())), gm.ctx)
        out = _result(gm, Y, cols, _stats(gm))
        F.check(gm.L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        return out


def assert_same_state(got, want, cols=True):
    np.testing.assert_array_equal(got["vl"], want["vl"])
    if "rhoe" in want:
        np.testing.assert_array_equal(got["rhoe"], want["rhoe"])
    if cols:
        np.testing.assert_array_equal(got["cols"], want["cols"])
    assert got["status"] == want["status"], (got["status"], want["status"])


def assert_counters(got, want, ncols):
    """The five summed counters are the chain's sums; max_steps and wave_steps are what per-column totals allow:
    no column attempts more than the chain's per-call maxima together, some column attempts at least the mean and
    at least the largest of any one call; a wave costs 64 x its slowest column."""
    s, c = got["stats"], want["stats"]
    for key in SUMMED:
        assert s[key] == c[key], (key, s, c)
    attempted = s["accepted"] + s["rejected"]
    calls = [p["max_steps"] for p in want["per_call"]]
    assert max(max(calls), -(-attempted // ncols)) <= s["max_steps"] <= sum(calls), (s, calls)
    nwaves = -(-ncols // 64)
    assert max(attempted, 64 * s["max_steps"]) <= s["wave_steps"] <= 64 * nwaves * s["max_steps"], s


# ------------------------------------------------------------------ 1. a uniform series is the chain, bitwise

FAMILIES = ["richards", "layered", "coupled"]
TOPS = [M.BC_FLUX, M.BC_DIRICHLET]
TOP_IDS = ["flux", "dirichlet"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_uniform_series_is_the_chain_bitwise(family, top, dtype):
    obj, sd = family_case(family, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(obj, top)
    h0 = spread_steps(NCOLS, sd)
    want = chain(obj, T, values, t0, t1, sd, h0=h0)
    assert want["stats"]["failed"] == 0 and len(want["per_call"]) == 4, want["stats"]
    got = series(obj, T, values, t0, t1, sd, h0=h0)
    print(family, top, np.dtype(dtype).name, got["stats"], [p["max_steps"] for p in want["per_call"]])
    assert_same_state(got, want)
    assert_counters(got, want, NCOLS)
    assert np.all(got["cols"] > 0)
    # the series is read: the value at t0 held through the call gives another state
    flat = {k: np.full_like(v, series_value(T, v, t0)) for k, v in values.items()}
    other = series(obj, T, flat, t0, t1, sd, h0=h0)
    assert np.max(np.abs(other["vl"].astype(np.float64) - got["vl"])) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_null_dt_cols_is_a_chain_from_a_zeroed_buffer(family, dtype):
    obj, sd = family_case(family, dtype, M.BC_FLUX)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(obj, M.BC_FLUX)
    want = chain(obj, T, values, t0, t1, 0.5 * sd)
    got = series(obj, T, values, t0, t1, 0.5 * sd, null_cols=True)
    assert_same_state(got, want, cols=False)
    assert_counters(got, want, NCOLS)
    # ... twice in one context: the library's buffer is zeroed for every call
    again = series(obj, T, values, t0, t1, 0.5 * sd, null_cols=True)
    assert_same_state(again, want, cols=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("family", ["richards", "layered"])
def test_fixed_steps_are_the_chain_bitwise(family, top, dtype):
    obj, sd = family_case(family, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(obj, top)
    dt = 2.0 * sd      # (no sub-interval is a multiple of it: every breakpoint clips a step)
    want = chain(obj, T, values, t0, t1, dt, fixed=True)
    got = series(obj, T, values, t0, t1, dt, fixed=True)
    assert_same_state(got, want)
    assert_counters(got, want, NCOLS)
    # steps of dt clipped at every breakpoint: ceil(length / dt) per sub-interval and column, the same for all
    bp = breakpoints(T, t0, t1)
    n = sum(int(np.ceil((b - a) / dt - 1e-9)) for a, b in zip(bp, bp[1:]))
    assert got["stats"]["accepted"] == n * NCOLS and got["stats"]["rejected"] == 0
    assert got["stats"]["max_steps"] == n and got["stats"]["wave_steps"] == 64 * 3 * n
    np.testing.assert_array_equal(got["cols"], np.full(NCOLS, np.float64(dtype(dt))))


# ------------------------------------------------------------------ 2. two knots

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_two_knots_on_t0_and_t1_is_one_call(family, dtype):
    obj, sd = family_case(family, dtype, M.BC_DIRICHLET)
    t0, t1 = 3.0 * sd, 17.0 * sd
    T = np.array([t0, t1])
    values = {k: v[[0, 3]] for k, v in uniform_values(obj, M.BC_DIRICHLET).items()}
    h0 = spread_steps(NCOLS, sd)
    want = chain(obj, T, values, t0, t1, sd, h0=h0)
    assert len(want["per_call"]) == 1
    got = series(obj, T, values, t0, t1, sd, h0=h0)
    assert_same_state(got, want)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])


# ------------------------------------------------------------------ 3. per-column series

def percol_values(values, ncols):
    """[nknots, ncols]: every column its own multiple (hydrology) or shift (energy) of the uniform series, per knot"""
    c = np.arange(ncols)
    out = {}
    for (f, k), v in values.items():
        u = np.stack([pc.uhash(c, 200 + 10 * j + k, 1) for j in range(len(v))])          # [nknots, ncols] in [0, 1)
        out[(f, k)] = v[:, None] * (0.8 + 0.4 * u) if k == M.COMP_HYDROLOGY else v[:, None] + 4.0 * (u - 0.5)
    return out


@pytest.mark.parametrize("transposed", [False, True], ids=["colstride1", "colstride_nknots"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_per_column_series_against_one_column_chains(family, dtype, transposed):
    top = M.BC_FLUX if transposed else M.BC_DIRICHLET
    obj, sd = family_case(family, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = percol_values(uniform_values(obj, top), NCOLS)
    h0 = spread_steps(NCOLS, sd)
    got = series(obj, T, values, t0, t1, sd, h0=h0, transposed=transposed)
    assert got["stats"]["failed"] == 0
    most = 0
    for c in (0, 70, NCOLS - 1):      # the first column, one of the middle wave, the last
        mine = {k: v[:, c] for k, v in values.items()}
        one = one_column(obj, c)
        want = chain(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        np.testing.assert_array_equal(got["vl"][c], want["vl"][0])
        if "rhoe" in want:
            np.testing.assert_array_equal(got["rhoe"][c], want["rhoe"][0])
        assert got["cols"][c] == want["cols"][0]
        # one column alone: its total of attempted steps is exact, and the wave costs 64 x it
        alone = series(one, T, mine, t0, t1, sd, h0=h0[c:c + 1])
        assert_same_state(alone, want)
        steps = want["stats"]["accepted"] + want["stats"]["rejected"]
        assert alone["stats"]["max_steps"] == steps and alone["stats"]["wave_steps"] == 64 * steps, (alone["stats"], steps)
        most = max(most, steps)
    assert got["stats"]["max_steps"] >= most


def test_a_series_wins_over_the_per_column_array_of_lh_set_bc():
    obj, sd = family_case("richards", np.float64, M.BC_DIRICHLET)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = percol_values(uniform_values(obj, M.BC_DIRICHLET), NCOLS)
    with_array = dataclasses.replace(obj, om=dataclasses.replace(
        obj.om, percol_bc={TOP_H: 0.30 + 0.1 * pc.uhash(np.arange(NCOLS), 5, 1)}))
    want = series(obj, T, values, t0, t1, sd)
    got = series(with_array, T, values, t0, t1, sd)
    assert_same_state(got, want)
    # (the array is in force without the series: another result)
    flat = chain(with_array, T, {}, t0, t1, sd, ends=[t0, t1])
    assert np.max(np.abs(flat["vl"] - want["vl"])) > 1e-6


# ------------------------------------------------------------------ 4. fixed steps against the NumPy reference

def test_fixed_step_parity_with_the_numpy_reference():
    """bonan_case, Float64: trbdf2_ref.trbdf2(adaptive=False, bcv=...) chained over the sub-intervals; within 1e-9
    (the bound test_boundary_values_linear_in_time holds for one interval), and an interior knot value is read."""
    case = bonan_case(ncols=2)
    T = np.array([0.0, 7.0, 18.0, 30.0, 44.0])
    v = np.array([0.20, 0.267, 0.22, 0.25, 0.267])
    t0, t1, dt = 2.0, 40.0, 4.0
    got = series(case, T, {TOP_H: v}, t0, t1, dt, fixed=True)
    assert got["status"] == 0 and got["stats"]["unconverged"] == 0
    y = case.vl[:1].astype(np.float64)
    bp = breakpoints(T, t0, t1)
    for a, b in zip(bp, bp[1:]):
        bcv = np.zeros((2, 2, 2))
        bcv[0][TOP_H], bcv[1][TOP_H] = series_value(T, v, a), series_value(T, v, b)
        y, _ = R.trbdf2(case.om, y, case.ti[:1], a, b, dt, adaptive=False, bcv=bcv)
    err = np.max(np.abs(got["vl"][0] - y[0]))
    print("fixed-step parity with the NumPy reference:", err)
    assert err < 1e-9, err
    moved = v.copy()
    moved[2] = 0.16
    other = series(case, T, {TOP_H: moved}, t0, t1, dt, fixed=True)
    assert np.max(np.abs(other["vl"] - got["vl"])) > 1e-6


# ------------------------------------------------------------------ 5. a failing column stops

def test_a_failing_column_stops():
    """Float32 with a tolerance it cannot meet (test_column_independence_and_failed_columns): every column fails in
    its first sub-interval and integrates no further."""
    c32 = richards_case(M.BC_FLUX, M.BC_FLUX, dtype=np.float32, ncols=64)
    sd = stable_dt(c32)
    T = np.array([0.0, 3.0, 5.0, 8.0, 11.0]) * sd
    values = {TOP_H: -2e-9 * SHAPE_H[M.BC_FLUX]}
    got = series(c32, T, values, 0.5 * sd, 10 * sd, sd, abstol=1e-14, reltol=1e-14)
    st = got["stats"]
    assert got["status"] & STATUS_FAILED and st["failed"] == 64, (got["status"], st)
    assert st["accepted"] == 0 and np.all(got["cols"] == 0)
    np.testing.assert_array_equal(got["vl"], c32.vl)
    # (a column that went on after failing would be counted once per sub-interval)
    one = chain(c32, T, values, 0.5 * sd, 10 * sd, sd, abstol=1e-14, reltol=1e-14, ends=[0.5 * sd, 3.0 * sd])
    assert st["rejected"] == one["stats"]["rejected"] and st["max_steps"] == one["stats"]["max_steps"]


# ------------------------------------------------------------------ 6. refusals and the contract

def _refused(gm, rc, code, *words):
    msg = gm.L.lh_last_error(gm.ctx).decode()
    assert rc == code, (rc, code, msg)
    for w in ("lh_integrate_series",) + words:
        assert w in msg, (w, msg)
    assert all(v == 0 for v in _stats(gm).values()), "statistics after a refused call"


def test_refusals_and_the_contract():
    obj, sd = family_case("richards", np.float64, M.BC_FLUX)
    T = KNOTS * sd
    vals = {TOP_H: obj.om.bc[TOP_H][1] * SHAPE_H[M.BC_FLUX]}
    nan, inf = float("nan"), float("inf")
    with pc.GpuModel(obj) as gm, pc.GpuModel(obj) as other:
        F, L = gm.F, gm.L
        EINVAL, EMODEL = F.LH_EINVAL, F.LH_EMODEL
        Y, Ya = gm.prognostic_and_aux()
        # ---- the series object: create, set, remove, destroy
        h = C.c_void_p()
        for bad, word in ((np.array([0.0]), "nknots"), (np.array([0.0, 1.0, 1.0]), "knot 2"), (np.array([0.0, nan, 2.0]), "knot 1"),
                          (np.array([0.0, 2.0, 1.0, 3.0]), "knot 2"), (np.array([0.0, inf]), "knot 1")):
            assert L.lh_bc_series_create(gm.ctx, len(bad), _dptr(bad), C.byref(h)) == EINVAL and not h.value
            assert word in L.lh_last_error(gm.ctx).decode(), (word, L.lh_last_error(gm.ctx))
        assert L.lh_bc_series_create(gm.ctx, 5, None, C.byref(h)) == EINVAL
        assert L.lh_bc_series_create(None, 5, _dptr(T), C.byref(h)) == EINVAL
        h = make_series(gm, T, vals)
        v0 = np.ascontiguousarray(vals[TOP_H])
        assert L.lh_bc_series_set(gm.ctx, h, 2, M.COMP_HYDROLOGY, _dptr(v0), 1, 0) == EINVAL
        assert L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, 2, _dptr(v0), 1, 0) == EINVAL
        assert L.lh_bc_series_set(gm.ctx, None, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(v0), 1, 0) == EINVAL
        assert L.lh_bc_series_set(other.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(v0), 1, 0) == EINVAL
        assert L.lh_bc_series_destroy(other.ctx, h) == EINVAL
        assert L.lh_bc_series_destroy(gm.ctx, None) == F.LH_OK

        def call(series_h=h, t0=T0 * sd, t1=T1 * sd, dt=sd, abstol=0.0, abstol_e=0.0, reltol=0.0, flags=0, ctx=gm, Y=Y, Ya=Ya):
            return L.lh_integrate_series(ctx.ctx, Y, Ya, series_h, t0, t1, dt, abstol, abstol_e, reltol, flags, None)

        # a run first, so that the statistics are not zero before the refusals
        F.check(call(), gm.ctx)
        ran = _stats(gm)
        assert ran["accepted"] > 0
        first = gm.download(Y, F.LH_VAR_VARTHETA_L)
        # ---- LH_EINVAL
        _refused(gm, call(series_h=None), EINVAL, "NULL")
        foreign = make_series(other, T, vals)
        _refused(gm, call(series_h=foreign), EINVAL, "not a series of this context")
        _refused(gm, call(t0=2.0 * sd, t1=1.0 * sd), EINVAL, "t0 <= t1")
        _refused(gm, call(t1=nan), EINVAL)
        _refused(gm, call(dt=0.0), EINVAL, "dt > 0")
        _refused(gm, call(dt=inf), EINVAL)
        _refused(gm, call(abstol=-1e-6), EINVAL, "tolerances")
        _refused(gm, call(reltol=nan), EINVAL, "tolerances")
        _refused(gm, call(flags=2), EINVAL, "unknown flags")
        _refused(gm, call(t0=-0.5 * sd), EINVAL, "no extrapolation")
        _refused(gm, call(t1=T[-1] + 0.5 * sd), EINVAL, "no extrapolation")
        # ---- the call goes on working, t0 == t1 does nothing, a removed component falls back to lh_set_bc's value
        F.check(call(), gm.ctx)
        before = gm.download(Y, F.LH_VAR_VARTHETA_L)
        assert np.max(np.abs(before - first)) > 0
        F.check(call(t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), before)
        assert all(v == 0 for v in _stats(gm).values())
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        Y2, _ = gm.prognostic_and_aux()
        Y3, _ = gm.prognostic_and_aux()
        F.check(call(Y=Y2, t0=T[1], t1=T[2]), gm.ctx)        # an empty series: one sub-interval with lh_set_bc's values
        F.check(L.lh_integrate_trbdf2(gm.ctx, Y3, Ya, T[1], T[2], sd, 0.0, 0.0, 0, None, None), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y2, F.LH_VAR_VARTHETA_L), gm.download(Y3, F.LH_VAR_VARTHETA_L))
        # ---- LH_EMODEL: a component the model does not have, a kind that reads no value
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_ENERGY, _dptr(v0), 1, 0), gm.ctx)
        _refused(gm, call(), EMODEL, "energy")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_ENERGY, None, 0, 0), gm.ctx)
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)   # free drainage
        _refused(gm, call(), EMODEL, "bottom hydrology", "reads no value")
        # ---- what lh_integrate_trbdf2 refuses: conductivity factors; a class map without the layered requirements
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)
        cf = M.default_cf(impedance=True)
        F.check(L.lh_set_conductivity_factors(gm.ctx, cf.viscosity_kind, cf.gamma, cf.T_ref, cf.impedance_kind, cf.Omega), gm.ctx)
        _refused(gm, call(), EMODEL, "conductivity factors")
        F.check(L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        assert L.lh_bc_series_destroy(gm.ctx, h) == EINVAL          # (no longer a series of the context)
        # (`foreign` is left to lh_destroy)
    # ---- a heat-only context; the coupled model: flags, and a class map
    heat = pc.make_case("heat_dirichlet_f64", ncols=64)
    with pc.GpuModel(heat) as gm:
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, {})
        _refused(gm, gm.L.lh_integrate_series(gm.ctx, Y, Ya, h, T[0], T[1], sd, 0.0, 0.0, 0.0, 0, None), gm.F.LH_EMODEL)
    cpl, sdc = family_case("coupled", np.float64, M.BC_FLUX)
    with pc.GpuModel(cpl) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        Tc = KNOTS * sdc
        h = make_series(gm, Tc, uniform_values(cpl, M.BC_FLUX))
        _refused(gm, L.lh_integrate_series(gm.ctx, Y, Ya, h, Tc[0], Tc[1], sdc, 0.0, 0.0, 0.0, F.LH_TRBDF2_FIXED, None),
                 F.LH_EINVAL, "unknown flags")
        _refused(gm, L.lh_integrate_series(gm.ctx, Y, Ya, h, Tc[0], Tc[1], sdc, 0.0, -1.0, 0.0, 0, None), F.LH_EINVAL, "tolerances")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_BOTTOM, M.COMP_ENERGY, _dptr(np.zeros(5)), 1, 0), gm.ctx)   # a flux: fine
        F.check(L.lh_integrate_series(gm.ctx, Y, Ya, h, Tc[0], Tc[1], sdc, 0.0, 0.0, 0.0, 0, None), gm.ctx)
        thermal = [(1.0e6, 7.0, 2700.0, 2.0, 4.0, 0.0, 0.0, 0.9)] * 2
        gm.set_soil_classes(SAND_OVER_CLAY, np.zeros(NLEV, dtype=np.uint8), thermal=thermal)
        _refused(gm, L.lh_integrate_series(gm.ctx, Y, Ya, h, Tc[0], Tc[1], sdc, 0.0, 0.0, 0.0, 0, None), F.LH_EMODEL,
                 "soil classes")
    # ---- a layered Richards context with per-column parameters: lh_integrate_layered_trbdf2's refusal
    lay, sdl = family_case("layered", np.float64, M.BC_FLUX)
    with layered_gpu(lay) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        Tl = KNOTS * sdl
        h = make_series(gm, Tl, uniform_values(lay, M.BC_FLUX))
        nu = np.full(NCOLS, 0.45)
        F.check(L.lh_set_percol_param(gm.ctx, F.LH_PC["nu"], _dptr(nu)), gm.ctx)
        _refused(gm, L.lh_integrate_series(gm.ctx, Y, Ya, h, Tl[0], Tl[1], sdl, 0.0, 0.0, 0.0, 0, None), F.LH_EMODEL,
                 "per-column parameter arrays")


# ------------------------------------------------------------------ 7. the host mirror

def test_host_mirror():
    lh = g.load_package()
    FT = np.float64
    sp, vg = pc.coupled_soil()
    flux0 = -2e-9

    def model_and_states():
        model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-0.24, 0.0), nelements=NLEV, ncolumns=NCOLS),
                             energy_model=lh.PrescribedTemperatureModel(),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(
                                 FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)),
                             boundary_conditions=lh.SoilColumnBC(
                                 top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(flux0)),
                                 bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                             soil_param_set=lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s), earth_param_set=lh.EarthParameterSet())
        init = lambda z, m: {"ϑ_l": 0.2 + 0.1 * np.exp(4.0 * z), "θ_i": 0.0 * z}
        return model, [lh.initialize_states(model, init, 0.0) for _ in range(2)]

    model, ((Y1, Ya), (Y2, _)) = model_and_states()
    sd = lh.stable_dt(model, Y1, Ya, 0.5)
    T = KNOTS * sd
    vals = flux0 * SHAPE_H[M.BC_FLUX][:, None] * (0.8 + 0.4 * pc.uhash(np.arange(NCOLS), 3, 1))[None, :]
    fs = lh.BoundarySeries(T, {("top", "hydrology"): vals})
    st = lh.integrate_series(model, Y1, Ya, fs, T0 * sd, T1 * sd, sd)
    assert st["failed"] == 0 and st["accepted"] >= 4 * NCOLS, st
    # the ctypes call on the same context, a series of its own
    F = lh._ffi
    L, be = F.lib(), model._backend()
    h = C.c_void_p()
    Tc = np.ascontiguousarray(T)
    F.check(L.lh_bc_series_create(be.ctx, 5, _dptr(Tc), C.byref(h)), be.ctx)
    a = np.ascontiguousarray(vals)
    F.check(L.lh_bc_series_set(be.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(a), NCOLS, 1), be.ctx)
    F.check(L.lh_integrate_series(be.ctx, Y2.handle, None, h, T0 * sd, T1 * sd, sd, 1e-6, 0.0, 1e-3, 0, None), be.ctx)
    np.testing.assert_array_equal(Y2.get("ϑ_l"), Y1.get("ϑ_l"))
    # Simulation over the whole series: one integrate_series call per advance
    model_b, ((Z1, Za), (Z2, _)) = model_and_states()
    sim = lh.Simulation(model_b, lh.TRBDF2(forcing=fs), Y_init=Z1, dt=sd, tspan=(T[0], T[-1]), Ya_init=Za)
    lh.run(sim)
    want_stats = lh.integrate_series(model_b, Z2, Za, fs, T[0], T[-1], sd)
    np.testing.assert_array_equal(Z1.get("ϑ_l"), Z2.get("ϑ_l"))
    assert sim.integrator.trbdf2_stats == want_stats, (sim.integrator.trbdf2_stats, want_stats)
    assert sim.integrator.t == T[-1] and want_stats["failed"] == 0
    with pytest.raises(ValueError):
        lh.integrate_series(model, Y1, Ya, fs, T[0] - 1.0, T[1], sd)
