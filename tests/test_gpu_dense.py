"""lh_integrate_dense: the adaptive TR-BDF2 integrators with output interpolated inside the launch (DESIGN.md section
4.29).  The integration must not see the output (bitwise the twin call), every snapshot is the cubic Hermite
interpolant of the accepted step that contains its time, and the clipped chain of existing calls is the yardstick
for accuracy and for what the output costs in steps."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import dense_ref as D
import layered_ref as LR
import parity_cases as pc
from test_gpu_bc_series import (KEYS, KNOTS, NCOLS, NLEV, SAND_OVER_CLAY, SHAPE_H, STATUS_FAILED, T0, T1, TOP_H, _case_of, _dptr,
                                _family_of, _open, _result, _stats, _step_buffer, assert_same_state, family_case,
                                make_series, one_column, series, spread_steps, uniform_values)
from test_gpu_implicit import richards_case, stable_dt

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
FAMILIES = ["richards", "layered", "coupled"]
TOPS = [M.BC_FLUX, M.BC_DIRICHLET]
TOP_IDS = ["flux", "dirichlet"]
# 9 save times in units of the stable step between T0 = 2.5 and T1 = 28 (knots at 0, 7, 12, 25, 31): t0 itself, two
# more inside the first knot interval, one on a knot, ..., one == t1
SAVES = np.array([2.5, 4.0, 5.5, 7.0, 9.0, 12.5, 18.0, 26.5, 28.0])


def _snapshots(gm, handles):
    F = gm.F
    out = []
    for h in handles:
        s = dict(vl=gm.download(h, F.LH_VAR_VARTHETA_L))
        if gm.case.om.model == M.MODEL_COUPLED:
            s["rhoe"] = gm.download(h, F.LH_VAR_RHOE_INT)
        out.append(s)
    return out


def _handles(snaps):
    return (C.c_void_p * max(len(snaps), 1))(*[s.value for s in snaps]) if len(snaps) else None


def dense(obj, t0, t1, dt, saves, T=None, values=None, h0=None, fixed=False, abstol=0.0, abstol_e=0.0, reltol=0.0,
          null_cols=False):
    """One lh_integrate_dense call; T = None: no series."""
    case = _case_of(obj)
    with _open(obj) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        cols = None if null_cols else _step_buffer(case, h0)
        h = None if T is None else make_series(gm, T, values)
        s = np.ascontiguousarray(saves, dtype=np.float64)
        snaps = [gm.state(0) for _ in range(len(s))]
        F.check(gm.L.lh_integrate_dense(gm.ctx, Y, Ya, h, t0, t1, dt, abstol, abstol_e, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                                        None if cols is None else C.c_void_p(cols.data_ptr()), len(s), _dptr(s) if len(s) else None,
                                        _handles(snaps)), gm.ctx)
        out = _result(gm, Y, cols, _stats(gm), snaps=_snapshots(gm, snaps))
        if h is not None:
            F.check(gm.L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        return out


def plain(obj, t0, t1, dt, h0=None, fixed=False, abstol=0.0, abstol_e=0.0, reltol=0.0, null_cols=False, stops=None):
    """The existing entry point with bcv = NULL; `stops`: a chain of calls clipped at these times (each ends a call,
    the last one is t1), the state downloaded after each."""
    case, family = _case_of(obj), _family_of(obj)
    with _open(obj) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        cols = None if null_cols else _step_buffer(case, h0)
        ptr = None if cols is None else C.c_void_p(cols.data_ptr())
        total = dict.fromkeys(KEYS, 0)
        states = []
        ends = [t0] + ([t1] if stops is None else [float(x) for x in stops])
        for a, b in zip(ends, ends[1:]):
            if family == "coupled":
                rc = L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, a, b, dt, abstol, abstol_e, reltol, 0, ptr, None)
            else:
                call = L.lh_integrate_layered_trbdf2 if family == "layered" else L.lh_integrate_trbdf2
                rc = call(gm.ctx, Y, Ya, a, b, dt, abstol, reltol, F.LH_TRBDF2_FIXED if fixed else 0, ptr, None)
            F.check(rc, gm.ctx)
            st = _stats(gm)
            for key in KEYS:
                total[key] = st[key] if stops is None else total[key] + st[key]
            if stops is not None:
                states.extend(_snapshots(gm, [Y]))
        return _result(gm, Y, cols, total, snaps=states)


def assert_invisible(got, twin):
    """Contract item 1: Y, dt_cols, the status word and all seven counters are the twin call's, bitwise."""
    assert_same_state(got, twin, cols=twin["cols"] is not None)
    assert got["stats"] == twin["stats"], (got["stats"], twin["stats"])


def assert_snapshot_is(snap, vl, rhoe=None):
    np.testing.assert_array_equal(snap["vl"], vl)
    if rhoe is not None:
        np.testing.assert_array_equal(snap["rhoe"], rhoe)


# ------------------------------------------------------------------ 1. the integration does not see the output

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_output_is_invisible_with_a_series(family, top, dtype):
    obj, sd = family_case(family, dtype, top)
    case = _case_of(obj)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(obj, top)
    h0 = spread_steps(NCOLS, sd)
    s = SAVES * sd
    assert s[0] == t0 and s[-1] == t1 and s[3] == T[1] and T[0] < s[1] < s[2] < T[1]
    twin = series(obj, T, values, t0, t1, sd, h0=h0)
    assert twin["stats"]["failed"] == 0 and twin["stats"]["accepted"] > 4 * NCOLS, twin["stats"]
    got = dense(obj, t0, t1, sd, s, T, values, h0=h0)
    assert_invisible(got, twin)
    # the endpoints: s == t0 is the state as passed, s == t1 the final Y
    assert_snapshot_is(got["snaps"][0], case.vl, case.rhoe if "rhoe" in got else None)
    assert_snapshot_is(got["snaps"][-1], got["vl"], got.get("rhoe"))
    # every snapshot in between was written (the states are created zeroed) and the state moves through them
    for k in range(1, len(s)):
        assert np.all(got["snaps"][k]["vl"] > 0) and np.all(np.isfinite(got["snaps"][k]["vl"]))
        assert np.max(np.abs(got["snaps"][k]["vl"].astype(np.float64) - got["snaps"][k - 1]["vl"])) > 0
    # nsave = 0 is the twin call
    none = dense(obj, t0, t1, sd, [], T, values, h0=h0)
    assert_invisible(none, twin)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,top,percol", [("richards", M.BC_DIRICHLET, True), ("richards", M.BC_FLUX, False),
                                               ("layered", M.BC_DIRICHLET, False), ("coupled", M.BC_FLUX, False)],
                         ids=["richards-percol-bc", "richards", "layered", "coupled"])
def test_output_is_invisible_without_a_series(family, top, percol, dtype):
    obj, sd = family_case(family, dtype, top)
    if percol:     # a per-column lh_set_bc array at the Dirichlet top
        obj = dataclasses.replace(obj, om=dataclasses.replace(
            obj.om, percol_bc={TOP_H: 0.30 + 0.1 * pc.uhash(np.arange(NCOLS), 5, 1)}))
    case = _case_of(obj)
    t0, t1 = T0 * sd, T1 * sd
    h0 = spread_steps(NCOLS, sd)
    twin = plain(obj, t0, t1, sd, h0=h0)
    assert twin["stats"]["failed"] == 0
    got = dense(obj, t0, t1, sd, SAVES * sd, h0=h0)
    assert_invisible(got, twin)
    assert_snapshot_is(got["snaps"][0], case.vl, case.rhoe if "rhoe" in got else None)
    assert_snapshot_is(got["snaps"][-1], got["vl"], got.get("rhoe"))
    assert_invisible(dense(obj, t0, t1, sd, [], h0=h0), twin)
    if percol:      # (the array is read: the uniform value gives another state)
        flat, _ = family_case(family, dtype, top)
        assert np.max(np.abs(plain(flat, t0, t1, sd, h0=h0)["vl"].astype(np.float64) - twin["vl"])) > 0
    # without step proposals from the caller, as the twin
    assert_invisible(dense(obj, t0, t1, sd, SAVES * sd, null_cols=True), plain(obj, t0, t1, sd, null_cols=True))


# ------------------------------------------------------------------ 2. the formula

GAMMA = 2.0 - np.sqrt(2.0)
D_TR = 0.5 * GAMMA


def _tendency(obj, vl):
    """lh_rhs at vl (the case's other fields and boundary values), and test_gpu_implicit.round_off's scale"""
    case = _case_of(obj)
    c1 = dataclasses.replace(case, vl=np.ascontiguousarray(vl))
    o1 = LR.Layered(c1, obj.classes, obj.class_map) if isinstance(obj, LR.Layered) else c1
    with _open(o1) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        return gm.tendencies(dY)["vl"].astype(np.float64)


# One fixed step of h from t0 = 0 (LH_TRBDF2_FIXED, t1 - t0 = dt = h) with snapshots at theta = 1/4, 1/2, 3/4, against
# dense_ref.hermite in Float64 from Y0, Y1 and lh_rhs at both.  The device's f0 IS lh_rhs(Y0) (the column routines'
# tendency is rhs_kernel's, bitwise), so it differs from the host's evaluation only
#   (a) through the roundings of evaluating the formula in FT, and
#   (b) through f1: the device takes h f1 = (Y1 - w2) / d, the host h lh_rhs(Y1); stage 2 solves
#       R2 = Y1 - w2 - d h f(Y1) = 0, so h f1 - h f(Y1) = R2 / d, which enters u with the coefficient
#       theta (theta - 1) * theta: |u_dev - u_host| <= |theta^2 (theta - 1)| |R2| / d.
# R2 is a Newton residual with the stage coefficient d h where backward Euler has dt: test_gpu_implicit's stated bound
# |R| <= 10 tol nu (1 + 4 dt / stable_dt) + round_off with dt = d h (tol = 1e-10 in Float64, 1e-5 in Float32: the fixed
# mode's Newton test is backward Euler's).  max over the three theta of |theta^2 (theta - 1)| is 9/64 at theta = 3/4.
# (a) is a handful of roundings of terms no larger than max(|v|, h |f|): round_off's 64 eps of that scale, with dt = h,
# covers them (and, since d < 1, the residual's own round_off term, which is therefore not added a second time).
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("family", ["richards", "layered"])
def test_the_formula_on_one_fixed_step(family, top, dtype):
    obj, sd = family_case(family, dtype, top)
    case = _case_of(obj)
    h = 10.0 * sd
    thetas = np.array([0.25, 0.5, 0.75])
    got = dense(obj, 0.0, h, h, thetas * h, fixed=True)
    assert got["stats"]["accepted"] == NCOLS and got["stats"]["unconverged"] == 0 and got["status"] == 0, got["stats"]
    y0, y1 = case.vl.astype(np.float64), got["vl"].astype(np.float64)
    f0, f1 = _tendency(obj, case.vl), _tendency(obj, got["vl"])
    tol = 1e-10 if dtype == np.float64 else 1e-5
    nu = float(np.max(obj.classes[:, 4])) if family == "layered" else case.om.soil.nu
    residual = 10 * tol * nu * (1 + 4 * D_TR * h / sd)
    big = np.maximum(np.abs(y1).max(axis=1), h * np.abs(f1).max(axis=1))
    round_off = 64 * np.finfo(dtype).eps * big                       # (test_gpu_implicit.round_off with dt = h)
    bound = np.max(np.abs(thetas ** 2 * (thetas - 1))) / D_TR * residual + round_off
    for th, snap in zip(thetas, got["snaps"]):
        want = D.hermite(th, h, y0, y1, f0, f1)
        err = np.max(np.abs(snap["vl"].astype(np.float64) - want), axis=1)
        print(family, top, np.dtype(dtype).name, "theta", th, "max error", float(err.max()), "bound", float(bound.min()))
        assert np.all(err <= bound), (th, float(err.max()), float(bound.min()))
        if dtype == np.float64:      # (the interpolant is far from the chord on this step: the test reads f0 and f1)
            assert np.max(np.abs(want - ((1 - th) * y0 + th * y1))) > 100 * float(bound.max())


# ------------------------------------------------------------------ 3. accuracy and the payoff, against the clipped chain

NSNAP = 25
# E_dense / max(E_chain, 1) as measured on the MI355X, per (family, dtype, top); the
# assertion allows twice the largest.  A ratio above 10 would be a defect to find, not a tolerance to set.
RECORDED_RATIO = {("richards", "flux", "f64"): 3.046, ("richards", "flux", "f32"): 3.046,
                  ("richards", "dirichlet", "f64"): 2.664, ("richards", "dirichlet", "f32"): 2.664,
                  ("layered", "flux", "f64"): 3.233, ("layered", "flux", "f32"): 3.233,
                  ("layered", "dirichlet", "f64"): 1.491, ("layered", "dirichlet", "f32"): 1.491,
                  ("coupled", "flux", "f64"): 0.9831, ("coupled", "flux", "f32"): 0.9831,
                  ("coupled", "dirichlet", "f64"): 1.011, ("coupled", "dirichlet", "f32"): 1.011}
RATIO_ALLOWED = 2.0 * max(RECORDED_RATIO.values())


@functools.lru_cache(maxsize=None)
def _truth(family, top):
    """The Float64 chain of existing calls clipped at the save times, at tolerances 100x tighter than the defaults"""
    obj, sd = family_case(family, np.float64, top)
    e = _case_of(obj).om.earth
    out = plain(obj, 0.0, NSNAP * sd, sd, h0=spread_steps(NCOLS, sd), abstol=1e-8, abstol_e=1e-8 * e.cp_l * e.rho_liq, reltol=1e-5,
                stops=np.arange(1, NSNAP + 1) * sd)
    assert out["stats"]["failed"] == 0 and out["status"] == 0
    return out["snaps"], sd


def _scaled_error(snaps, truth, abstol_e):
    worst = 0.0
    for s, t in zip(snaps, truth):
        v = t["vl"]
        worst = max(worst, float(np.max(np.abs(s["vl"].astype(np.float64) - v) / (1e-6 + 1e-3 * np.abs(v)))))
        if "rhoe" in t:
            x = t["rhoe"]
            worst = max(worst, float(np.max(np.abs(s["rhoe"].astype(np.float64) - x) / (abstol_e + 1e-3 * np.abs(x)))))
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_accuracy_and_step_counts_against_the_clipped_chain(family, top, dtype):
    truth, sd = _truth(family, top)          # (the Float64 case's stable step: the save times are the truth's)
    obj, _ = family_case(family, dtype, top)
    e = _case_of(obj).om.earth
    abstol_e = 1e-6 * e.cp_l * e.rho_liq       # (the library's default, spelled out for the scaling)
    s = np.arange(1, NSNAP + 1) * sd
    h0 = spread_steps(NCOLS, sd)
    clipped = plain(obj, 0.0, s[-1], sd, h0=h0, stops=s)
    assert clipped["stats"]["failed"] == 0 and clipped["status"] == 0, clipped["stats"]
    got = dense(obj, 0.0, s[-1], sd, s, h0=h0)
    assert got["stats"]["failed"] == 0 and got["status"] == 0, got["stats"]
    E_chain = _scaled_error(clipped["snaps"], truth, abstol_e)
    E_dense = _scaled_error(got["snaps"], truth, abstol_e)
    ratio = E_dense / max(E_chain, 1.0)
    print("dense-accuracy", family, TOP_IDS[TOPS.index(top)], np.dtype(dtype).name, "E_chain %.4g E_dense %.4g ratio %.4g" %
          (E_chain, E_dense, ratio), "accepted chain/dense", clipped["stats"]["accepted"], got["stats"]["accepted"],
          "newton chain/dense", clipped["stats"]["newton_iterations"], got["stats"]["newton_iterations"])
    assert ratio <= RATIO_ALLOWED, (ratio, RATIO_ALLOWED)
    # the payoff: the output no longer sets the steps
    assert got["stats"]["accepted"] <= clipped["stats"]["accepted"], (got["stats"], clipped["stats"])
    assert got["stats"]["newton_iterations"] <= clipped["stats"]["newton_iterations"], (got["stats"], clipped["stats"])


# ------------------------------------------------------------------ 4. column independence

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_a_columns_snapshots_are_its_own(family, dtype):
    top = M.BC_DIRICHLET if family == "layered" else M.BC_FLUX
    obj, sd = family_case(family, dtype, top)
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    values = uniform_values(obj, top)
    h0 = spread_steps(NCOLS, sd)
    s = SAVES * sd
    got = dense(obj, t0, t1, sd, s, T, values, h0=h0)
    assert got["stats"]["failed"] == 0
    for c in (0, 37, 64, 101, NCOLS - 1):      # spread over the three waves
        alone = dense(one_column(obj, c), t0, t1, sd, s, T, values, h0=h0[c:c + 1])
        for k in range(len(s)):
            np.testing.assert_array_equal(got["snaps"][k]["vl"][c], alone["snaps"][k]["vl"][0])
            if "rhoe" in got:
                np.testing.assert_array_equal(got["snaps"][k]["rhoe"][c], alone["snaps"][k]["rhoe"][0])
        np.testing.assert_array_equal(got["vl"][c], alone["vl"][0])
        assert got["cols"][c] == alone["cols"][0]


# ------------------------------------------------------------------ 5. a failing column

def test_a_failing_column_fills_its_snapshots_with_its_kept_state():
    """test_gpu_bc_series.test_a_failing_column_stops' setup: Float32 with tolerances it cannot meet."""
    c32 = richards_case(M.BC_FLUX, M.BC_FLUX, dtype=np.float32, ncols=64)
    sd = stable_dt(c32)
    T = np.array([0.0, 3.0, 5.0, 8.0, 11.0]) * sd
    values = {TOP_H: -2e-9 * SHAPE_H[M.BC_FLUX]}
    t0, t1 = 0.5 * sd, 10 * sd
    # (the reference run: the same call without output fails every column in its first sub-interval)
    ref = series(c32, T, values, t0, t1, sd, abstol=1e-14, reltol=1e-14)
    assert ref["status"] & STATUS_FAILED and ref["stats"]["failed"] == 64 and ref["stats"]["accepted"] == 0, ref["stats"]
    got = dense(c32, t0, t1, sd, np.array([0.5, 2.0, 3.0, 6.0, 10.0]) * sd, T, values, abstol=1e-14, reltol=1e-14)
    assert got["status"] & STATUS_FAILED and got["stats"]["failed"] == 64, (got["status"], got["stats"])
    assert got["stats"] == ref["stats"]
    assert np.all(got["cols"] == 0)
    np.testing.assert_array_equal(got["vl"], c32.vl)
    for snap in got["snaps"]:
        np.testing.assert_array_equal(snap["vl"], c32.vl)


# ------------------------------------------------------------------ 6. refusals

def _refused(gm, rc, code, *words):
    msg = gm.L.lh_last_error(gm.ctx).decode()
    assert rc == code, (rc, code, msg)
    for w in ("lh_integrate_dense",) + words:
        assert w in msg, (w, msg)
    assert all(v == 0 for v in _stats(gm).values()), "statistics after a refused call"


def test_refusals_leave_everything_untouched():
    obj, sd = family_case("richards", np.float64, M.BC_FLUX)
    T = KNOTS * sd
    vals = {TOP_H: obj.om.bc[TOP_H][1] * SHAPE_H[M.BC_FLUX]}
    nan = float("nan")
    t0, t1 = T0 * sd, T1 * sd
    with pc.GpuModel(obj) as gm, pc.GpuModel(obj) as other:
        F, L = gm.F, gm.L
        EINVAL = F.LH_EINVAL
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)
        marks = [np.full((NCOLS, NLEV), 0.1 * (k + 1)) for k in range(3)]
        snaps = [gm.state(0) for _ in range(3)]
        for sn, a in zip(snaps, marks):
            gm.upload(sn, F.LH_VAR_VARTHETA_L, a)
        no_water = gm.state(1 << F.LH_VAR_THETA_I)
        foreign = other.state(0)
        good = np.array([3.0, 9.0, 20.0]) * sd

        def call(times=good, states=snaps, nsave=None, series_h=h, dt=sd, t0=t0, t1=t1, null_times=False, null_states=False):
            s = np.ascontiguousarray(times, dtype=np.float64)
            arr = (C.c_void_p * max(len(states), 1))(*[None if x is None else x.value for x in states])
            return L.lh_integrate_dense(gm.ctx, Y, Ya, series_h, t0, t1, dt, 0.0, 0.0, 0.0, 0, None,
                                        len(s) if nsave is None else nsave, None if null_times else _dptr(s),
                                        None if null_states else arr)

        # a run first, so that the statistics are not zero before the refusals (into states of its own)
        F.check(call(states=[gm.state(0) for _ in range(3)]), gm.ctx)
        assert _stats(gm)["accepted"] > 0
        before = gm.download(Y, F.LH_VAR_VARTHETA_L)
        # ---- the wrapped call's refusals come first
        _refused(gm, call(dt=0.0, nsave=-1), EINVAL, "dt > 0")
        _refused(gm, call(t0=-0.5 * sd, nsave=-1), EINVAL, "no extrapolation")
        _refused(gm, call(series_h=make_series(other, T, vals)), EINVAL, "not a series of this context")
        # ---- the new ones
        _refused(gm, call(nsave=-1), EINVAL, "nsave = -1")
        _refused(gm, call(nsave=65537), EINVAL, "nsave = 65537")
        _refused(gm, call(null_times=True), EINVAL, "NULL", "save_times")
        _refused(gm, call(null_states=True), EINVAL, "NULL", "snapshots")
        _refused(gm, call(times=np.array([3.0, 20.0, 9.0]) * sd), EINVAL, "save time 2", "strictly increasing")
        _refused(gm, call(times=np.array([3.0, 3.0, 9.0]) * sd), EINVAL, "save time 1", "strictly increasing")
        _refused(gm, call(times=np.array([3.0, nan, 9.0]) * sd), EINVAL, "save time 1", "not finite")
        _refused(gm, call(times=np.array([2.0, 9.0, 20.0]) * sd), EINVAL, "save time 0", "outside")
        _refused(gm, call(times=np.array([3.0, 9.0, 28.5]) * sd), EINVAL, "save time 2", "outside")
        _refused(gm, call(states=[snaps[0], None, snaps[2]]), EINVAL, "snapshot 1", "NULL")
        _refused(gm, call(states=[snaps[0], snaps[1], foreign]), EINVAL, "snapshot 2", "not a state of this context")
        _refused(gm, call(states=[snaps[0], Y, snaps[2]]), EINVAL, "snapshot 1 is Y")
        _refused(gm, call(states=[snaps[0], snaps[1], snaps[0]]), EINVAL, "snapshot 2 is snapshot 0")
        _refused(gm, call(states=[no_water, snaps[1], snaps[2]]), EINVAL, "snapshot 0", "lacks a plane")
        # ---- Y and the snapshots are as they were
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), before)
        for sn, a in zip(snaps, marks):
            np.testing.assert_array_equal(gm.download(sn, F.LH_VAR_VARTHETA_L), a)
        # ---- and the call goes on working: only vartheta_l of a snapshot is written, t0 == t1 writes Y as passed
        ti_mark = np.full((NCOLS, NLEV), 0.0125)
        gm.upload(snaps[0], F.LH_VAR_THETA_I, ti_mark)
        F.check(call(), gm.ctx)
        assert np.max(np.abs(gm.download(snaps[0], F.LH_VAR_VARTHETA_L) - marks[0])) > 0
        np.testing.assert_array_equal(gm.download(snaps[0], F.LH_VAR_THETA_I), ti_mark)
        now = gm.download(Y, F.LH_VAR_VARTHETA_L)
        F.check(call(times=[3.0 * sd], states=snaps[:1], t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(snaps[0], F.LH_VAR_VARTHETA_L), now)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), now)
        assert all(v == 0 for v in _stats(gm).values())
    # ---- a coupled context: Ya as a snapshot where there is one, a snapshot without rhoe_int; then a class map
    cpl, sdc = family_case("coupled", np.float64, M.BC_FLUX)
    with pc.GpuModel(cpl) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        s = np.array([1.0, 2.0]) * sdc
        water_only = gm.state((1 << F.LH_VAR_VARTHETA_L) | (1 << F.LH_VAR_THETA_I))
        full = gm.state(0)

        def ccall(states):
            arr = (C.c_void_p * 2)(*[x.value for x in states])
            return L.lh_integrate_dense(gm.ctx, Y, Ya, None, 0.0, 3.0 * sdc, sdc, 0.0, 0.0, 0.0, 0, None, 2, _dptr(s), arr)

        _refused(gm, ccall([full, water_only]), F.LH_EINVAL, "snapshot 1", "lacks a plane")
        if Ya is not None:
            _refused(gm, ccall([full, Ya]), F.LH_EINVAL, "snapshot 1 is Ya")
        _refused(gm, L.lh_integrate_dense(gm.ctx, Y, Ya, None, 0.0, 3.0 * sdc, sdc, 0.0, 0.0, 0.0, F.LH_TRBDF2_FIXED, None, 0, None, None),
                 F.LH_EINVAL, "unknown flags")
        thermal = [(1.0e6, 7.0, 2700.0, 2.0, 4.0, 0.0, 0.0, 0.9)] * 2
        gm.set_soil_classes(SAND_OVER_CLAY, np.zeros(NLEV, dtype=np.uint8), thermal=thermal)
        _refused(gm, ccall([full, gm.state(0)]), F.LH_EMODEL, "soil classes")
    heat = pc.make_case("heat_dirichlet_f64", ncols=64)
    with pc.GpuModel(heat) as gm:
        Y, Ya = gm.prognostic_and_aux()
        _refused(gm, gm.L.lh_integrate_dense(gm.ctx, Y, Ya, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None, 0, None, None), gm.F.LH_EMODEL)


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
    s = SAVES * sd
    st, snaps = lh.integrate_dense(model, Y1, Ya, T0 * sd, T1 * sd, sd, s, series=fs)
    assert st["failed"] == 0 and st["accepted"] >= 4 * NCOLS and len(snaps) == len(s), st
    # the integration is integrate_series', and the last snapshot is Y
    st2 = lh.integrate_series(model, Y2, Ya, fs, T0 * sd, T1 * sd, sd)
    assert st == st2, (st, st2)
    np.testing.assert_array_equal(Y1.get("ϑ_l"), Y2.get("ϑ_l"))
    np.testing.assert_array_equal(snaps[-1].get("ϑ_l"), Y1.get("ϑ_l"))
    # the ctypes call on the same context
    F = lh._ffi
    L, be = F.lib(), model._backend()
    Z = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.2 + 0.1 * np.exp(4.0 * z), "θ_i": 0.0 * z}, 0.0)[0]
    mine = [Z.similar() for _ in s]
    arr = (C.c_void_p * len(s))(*[x.handle.value for x in mine])
    F.check(L.lh_integrate_dense(be.ctx, Z.handle, None, fs._device(model), T0 * sd, T1 * sd, sd, 1e-6, 0.0, 1e-3, 0, None,
                                 len(s), _dptr(np.ascontiguousarray(s)), arr), be.ctx)
    for a, b in zip(snaps, mine):
        np.testing.assert_array_equal(a.get("ϑ_l"), b.get("ϑ_l"))
    # no series, no output
    st3, none = lh.integrate_dense(model, Y1, Ya, T1 * sd, T1 * sd + 5 * sd, sd, [])
    assert none == [] and st3["accepted"] > 0
    with pytest.raises(ValueError):
        lh.integrate_dense(model, Y1, Ya, T0 * sd, T1 * sd, sd, [5 * sd, 4 * sd], series=fs)
    with pytest.raises(ValueError):
        lh.integrate_dense(model, Y1, Ya, T0 * sd, T1 * sd, sd, [T1 * sd + 1.0], series=fs)
