"""lh_integrate_heat_dense: the adaptive TR-BDF2 of the heat-only model, without and with a class map, with output
interpolated inside the launch.  tests/test_gpu_dense.py's construction on the families of
tests/test_gpu_heat_series.py: the integration must not see the output (bitwise the twin call), every snapshot is the
cubic Hermite interpolant of the accepted step that contains its time, and the clipped chain of existing calls is the
yardstick for accuracy and for what the output costs in steps.

The helpers take a family object (test_gpu_heat_series.Heat, test_gpu_layered_coupled_series.LayeredCoupled), so
tests/test_gpu_dense_layered_coupled.py runs the same checks on lh_integrate_layered_coupled_dense."""
import ctypes as C
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import dense_ref as D
import heat_implicit_ref as H
import heat_trbdf2_ref as T
import layered_heat_trbdf2_ref as LT
import parity_cases as pc
from test_gpu_bc_series import KEYS, KNOTS, NCOLS, T0, T1, _dptr, _step_buffer, spread_steps
from test_gpu_dense import SAVES
from test_gpu_heat_series import (KINDS, SHAPE_FLUX, STATUS_FAILED, TOP_E, Heat, _host_model, _result, _stats, assert_same_state,
                                  family, make_series, series, top_values)
from test_gpu_heat_trbdf2 import K_BOUND, MULTS

pytestmark = pytest.mark.gpu
NAME = "lh_integrate_heat_dense"
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TOPS = [M.BC_FLUX, M.BC_DIRICHLET]
TOP_IDS = ["flux", "dirichlet"]
ALONE = (0, 37, 64, 101, NCOLS - 1)      # spread over the three waves


# ------------------------------------------------------------------ the calls, for any family object

def dense_entry(fam):
    return NAME if isinstance(fam, Heat) else "lh_integrate_layered_coupled_dense"


def tolerances(fam, abstol=0.0, abstol_e=0.0, reltol=0.0):
    """the tolerance arguments of the family's calls, in their order"""
    return (abstol_e, reltol) if isinstance(fam, Heat) else (abstol, abstol_e, reltol)


def tol_kw(fam, **tols):
    """... and as the keywords of fam.call_wrapped / fam.call_series (a heat-only family has no abstol)"""
    return {k: v for k, v in tols.items() if not (isinstance(fam, Heat) and k == "abstol")}


def handles(snaps):
    return (C.c_void_p * max(len(snaps), 1))(*[None if s is None else s.value for s in snaps]) if len(snaps) else None


def call_dense(fam, gm, Y, Ya, h, t0, t1, dt, cols_ptr, nsave, times, snaps, flags=0, **tols):
    return getattr(gm.L, dense_entry(fam))(gm.ctx, Y, Ya, h, t0, t1, dt, *tolerances(fam, **tols), flags, cols_ptr, nsave, times,
                                            snaps)


def dense(fam, t0, t1, dt, saves, T=None, values=None, h0=None, null_cols=False, **tols):
    """One dense call; T = None: no series.  The result's "snaps": the written planes of every snapshot."""
    with fam.open() as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        cols = None if null_cols else _step_buffer(fam.case, h0)
        h = None if T is None else make_series(gm, T, values)
        s = np.ascontiguousarray(saves, dtype=np.float64)
        snaps = [gm.state(0) for _ in range(len(s))]
        F.check(call_dense(fam, gm, Y, Ya, h, t0, t1, dt, None if cols is None else C.c_void_p(cols.data_ptr()), len(s),
                           _dptr(s) if len(s) else None, handles(snaps), **tols), gm.ctx)
        out = _result(fam, gm, Y, cols, _stats(gm), snaps=[fam.state(gm, sn) for sn in snaps])
        if h is not None:
            F.check(gm.L.lh_bc_series_destroy(gm.ctx, h), gm.ctx)
        return out


def plain(fam, t0, t1, dt, h0=None, null_cols=False, stops=None, **tols):
    """The existing entry point with bcv = NULL; `stops`: a chain of calls clipped at these times (each ends a call, the
    last one is t1), the state downloaded after each."""
    with fam.open() as gm:
        Y, Ya = gm.prognostic_and_aux()
        cols = None if null_cols else _step_buffer(fam.case, h0)
        ptr = None if cols is None else C.c_void_p(cols.data_ptr())
        total = dict.fromkeys(KEYS, 0)
        states = []
        ends = [t0] + ([t1] if stops is None else [float(x) for x in stops])
        for a, b in zip(ends, ends[1:]):
            gm.F.check(fam.call_wrapped(gm, Y, Ya, a, b, dt, ptr, None, **tol_kw(fam, **tols)), gm.ctx)
            st = _stats(gm)
            for key in KEYS:
                total[key] = st[key] if stops is None else total[key] + st[key]
            if stops is not None:
                states.append(fam.state(gm, Y))
        return _result(fam, gm, Y, cols, total, snaps=states)


def initial(fam):
    """the state as passed, in the layout of fam.state"""
    out = dict(rhoe=fam.case.rhoe)
    if not isinstance(fam, Heat):
        out["vl"] = fam.case.vl
    return out


def assert_invisible(got, twin):
    """Contract item 1: Y, dt_cols, the status word and all seven counters are the twin call's, bitwise."""
    assert_same_state(got, twin, cols=twin["cols"] is not None)
    assert got["stats"] == twin["stats"], (got["stats"], twin["stats"])


def assert_snapshot_is(snap, state):
    for key in snap:
        np.testing.assert_array_equal(snap[key], state[key])


def check_invisible_with_a_series(fam, sd, values):
    """Item 1 of the contract with every assertion of the issue's first test"""
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    h0 = spread_steps(fam.case.ncols, sd)
    s = SAVES * sd
    assert s[0] == t0 and s[-1] == t1 and s[3] == T[1] and T[0] < s[1] < s[2] < T[1]
    twin = series(fam, T, values, t0, t1, sd, h0=h0)
    assert twin["stats"]["failed"] == 0 and twin["stats"]["accepted"] >= 4 * fam.case.ncols, twin["stats"]
    got = dense(fam, t0, t1, sd, s, T, values, h0=h0)
    assert_invisible(got, twin)
    # the endpoints: s == t0 is the state as passed, s == t1 the final Y
    assert_snapshot_is(got["snaps"][0], initial(fam))
    assert_snapshot_is(got["snaps"][-1], got)
    # the snapshot on the knot is the state of a series call that ends on that knot
    assert_snapshot_is(got["snaps"][3], series(fam, T, values, t0, T[1], sd, h0=h0))
    # every snapshot in between was written (the states are created zeroed) and the state moves through them
    for k in range(1, len(s)):
        for key, a in got["snaps"][k].items():
            assert np.all(np.isfinite(a)) and np.all(a != 0), (k, key)
            assert np.max(np.abs(a.astype(np.float64) - got["snaps"][k - 1][key])) > 0, (k, key)
    # nsave = 0 is the twin call
    assert_invisible(dense(fam, t0, t1, sd, [], T, values, h0=h0), twin)
    return got


def check_invisible_without_a_series(fam, sd):
    t0, t1 = T0 * sd, T1 * sd
    h0 = spread_steps(fam.case.ncols, sd)
    twin = plain(fam, t0, t1, sd, h0=h0)
    assert twin["stats"]["failed"] == 0 and twin["stats"]["accepted"] >= fam.case.ncols
    got = dense(fam, t0, t1, sd, SAVES * sd, h0=h0)
    assert_invisible(got, twin)
    assert_snapshot_is(got["snaps"][0], initial(fam))
    assert_snapshot_is(got["snaps"][-1], got)
    assert_invisible(dense(fam, t0, t1, sd, [], h0=h0), twin)
    # without step proposals from the caller, as the twin
    assert_invisible(dense(fam, t0, t1, sd, SAVES * sd, null_cols=True), plain(fam, t0, t1, sd, null_cols=True))


def check_nested_save_sets(fam, sd, values):
    """The snapshots at the times of S do not depend on what else is saved inside the same steps."""
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    h0 = spread_steps(fam.case.ncols, sd)
    S = SAVES * sd
    more = np.sort(np.concatenate([S, 0.5 * (S[:-1] + S[1:]), S[:-1] + 0.25 * (S[1:] - S[:-1])]))
    assert len(more) == 3 * len(S) - 2 and np.all(np.diff(more) > 0)
    a = dense(fam, t0, t1, sd, S, T, values, h0=h0)
    b = dense(fam, t0, t1, sd, more, T, values, h0=h0)
    # (what makes this meaningful: some step holds more than one save time)
    assert b["stats"]["accepted"] < fam.case.ncols * len(more), (b["stats"], len(more))
    assert_invisible(b, a)
    at = {float(t): k for k, t in enumerate(more)}
    for k, t in enumerate(S):
        assert_snapshot_is(a["snaps"][k], b["snaps"][at[float(t)]])


def check_columns_alone(fam, sd, values):
    T, t0, t1 = KNOTS * sd, T0 * sd, T1 * sd
    h0 = spread_steps(fam.case.ncols, sd)
    s = SAVES * sd
    got = dense(fam, t0, t1, sd, s, T, values, h0=h0)
    assert got["stats"]["failed"] == 0
    for c in ALONE:
        alone = dense(fam.column(c), t0, t1, sd, s, T, values, h0=h0[c:c + 1])
        for k in range(len(s)):
            for key, a in got["snaps"][k].items():
                np.testing.assert_array_equal(a[c], alone["snaps"][k][key][0])
        for key in initial(fam):
            np.testing.assert_array_equal(got[key][c], alone[key][0])
        assert got["cols"][c] == alone["cols"][0]


def check_a_failing_column(fam, sd, values, ncols):
    """Tolerances Float32 cannot meet (1e-14 each): every column fails in its first sub-interval, which sets status
    bit 4 and is not a fault."""
    T = np.array([0.0, 3.0, 5.0, 8.0, 11.0]) * sd
    t0, t1 = 0.5 * sd, 10 * sd
    tols = tol_kw(fam, abstol=1e-14, abstol_e=1e-14, reltol=1e-14)
    ref = series(fam, T, values, t0, t1, sd, **tols)
    assert ref["status"] & STATUS_FAILED and ref["stats"]["failed"] == ncols and ref["stats"]["accepted"] == 0, ref["stats"]
    got = dense(fam, t0, t1, sd, np.array([0.5, 2.0, 3.0, 6.0, 10.0]) * sd, T, values, abstol=1e-14, abstol_e=1e-14, reltol=1e-14)
    assert got["status"] & STATUS_FAILED and got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
    assert np.all(got["cols"] == 0)
    assert_snapshot_is(initial(fam), got)
    for snap in got["snaps"]:
        assert_snapshot_is(snap, initial(fam))


# ------------------------------------------------------------------ 1. the integration does not see the output

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_output_is_invisible_with_a_series(kind, top, dtype):
    fam, sd = family(kind, dtype, top)
    check_invisible_with_a_series(fam, sd, top_values(fam, top))


# ------------------------------------------------------------------ 2. ... nor without a series

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,top,kw", [("scalar", M.BC_DIRICHLET, dict(ice=True, variant="percol")),
                                         ("layered", M.BC_FLUX, dict(ice=True))],
                         ids=["scalar-percol-libm", "layered-ice"])
def test_output_is_invisible_without_a_series(kind, top, kw, dtype):
    """a porosity per column under LH_MATH_LIBM (the PERCOL instantiation of the libm kernel); a class map with ice"""
    fam, sd = family(kind, dtype, top, **kw)
    if kind == "scalar":
        fam = Heat(fam.obj, math_mode=1)
    check_invisible_without_a_series(fam, sd)


# ------------------------------------------------------------------ 3. nested save sets

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_nested_save_sets(kind, dtype):
    fam, sd = family(kind, dtype, M.BC_FLUX)
    check_nested_save_sets(fam, sd, top_values(fam, M.BC_FLUX))


# ------------------------------------------------------------------ 4. one and two levels

@pytest.mark.parametrize("nlev", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_one_and_two_levels(kind, nlev):
    """both faces on one cell; no interior cell"""
    fam, sd = family(kind, np.float64, M.BC_FLUX, nlev=nlev)
    check_invisible_with_a_series(fam, sd, top_values(fam, M.BC_FLUX))


# ------------------------------------------------------------------ 5. the formula

GAMMA = 2.0 - np.sqrt(2.0)
D_TR = 0.5 * GAMMA
C_W2 = 1.0 / (GAMMA * (2.0 - GAMMA))


# One attempt of h = MULTS[0] = 1/4 stable step from t0 = 0 (t1 - t0 = dt = h, no series) with snapshots at
# theta = 1/4, 1/2, 3/4, against dense_ref.hermite evaluated in Float64 from the reference attempt's y0, y1, f0 and
# f1 = (y1 - w2) / (d h) (heat_trbdf2_ref.attempt; layered_heat_trbdf2_ref's Problem for the layered kind).  Of the two
# MULTS it is the one every column accepts: the reference's error norm of that attempt is at most 0.1 in all eight
# cases, while at one stable step it reaches 1.34 (scalar) and 2.85 (layered) under a Dirichlet top, whose first step
# is then rejected -- and a rejected attempt is not the one attempt the comparison is about.
#
# The interpolant is linear in (y0, y1, h f0, h f1):
#   u = p0 y0 + p1 y1 + q0 (h f0) + q1 (h f1),
#   p1 = theta + theta (theta - 1)(1 - 2 theta) = 3 theta^2 - 2 theta^3 in [0, 1],  q0 = theta (theta - 1)^2,
#   q1 = theta^2 (theta - 1),  max |q0| = max |q1| = 4/27 over [0, 1],
# so |u_dev - u_ref| <= p1 dy1 + |q1| d(h f1) + |q0| d(h f0) + the round-off of evaluating the formula in FT, with
# the device's and the reference's data differing as follows (y0 is the same number on both sides).
#   B = K_BOUND eps cond_inf(I - d h A) ||rhoe||_inf is the project's own bound on one solve with M = I - d h A
#   (tests/test_gpu_heat_trbdf2.py, from tests/test_gpu_heat_implicit.py): it holds for Y_gamma and for Y_1.
#   * dy1 <= B.
#   * h f1 = (y1 - w2) / d with w2 = c_w2 (Y_gamma - (1 - gamma)^2 y0), c_w2 = 1 / (gamma (2 - gamma)) = 1.2071:
#     d(h f1) <= (dy1 + c_w2 dY_gamma) / d <= (1 + c_w2) B / d = 7.536 B.
#   * h f0 = (c f0) / d with c = d h.  f0 is the prologue's fresh tendency, a round-off of order eps ||h A|| ||rhoe||.
#     It is the device's own f0 that enters stage 1, M Y_gamma = y0 + c f0 + c b: the share of dY_gamma that comes from
#     it is M^-1 d(c f0), and B bounds it, so d(c f0) <= ||M||_inf B and d(h f0) <= ||M||_inf B / d, where
#     ||M||_inf = 1 + d ||h A||_inf (A's diagonal is negative, its off-diagonals positive): about 1.15 at a quarter of
#     a stable step, 1.6 at one.
#   * the evaluation: six coefficients rounded to FT and nine operations on terms no larger than
#     S = max(|y0|, |y1|, |h f0|, |h f1|): 16 eps S (B is at least 41 eps ||rhoe||, so this term is small beside it).
# Together: bound(theta) = (p1 + |q1| (1 + c_w2) / d + |q0| ||M||_inf / d) B + 16 eps S, which at theta = 1/2 and
# ||M||_inf = 1.15 is (0.5 + 0.942 + 0.491) B = 1.9 B, and for any theta and any step up to a stable one at most
# (1 + 1.116 + 0.809) B = 2.9 B: the "roughly 3 B" of the issue, with the constant computed per column from its own
# matrix.
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_formula_on_one_attempt(kind, top, dtype):
    fam, sd = family(kind, dtype, top)
    P = LT.problem(fam.obj) if fam.layered else T.problem(fam.case)
    y0 = fam.case.rhoe.astype(np.float64)
    h = MULTS[0] * sd
    thetas = np.array([0.25, 0.5, 0.75])
    got = dense(fam, 0.0, h, h, thetas * h)
    assert got["stats"]["accepted"] == NCOLS and got["stats"]["rejected"] == 0 and got["status"] == 0, got["stats"]
    f0 = T.fresh_tendency(P, y0, None)
    r = T.attempt(P, y0, f0, np.zeros(NCOLS), np.full(NCOLS, h))
    y1, f1 = r["y1"], r["fn1"]
    eps = float(np.finfo(dtype).eps)
    B = K_BOUND[np.dtype(dtype)] * eps * H.cond_inf(P.bands, D_TR * h) * np.max(np.abs(y1), axis=1)
    normM = np.abs(H.matrix(P.bands, D_TR * h)).sum(axis=2).max(axis=1)
    S = np.max(np.maximum(np.maximum(np.abs(y0), np.abs(y1)), h * np.maximum(np.abs(f0), np.abs(f1))), axis=1)
    for th, snap in zip(thetas, got["snaps"]):
        p1, q0, q1 = 3 * th ** 2 - 2 * th ** 3, th * (th - 1) ** 2, th ** 2 * (th - 1)
        bound = (p1 + abs(q1) * (1 + C_W2) / D_TR + abs(q0) * normM / D_TR) * B + 16 * eps * S
        want = D.hermite(th, h, y0, y1, f0, f1)
        err = np.max(np.abs(snap["rhoe"].astype(np.float64) - want), axis=1)
        print("dense-heat-formula", kind, TOP_IDS[TOPS.index(top)], np.dtype(dtype).name, "theta", th, "max error %.4g" % err.max(),
              "bound %.4g" % bound.min(), "worst share %.4g" % float(np.max(err / bound)), "bound / B %.3f" % float(np.max(bound / B)))
        assert np.all(err <= bound), (th, float(np.max(err / bound)))
        if dtype == np.float64:      # (the interpolant is far from the chord on this step: the test reads f0 and f1)
            assert np.max(np.abs(want - ((1 - th) * y0 + th * y1))) > 100 * float(bound.max())


# ------------------------------------------------------------------ 6. accuracy and the payoff, against the clipped chain

NSNAP = 25
SPACING = 4.0       # stable steps between two save times: the heat-only steps grow far beyond it
# E_dense / max(E_chain, 1) as measured on the MI355X, per (kind, top, dtype); the assertion
# allows twice the largest.  None is above 10.
RECORDED_RATIO = {("scalar", "flux", "f64"): 1.170, ("scalar", "flux", "f32"): 1.170,
                  ("scalar", "dirichlet", "f64"): 1.152, ("scalar", "dirichlet", "f32"): 1.152,
                  ("layered", "flux", "f64"): 1.291, ("layered", "flux", "f32"): 1.291,
                  ("layered", "dirichlet", "f64"): 1.125, ("layered", "dirichlet", "f32"): 1.125}
RATIO_ALLOWED = 2.0 * max(RECORDED_RATIO.values())
TIGHT = dict(abstol=1e-8, reltol=1e-5)      # 100x tighter than the defaults (abstol_e: that of 1e-8 K in water)


def check_accuracy_against_the_clipped_chain(label, fam, sd, spacing, allowed, truth):
    """`truth`: the Float64 chain of existing calls clipped at the save times at TIGHT.  Returns (dense, chain)."""
    e = fam.case.om.earth
    abstol_e = 1e-6 * e.cp_l * e.rho_liq       # (the library's default, spelled out for the scaling)
    s = np.arange(1, NSNAP + 1) * spacing * sd
    h0 = spread_steps(NCOLS, sd)
    clipped = plain(fam, 0.0, s[-1], sd, h0=h0, stops=s)
    assert clipped["stats"]["failed"] == 0 and clipped["status"] == 0, clipped["stats"]
    got = dense(fam, 0.0, s[-1], sd, s, h0=h0)
    assert got["stats"]["failed"] == 0 and got["status"] == 0, got["stats"]

    def scaled_error(snaps):
        worst = 0.0
        for sn, tr in zip(snaps, truth):
            for key, v in tr.items():
                scale = (abstol_e if key == "rhoe" else 1e-6) + 1e-3 * np.abs(v)
                worst = max(worst, float(np.max(np.abs(sn[key].astype(np.float64) - v) / scale)))
        return worst

    E_chain, E_dense = scaled_error(clipped["snaps"]), scaled_error(got["snaps"])
    ratio = E_dense / max(E_chain, 1.0)
    print("dense-accuracy", label, "E_chain %.4g E_dense %.4g ratio %.4g" % (E_chain, E_dense, ratio), "accepted chain/dense",
          clipped["stats"]["accepted"], got["stats"]["accepted"], "newton chain/dense", clipped["stats"]["newton_iterations"],
          got["stats"]["newton_iterations"])
    assert ratio <= allowed, (ratio, allowed)
    # the payoff: the output no longer sets the steps
    assert got["stats"]["accepted"] <= clipped["stats"]["accepted"], (got["stats"], clipped["stats"])
    return got, clipped


def truth_of(fam64, sd, spacing):
    e = fam64.case.om.earth
    out = plain(fam64, 0.0, NSNAP * spacing * sd, sd, h0=spread_steps(NCOLS, sd), stops=np.arange(1, NSNAP + 1) * spacing * sd,
                abstol_e=1e-8 * e.cp_l * e.rho_liq, **TIGHT)
    assert out["stats"]["failed"] == 0 and out["status"] == 0
    return out["snaps"]


@functools.lru_cache(maxsize=None)
def _truth(kind, top):
    fam64, sd = family(kind, np.float64, top)
    return truth_of(fam64, sd, SPACING), sd


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("top", TOPS, ids=TOP_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_and_step_counts_against_the_clipped_chain(kind, top, dtype):
    truth, sd = _truth(kind, top)          # (the Float64 case's stable step: the save times are the truth's)
    fam, _ = family(kind, dtype, top)
    label = "%s %s %s" % (kind, TOP_IDS[TOPS.index(top)], np.dtype(dtype).name)
    got, clipped = check_accuracy_against_the_clipped_chain(label, fam, sd, SPACING, RATIO_ALLOWED, truth)
    # 25 save times 4 stable steps apart: the chain takes at least one step per save time, the dense run at most half
    assert 2 * got["stats"]["accepted"] <= clipped["stats"]["accepted"], (got["stats"], clipped["stats"])


# ------------------------------------------------------------------ 7. column independence

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_columns_snapshots_are_its_own(kind, dtype):
    top = M.BC_DIRICHLET if kind == "layered" else M.BC_FLUX
    fam, sd = family(kind, dtype, top)
    check_columns_alone(fam, sd, top_values(fam, top))


# ------------------------------------------------------------------ 8. a failing column

@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_column_fills_its_snapshots_with_its_kept_state(kind):
    fam, sd = family(kind, np.float32, M.BC_FLUX, ncols=64)
    check_a_failing_column(fam, sd, top_values(fam, M.BC_FLUX), 64)


# ------------------------------------------------------------------ 9. refusals

def refused(gm, rc, code, *words, name=NAME):
    msg = gm.L.lh_last_error(gm.ctx).decode()
    assert rc == code, (rc, code, msg)
    for w in (name,) + words:
        assert w in msg, (w, msg)
    assert all(v == 0 for v in _stats(gm).values()), "statistics after a refused call"


def check_dense_refusals(fam, gm, other, call, snaps, lacking, Y, Ya, sd):
    """Every dense_refusals case names its index; `call(times=, states=, nsave=, null_times=, null_states=)`."""
    EINVAL = gm.F.LH_EINVAL
    name = dense_entry(fam)
    nan = float("nan")
    foreign = other.state(0)
    ref = lambda rc, *words: refused(gm, rc, EINVAL, *words, name=name)
    ref(call(nsave=-1), "nsave = -1")
    ref(call(nsave=65537), "nsave = 65537")
    ref(call(null_times=True), "NULL", "save_times")
    ref(call(null_states=True), "NULL", "snapshots")
    ref(call(times=np.array([3.0, 20.0, 9.0]) * sd), "save time 2", "strictly increasing")
    ref(call(times=np.array([3.0, 3.0, 9.0]) * sd), "save time 1", "strictly increasing")
    ref(call(times=np.array([3.0, nan, 9.0]) * sd), "save time 1", "not finite")
    ref(call(times=np.array([2.0, 9.0, 20.0]) * sd), "save time 0", "outside")
    ref(call(times=np.array([3.0, 9.0, 28.5]) * sd), "save time 2", "outside")
    ref(call(states=[snaps[0], None, snaps[2]]), "snapshot 1", "NULL")
    ref(call(states=[snaps[0], snaps[1], foreign]), "snapshot 2", "not a state of this context")
    ref(call(states=[snaps[0], Y, snaps[2]]), "snapshot 1 is Y")
    if Ya is not None:
        ref(call(states=[snaps[0], snaps[1], Ya]), "snapshot 2 is Ya")
    ref(call(states=[snaps[0], snaps[1], snaps[0]]), "snapshot 2 is snapshot 0")
    ref(call(states=[lacking, snaps[1], snaps[2]]), "snapshot 0", "lacks a plane")


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_everything_untouched(kind):
    fam, sd = family(kind, np.float64, M.BC_FLUX, ncols=67)
    T = KNOTS * sd
    vals = top_values(fam, M.BC_FLUX)
    t0, t1 = T0 * sd, T1 * sd
    nlev = fam.case.om.nlev
    with fam.open() as gm, fam.open() as other:
        F, L = gm.F, gm.L
        EINVAL, EMODEL = F.LH_EINVAL, F.LH_EMODEL
        Y, Ya = gm.prognostic_and_aux()
        h = make_series(gm, T, vals)
        marks = [np.full((67, nlev), 1.0e6 * (k + 1)) for k in range(3)]
        snaps = [gm.state((1 << F.LH_VAR_RHOE_INT) | (1 << F.LH_VAR_VARTHETA_L)) for _ in range(3)]
        for sn, a in zip(snaps, marks):
            gm.upload(sn, F.LH_VAR_RHOE_INT, a)
        no_energy =gm.state((1 << F.LH_VAR_VARTHETA_L) | (1 << F.LH_VAR_THETA_I))
        good = np.array([3.0, 9.0, 20.0]) * sd
        cols = _step_buffer(fam.case, np.full(67, 0.5 * sd))
        cols_before = cols.cpu().numpy().copy()

        def call(times=good, states=snaps, nsave=None, series_h=h, dt=sd, t0=t0, t1=t1, null_times=False, null_states=False,
                 flags=0, reltol=0.0, with_cols=True):
            s = np.ascontiguousarray(times, dtype=np.float64)
            return call_dense(fam, gm, Y, Ya, series_h, t0, t1, dt, C.c_void_p(cols.data_ptr()) if with_cols else None,
                              len(s) if nsave is None else nsave, None if null_times else _dptr(s),
                              None if null_states else handles(states), flags=flags, reltol=reltol)

        # a run first, so that the statistics are not zero before the refusals (into states of its own, no step buffer)
        F.check(call(states=[gm.state(0) for _ in range(3)], with_cols=False), gm.ctx)
        assert _stats(gm)["accepted"] >= 67
        before = gm.download(Y, F.LH_VAR_RHOE_INT)
        # ---- the wrapped series call's refusals come first, in its words: arguments, then the series; with a bad
        # nsave in the same call
        refused(gm, call(t0=2.0 * sd, t1=1.0 * sd, nsave=-1), EINVAL, ": need finite t0 <= t1")
        refused(gm, call(dt=0.0, nsave=-1), EINVAL, ": need a finite dt > 0")
        refused(gm, call(reltol=-1.0, nsave=-1), EINVAL, ": tolerances must be finite and >= 0")
        refused(gm, call(flags=1, nsave=-1), EINVAL, ": unknown flags 0x1")
        refused(gm, call(series_h=make_series(other, T, vals), nsave=-1), EINVAL, "not a series of this context")
        refused(gm, call(t0=-0.5 * sd, nsave=-1), EINVAL, "no extrapolation")
        v0 = np.ascontiguousarray(vals[TOP_E])
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, _dptr(v0), 1, 0), gm.ctx)
        refused(gm, call(nsave=-1), EMODEL, "top hydrology values", "a heat-only model has no hydrology component")
        F.check(L.lh_bc_series_set(gm.ctx, h, M.FACE_TOP, M.COMP_HYDROLOGY, None, 0, 0), gm.ctx)
        # (series == NULL is no refusal here: the series' checks apply only with a series)
        refused(gm, call(series_h=None, nsave=-1), EINVAL, "nsave = -1")
        assert getattr(L, NAME)(None, Y, Ya, h, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, 0, None, None) == EINVAL
        # ---- then dense_refusals; a snapshot must hold rhoe_int
        check_dense_refusals(fam, gm, other, call, snaps, no_energy, Y, Ya, sd)
        # ---- Y, the snapshots and dt_cols are as they were
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before)
        for sn, a in zip(snaps, marks):
            np.testing.assert_array_equal(gm.download(sn, F.LH_VAR_RHOE_INT), a)
        np.testing.assert_array_equal(cols.cpu().numpy(), cols_before)
        # ---- and the call goes on working: vartheta_l is not required of a snapshot, only rhoe_int is written; t0 == t1
        # writes Y as passed
        energy_only = gm.state(1 << F.LH_VAR_RHOE_INT)
        vl_mark = np.full((67, nlev), 0.0125)
        gm.upload(snaps[0], F.LH_VAR_VARTHETA_L, vl_mark)
        F.check(call(states=[snaps[0], energy_only, snaps[2]]), gm.ctx)
        assert np.max(np.abs(gm.download(snaps[0], F.LH_VAR_RHOE_INT) - marks[0])) > 0
        assert np.all(gm.download(energy_only, F.LH_VAR_RHOE_INT) != 0)
        np.testing.assert_array_equal(gm.download(snaps[0], F.LH_VAR_VARTHETA_L), vl_mark)
        now = gm.download(Y, F.LH_VAR_RHOE_INT)
        F.check(call(times=[3.0 * sd], states=snaps[:1], t0=3.0 * sd, t1=3.0 * sd), gm.ctx)
        np.testing.assert_array_equal(gm.download(snaps[0], F.LH_VAR_RHOE_INT), now)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), now)
        assert all(v == 0 for v in _stats(gm).values())
        # ---- lh_integrate_dense still refuses this context
        rc = L.lh_integrate_dense(gm.ctx, Y, Ya, None, t0, t1, sd, 0.0, 0.0, 0.0, 0, None, 0, None, None)
        refused(gm, rc, EMODEL, name="lh_integrate_dense")
    # ---- and the new call refuses the contexts lh_integrate_dense serves, arguments first
    for name in ("c2_richards_f64", "coupled_f64_small"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            L = gm.L
            refused(gm, getattr(L, NAME)(gm.ctx, Y, Ya, None, T[0], T[1], 0.0, 0.0, 0.0, 0, None, 0, None, None), gm.F.LH_EINVAL, "dt > 0")
            rc = getattr(L, NAME)(gm.ctx, Y, Ya, None, T[0], T[1], sd, 0.0, 0.0, 0, None, -1, None, None)
            refused(gm, rc, gm.F.LH_EMODEL)
            assert L.lh_last_error(gm.ctx).decode() == NAME + ": heat-only models (SoilEnergyModel + PrescribedHydrologyModel)"


# ------------------------------------------------------------------ 10. the host mirror

def stats_of(lh, be):
    st = (C.c_int64 * lh._ffi.LH_TRBDF2_NSTATS)()
    lh._ffi.check(lh._ffi.lib().lh_trbdf2_stats(be.ctx, st), be.ctx)
    return dict(zip(KEYS, list(st)))


@pytest.mark.parametrize("kind", KINDS)
def test_host_mirror(kind):
    """integrate_heat_dense with and without a series: the statistics and the snapshots are those of the C call."""
    lh = g.load_package()
    N = 5
    lay = family("layered", np.float64, M.BC_FLUX, ncols=N)[0].obj if kind == "layered" else None
    ic = lambda z, m: {"ρe_int": 2.5e7 + 4.0e6 * np.sin(9.0 * z)}
    model = _host_model(lh, lay, N=N)
    (Y1, Ya), (Y2, _), (Y3, _), (Y4, _) = [lh.initialize_states(model, ic, 0.0) for _ in range(4)]
    sd = lh.stable_dt(model, Y1, Ya, 0.5)
    T = KNOTS * sd
    vals = -2.0 * SHAPE_FLUX[:, None] * (0.8 + 0.4 * pc.uhash(np.arange(N), 3, 1))[None, :]
    fs = lh.BoundarySeries(T, {("top", "energy"): vals})
    s = np.ascontiguousarray(SAVES * sd)
    F = lh._ffi
    L, be = F.lib(), model._backend()
    for series_, Ym, Yc in ((fs, Y1, Y2), (None, Y3, Y4)):
        st, snaps = lh.integrate_heat_dense(model, Ym, Ya, T0 * sd, T1 * sd, sd, s, series=series_, reltol=1e-4)
        assert st["failed"] == 0 and st["accepted"] >= N and len(snaps) == len(s), st
        np.testing.assert_array_equal(snaps[-1].get("ρe_int"), Ym.get("ρe_int"))
        mine = [Yc.similar() for _ in s]
        arr = (C.c_void_p * len(s))(*[x.handle.value for x in mine])
        F.check(L.lh_integrate_heat_dense(be.ctx, Yc.handle, Ya.handle, None if series_ is None else fs._device(model), T0 * sd,
                                          T1 * sd, sd, 0.0, 1e-4, 0, None, len(s), _dptr(s), arr), be.ctx)
        assert stats_of(lh, be) == st
        np.testing.assert_array_equal(Yc.get("ρe_int"), Ym.get("ρe_int"))
        for a, b in zip(snaps, mine):
            np.testing.assert_array_equal(a.get("ρe_int"), b.get("ρe_int"))
    assert np.max(np.abs(Y1.get("ρe_int") - Y3.get("ρe_int"))) > 0      # (the series is read)
    # the integration is integrate_heat_series'; no output is the empty list
    (Y5, _), (Y6, _) = [lh.initialize_states(model, ic, 0.0) for _ in range(2)]
    want = lh.integrate_heat_series(model, Y5, Ya, fs, T0 * sd, T1 * sd, sd, reltol=1e-4)
    st, none = lh.integrate_heat_dense(model, Y6, Ya, T0 * sd, T1 * sd, sd, [], series=fs, reltol=1e-4)
    assert none == [] and st == want
    np.testing.assert_array_equal(Y5.get("ρe_int"), Y1.get("ρe_int"))
    np.testing.assert_array_equal(Y6.get("ρe_int"), Y1.get("ρe_int"))
    with pytest.raises(ValueError, match="integrate_heat_dense: save time 1"):
        lh.integrate_heat_dense(model, Y1, Ya, T0 * sd, T1 * sd, sd, [5 * sd, 4 * sd], series=fs)
    with pytest.raises(ValueError, match="no extrapolation"):
        lh.integrate_heat_dense(model, Y1, Ya, T[0] - 1.0, T[1], sd, [T[0]], series=fs)
    model.close()
