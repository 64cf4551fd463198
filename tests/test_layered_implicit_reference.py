"""The NumPy backward Euler and TR-BDF2 of layered soils (tests/layered_implicit_ref.py), pinned without a
device: to the oracle-based references on column-uniform maps, to second order, to rest and to the water
budget."""
import functools

import numpy as np

import implicit_ref as IR
import layered_implicit_ref as LI
import layered_ref as R
import trbdf2_ref as TR

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def uniform_case():
    return R.make_layered(np.float64, 16, 64, R.uniform_map(16, 64), bc="flux_drain")


@functools.lru_cache(maxsize=None)
def horizon_case(bc):
    return R.make_layered(np.float64, 24, 64, R.horizon_map(24, 64), bc=bc)


def test_column_uniform_maps_agree_with_the_oracle_based_references():
    """Sixteen columns, column c of class c at every level: the per-cell Newton is the per-column Newton of
    tests/implicit_ref.py and tests/trbdf2_ref.py on the same parameters (with_percol), to the project's
    Float64 parity bound of these solvers, 1e-10."""
    lay = uniform_case()
    case = R.with_percol(lay)
    dt = 30 * R.stable_dt(lay)
    got, _ = LI.implicit_euler(lay, dt, 3)
    want, _ = IR.implicit_euler(case.om, case.vl, case.ti, dt, 3)
    err = np.max(np.abs(got - want))
    print("backward Euler, 3 steps at 30x: %.3g" % err)
    assert err <= 1e-10 and np.max(np.abs(got - lay.case.vl)) > 1e-6
    for adaptive in (False, True):
        got, gi = LI.trbdf2(lay, 0.0, 3 * dt, dt, adaptive=adaptive)
        want, wi = TR.trbdf2(case.om, case.vl, case.ti, 0.0, 3 * dt, dt, adaptive=adaptive)
        err = np.max(np.abs(got - want))
        print("TR-BDF2 adaptive=%s: %.3g, accepted %s" % (adaptive, err, gi["accepted"]))
        assert err <= 1e-10
        assert np.array_equal(gi["accepted"], wi["accepted"]) and np.array_equal(gi["rejected"], wi["rejected"])


def test_fixed_step_trbdf2_is_second_order():
    """200 stable steps of the four-horizon case in 25, 50 and 100 steps against SSPRK33 at a quarter of the
    stable step: the error falls 3.5-4.5x per halving, the band of the existing order test."""
    lay = horizon_case("flux_drain")
    sd = R.stable_dt(lay)
    T = 200 * sd
    ref = R.ssprk33(lay, sd / 4, 800)
    errs = [np.max(np.abs(LI.trbdf2(lay, 0.0, T, T / k, adaptive=False)[0] - ref)) for k in (25, 50, 100)]
    r = [a / b for a, b in zip(errs, errs[1:])]
    print("errors %s, ratios %s" % (errs, r))
    assert all(3.5 <= x <= 4.5 for x in r), (errs, r)


def test_hydrostatic_three_horizon_column_stays_at_rest():
    """One backward-Euler step of a day: the column moves by less than Newton's own tolerance scale,
    10 tol nu with tol = 1e-10 (the device's Float64 default)."""
    lay = R.hydrostatic(np.float64)
    v1, iters = LI.implicit_euler(lay, 86400.0, 1)
    moved = np.max(np.abs(v1 - lay.case.vl))
    print("moved %.3g in %d iterations" % (moved, iters.max()))
    assert moved <= 10 * 1e-10 * lay.classes[:, 4].max()


def test_flux_faces_conserve_water():
    """Flux at both faces, 100x the stable step: sum (v1 - v0) dz = dt (F_bot - F_top).  Every unclipped Newton
    update conserves water exactly (the columns of the Jacobian sum to 1), so what is left is the round-off of
    nlev residuals, each 64 eps times the larger of |v| and dt |f| (test_gpu_implicit.py's round_off)."""
    lay = horizon_case("flux")
    om = lay.case.om
    dz = (om.zmax - om.zmin) / om.nlev
    dt = 100 * R.stable_dt(lay)
    v1, _ = LI.implicit_euler(lay, dt, 1)
    f, f_bot, f_top = R.rhs(lay, v1, faces=True)
    change = np.sum(v1 - lay.case.vl, axis=1) * dz
    want = dt * (f_bot - f_top)
    big = np.maximum(np.abs(v1).max(axis=1), dt * np.abs(f).max(axis=1))
    err = np.abs(change - want)
    print("budget error %.3g against %.3g" % (err.max(), np.abs(want).max()))
    assert np.all(err <= om.nlev * dz * 64 * EPS * big), float(err.max())
    assert np.abs(want).min() > 1e-7
