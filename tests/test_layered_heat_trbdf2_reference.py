"""The NumPy reference of the adaptive TR-BDF2 of layered heat-only soils (tests/layered_heat_trbdf2_ref.py) against
what the GPU tests rest on (no GPU): the estimate against the true local error, the integration against fine fixed
steps, the reject path and the failure case, on a three-horizon map."""
import numpy as np
import pytest

import heat_trbdf2_ref as T
import layered_heat_implicit_ref as LI
import layered_heat_trbdf2_ref as LT

SPAN = 2000.0   # stable steps


@pytest.fixture(scope="module")
def horizons():
    """three horizons, 4 x 60, Dirichlet faces: (lay, problem, state, stable step, the fine fixed-step solution)"""
    lay = LI.layered_case(np.float64, 4, 60, kind="horizons")
    P = LT.problem(lay)
    y0, sd = LI.state64(lay), LI.stable_dt(lay)
    return lay, P, y0, sd, LT.fixed_trbdf2(P, y0, 0.0, SPAN * sd, 4000)


def test_the_integrator_is_the_scalar_references():
    assert LT.integrate is T.integrate and LT.attempt is T.attempt and LT.error_norm is T.error_norm


@pytest.mark.parametrize("kind", ["horizons", "cells"])
def test_estimate_against_the_true_local_error(kind):
    """E of one attempt against the norm of Y_1 minus 32 sub-steps of the same span, at 0.25 and 1 stable step: within
    [0.9, 1.2], DESIGN section 4.17's band for the same estimator."""
    lay = LI.layered_case(np.float64, 4, 60, kind=kind)
    P = LT.problem(lay)
    y0, sd = LI.state64(lay), LI.stable_dt(lay)
    fn = LT.fresh_tendency(P, y0, None)
    atol = LT.abstol_e_default(lay.case.om)
    for mult in (0.25, 1.0):
        hh = np.full(4, mult * sd)
        r = LT.attempt(P, y0, fn, np.zeros(4), hh)
        E = LT.error_norm(r["e"], y0, r["y1"], atol, 1e-3)
        Et = LT.error_norm(LT.true_local_error(P, y0, fn, np.zeros(4), hh), y0, r["y1"], atol, 1e-3)
        print("layered", kind, "estimate / truth at", mult, "stable steps:", E / Et, "E", E)
        assert np.all((E / Et >= 0.9) & (E / Et <= 1.2)), (kind, mult, E / Et)


def test_integration_against_fine_fixed_steps(horizons):
    lay, P, y0, sd, fine = horizons
    errs = []
    for rt in (1e-3, 1e-4, 1e-5):
        y, info = LT.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=rt)
        assert not info["failed"].any() and np.all(info["t"] == SPAN * sd)
        errs.append(float(np.max(np.abs(y - fine))))
        print("layered reltol", rt, "accepted", info["accepted"], "rejected", info["rejected"], "error", errs[-1],
              "field scale", float(np.max(np.abs(y0))))
    assert errs[0] > errs[1] > errs[2], errs


def test_reject_path_and_failure(horizons):
    lay, P, y0, sd, _ = horizons
    y, info = LT.integrate(P, y0, 0.0, SPAN * sd, SPAN * sd)
    print("layered h0 = span: accepted", info["accepted"], "rejected", info["rejected"])
    assert not info["failed"].any() and np.all(info["t"] == SPAN * sd) and np.all(info["rejected"] >= 1)
    y32 = y0.astype(np.float32).astype(np.float64)
    y, info = LT.integrate(P, y32, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14, ft=np.float32)
    assert info["failed"].all() and not info["accepted"].any()
    assert np.array_equal(y, y32) and not info["dt_cols"].any()


def test_sixteen_classes_make_a_case():
    lay = LT.sixteen_class_case(np.float64, 3, 16)
    assert len(set(lay.class_map.reshape(-1).tolist())) == 16
    P = LT.problem(lay)
    y, info = LT.integrate(P, LI.state64(lay), 0.0, 10 * LI.stable_dt(lay), LI.stable_dt(lay))
    assert not info["failed"].any() and np.all(np.isfinite(y))
