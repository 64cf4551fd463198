"""The NumPy reference of the adaptive heat-only TR-BDF2 (tests/heat_trbdf2_ref.py) against what the GPU tests rest
on (no GPU): its error estimate against the true local error, its integration against fine fixed steps, its reject
path, the reference's analytic test, and the two entry points in the header, the ctypes table, the Julia shim and
INTEGRATION.md."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import heat_implicit_ref as H
import heat_trbdf2_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lh_integrate_heat_trbdf2", "lh_integrate_layered_heat_trbdf2")
SPAN = 2000.0   # stable steps


@pytest.fixture(scope="module")
def lh():
    return g.load_package()


@pytest.fixture(scope="module")
def soil():
    """heat_case(4, 60), Dirichlet faces: (case, problem, state, stable step, the fine fixed-step solution)"""
    case = H.heat_case(4, 60)
    P = T.problem(case)
    y0 = H.f64(case)[2]
    sd = H.stable_dt(case)
    return case, P, y0, sd, T.fixed_trbdf2(P, y0, 0.0, SPAN * sd, 4000)


def test_estimate_against_the_true_local_error(soil):
    """E of one attempt against the norm of Y_1 minus 32 sub-steps of the same span, at 0.25 and 1 stable step:
    the ratio the same estimator measured in DESIGN section 4.17 (1.008-1.063), with room."""
    case, P, y0, sd, _ = soil
    fn = T.fresh_tendency(P, y0, None)
    atol = T.abstol_e_default(case.om)
    for mult in (0.25, 1.0):
        hh = np.full(4, mult * sd)
        r = T.attempt(P, y0, fn, np.zeros(4), hh)
        E = T.error_norm(r["e"], y0, r["y1"], atol, 1e-3)
        Et = T.error_norm(T.true_local_error(P, y0, fn, np.zeros(4), hh), y0, r["y1"], atol, 1e-3)
        ratio = E / Et
        print("estimate / truth at", mult, "stable steps:", ratio)
        assert np.all((ratio >= 0.9) & (ratio <= 1.2)), (mult, ratio)


def test_integration_against_fine_fixed_steps(soil):
    """2000 stable steps from h0 = the stable step: the error against fixed TR-BDF2 at span / 4000 falls with reltol,
    no column fails."""
    case, P, y0, sd, fine = soil
    errs = []
    for rt in (1e-3, 1e-4, 1e-5):
        y, info = T.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=rt)
        assert not info["failed"].any() and np.all(info["t"] == SPAN * sd)
        errs.append(float(np.max(np.abs(y - fine))))
        print("reltol", rt, "accepted", info["accepted"], "rejected", info["rejected"], "error", errs[-1])
    assert errs[0] > errs[1] > errs[2], errs
    assert errs[0] < 1e-3 * np.max(np.abs(y0))   # (the field scale is 4.4e7: reltol 1e-3 holds it to 6.7e3)


def test_flux_faces_integrate(soil):
    case = H.heat_case(4, 60, bottom=M.BC_FLUX, top=M.BC_FLUX)
    P = T.problem(case)
    y0, sd = H.f64(case)[2], H.stable_dt(case)
    fine = T.fixed_trbdf2(P, y0, 0.0, SPAN * sd, 4000)
    errs = []
    for rt in (1e-3, 1e-4, 1e-5):
        y, info = T.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=rt)
        assert not info["failed"].any()
        errs.append(float(np.max(np.abs(y - fine))))
        print("flux faces, reltol", rt, "accepted", info["accepted"], "rejected", info["rejected"], "error", errs[-1])
    assert errs[0] > errs[1] > errs[2], errs


def test_reject_path(soil):
    """h0 = the whole span is rejected several times and the column still lands on t1; one attempt at 30 stable steps
    rejects, at 0.25 and 1 it accepts at once."""
    case, P, y0, sd, _ = soil
    y, info = T.integrate(P, y0, 0.0, SPAN * sd, SPAN * sd)
    print("h0 = span: accepted", info["accepted"], "rejected", info["rejected"])
    assert not info["failed"].any() and np.all(info["t"] == SPAN * sd)
    assert np.all((info["rejected"] >= 6) & (info["rejected"] <= 8))
    for mult, rejected in ((0.25, False), (1.0, False), (30.0, True)):
        y, info = T.integrate(P, y0, 0.0, mult * sd, mult * sd)
        assert not info["failed"].any()
        assert np.all((info["rejected"] > 0) == rejected), (mult, info["rejected"])
        if not rejected:
            assert np.all(info["accepted"] == 1)


def test_failed_columns_keep_their_state(soil):
    """Float32 planes with both tolerances 1e-14: the estimate's rounding floor (about eps32 |rhoe| / d) is far above
    the tolerance, so every column ends at the step floor with nothing accepted."""
    case, P, y0, sd, _ = soil
    y32 = y0.astype(np.float32).astype(np.float64)
    y, info = T.integrate(P, y32, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14, ft=np.float32)
    assert info["failed"].all() and not info["accepted"].any()
    assert np.array_equal(y, y32) and not info["dt_cols"].any()


def test_the_references_analytic_test():
    """heat_test_interface.jl: bottom 5 cos 2 pi t to t = 2 s, as 200 chained calls of 0.01 s with the boundary sampled at
    the interval ends and the proposals carried; abstol_e = 1e-3 rho_c_ds (the default is 10 K in this toy soil)."""
    case = H.analytic_case()
    P = T.problem(case)
    for rt in (1e-3, 1e-4, 1e-5):
        y, h0, acc, rej = H.f64(case)[2], None, 0, 0
        for k in range(200):
            ta, tb = 0.01 * k, 0.01 * (k + 1)
            y, info = T.integrate(P, y, ta, tb, 0.01, abstol_e=1e-3 * case.om.soil.rho_c_ds, reltol=rt,
                                  bcv=H.analytic_bcv(tb - ta, 1, ta), h0=h0)
            assert not info["failed"].any()
            h0, acc, rej = info["dt_cols"], acc + int(info["accepted"][0]), rej + int(info["rejected"][0])
        mse = H.analytic_mse(case, y, 2.0)
        print("analytic, reltol", rt, "accepted", acc, "rejected", rej, "mse", mse)
        assert mse < 1e-6


def test_ft_rounding_is_an_option(soil):
    case, P, y0, sd, _ = soil
    fn = T.fresh_tendency(P, y0, None)
    r32 = T.attempt(P, y0.astype(np.float32).astype(np.float64), fn, np.zeros(4), np.full(4, sd), ft=np.float32)
    for k in ("y1", "fn1", "yg", "w2"):
        assert np.array_equal(r32[k], r32[k].astype(np.float32).astype(np.float64)), k
    r64 = T.attempt(P, y0, fn, np.zeros(4), np.full(4, sd))
    assert np.max(np.abs(r32["y1"] - r64["y1"])) < 8 * np.finfo(np.float32).eps * np.max(np.abs(y0))


def test_the_two_names_are_everywhere(lh):
    header = open(os.path.join(ROOT, "include", "landhydro.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    shim = open(os.path.join(g.PKG_DIR, "julia", "LandHydrologyHIP.jl"), encoding="utf-8").read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    api = open(os.path.join(g.PKG_DIR, "csrc", "lh_api.hip")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), f"{n} is not declared in landhydro.h"
        assert n in lh._ffi.SIGNATURES, f"{n} is not in _ffi.SIGNATURES"
        assert len(lh._ffi.SIGNATURES[n][1]) == 11
        assert f"ccall((:{n}, lib)" in shim, f"the Julia shim never calls {n}"
        assert f"`{n}" in doc, f"INTEGRATION.md does not list {n}"
        assert re.search(r"^int %s\(" % n, api, flags=re.M), f"{n} is not defined in lh_api.hip"


def test_the_markers_exist_and_take_no_forcing(lh):
    for cls in (lh.HeatAdaptiveTRBDF2, lh.LayeredHeatAdaptiveTRBDF2):
        m = cls()
        assert (m.abstol_e, m.reltol) == (0.0, 0.0)
        m = cls(abstol_e=2.0, reltol=1e-4)
        assert (m.abstol_e, m.reltol) == (2.0, 1e-4)
        with pytest.raises(TypeError):
            cls(forcing=lh.BoundarySeries([0.0, 1.0], {}))
    assert issubclass(lh.LayeredHeatAdaptiveTRBDF2, lh.HeatAdaptiveTRBDF2)
    assert callable(lh.integrate_heat_trbdf2) and callable(lh.integrate_layered_heat_trbdf2)
