"""lh_integrate_heat_dense / lh_integrate_layered_coupled_dense without a device: the host
mirror's two functions and their saveat validation, the entry points in the header, the ctypes table and the Julia
text, and the order of the heat-only interpolant on the NumPy reference the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import dense_ref as D
import heat_implicit_ref as H
import heat_trbdf2_ref as T
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_heat_trbdf2_ref as LT
import layered_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("integrate_heat_dense", "integrate_layered_coupled_dense")


@pytest.fixture(scope="module")
def lh():
    return g.load_package()


def heat_model(lh, FT=np.float64):
    return lh.SoilModel(FT, domain=lh.Column(FT, zlim=(0.0, 0.2), nelements=12, ncolumns=3), energy_model=lh.SoilEnergyModel(),
                        hydrology_model=lh.PrescribedHydrologyModel(),
                        boundary_conditions=lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(-2.0)),
                                                            bottom=lh.SoilComponentBC(energy=lh.Dirichlet(lambda t: 284.0))),
                        soil_param_set=lh.SoilParams(FT, ν=0.495, ν_ss_gravel=0.1, ν_ss_om=0.1, ν_ss_quartz=0.1, ρc_ds=2.0e6,
                                                     κ_solid=8.0, κ_sat_unfrozen=0.57, κ_sat_frozen=2.29),
                        earth_param_set=lh.EarthParameterSet())


def test_the_two_functions_exist_and_are_exported(lh):
    for name in NAMES:
        assert callable(getattr(lh, name)) and name in lh.__all__, name
        assert callable(getattr(lh.soil, name))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("saveat,word", [
    ([3.0, 2.0], "save time 1"),                 # unsorted
    ([1.0, 1.0], "save time 1"),                 # not strictly increasing
    ([1.0, float("nan")], "save time 1"),
    ([float("inf")], "save time 0"),
    ([-1.0, 2.0], "save time 0"),                # before t0
    ([1.0, 11.0], "save time 1"),                # after t1
    ([[1.0, 2.0]], "sequence"),
])
def test_saveat_is_validated_under_the_functions_own_name_before_any_library_call(lh, name, saveat, word):
    """No device is touched: Y and Ya are never looked at (None), the model has no backend yet, and the scope (a
    heat-only model handed to the coupled function) is not looked at either: saveat comes first."""
    model = heat_model(lh)
    with pytest.raises(ValueError) as e:
        getattr(lh, name)(model, None, None, 0.0, 10.0, 1.0, saveat)
    msg = str(e.value)
    assert msg.startswith(name + ":") and word in msg, msg


def test_check_saveat_keeps_todays_words_by_default(lh):
    with pytest.raises(ValueError, match=r"^integrate_dense: save time 1 is not after save time 0"):
        lh.soil._check_saveat([2.0, 1.0], 0.0, 10.0)
    with pytest.raises(ValueError, match=r"^integrate_heat_dense: at most 65536 save times"):
        lh.soil._check_saveat(np.arange(65537.0), 0.0, 1e6, "integrate_heat_dense")
    np.testing.assert_array_equal(lh.soil._check_saveat([0.0, 10.0], 0.0, 10.0, "integrate_heat_dense"), [0.0, 10.0])


def test_a_series_must_be_a_boundary_series_or_none_and_the_scope_is_the_series_twins(lh):
    model = heat_model(lh)
    with pytest.raises(TypeError, match="integrate_heat_dense: series must be a BoundarySeries or None"):
        lh.integrate_heat_dense(model, None, None, 0.0, 10.0, 1.0, [1.0], series="not a series")
    # a heat-only model is not the coupled function's, a model without soil classes neither: the series twin's words
    with pytest.raises(NotImplementedError, match="coupled models only"):
        lh.integrate_layered_coupled_dense(model, None, None, 0.0, 10.0, 1.0, [1.0])


def _declared(name):
    header = open(os.path.join(ROOT, "include", "landhydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert m, name + " is not declared in landhydro.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_in_header_ffi_and_julia(lh):
    F = lh._ffi
    tail = ["void* dt_cols_device_ft", "int32_t nsave", "const double* save_times", "lh_state* const* snapshots"]
    head = ["lh_ctx*", "lh_state* Y", "const lh_state* Ya", "const lh_bc_series* series", "double t0", "double t1", "double dt"]
    assert _declared("lh_integrate_heat_dense") == head + ["double abstol_e", "double reltol", "uint32_t flags"] + tail
    assert _declared("lh_integrate_layered_coupled_dense") == head + ["double abstol", "double abstol_e", "double reltol",
                                                                      "uint32_t flags"] + tail
    # the bindings: the series twin's arguments, then lh_integrate_dense's three
    dense_tail = F.SIGNATURES["lh_integrate_dense"][1][12:]
    for name, twin in (("lh_integrate_heat_dense", "lh_integrate_heat_series"),
                       ("lh_integrate_layered_coupled_dense", "lh_integrate_layered_coupled_series")):
        res, args = F.SIGNATURES[name]
        twin_res, twin_args = F.SIGNATURES[twin]
        assert res is twin_res and args == twin_args + dense_tail, name
    text = open(os.path.join(g.PKG_DIR, "julia", "LandHydrologyHIP.jl"), encoding="utf-8").read()
    for name in NAMES:
        assert "ccall((:lh_%s, lib), Cint" % name in text and "function %s!(" % name in text, name


# ------------------------------------------------------------------ the heat-only interpolant on the NumPy reference

def _families():
    """(label, Problem, rhoe_int, stable step) of a scalar and a layered heat-only case, 5 columns x 12 levels"""
    case = H.heat_case(5, 12, np.float64, bottom=M.BC_DIRICHLET, top=M.BC_FLUX)
    yield "scalar", T.problem(case), H.f64(case)[2], H.stable_dt(case)
    c, lev = np.arange(5)[:, None], np.arange(12)[None, :]
    cmap = ((lev >= 3 + c % 3).astype(np.uint8) + (lev >= 8 + c % 4).astype(np.uint8))
    lay = LH.make_layered_heat(np.float64, 5, 12, cmap, model=M.MODEL_HEAT, classes=R.texture_classes()[[0, 5, 2]],
                               thermal=LH.thermal_classes()[[0, 4, 2]], bc="dirichlet", name="dense_heat_cpu")
    yield "layered", LT.problem(lay), lay.case.rhoe.astype(np.float64), LI.stable_dt(lay)


def _interpolant_error(P, y0, h, theta, sub=32):
    """(largest error of the interpolant of one attempt of h at theta against `sub` equal sub-steps of the span, the
    attempt): heat_trbdf2_ref.true_local_error's yardstick, read at the sub-step that ends at t + theta h"""
    n = y0.shape[0]
    fn = T.fresh_tendency(P, y0, None)
    r = T.attempt(P, y0, fn, np.zeros(n), np.full(n, h))
    u = D.hermite(theta, h, y0, r["y1"], fn, r["fn1"])
    k_end = theta * sub
    assert k_end == int(k_end)
    yy, ff = y0, fn
    for k in range(int(k_end)):
        q = T.attempt(P, yy, ff, np.full(n, k * h / sub), np.full(n, h / sub))
        yy, ff = q["y1"], q["fn1"]
    return float(np.max(np.abs(u - yy))), r, fn


def test_the_heat_interpolant_is_exact_at_the_ends_and_third_order():
    """theta = 0 / 1 give y / y1 of heat_trbdf2_ref.attempt exactly.  Against the 32-sub-step refinement the error
    behaves as C h^3 (1 - c h): the interpolant's own error is O(h^4), what remains is TR-BDF2's third-order local
    error in y1 and f_n+1.  The factor by which it falls when h is halved therefore tends to 8 FROM BELOW -- measured on
    this reference in the scalar case at theta = 1/2: 6.58 from 1 stable step to 1/2, 7.17 to 1/4, 7.56 to 1/8, 7.77 to
    1/16 -- and does not reach it at a usable step.  A factor of "at least 8" is therefore not what a third-order
    quantity shows here; the check is the order itself: the factor rises from halving to halving, and between 1/8 and
    1/16 of a stable step it is above 2^2.9 = 7.46 and not above 8 (an observed order between 2.9 and 3)."""
    for label, P, y0, sd in _families():
        _, r, fn = _interpolant_error(P, y0, sd, 0.5)
        np.testing.assert_array_equal(D.hermite(0.0, sd, y0, r["y1"], fn, r["fn1"]), y0)
        np.testing.assert_array_equal(D.hermite(1.0, sd, y0, r["y1"], fn, r["fn1"]), r["y1"])
        assert np.max(np.abs(r["y1"] - y0)) > 0
        for theta in (0.25, 0.5, 0.75):
            errs = [_interpolant_error(P, y0, sd / 2 ** k, theta)[0] for k in range(5)]
            factors = [a / b for a, b in zip(errs, errs[1:])]
            print(label, "theta", theta, "errors", ["%.4g" % e for e in errs], "factors", ["%.3f" % f for f in factors])
            assert all(b > a for a, b in zip(factors, factors[1:])), (label, theta, factors)
            assert 2.0 ** 2.9 < factors[-1] <= 8.0, (label, theta, factors)
