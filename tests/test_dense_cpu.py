"""lh_integrate_dense without a device: the host mirror's saveat validation, the entry point in the header, the
ctypes table and the Julia text, and the NumPy interpolant the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import dense_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lh():
    return g.load_package()


def richards_model(lh, FT=np.float64):
    return lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-0.24, 0.0), nelements=12, ncolumns=3),
                        energy_model=lh.PrescribedTemperatureModel(),
                        hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(
                            FT, n=2.0, α=2.6, Ksat=1e-6, θr=0.05)),
                        boundary_conditions=lh.SoilColumnBC(
                            top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-2e-9)),
                            bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                        soil_param_set=lh.SoilParams(FT, ν=0.45, S_s=1e-3), earth_param_set=lh.EarthParameterSet())


@pytest.mark.parametrize("saveat,word", [
    ([3.0, 2.0], "save time 1"),                 # unsorted
    ([1.0, 1.0], "save time 1"),                 # not strictly increasing
    ([1.0, float("nan")], "save time 1"),
    ([float("inf")], "save time 0"),
    ([-1.0, 2.0], "save time 0"),                # before t0
    ([1.0, 11.0], "save time 1"),                # after t1
    ([[1.0, 2.0]], "sequence"),
])
def test_saveat_is_validated_before_any_library_call(lh, saveat, word):
    """No device is touched: Y and Ya are never looked at (None), and the model has no backend yet."""
    model = richards_model(lh)
    with pytest.raises(ValueError) as e:
        lh.integrate_dense(model, None, None, 0.0, 10.0, 1.0, saveat)
    assert "integrate_dense" in str(e.value) and word in str(e.value), str(e.value)


def test_saveat_accepts_the_ends_and_an_empty_list(lh):
    soil = lh.soil
    np.testing.assert_array_equal(soil._check_saveat([0.0, 2.5, 10.0], 0.0, 10.0), [0.0, 2.5, 10.0])
    assert soil._check_saveat([], 0.0, 10.0).size == 0
    with pytest.raises(ValueError):
        soil._check_saveat(np.arange(65537.0), 0.0, 1e6)
    with pytest.raises(TypeError):
        lh.integrate_dense(richards_model(lh), None, None, 0.0, 10.0, 1.0, [1.0], series="not a series")


def test_entry_point_in_header_ffi_and_julia(lh):
    header = open(os.path.join(ROOT, "include", "landhydro.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+lh_integrate_dense\s*\(([^;]*)\)\s*;", code)
    assert m, "lh_integrate_dense is not declared in landhydro.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 15 and args[3].startswith("const lh_bc_series*") and args[12].startswith("int32_t")
    assert args[13].startswith("const double*") and args[14].startswith("lh_state* const*")
    res, argtypes = lh._ffi.SIGNATURES["lh_integrate_dense"]
    series_res, series_args = lh._ffi.SIGNATURES["lh_integrate_series"]
    assert res is series_res and len(argtypes) == 15 and argtypes[:12] == series_args
    text = open(os.path.join(g.PKG_DIR, "julia", "LandHydrologyHIP.jl"), encoding="utf-8").read()
    assert "ccall((:lh_integrate_dense, lib), Cint" in text and "function integrate_dense!(" in text
    assert "integrate_dense" in lh.__all__


def test_hermite_reference():
    rng = np.random.default_rng(7)
    y0, y1, f0, f1 = rng.normal(size=(4, 5, 12))
    h = 37.5
    # exact at both ends
    np.testing.assert_array_equal(D.hermite(0.0, h, y0, y1, f0, f1), y0)
    np.testing.assert_array_equal(D.hermite(1.0, h, y0, y1, f0, f1), y1)
    # reproduces a cubic to round-off: p(t) = a + b t + c t^2 + d t^3 on [t0, t0 + h]
    a, b, c, d = 0.3, -0.02, 1.5e-3, -4e-5
    p = lambda t: a + t * (b + t * (c + t * d))
    dp = lambda t: b + t * (2 * c + t * 3 * d)
    t0 = 2.0
    for theta in (0.125, 0.25, 0.5, 0.75, 0.9):
        got = D.hermite(theta, h, p(t0), p(t0 + h), dp(t0), dp(t0 + h))
        want = p(t0 + theta * h)
        scale = max(abs(p(t0)), abs(p(t0 + h)), h * abs(dp(t0)), h * abs(dp(t0 + h)))
        assert abs(got - want) <= 16 * np.finfo(np.float64).eps * scale, (theta, got, want)
    # ... and its slope at the ends is f0, f1 (central difference of the polynomial in theta, h = 1)
    e = 1e-6
    s0 = (D.hermite(e, 1.0, 0.2, 0.7, 3.0, -2.0) - D.hermite(-e, 1.0, 0.2, 0.7, 3.0, -2.0)) / (2 * e)
    s1 = (D.hermite(1 + e, 1.0, 0.2, 0.7, 3.0, -2.0) - D.hermite(1 - e, 1.0, 0.2, 0.7, 3.0, -2.0)) / (2 * e)
    assert abs(s0 - 3.0) < 1e-8 and abs(s1 + 2.0) < 1e-8
