"""tests/layered_heat_implicit_ref.py, the NumPy reference of lh_step_layered_heat_implicit, on the CPU: the
affinity of the layered heat tendency that everything rests on, the order of both methods on a three-horizon
column, the scalar reference on classes that all equal the context's scalars -- and the new entry point's place in
the header, the binding, the built library and the Julia shim."""
import dataclasses
import os
import re

import numpy as np
import pytest

import case_model as M
import heat_implicit_ref as H
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc

NAME = "lh_step_layered_heat_implicit"
ROOT = pc.ROOT


@pytest.mark.parametrize("kind", ["cells", "horizons"])
@pytest.mark.parametrize("bc", ["dirichlet", "flux", "mixed"])
@pytest.mark.parametrize("nlev", [1, 3, 12])
def test_the_layered_heat_tendency_is_affine(kind, bc, nlev):
    """f(a x + (1 - a) y) = a f(x) + (1 - a) f(y) to 1e-13 of the largest tendency, on per-cell and three-horizon
    maps, with ice."""
    lay = LI.layered_case(np.float64, 8, nlev, kind=kind, bc=bc, ice=True, percol_bc=(bc == "mixed"))
    x = LI.state64(lay)
    c = np.arange(8)[:, None]
    y = x * (0.7 + 0.6 * pc.uhash(c, np.arange(nlev)[None, :] + 3, 1000))   # another state, +-30 %
    f = lambda r: LI.tendency(lay, r)
    scale = float(max(np.max(np.abs(f(x))), np.max(np.abs(f(y)))))
    worst = 0.0
    for a in (0.25, -0.5, 1.75):
        err = np.max(np.abs(f(a * x + (1 - a) * y) - (a * f(x) + (1 - a) * f(y))))
        worst = max(worst, float(err) / scale)
    print("affine to %.3g of the largest tendency" % worst)
    assert scale > 0 and worst <= 1e-13
    if nlev > 1:
        assert np.max(np.abs(f(x) - f(y))) > 0


def test_bands_reproduce_the_tendency_and_form_an_m_matrix():
    lay = LI.layered_case(np.float64, 5, 12, ice=True)
    y = LI.state64(lay)
    (lo, di, up), f0 = LI.affine_parts(lay)
    Ay = di * y
    Ay[:, 1:] += lo[:, 1:] * y[:, :-1]
    Ay[:, :-1] += up[:, :-1] * y[:, 1:]
    want = LI.tendency(lay, y)
    assert np.max(np.abs(Ay + f0 - want)) <= 1e-13 * np.max(np.abs(di) * np.abs(y))
    assert np.all(di < 0) and np.all(lo >= 0) and np.all(up >= 0)
    # the classes differ across the faces: the bands are not symmetric in rho_c_s, and rows of different columns differ
    assert np.ptp(di[:, 5]) > 0.01 * np.abs(di[:, 5]).max()


@pytest.mark.parametrize("method", ["euler", "trbdf2"])
def test_order(method):
    """Error ratio per halving of dt over 2000 stable steps of 24-level three-horizon columns with constant
    Dirichlet values (layered_heat_implicit_ref.order_case).  Measured: backward Euler (4, 8, 16, 32 steps) 2.08,
    2.07, 2.05; TR-BDF2 (8, 16, 32) 4.08, 4.04 (from 4 to 8 steps 4.95: not yet asymptotic, not asserted)."""
    lo, hi = LI.ORDER_BANDS[method]
    errs = LI.order_errors(method, lambda lay, dt, n: LI.heat_implicit(lay, LI.state64(lay), dt, n, method))
    r = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
    print(method, errs, r)
    assert all(lo <= x <= hi for x in r), (errs, r)


def _oracle_built():
    try:
        pc.O.rhs
        return True
    except Exception:
        return False


@pytest.mark.parametrize("method", ["euler", "trbdf2"])
@pytest.mark.parametrize("bc", ["dirichlet", "flux"])
def test_classes_equal_to_the_scalars_give_the_scalar_reference(method, bc):
    """Every class the context's own scalars: the layered reference equals heat_implicit_ref.heat_implicit (built on
    the oracle's tendency) on the same case, to 1e-12 of the field scale."""
    if not _oracle_built():
        pytest.skip("the CPU oracle is not built")
    ncols, nlev = 6, 12
    base = LI.layered_case(np.float64, ncols, nlev, kind="horizons", bc=bc, ice=True)
    om = base.case.om
    k = [om.vg.n, om.vg.alpha, om.vg.theta_r, om.vg.Ksat, om.soil.nu, om.soil.S_s]
    th = [getattr(om.soil, n) for n in LH.THERMAL_FIELDS]
    lay = LH.LayeredHeat(base.case, np.array([k] * 3), np.array([th] * 3), base.class_map)
    vl, ti, re = (np.asarray(a, np.float64) for a in (lay.case.vl, lay.case.ti, lay.case.rhoe))
    sd = LI.stable_dt(lay)
    bcv = None
    if bc == "dirichlet":
        bcv = np.zeros((4, 2, 2))
        bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = 281.0 + np.arange(4)
        bcv[:, M.FACE_TOP, M.COMP_ENERGY] = 287.0 - 0.5 * np.arange(4)
    for mult in (1.0, 30.0, 1000.0):
        got = LI.heat_implicit(lay, re, mult * sd, 3, method, bcv=bcv)
        want = H.heat_implicit(om, vl, ti, re, mult * sd, 3, method, bcv=bcv)
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("%s %s %gx: %.3g of the field scale" % (method, bc, mult, err))
        assert err <= 1e-12
        assert np.max(np.abs(want - re)) > 0


def test_the_entry_point_is_declared_bound_exported_and_called():
    """lh_step_layered_heat_implicit in include/landhydro.h, in _ffi.SIGNATURES with lh_step_heat_implicit's
    signature, exported by the built library, defined in lh_api.hip and called once by the Julia shim."""
    lh = pc._pkg()
    read = lambda *p: open(os.path.join(ROOT, *p), encoding="utf-8").read()
    header = read("include", "landhydro.h")
    assert re.search(r"^int\s+%s\s*\(" % NAME, header, flags=re.M), "%s is not declared in landhydro.h" % NAME
    assert NAME in lh._ffi.SIGNATURES, "%s is not in _ffi.SIGNATURES" % NAME
    res, args = lh._ffi.SIGNATURES[NAME]
    assert (res, args) == lh._ffi.SIGNATURES["lh_step_heat_implicit"]
    assert hasattr(lh._ffi.lib(), NAME), "%s is not exported by the library" % NAME
    assert re.search(r"^int %s\(" % NAME, read("landhydrology.jl_amd", "csrc", "lh_api.hip"), flags=re.M)
    assert read("landhydrology.jl_amd", "julia", "LandHydrologyHIP.jl").count("ccall((:%s, lib)" % NAME) == 1
    assert "`%s`" % NAME in read("INTEGRATION.md")


def test_the_markers_check_their_scope_without_a_device():
    """LayeredHeatImplicitEuler / LayeredHeatTRBDF2: a heat-only model with soil_classes; the scalar markers keep
    refusing such a model."""
    lh = pc._pkg()
    FT = np.float64
    assert issubclass(lh.LayeredHeatImplicitEuler, lh.HeatImplicitEuler)
    assert issubclass(lh.LayeredHeatTRBDF2, lh.LayeredHeatImplicitEuler)
    assert lh.LayeredHeatImplicitEuler.method == "euler" and lh.LayeredHeatTRBDF2.method == "trbdf2"
    dom = lh.Column(FT, zlim=(-0.2, 0.0), nelements=10)
    ebc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)), bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)))
    heat = lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.PrescribedHydrologyModel(),
                        boundary_conditions=ebc, earth_param_set=lh.EarthParameterSet())
    for marker in (lh.LayeredHeatImplicitEuler(), lh.LayeredHeatTRBDF2()):
        with pytest.raises(NotImplementedError, match=type(marker).__name__ + ".*HeatImplicitEuler"):
            marker.check_scope(heat)
    with pytest.raises(NotImplementedError, match="soil_classes"):
        lh.step_implicit_layered_heat(heat, object(), None)
    with pytest.raises(ValueError):
        lh.step_implicit_layered_heat(heat, object(), None, method="rk4")
