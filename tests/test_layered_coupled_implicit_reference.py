"""tests/layered_coupled_implicit_ref.py, the NumPy reference of lh_step_layered_coupled_implicit, on the CPU: the
block structure of the layered coupled tendency that everything rests on, the scalar reference on classes that all
equal the context's scalars, the full residual of a step, the order of both methods -- and the new entry point's
place in the header, the binding, the built library and the Julia shim."""
import os
import re

import numpy as np
import pytest

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import parity_cases as pc

NAME = "lh_step_layered_coupled_implicit"
ROOT = pc.ROOT
HYDS = {"flux": (M.BC_FLUX, M.BC_FLUX), "dirichlet_drain": (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE),
        "dirichlet": (M.BC_DIRICHLET, M.BC_DIRICHLET)}


@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
@pytest.mark.parametrize("hyd,energy", [("flux", "flux"), ("dirichlet_drain", "dirichlet"), ("dirichlet", "mixed")])
@pytest.mark.parametrize("kind", ["horizons", "cells"])
def test_the_stage_jacobian_is_block_lower_triangular(kind, hyd, energy, ice):
    """On 8 x 24 columns: the water tendency is bitwise unchanged when rhoe_int is replaced by 1.37 rhoe_int + 5e5,
    and the second difference of the energy tendency in rhoe_int is at most 1e-10 of its largest value."""
    lay = LH.as64(LC.layered_case(np.float64, 8, 24, kind=kind, hyd=HYDS[hyd], energy=energy, ice=ice))
    vl, e = LC.state64(lay)
    fw, fe = LC.tendencies(lay, vl, e)
    fw2, _ = LC.tendencies(lay, vl, 1.37 * e + 5e5)
    np.testing.assert_array_equal(fw, fw2)
    assert np.max(np.abs(fw)) > 0
    c = np.arange(8)[:, None]
    d = np.abs(e).max() * (0.1 + 0.2 * pc.uhash(c, np.arange(24)[None, :] + 3, 1000))
    second = LC.tendencies(lay, vl, e + d)[1] - 2.0 * fe + LC.tendencies(lay, vl, e - d)[1]
    worst = float(np.max(np.abs(second)) / np.max(np.abs(fe)))
    print("second difference of f_e: %.3g of its largest value" % worst)
    assert worst <= 1e-10
    assert np.max(np.abs(LC.tendencies(lay, vl, e + d)[1] - fe)) > 0


@pytest.mark.parametrize("method", ["euler", "trbdf2"])
def test_classes_equal_to_the_scalars_give_the_scalar_reference(method):
    """Every class the context's own scalars: the layered reference equals coupled_implicit_ref.coupled_implicit
    (built on the oracle's tendency) on the same case, to 1e-12 of the field scale of each component."""
    import coupled_implicit_ref as CR
    base = LC.layered_case(np.float64, 6, 12, kind="horizons", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)
    om = base.case.om
    k = [om.vg.n, om.vg.alpha, om.vg.theta_r, om.vg.Ksat, om.soil.nu, om.soil.S_s]
    th = [getattr(om.soil, n) for n in LH.THERMAL_FIELDS]
    lay = LH.LayeredHeat(base.case, np.array([k] * 3), np.array([th] * 3), base.class_map)
    vl, e = LC.state64(lay)
    ti = np.asarray(lay.case.ti, np.float64)
    sd = LC.stable_dt(lay)
    bcv = np.zeros((4, 2, 2))
    bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = 281.0 + np.arange(4)
    bcv[:, M.FACE_TOP, M.COMP_ENERGY] = 287.0 - 0.5 * np.arange(4)
    bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = 0.30 + 0.005 * np.arange(4)
    for mult in (1.0, 30.0):
        gv, ge, gi = LC.coupled_implicit(lay, vl, e, mult * sd, 3, method, bcv=bcv)
        wv, we, wi = CR.coupled_implicit(om, vl, ti, e, mult * sd, 3, method, bcv=bcv)
        ev = float(np.max(np.abs(gv - wv)) / np.max(np.abs(wv)))
        ee = float(np.max(np.abs(ge - we)) / np.max(np.abs(we)))
        print("%s %gx: vl %.3g, rhoe %.3g of the field scale" % (method, mult, ev, ee))
        assert ev <= 1e-12 and ee <= 1e-12
        assert gi["unconverged"] == 0 and wi["unconverged"] == 0
        assert np.max(np.abs(wv - vl)) > 0 and np.max(np.abs(we - e)) > 0


@pytest.mark.parametrize("kind", ["horizons", "cells"])
def test_residual_of_a_backward_euler_step(kind):
    """The full residual Y1 - Yn - dt f(Y1) of one reference step at 10x and 100x the stable step: the water to
    1e-12 of nu (Newton to round-off), the energy to 1e-12 of ||rhoe_int|| (one exact solve)."""
    lay = LC.layered_case(np.float64, 6, 24, kind=kind, hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)
    vl, e = LC.state64(lay)
    sd = LC.stable_dt(lay)
    for mult in (10.0, 100.0):
        v1, e1, info = LC.coupled_implicit(lay, vl, e, mult * sd, 1)
        rw, re = LC.residual(lay, vl, e, v1, e1, mult * sd)
        print("%s %gx: iterations %d, water %.3g, energy %.3g of ||rhoe_int||" %
              (kind, mult, info["iters"], np.max(np.abs(rw)), np.max(np.abs(re)) / np.max(np.abs(e))))
        assert info["unconverged"] == 0
        assert np.max(np.abs(rw)) <= 1e-12 * float(lay.classes[:, 4].max())
        assert np.max(np.abs(re)) <= 1e-12 * np.max(np.abs(e))
        assert np.max(np.abs(v1 - vl)) > 0 and np.max(np.abs(e1 - e)) > 0


@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
def test_the_reference_newton_at_100x_with_class_0_on_a_wetted_dirichlet_face(ice):
    """The fact behind one choice of tests/test_gpu_layered_coupled_implicit.py::test_residual_through_the_tendency:
    130 x 24 with the three horizons 0, 5, 2 (bottom to top) under a free-draining top and a Dirichlet bottom.  Under
    the device's rule and cap (tol 1e-10, 50 iterations) the reference's safeguarded Newton converges in every column
    at 10x the stable step and leaves some unconverged at 100x (measured: 7 without ice, 3 with); with the horizons
    2, 5, 0 it converges in every column at both."""
    import layered_ref as R
    hyd = (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET)
    left = {}
    for name, classes in (("0,5,2", None), ("2,5,0", R.texture_classes()[[2, 5, 0]])):
        lay = LC.layered_case(np.float64, 130, 24, kind="horizons", hyd=hyd, energy="dirichlet", ice=ice, classes=classes)
        vl, _ = LC.state64(lay)
        sd = LC.stable_dt(lay)
        for mult in (10.0, 100.0):
            _, its, conv = LC.newton_stage(LC.with_bc(lay, None), vl, vl, mult * sd, 1e-10, 50)
            left[(name, mult)] = int((~conv).sum())
            print("horizons %s ice=%s %gx: iterations at most %d, unconverged %d of 130" % (name, ice, mult, its.max(), left[(name, mult)]))
    assert left[("0,5,2", 10.0)] == 0 and left[("0,5,2", 100.0)] > 0
    assert left[("2,5,0", 10.0)] == 0 and left[("2,5,0", 100.0)] == 0


def test_the_entry_point_is_declared_bound_exported_and_called():
    """lh_step_layered_coupled_implicit in include/landhydro.h, in _ffi.SIGNATURES with lh_step_coupled_implicit's
    signature, exported by the built library, defined in lh_api.hip and called once by the Julia shim."""
    lh = pc._pkg()
    read = lambda *p: open(os.path.join(ROOT, *p), encoding="utf-8").read()
    header = read("include", "landhydro.h")
    assert re.search(r"^int\s+%s\s*\(" % NAME, header, flags=re.M), "%s is not declared in landhydro.h" % NAME
    assert NAME in lh._ffi.SIGNATURES, "%s is not in _ffi.SIGNATURES" % NAME
    assert lh._ffi.SIGNATURES[NAME] == lh._ffi.SIGNATURES["lh_step_coupled_implicit"]
    assert hasattr(lh._ffi.lib(), NAME), "%s is not exported by the library" % NAME
    assert re.search(r"^int %s\(" % NAME, read("landhydrology.jl_amd", "csrc", "lh_api.hip"), flags=re.M)
    assert read("landhydrology.jl_amd", "julia", "LandHydrologyHIP.jl").count("ccall((:%s, lib)" % NAME) == 1
    assert "`%s`" % NAME in read("INTEGRATION.md")


def test_the_markers_check_their_scope_without_a_device():
    """LayeredCoupledImplicitEuler / LayeredCoupledTRBDF2 are coupled markers; on a coupled model without
    soil_classes and on a heat-only model they raise in the library's words."""
    lh = pc._pkg()
    FT = np.float64
    assert issubclass(lh.LayeredCoupledImplicitEuler, lh.CoupledImplicitEuler)
    assert issubclass(lh.LayeredCoupledTRBDF2, lh.LayeredCoupledImplicitEuler)
    assert lh.LayeredCoupledImplicitEuler.method == "euler" and lh.LayeredCoupledTRBDF2.method == "trbdf2"
    dom = lh.Column(FT, zlim=(-0.2, 0.0), nelements=10)
    flux = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                           bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    coupled = lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                           boundary_conditions=flux, earth_param_set=lh.EarthParameterSet())
    ebc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)), bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)))
    heat = lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.PrescribedHydrologyModel(),
                        boundary_conditions=ebc, earth_param_set=lh.EarthParameterSet())
    for marker in (lh.LayeredCoupledImplicitEuler(), lh.LayeredCoupledTRBDF2()):
        with pytest.raises(NotImplementedError, match=type(marker).__name__ + ": the context has no class map"):
            marker.check_scope(coupled)
        with pytest.raises(NotImplementedError, match=type(marker).__name__ + ": coupled models only"):
            marker.check_scope(heat)
    with pytest.raises(NotImplementedError, match="lh_step_coupled_implicit steps a model without soil classes"):
        lh.step_implicit_layered_coupled(coupled, object(), None)
    with pytest.raises(ValueError):
        lh.step_implicit_layered_coupled(coupled, object(), None, method="rk4")


@pytest.mark.parametrize("method", ["euler", "trbdf2"])
def test_order(method):
    """Error ratios per halving of h over 16 stable steps of 24-level three-horizon columns with ice, against
    layered_heat_ref.ssprk33 at an eighth of the stable step, within coupled_implicit_ref.ORDER_BANDS."""
    lo, hi = LC.ORDER_BANDS[method]
    solve = lambda lay, dt, n: LC.coupled_implicit(lay, *LC.state64(lay), dt, n, method)[:2]
    ratios, errs = LC.order_ratios(method, solve)
    print(method, errs, ratios)
    assert all(lo <= r <= hi for rs in ratios.values() for r in rs), (errs, ratios)
