"""lh_integrate_heat_series / lh_integrate_layered_coupled_series without a device: the two entry points through every
layer that names them (header, library source, ctypes signatures, the Julia shim), the three series
markers, and the chain the entry points stand for, driven through the NumPy reference (tests/heat_trbdf2_ref.py) with
BoundarySeries.breakpoints / value_at and held against the energy budget of the series' own boundary flux."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import heat_implicit_ref as H
import heat_trbdf2_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "landhydrology.jl_amd")
ENTRIES = {"lh_integrate_heat_series": 11, "lh_integrate_layered_coupled_series": 12}
JULIA = {"lh_integrate_heat_series": "integrate_heat_series!", "lh_integrate_layered_coupled_series": "integrate_layered_coupled_series!"}


def _read(*parts):
    with open(os.path.join(*parts), encoding="utf-8") as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_entry_points_exist_in_every_layer(name):
    lh = g.load_package()
    header = _read(ROOT, "include", "landhydro.h")
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, name + " is not declared in include/landhydro.h"
    assert len(m.group(1).split(",")) == ENTRIES[name]
    api = _read(PKG, "csrc", "lh_api.hip")
    assert re.search(r"^int %s\(lh_ctx\* c," % name, api, re.M), name + " is not defined in lh_api.hip"
    restype, argtypes = lh._ffi.SIGNATURES[name]
    assert len(argtypes) == ENTRIES[name]
    julia = _read(PKG, "julia", "LandHydrologyHIP.jl")
    assert ":" + name in julia and "function " + JULIA[name] in julia
    assert "`%s`" % name in _read(ROOT, "INTEGRATION.md")


def _series(lh):
    return lh.BoundarySeries([0.0, 1.0, 3.0], {("top", "energy"): [1.0, 2.0, 0.5]})


def test_the_series_markers_require_a_boundary_series():
    lh = g.load_package()
    fs = _series(lh)
    parents = {lh.HeatSeriesTRBDF2: lh.HeatAdaptiveTRBDF2, lh.LayeredHeatSeriesTRBDF2: lh.LayeredHeatAdaptiveTRBDF2,
               lh.LayeredCoupledSeriesTRBDF2: lh.LayeredCoupledAdaptiveTRBDF2}
    for marker, parent in parents.items():
        assert issubclass(marker, parent)
        m = marker(forcing=fs)
        assert m.forcing is fs and marker(fs).forcing is fs
        assert marker.check_scope is parent.check_scope
        for bad in (None, 3.0, {("top", "energy"): [1.0]}):
            with pytest.raises(TypeError, match=marker.__name__ + ": forcing must be a BoundarySeries"):
                marker(forcing=bad)
        with pytest.raises(TypeError):
            marker()
    assert issubclass(lh.LayeredHeatSeriesTRBDF2, lh.HeatAdaptiveTRBDF2)
    assert issubclass(lh.LayeredCoupledSeriesTRBDF2, lh.CoupledAdaptiveTRBDF2)
    m = lh.HeatSeriesTRBDF2(fs, abstol_e=2.0, reltol=1e-5)
    assert (m.abstol_e, m.reltol) == (2.0, 1e-5)
    m = lh.LayeredCoupledSeriesTRBDF2(fs, abstol=1e-7, abstol_e=3.0, reltol=1e-4)
    assert (m.abstol, m.abstol_e, m.reltol) == (1e-7, 3.0, 1e-4)


def test_the_old_markers_still_take_no_forcing():
    lh = g.load_package()
    fs = _series(lh)
    for marker in (lh.HeatAdaptiveTRBDF2, lh.LayeredHeatAdaptiveTRBDF2, lh.LayeredCoupledAdaptiveTRBDF2):
        with pytest.raises(TypeError):
            marker(forcing=fs)
        with pytest.raises(TypeError):
            marker(forcing=None)
        assert getattr(marker(), "forcing", None) is None


def test_the_two_functions_require_a_boundary_series():
    lh = g.load_package()
    for call in (lh.integrate_heat_series, lh.integrate_layered_coupled_series):
        for bad in (None, [0.0, 1.0], object()):
            with pytest.raises(TypeError, match=call.__name__ + ": series must be a BoundarySeries"):
                call(object(), object(), None, bad, 0.0, 1.0, 1.0)


@pytest.mark.parametrize("reltol", [1e-3, 1e-5])
def test_the_chain_keeps_the_budget_of_the_series_flux(reltol):
    """A flux at both faces, the top one a series: the reference integrator chained over BoundarySeries.breakpoints with
    bcv = value_at at both ends of every sub-interval.  sum_i rhoe_int changes by the trapezoid integral over the
    breakpoints of (F_bottom - F_top) / dz -- TR-BDF2 integrates a source that is linear in time exactly, whatever steps
    a column chose -- to rounding: nlev 4 eps sum |rhoe_int|, the bound of
    tests/test_gpu_heat_trbdf2.py::test_conservation_with_flux_faces."""
    lh = g.load_package()
    case = H.heat_case(8, 12, np.float64, bottom=M.BC_FLUX, top=M.BC_FLUX, ice=True)
    P = T.problem(case)
    y0, sd = H.f64(case)[2], H.stable_dt(case)
    fb, ft = H.BC_VALUES[M.BC_FLUX]
    knots = np.array([0.0, 7.0, 12.0, 25.0, 31.0]) * sd
    top = ft * np.array([1.0, 3.0, 0.5, -2.0, 1.5])
    fs = lh.BoundarySeries(knots, {("top", "energy"): top})
    t0, t1 = 2.5 * sd, 28.0 * sd
    bp = fs.breakpoints(t0, t1)
    assert len(bp) == 5 and bp[0] == t0 and bp[-1] == t1 and bp[1:-1] == [float(x) for x in knots[1:4]]
    y, h0 = y0, None
    integral, steps = 0.0, 0
    for a, b in zip(bp, bp[1:]):
        bcv = np.zeros((2, 2, 2))
        bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = fb
        va, vb = fs.value_at(("top", "energy"), a), fs.value_at(("top", "energy"), b)
        bcv[0, M.FACE_TOP, M.COMP_ENERGY], bcv[1, M.FACE_TOP, M.COMP_ENERGY] = va, vb
        y, info = T.integrate(P, y, a, b, sd, reltol=reltol, bcv=bcv, h0=h0)
        assert not info["failed"].any()
        h0 = info["dt_cols"]                                   # the proposals are carried from call to call
        steps += int(info["accepted"].sum())
        integral += 0.5 * (b - a) * ((fb - va) + (fb - vb))    # (the series is linear on [a, b]: the trapezoid is exact)
    dz = (case.om.zmax - case.om.zmin) / case.om.nlev
    change = y.sum(axis=1) - y0.sum(axis=1)
    want = integral / dz
    allowed = case.om.nlev * 4 * float(np.finfo(np.float64).eps) * np.abs(y0).sum(axis=1)
    print(f"series budget, reltol {reltol}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, expected change "
          f"{want:.6g}, accepted steps {steps}")
    assert abs(want) > 1e3 * np.max(allowed) and steps >= 4 * 8
    assert np.all(np.abs(change - want) <= allowed), float(np.max(np.abs(change - want) / allowed))
    # (the interior knots are read: the series' ends alone give another integral)
    flat = 0.5 * (t1 - t0) * ((fb - fs.value_at(("top", "energy"), t0)) + (fb - fs.value_at(("top", "energy"), t1)))
    assert abs(flat - integral) > 0.01 * abs(integral)


def test_advance_without_the_hook_still_calls_integrate_series(monkeypatch):
    """A method object that carries `forcing` and the tolerances only (no integrate_forcing) takes the path it took
    before the hook existed: one integrate_series call with its own arguments; one with the hook takes the hook."""
    import types
    lh = g.load_package()
    soil = lh.soil
    fs = _series(lh)
    calls = []
    stats = dict(accepted=3, rejected=1, newton_iterations=0, max_steps=2, failed=0, wave_steps=128, unconverged=0)
    monkeypatch.setattr(soil, "integrate_series", lambda *a: calls.append(a) or dict(stats))
    it = types.SimpleNamespace(t=0.0, dt=0.5, u="Y", p="Ya", _dt_cols="cols", trbdf2_stats=dict.fromkeys(stats, 0))
    plain = types.SimpleNamespace(forcing=fs, abstol=1e-7, reltol=1e-4)
    sim = types.SimpleNamespace(integrator=it, method=plain, model="model")
    assert soil._advance_trbdf2(sim, 2.0) == 2.0 and it.t == 2.0
    assert calls == [("model", "Y", "Ya", fs, 0.0, 2.0, 0.5, 1e-7, None, 1e-4, True, "cols")]
    assert it.trbdf2_stats == stats
    hooked = lh.HeatSeriesTRBDF2(fs)
    hooked.integrate_forcing = lambda *a: calls.append(("hook",) + a) or dict(stats)
    sim.method = hooked
    assert soil._advance_trbdf2(sim, 3.0) == 3.0
    assert calls[-1] == ("hook", "model", "Y", "Ya", 2.0, 3.0, 0.5, "cols") and it.trbdf2_stats["accepted"] == 6
