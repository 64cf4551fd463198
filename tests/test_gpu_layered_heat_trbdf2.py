"""lh_integrate_layered_heat_trbdf2 / LayeredHeatAdaptiveTRBDF2: adaptive TR-BDF2 of a heat-only model with per-cell
soil classes on the device, against the NumPy reference (tests/layered_heat_trbdf2_ref.py), against
lh_integrate_heat_trbdf2 where every column has one class, and its host contract.  Mirrors
tests/test_gpu_heat_trbdf2.py, whose helpers and bounds it takes."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import case_model as M
import heat_implicit_ref as H
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_heat_trbdf2_ref as LT
import parity_cases as pc
from test_gpu_heat_trbdf2 import (DTYPES, IDS, MULTS, SPAN, STATUS_FAILED, bcv_of, check_against_reference,
                                  integrate_on, on_device as scalar_on_device, refused)

pytestmark = pytest.mark.gpu
NAME, SCALAR = "lh_integrate_layered_heat_trbdf2", "lh_integrate_heat_trbdf2"


def heat_gpu(lay, **kw):
    """A context with the case's classes, their thermal supplement and its class map."""
    g = pc.GpuModel(lay.case, **kw)
    g.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    return g


def on_device(lay, t0, t1, dt, **kw):
    with heat_gpu(lay) as gm:
        Y, Ya = gm.prognostic_and_aux()
        return integrate_on(gm, Y, Ya, lay.case.ncols, lay.case.dtype, t0, t1, dt, name=NAME, **kw)


def make(dtype, ncols, nlev, kind, **kw):
    if kind == "sixteen":
        return LT.sixteen_class_case(dtype, ncols, nlev, **kw)
    return LI.layered_case(dtype, ncols, nlev, kind=kind, **kw)


def check_one_attempt(lay, label):
    P = LT.problem(lay)
    y0, sd = LI.state64(lay), LI.stable_dt(lay)
    run = lambda t1, dt, **kw: on_device(lay, 0.0, t1, dt, **kw)
    c = lay.case
    for mult in MULTS:
        got, st, _ = check_against_reference(f"layered one attempt {label} {c.ncols}x{c.om.nlev} {mult} sd", c.dtype, P, y0, run,
                                             mult * sd, mult * sd)
        assert st["accepted"] + st["rejected"] >= c.ncols
    if c.om.nlev > 1:
        assert np.max(np.abs(got.astype(np.float64) - y0)) > 0


# ------------------------------------------------------------------ 1. one attempt against the reference

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 60])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_one_attempt_shapes(ncols, nlev, dtype):
    """A class per cell (5 classes, two of them organic), Dirichlet faces; one attempt of 0.25 and 1 stable step."""
    check_one_attempt(make(dtype, ncols, nlev, "cells"), "cells")


VARIANTS = {
    "horizons": ("horizons", {}),
    "sixteen": ("sixteen", {}),
    "cells_flux_flux": ("cells", dict(bc="flux")),
    "cells_dirichlet_flux": ("cells", dict(bc="mixed")),
    "cells_ice": ("cells", dict(ice=True)),
    "horizons_percol_dirichlet": ("horizons", dict(percol_bc=True)),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_one_attempt_maps_boundaries_and_ice(name, dtype):
    kind, kw = VARIANTS[name]
    check_one_attempt(make(dtype, 67, 60, kind, **kw), name)


# ------------------------------------------------------------------ 2. integration

_FINE = {}


def integration_case(bc, dtype):
    key = (bc, np.dtype(dtype).name)
    if key not in _FINE:
        lay = LI.layered_case(dtype, 8, 60, kind="horizons", bc=bc)
        P = LT.problem(lay)
        y0, sd = LI.state64(lay), LI.stable_dt(lay)
        _FINE[key] = (lay, P, y0, sd, LT.fixed_trbdf2(P, y0, 0.0, SPAN * sd, 4000))
    return _FINE[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["dirichlet", "flux"])
def test_integration_against_fine_fixed_steps(bc, dtype):
    """Three horizons, 8 x 60, over 2000 stable steps from h0 = the stable step at reltol 1e-3, 1e-4, 1e-5: the bounds of
    tests/test_gpu_heat_trbdf2.py's integration test."""
    lay, P, y0, sd, fine = integration_case(bc, dtype)
    ft = None if dtype == np.float64 else np.float32
    for reltol in (1e-3, 1e-4, 1e-5):
        yr, info = LT.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=reltol, ft=ft)
        got, st, status, cols = on_device(lay, 0.0, SPAN * sd, sd, reltol=reltol)
        assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (reltol, status, st)
        assert not info["failed"].any()
        dev = float(np.max(np.abs(got.astype(np.float64) - fine)))
        ref = float(np.max(np.abs(yr - fine)))
        per_col, want = st["accepted"] / 8.0, float(np.mean(info["accepted"]))
        print(f"layered integration {bc} {np.dtype(dtype).name} reltol {reltol}: error device {dev:.4g}, reference {ref:.4g}; "
              f"accepted per column {per_col:.2f} (reference {want:.2f}), rejected {st['rejected'] / 8.0:.2f} (reference "
              f"{np.mean(info['rejected']):.2f}), max attempts {st['max_steps']}, wave_steps {st['wave_steps']}")
        assert abs(per_col - want) <= 0.08 * want, (reltol, per_col, want)
        assert dev <= 2.0 * ref, (reltol, dev, ref)
        assert st["wave_steps"] >= st["accepted"] + st["rejected"]
        if dtype == np.float32:
            yu, iu = LT.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=reltol)
            own, steps = float(np.max(np.abs(yu - fine))), int(np.max(iu["accepted"] + iu["rejected"]))
            unit = float(np.finfo(np.float32).eps) * float(np.max(np.abs(y0)))
            print(f"  Float32 rounding: (device - unrounded reference) / (eps32 max|rhoe|) per attempted step "
                  f"{(dev - own) / unit / steps:.2f} ({steps} steps)")
            assert dev <= own + steps * unit, (reltol, dev, own, steps, unit)


# ------------------------------------------------------------------ 3. columns and lanes

def reorder(lay, order):
    case = dataclasses.replace(pc._w.reorder_columns(lay.case, order), ncols=len(order))
    return LH.LayeredHeat(case, lay.classes, lay.thermal, np.ascontiguousarray(lay.class_map[order]))


def test_permutation_subset_and_single_columns():
    """700 columns with a class per cell, ice and per-column Dirichlet values: a permutation permutes rhoe_int and
    dt_cols bitwise, a 128-column subset is its slice, a column alone is what it is in the ensemble."""
    lay = LI.layered_case(np.float64, 700, 60, kind="cells", percol_bc=True, ice=True)
    sd = LI.stable_dt(lay)
    T1 = 300 * sd
    got, st, status, cols = on_device(lay, 0.0, T1, sd)
    assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (status, st)
    order = np.random.default_rng(5).permutation(700)
    g_p, _, _, c_p = on_device(reorder(lay, order), 0.0, T1, sd)
    np.testing.assert_array_equal(g_p, got[order])
    np.testing.assert_array_equal(c_p, cols[order])
    g_s, _, _, c_s = on_device(reorder(lay, np.arange(100, 228)), 0.0, T1, sd)
    np.testing.assert_array_equal(g_s, got[100:228])
    np.testing.assert_array_equal(c_s, cols[100:228])
    for k in (0, 699):
        g1, _, _, c1 = on_device(reorder(lay, np.array([k])), 0.0, T1, sd)
        np.testing.assert_array_equal(g1[0], got[k])
        assert c1[0] == cols[k]
    assert st["wave_steps"] >= st["accepted"] + st["rejected"]
    assert len(set(cols.tolist())) > 1   # the columns did choose their own steps


# ------------------------------------------------------------------ 4. reject and restore

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_first_step_of_the_whole_span_is_rejected(dtype):
    lay, P, y0, sd, _ = integration_case("dirichlet", dtype)
    run = lambda t1, dt, **kw: on_device(lay, 0.0, t1, dt, **kw)
    got, st, cols = check_against_reference("layered h0 = span", dtype, P, y0, run, SPAN * sd, SPAN * sd)
    assert st["rejected"] >= 8 and st["accepted"] >= 8


def test_a_tolerance_float32_cannot_meet_fails_every_column():
    """Float32, both tolerances 1e-14: every column ends at the step floor (status bit 4) with nothing accepted, rhoe_int
    is bitwise the initial state and dt_cols is 0; the FT-rounded reference fails every column too (checked first)."""
    lay = LI.layered_case(np.float32, 64, 60, kind="horizons")
    P = LT.problem(lay)
    y0, sd = LI.state64(lay), LI.stable_dt(lay)
    yr, info = LT.integrate(P, y0, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14, ft=np.float32)
    assert info["failed"].all() and not info["accepted"].any() and np.array_equal(yr, y0)
    got, st, status, cols = on_device(lay, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 64 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0 and st["rejected"] >= 64
    np.testing.assert_array_equal(got, lay.case.rhoe)


# ------------------------------------------------------------------ 5. boundary values in time

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_boundary_table_is_the_null_call(dtype):
    lay = LI.layered_case(dtype, 67, 60, kind="cells", ice=True)
    sd = LI.stable_dt(lay)
    g0, st0, s0, c0 = on_device(lay, 0.0, 100 * sd, sd)
    bcv = bcv_of(lay.case)
    g1, st1, s1, c1 = on_device(lay, 0.0, 100 * sd, sd, bcv=bcv)
    bcv[:, :, M.COMP_HYDROLOGY] = [[0.3, -7.0], [1e9, 0.125]]
    g2, st2, s2, c2 = on_device(lay, 0.0, 100 * sd, sd, bcv=bcv)
    assert s0 == 0 and s1 == 0 and s2 == 0 and st0 == st1 == st2
    for a, b in ((g1, c1), (g2, c2)):
        np.testing.assert_array_equal(a, g0)
        np.testing.assert_array_equal(b, c0)


@pytest.mark.parametrize("reltol", [1e-3, 1e-4])
def test_ramped_dirichlet_top_against_the_reference(reltol):
    """The Dirichlet top ramped by 20 K over 500 stable steps through bcv: the reference reading the same table."""
    lay, P, y0, sd, _ = integration_case("dirichlet", np.float64)
    top = lay.case.om.bc[(M.FACE_TOP, M.COMP_ENERGY)][1]
    bcv = bcv_of(lay.case, {(M.FACE_TOP, M.COMP_ENERGY): top + 20.0})
    run = lambda t1, dt, **kw: on_device(lay, 0.0, t1, dt, **kw)
    got, st, _ = check_against_reference(f"layered ramp reltol {reltol}", np.float64, P, y0, run, 500 * sd, sd, bcv=bcv, reltol=reltol)
    flat, *_ = on_device(lay, 0.0, 500 * sd, sd, bcv=bcv_of(lay.case), reltol=reltol)
    assert np.max(np.abs(got - flat)) > 0


# ------------------------------------------------------------------ 6. conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conservation_with_flux_faces(dtype):
    """sum_i rhoe_int changes by (t1 - t0) (F_bottom - F_top) / dz, to nlev 4 eps sum |rhoe_int|."""
    lay = LI.layered_case(dtype, 67, 60, kind="cells", bc="flux", ice=True)
    om = lay.case.om
    fb, ft = om.bc[(M.FACE_BOTTOM, M.COMP_ENERGY)][1], om.bc[(M.FACE_TOP, M.COMP_ENERGY)][1]
    sd = LI.stable_dt(lay)
    T1 = SPAN * sd
    dz = (om.zmax - om.zmin) / om.nlev
    got, st, status, cols = on_device(lay, 0.0, T1, sd)
    assert status == 0 and st["failed"] == 0
    re = lay.case.rhoe.astype(np.float64)
    change = got.astype(np.float64).sum(axis=1) - re.sum(axis=1)
    want = T1 * (fb - ft) / dz
    allowed = om.nlev * 4 * float(np.finfo(dtype).eps) * np.abs(re).sum(axis=1)
    print(f"layered conservation {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, "
          f"expected change {want:.3g}, steps per column {st['accepted'] / 67.0:.1f}")
    assert abs(want) > 0
    assert np.all(np.abs(change - want) <= allowed), float(np.max(np.abs(change - want) / allowed))


# ------------------------------------------------------------------ 7. layered against scalar

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_uniform_map_against_the_scalar_call(dtype):
    """67 columns x 12 levels, 3 classes, every column one class: the layered call against lh_integrate_heat_trbdf2 on
    the per-class scalar contexts (the class's numbers as the context's scalars) over 300 stable steps.  As
    tests/test_gpu_layered_heat_implicit.py::test_column_uniform_map_against_the_scalar_call: bitwise equal (the
    closures are the scalar closures operation for operation and the time loop is one text)."""
    lay = LI.layered_case(dtype, 67, 12, kind="columns")
    sd = LI.stable_dt(lay)
    layered, st, status, cols = on_device(lay, 0.0, 300 * sd, sd)
    assert status == 0 and st["failed"] == 0
    scalar, scols = np.zeros_like(layered), np.zeros_like(cols)
    for idx, case in LH.per_class_cases(lay):
        got, st1, s1, c1 = scalar_on_device(case, 0.0, 300 * sd, sd)
        assert s1 == 0
        scalar[idx], scols[idx] = got, c1
    gap = np.max(np.abs(layered.astype(np.float64) - scalar))
    print(f"layered against scalar {np.dtype(dtype).name}: largest difference {gap:.3g}, bitwise equal: "
          f"{np.array_equal(layered, scalar)}, proposals equal: {np.array_equal(cols, scols)}")
    np.testing.assert_array_equal(layered, scalar)
    np.testing.assert_array_equal(cols, scols)
    assert np.max(np.abs(layered.astype(np.float64) - LI.state64(lay))) > 0


# ------------------------------------------------------------------ 8. defaults and refusals

def test_each_tolerance_defaults_on_its_own():
    lay = LI.layered_case(np.float64, 64, 60, kind="horizons")
    sd = LI.stable_dt(lay)
    T1 = 300 * sd
    ae = LT.abstol_e_default(lay.case.om)
    ref = on_device(lay, 0.0, T1, sd, abstol_e=ae, reltol=1e-3)
    for a, r in ((0.0, 1e-3), (ae, 0.0), (0.0, 0.0)):
        got = on_device(lay, 0.0, T1, sd, abstol_e=a, reltol=r)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[3], ref[3])
    tight = on_device(lay, 0.0, T1, sd, abstol_e=0.0, reltol=1e-5)
    assert np.max(np.abs(tight[0] - ref[0])) > 0 and tight[2] == 0


def test_refusals_in_order():
    """The argument checks first, then any model but the heat-only one, the states, the map: the layered call refuses a
    context without a map and names the scalar call, which then integrates it; the scalar call refuses a map."""
    lay = LI.layered_case(np.float64, 67, 3, kind="horizons")
    with heat_gpu(lay) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        _, st, status, _ = integrate_on(gm, Y, Ya, 67, np.float64, 0.0, 100.0, 10.0, name=NAME)
        assert status == 0 and st["accepted"] >= 67
        refused(gm, Y, Ya, F.LH_EINVAL, "need finite t0 <= t1", name=NAME, t0=1.0, t1=0.0)
        refused(gm, Y, Ya, F.LH_EINVAL, "need a finite dt > 0", name=NAME, dt=0.0)
        refused(gm, Y, Ya, F.LH_EINVAL, "tolerances must be finite and >= 0", name=NAME, abstol_e=-1.0)
        refused(gm, Y, Ya, F.LH_EINVAL, "tolerances must be finite and >= 0", name=NAME, reltol=float("nan"))
        refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x1", name=NAME, flags=1)
        before = gm.download(Y, F.LH_VAR_RHOE_INT)
        F.check(getattr(L, NAME)(gm.ctx, Y, Ya, 2.0, 2.0, 1.0, 0.0, 0.0, 0, None, None), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before)
        assert getattr(L, NAME)(gm.ctx, Y, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_ESTATE
        # the scalar call refuses a context with a map (the states come before the map)
        assert getattr(L, SCALAR)(gm.ctx, Y, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_ESTATE
        assert getattr(L, SCALAR)(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EMODEL
        assert L.lh_last_error(gm.ctx).decode().startswith(SCALAR + " is not available with soil classes (a class map is set)")
        assert gm.status() == 0
    # a context without a map: the layered call names the scalar call, which integrates it
    case = H.heat_case(67, 3)
    with pc.GpuModel(case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        refused(gm, Y, Ya, gm.F.LH_EINVAL, "need a finite dt > 0", name=NAME, dt=0.0)
        refused(gm, Y, Ya, gm.F.LH_EMODEL, "the context has no class map (lh_set_soil_class_map); " + SCALAR +
                " steps a model without soil classes", name=NAME)
        assert getattr(gm.L, NAME)(gm.ctx, Y, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == gm.F.LH_ESTATE
        _, st, status, _ = integrate_on(gm, Y, Ya, 67, np.float64, 0.0, 100.0, 10.0, name=SCALAR)
        assert status == 0 and st["accepted"] >= 67
    # any other model
    for name in ("coupled_f64_small", "c2_richards_f64"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            refused(gm, Y, Ya, gm.F.LH_EMODEL, "heat-only models (SoilEnergyModel + PrescribedHydrologyModel)", name=NAME)


# ------------------------------------------------------------------ 9. the host mirror

def test_host_mirror_through_simulation():
    """A three-horizon heat-only SoilModel with a diurnal sine as its Dirichlet top through
    Simulation(model, LayeredHeatAdaptiveTRBDF2(reltol=1e-4), saveat=...): bitwise the chain of direct C calls, one per
    dt interval, with the table sampled at the interval's two ends and dt_cols carried from call to call (also across
    the saveat chunks).  The scalar marker keeps refusing the layered model."""
    import torch
    lh = pc._pkg()
    FT = np.float64
    n, N = 12, 5
    lay = LI.layered_case(FT, N, n, kind="horizons")
    om = lay.case.om
    vl_row = np.ascontiguousarray(lay.case.vl[0])
    case = dataclasses.replace(lay.case, vl=np.ascontiguousarray(np.repeat(vl_row[None, :], N, axis=0)))
    lay = LH.LayeredHeat(case, lay.classes, lay.thermal, lay.class_map)
    bottom, day = 281.0, 86400.0
    top = lambda t: 287.0 + 4.0 * math.sin(2.0 * math.pi * t / day)
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(LH.THERMAL_FIELDS, t))))
                         for k, t in zip(lay.classes, lay.thermal)], lay.class_map[0].astype(np.int64))
    dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.Dirichlet(top)), bottom=lh.SoilComponentBC(energy=lh.Dirichlet(bottom)))
    kw = dict(domain=dom, boundary_conditions=bc, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet())
    model = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.PrescribedHydrologyModel(vartheta_l_profile=lambda z, t: vl_row + 0.0 * z),
                         soil_classes=sc, **kw)
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ρe_int": 1e7 + 0.0 * z}, 0.0)
    Y.soil.ρe_int = case.rhoe
    dt, total, chunk = 3600.0, 6, 3
    sim = lh.Simulation(model, lh.LayeredHeatAdaptiveTRBDF2(reltol=1e-4), Y_init=Y, dt=dt, tspan=(0.0, total * dt), Ya_init=Ya,
                        saveat=chunk * dt)
    sol = lh.run(sim)
    got = np.array(sim.integrator.u.soil.ρe_int)
    stats = sim.integrator.trbdf2_stats
    assert len(sol.t) == total // chunk + 1 and sol.t[-1] == total * dt and stats["failed"] == 0, stats
    with heat_gpu(lay) as g:
        F = g.F
        Yd, Yad = g.prognostic_and_aux()
        cols = torch.zeros(N, dtype=torch.float64, device="cuda")
        accepted = 0
        ends = []
        for c in range(total // chunk):
            T0 = ends[-1] if ends else 0.0
            ends += [T0 + (k + 1) * dt for k in range(chunk - 1)] + [total * dt if c == total // chunk - 1 else (c + 1) * chunk * dt]
        t = 0.0
        for te in ends:
            bcv = np.zeros((2, 2, 2))
            bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = bottom
            bcv[:, M.FACE_TOP, M.COMP_ENERGY] = top(t), top(te)
            F.check(getattr(g.L, NAME)(g.ctx, Yd, Yad, t, te, dt, 0.0, 1e-4, 0, C.c_void_p(cols.data_ptr()),
                                       bcv.ctypes.data_as(C.POINTER(C.c_double))), g.ctx)
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(g.L.lh_trbdf2_stats(g.ctx, st), g.ctx)
            accepted += st[0]
            t = te
        want = g.download(Yd, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    np.testing.assert_array_equal(got, want)
    assert stats["accepted"] == accepted
    assert np.max(np.abs(want - case.rhoe)) > 1e-4 * np.max(np.abs(case.rhoe))
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.Simulation(model, lh.HeatAdaptiveTRBDF2(), Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    model.close()
