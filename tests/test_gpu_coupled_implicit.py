"""lh_step_coupled_implicit / CoupledImplicitEuler / CoupledTRBDF2: implicit steps of the coupled water and heat
model on the device, checked through the library's own tendency (lh_rhs), against lh_step_implicit_euler on the
Richards model with the same hydrology, and against the NumPy reference (tests/coupled_implicit_ref.py)."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import coupled_implicit_ref as CR
import parity_cases as pc

pytestmark = pytest.mark.gpu
STATUS_NONFINITE, STATUS_UNCONVERGED = 1, 8
METHODS = ("euler", "trbdf2")
DTYPES = [np.float64, np.float32]
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}   # the library's defaults
VL_BOUND = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 2e-5}   # the project's parity bounds on vartheta_l
WHO = "lh_step_coupled_implicit: "


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def flags_of(F, method):
    return F.LH_COUPLED_TRBDF2 if method == "trbdf2" else 0


def device_steps(case, dt, nsteps, method="euler", bcv=None, tol=0.0, max_iter=0, math_mode=None):
    """(vl, rhoe, max iterations, unconverged, status) after one call of nsteps."""
    with pc.GpuModel(case, math_mode) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        b = None if bcv is None else np.ascontiguousarray(bcv, dtype=np.float64)
        F.check(gm.L.lh_step_coupled_implicit(gm.ctx, Y, Ya, 0.0, dt, nsteps, flags_of(F, method), ptr(b), tol, max_iter),
                gm.ctx)
        mi, un = C.c_int32(), C.c_int64()
        F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
        return (gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT), mi.value, un.value, gm.status())


def lh_rhs_of(case, vl, rhoe):
    """(d vl, d rhoe) = lh_rhs on the coupled model at (vl, rhoe), Float64 arrays of FT values."""
    c1 = dataclasses.replace(case, vl=np.ascontiguousarray(vl, dtype=case.dtype),
                             rhoe=np.ascontiguousarray(rhoe, dtype=case.dtype))
    with pc.GpuModel(c1) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        t = gm.tendencies(dY)
        return t["vl"].astype(np.float64), t["rhoe"].astype(np.float64)


def build_case(kinds, variant, dtype, ncols=130, **kw):
    return CR.coupled_case(*kinds, dtype=dtype, ncols=ncols, ice=variant == "ice", percol=variant == "percol", **kw)


# ------------------------------------------------------------------ 1. the residual through the tendency

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["plain", "ice", "percol"])
@pytest.mark.parametrize("kinds", CR.KINDS)
def test_residual_through_the_tendency(kinds, variant, dtype):
    """One backward-Euler step at 10x and 100x the stable step, R = Y1 - Yn - dt lh_rhs(Y1) on the coupled model.
    Water: <= 10 tol nu (1 + 4 mult) + the round-off of evaluating R (tests/test_gpu_implicit.py's bound), every
    column converged.  Energy: <= max(4 r_ref, 8 eps ||rhoe_int||), r_ref the same residual of the reference
    solution rounded to FT (tests/test_gpu_heat_implicit.py's rule)."""
    case = build_case(kinds, variant, dtype)
    vl0, ti, re0 = CR.f64(case)
    tol, eps = TOL[np.dtype(dtype)], float(np.finfo(dtype).eps)
    sd = CR.stable_dt(case)
    for mult in (10.0, 100.0):
        dt = mult * sd
        v1, e1, mi, un, st = device_steps(case, dt, 1)
        assert un == 0 and st == 0, (mult, mi, un, st)
        assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1))

        def res(v, e):
            fv, fe = lh_rhs_of(case, v, e)
            v, e = v.astype(np.float64), e.astype(np.float64)
            big = np.maximum(np.abs(v).max(axis=1), dt * np.abs(fv).max(axis=1))
            return np.max(np.abs(v - vl0 - dt * fv), axis=1), 64 * eps * big, float(np.max(np.abs(e - re0 - dt * fe)))

        rw, round_off, r_dev = res(v1, e1)
        bound = 10 * tol * case.om.soil.nu * (1 + 4 * mult) + round_off
        vr, er, _ = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1)
        _, _, r_ref = res(vr.astype(dtype), er.astype(dtype))
        floor = 8 * eps * np.max(np.abs(re0))
        print(f"residual {kinds} {variant} {np.dtype(dtype).name} {mult}x: iterations {mi}, water {rw.max():.3g} "
              f"(bound {bound.min():.3g}), energy device {r_dev:.3g} reference {r_ref:.3g} floor {floor:.3g}")
        assert np.all(rw <= bound), (mult, float(np.max(rw / bound)))
        assert r_dev <= max(4 * r_ref, floor), (mult, r_dev, r_ref, floor)
        assert np.max(np.abs(v1 - case.vl)) > 0 and np.max(np.abs(e1 - case.rhoe)) > 0


# ------------------------------------------------------------------ 2. the water stage is backward Euler's

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["plain", "ice", "percol"])
def test_the_water_stage_is_lh_step_implicit_euler(variant, dtype):
    """vartheta_l after coupled backward-Euler steps is bitwise lh_step_implicit_euler's on the Richards model
    with the same hydrology, parameters, ice and hydrology BCs: newton_stage runs on the same closures."""
    for kinds in (CR.KINDS[1], CR.KINDS[2]):
        case = build_case(kinds, variant, dtype, ncols=600)   # (more than one workgroup, a ragged last wave)
        twin = build_case(kinds, variant, dtype, ncols=600, model=M.MODEL_RICHARDS)
        np.testing.assert_array_equal(twin.vl, case.vl)
        dt = 30 * CR.stable_dt(case)
        v1, e1, mi, un, st = device_steps(case, dt, 2)
        with pc.GpuModel(twin) as gm:
            Y, Ya = gm.prognostic_and_aux()
            gm.F.check(gm.L.lh_step_implicit_euler(gm.ctx, Y, Ya, 0.0, dt, 2, None, 0.0, 0), gm.ctx)
            mr, ur = C.c_int32(), C.c_int64()
            gm.F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mr), C.byref(ur)), gm.ctx)
            vr = gm.download(Y, gm.F.LH_VAR_VARTHETA_L)
        np.testing.assert_array_equal(v1, vr)
        assert (mi, un) == (mr.value, ur.value) and un == 0 and st == 0
        assert np.max(np.abs(v1 - case.vl)) > 0


# ------------------------------------------------------------------ 3, 4. parity with the reference

_REFERENCES = {}   # computed once per (case, columns, step, method, table), shared, never modified


def _references(case, dt, nsteps, method, cols, bcv):
    """(the reference iterated to round-off, d, ||rhoe_int||): d is what the device's stopping rule alone costs
    (Float64) or what storing the state in Float32 alone costs."""
    key = (case.name, np.dtype(case.dtype).name, case.ncols, case.om.nlev, repr(sorted(case.om.bc.items())),
           (cols.start, cols.stop, cols.step), float(dt), nsteps, method, None if bcv is None else bcv.tobytes())
    if key not in _REFERENCES:
        vl, ti, re = (a[cols] for a in CR.f64(case))
        run = lambda **kw: CR.coupled_implicit(case.om, vl, ti, re, dt, nsteps, method, bcv=bcv, **kw)
        exact = run()
        other = run(tol=TOL[np.dtype(np.float64)]) if case.dtype == np.float64 else run(round_to=np.float32)
        _REFERENCES[key] = (exact, float(np.max(np.abs(other[1] - exact[1]))), float(np.max(np.abs(re))))
    return _REFERENCES[key]


def check_parity(case, dt, nsteps, method, cols=slice(None), bcv=None, label=""):
    """vartheta_l within the project's bound; rhoe_int within 4 d + 64 eps ||rhoe_int||, d = d_ref (Float64: the
    reference stopped by the device's Newton rule against the reference iterated to round-off) or d32 (Float32:
    the reference on the Float32 inputs against itself with every stage output rounded to Float32)."""
    (vr, er, info), d, scale = _references(case, dt, nsteps, method, cols, bcv)
    v1, e1, mi, un, st = device_steps(case, dt, nsteps, method, bcv=bcv)
    assert un == 0 and st == 0 and info["unconverged"] == 0, (mi, un, st, info)
    eps = float(np.finfo(case.dtype).eps)
    dv = float(np.max(np.abs(v1[cols].astype(np.float64) - vr)))
    de = float(np.max(np.abs(e1[cols].astype(np.float64) - er)))
    bound = 4 * d + 64 * eps * scale
    print(f"parity {label} {method} {np.dtype(case.dtype).name} ncols={case.ncols} nlev={case.om.nlev} nsteps={nsteps}: "
          f"vl {dv:.3g}, rhoe {de:.3g}, d {d:.3g}, bound {bound:.3g}, ratio {de / bound:.3g}")
    assert dv <= VL_BOUND[np.dtype(case.dtype)], dv
    assert de <= bound, (de, d, bound)
    return v1, e1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_parity_with_the_cpu_reference(method, dtype):
    """3 steps at 30x the stable step, ice, Dirichlet top / free-drainage bottom, columns 0::9 of 128."""
    case = build_case((M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), "ice", dtype, ncols=128)
    v1, e1 = check_parity(case, 30 * CR.stable_dt(case), 3, method, cols=slice(0, 128, 9), label="ensemble")
    assert np.max(np.abs(e1 - case.rhoe)) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 64])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_parity_shapes(ncols, nlev, method, dtype):
    """A ragged last wave (67, 130 columns), both faces on one cell, no interior face, one interior cell; one
    and five steps at 30x the stable step."""
    case = build_case((M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), "ice", dtype, ncols=ncols, nlev=nlev)
    dt = 30 * CR.stable_dt(case)
    for nsteps in (1, 5):
        check_parity(case, dt, nsteps, method, label="shapes")


ENERGY_BOTTOM_DIRICHLET = {"dirichlet_dirichlet": ((M.BC_DIRICHLET, 276.0), (M.BC_DIRICHLET, 288.0)),
                           "flux_dirichlet": ((M.BC_FLUX, -2.0), (M.BC_DIRICHLET, 288.0))}   # (top, bottom)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("energy", sorted(ENERGY_BOTTOM_DIRICHLET))
def test_dirichlet_energy_at_the_bottom(energy, dtype):
    """The bottom face's conductance G_b (in the pivot of cell 0, in the right-hand side and in the tendency
    sweep of TR-BDF2): a Dirichlet T at the bottom, with a Dirichlet or a flux top, free-drainage and Dirichlet
    water below it; test 1's energy residual rule for one backward-Euler step at 100x, test 3's parity bounds for
    3 steps of both methods at 30x."""
    for kinds in (CR.KINDS[1], CR.KINDS[2]):
        case = build_case(kinds, "ice", dtype, ncols=67, energy=ENERGY_BOTTOM_DIRICHLET[energy])
        vl0, ti, re0 = CR.f64(case)
        sd, eps = CR.stable_dt(case), float(np.finfo(dtype).eps)
        dt = 100 * sd
        v1, e1, mi, un, st = device_steps(case, dt, 1)
        assert un == 0 and st == 0
        vr, er, _ = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1)
        res = lambda v, e: float(np.max(np.abs(e.astype(np.float64) - re0 - dt * lh_rhs_of(case, v, e)[1])))
        r_dev, r_ref, floor = res(v1, e1), res(vr.astype(dtype), er.astype(dtype)), 8 * eps * np.max(np.abs(re0))
        print(f"bottom Dirichlet {energy} {kinds} {np.dtype(dtype).name}: energy residual device {r_dev:.3g} "
              f"reference {r_ref:.3g} floor {floor:.3g}")
        assert r_dev <= max(4 * r_ref, floor), (r_dev, r_ref, floor)
        for method in METHODS:
            check_parity(case, 30 * sd, 3, method, label="bottom " + energy)


# ------------------------------------------------------------------ 5. conservation

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_conservation_with_flux_faces(method, dtype):
    """Flux faces in both components, ice, 50 steps at 30x the stable step: sum_i rhoe_int changes by
    nsteps dt (F_b - F_t) / dz to nlev 4 eps sum |rhoe_int| (DESIGN section 4.15's bound), sum_i vartheta_l by the
    same expression to nlev (4 eps sum |vartheta_l| + tol nu); both expected changes are non-zero."""
    fe_t, fe_b, fw_t, fw_b = -2.0, 3.0, -2e-9, -5e-10
    case = CR.coupled_case(M.BC_FLUX, M.BC_FLUX, dtype=dtype, ncols=67, ice=True,
                           energy=((M.BC_FLUX, fe_t), (M.BC_FLUX, fe_b)))
    case.om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (M.BC_FLUX, fw_b)
    nsteps, dt = 50, 30 * CR.stable_dt(case)
    n, eps, tol = case.om.nlev, float(np.finfo(dtype).eps), TOL[np.dtype(dtype)]
    v1, e1, mi, un, st = device_steps(case, dt, nsteps, method)
    assert un == 0 and st == 0
    vl0, ti, re0 = CR.f64(case)
    for name, got, was, fb, ft, extra in (("rhoe", e1, re0, fe_b, fe_t, 0.0), ("vl", v1, vl0, fw_b, fw_t, tol * case.om.soil.nu)):
        change = got.astype(np.float64).sum(axis=1) - was.sum(axis=1)
        want = nsteps * dt * (fb - ft) / CR.DZ
        allowed = n * (4 * eps * np.abs(was).sum(axis=1) + extra)
        print(f"conservation {name} {method} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} "
              f"of the bound, expected change {want:.3g}")
        assert abs(want) > 0
        assert np.all(np.abs(change - want) <= allowed), (name, float(np.max(np.abs(change - want) / allowed)))


# ------------------------------------------------------------------ 6. order

@pytest.mark.parametrize("method", METHODS)
def test_order_on_the_device(method):
    """The CPU order test's case, steps and reference (oracle SSPRK33 at sd / 8), the device in place of the
    NumPy solver: the same bands, Float64."""
    solve = lambda case, dt, n: device_steps(case, dt, n, method)[:2]
    ratios, errs = CR.order_ratios(method, solve)
    print(method, errs, ratios)
    lo, hi = CR.ORDER_BANDS[method]
    assert all(lo <= r <= hi for rs in ratios.values() for r in rs), (errs, ratios)


# ------------------------------------------------------------------ 7. boundary values in time

@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_values_in_time(dtype):
    """A ramped Dirichlet T and vartheta_l at the top through bcv over 4 steps: backward Euler is bitwise four
    one-step calls with lh_set_bc at the sampled times t_k+1; TR-BDF2 agrees with the reference reading the same
    table."""
    case = build_case((M.BC_DIRICHLET, M.BC_DIRICHLET), "ice", dtype, ncols=67)
    n, dt = 4, 30 * CR.stable_dt(case)
    bcv = np.zeros((n + 1, 2, 2))
    for (f, c), (kind, v) in case.om.bc.items():
        bcv[:, f, c] = v
    T_top = lambda k: 276.0 + 1.5 * k
    vl_top = lambda k: 0.34 - 0.02 * k
    bcv[:, M.FACE_TOP, M.COMP_ENERGY] = [T_top(k) for k in range(n + 1)]
    bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = [vl_top(k) for k in range(n + 1)]
    v_call, e_call, mi, un, st = device_steps(case, dt, n, "euler", bcv=bcv)
    assert un == 0 and st == 0
    with pc.GpuModel(case) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        for k in range(n):
            F.check(gm.L.lh_set_bc(gm.ctx, M.FACE_TOP, M.COMP_ENERGY, M.BC_DIRICHLET, T_top(k + 1), None), gm.ctx)
            F.check(gm.L.lh_set_bc(gm.ctx, M.FACE_TOP, M.COMP_HYDROLOGY, M.BC_DIRICHLET, vl_top(k + 1), None), gm.ctx)
            F.check(gm.L.lh_step_coupled_implicit(gm.ctx, Y, Ya, k * dt, dt, 1, 0, None, 0.0, 0), gm.ctx)
        v_one, e_one = gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT)
    np.testing.assert_array_equal(v_call, v_one)
    np.testing.assert_array_equal(e_call, e_one)
    v_const, e_const, *_ = device_steps(case, dt, n, "euler")
    assert np.max(np.abs(e_call - e_const)) > 0 and np.max(np.abs(v_call - v_const)) > 0
    check_parity(case, dt, n, "trbdf2", bcv=bcv, label="bcv")
    check_parity(case, dt, n, "euler", bcv=bcv, label="bcv")


# ------------------------------------------------------------------ 8. refusals and statistics

def _refused(gm, Y, Ya, rc, message, dt=1.0, nsteps=1, flags=0):
    got = gm.L.lh_step_coupled_implicit(gm.ctx, Y, Ya, 0.0, dt, nsteps, flags, None, 0.0, 0)
    assert got == rc, (got, rc, message)
    assert gm.L.lh_last_error(gm.ctx).decode() == WHO + message, gm.L.lh_last_error(gm.ctx)


def test_refusals_in_order():
    case = build_case(CR.KINDS[1], "ice", np.float64, ncols=67, nlev=3)
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        for dt, nsteps in ((0.0, 1), (-1.0, 1), (float("nan"), 1), (float("inf"), 1), (1.0, -1)):
            _refused(gm, Y, Ya, F.LH_EINVAL, "need nsteps >= 0 and a finite dt > 0", dt, nsteps)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x2", flags=2)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x80000001", flags=0x80000001)
        assert L.lh_step_coupled_implicit(None, Y, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0) == F.LH_EINVAL
        # nsteps == 0 does nothing
        for flags in (0, F.LH_COUPLED_TRBDF2):
            F.check(L.lh_step_coupled_implicit(gm.ctx, Y, Ya, 0.0, 1.0, 0, flags, None, 0.0, 0), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), case.vl)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), case.rhoe)
        lacking = gm.state(0b0011)   # a state without rhoe_int
        assert L.lh_step_coupled_implicit(gm.ctx, lacking, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0) == F.LH_ESTATE
        assert gm.status() == 0
    # bad arguments come before the model
    for name in ("c2_richards_f64", "heat_dirichlet_f64"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            _refused(gm, Y, Ya, gm.F.LH_EINVAL, "need nsteps >= 0 and a finite dt > 0", dt=0.0)
            _refused(gm, Y, Ya, gm.F.LH_EMODEL, "coupled models only (SoilEnergyModel + SoilHydrologyModel)")
    # the model before the factors, the factors before the atmosphere
    fac = build_case(CR.KINDS[0], "plain", np.float64, ncols=64, nlev=3)
    fac.om = copy.deepcopy(fac.om)
    fac.om.cf = M.default_cf(viscosity=True)
    atm = build_case(CR.KINDS[0], "plain", np.float64, ncols=64, nlev=3)
    atm.om = copy.deepcopy(atm.om)
    atm.om.atmos = M.AtmosForcing()
    for k in [k for k in atm.om.bc if k[0] == M.FACE_TOP]:
        del atm.om.bc[k]
    both = dataclasses.replace(atm, om=copy.deepcopy(atm.om))
    both.om.cf = M.default_cf(impedance=True)
    for c, msg in ((fac, "conductivity factors other than NoEffect are not supported"),
                   (both, "conductivity factors other than NoEffect are not supported"),
                   (atm, "a prescribed-atmosphere top is not supported")):
        with pc.GpuModel(c) as gm:
            Y, Ya = gm.prognostic_and_aux()
            _refused(gm, Y, Ya, gm.F.LH_EMODEL, msg)
            mi, un = C.c_int32(7), C.c_int64(7)   # a refused call reports zeros
            gm.F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
            assert (mi.value, un.value) == (0, 0)


def test_statistics_and_the_iteration_cap():
    case = build_case(CR.KINDS[1], "ice", np.float64, ncols=130)
    sd = CR.stable_dt(case)
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        F.check(L.lh_step_coupled_implicit(gm.ctx, Y, Ya, 0.0, 30 * sd, 2, F.LH_COUPLED_TRBDF2, None, 0.0, 0), gm.ctx)
        mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
        F.check(L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
        F.check(L.lh_implicit_iterations(gm.ctx, C.byref(tot)), gm.ctx)
        assert mi.value >= 1 and un.value == 0 and gm.status() == 0
        assert 130 * 2 * 2 <= tot.value <= 130 * 2 * 2 * mi.value   # two water stages per step
    # max_iter = 1 at 100x: no column converges, every one keeps its first iterate and gets its energy solve
    v1, e1, mi, un, st = device_steps(case, 100 * sd, 1, "euler", max_iter=1)
    assert mi == 1 and un == 130 and (st & STATUS_UNCONVERGED) and not (st & STATUS_NONFINITE)
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1))
    assert np.max(np.abs(e1 - case.rhoe)) > 0
    v2, e2, mi, un, st = device_steps(case, 100 * sd, 3, "trbdf2", max_iter=1)
    assert un == 130 * 3 * 2 and (st & STATUS_UNCONVERGED) and np.all(np.isfinite(e2))


def test_nonfinite_result_sets_status_bit_0():
    case = build_case(CR.KINDS[0], "plain", np.float64, ncols=67, nlev=3)
    case.rhoe = case.rhoe.copy()
    case.rhoe[5, 1] = np.nan
    *_, st = device_steps(case, 100.0, 1)
    assert st & STATUS_NONFINITE


def test_libm_math_and_per_column_parameters():
    """LH_MATH_LIBM and the per-column variants solve the same equations: the residual bound of test 1."""
    for variant, mm in (("ice", 1), ("percol", 1)):
        case = build_case(CR.KINDS[3], variant, np.float64, ncols=67)
        vl0, ti, re0 = CR.f64(case)
        dt = 10 * CR.stable_dt(case)
        for method in METHODS:
            v1, e1, mi, un, st = device_steps(case, dt, 1, method, math_mode=mm)
            vr, er, _ = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1, method)
            assert un == 0 and st == 0
            assert np.max(np.abs(v1 - vr)) <= 1e-10 and np.max(np.abs(e1 - er)) <= 1e-9 * np.max(np.abs(re0))


# ------------------------------------------------------------------ 9. through Simulation

def test_host_mirror_markers_refuse_in_the_library_s_words():
    lh = g.load_package()
    FT = np.float64
    domain = lh.Column(FT, zlim=(-1.0, 0.0), nelements=10)
    flux = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                           bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    ep = lh.EarthParameterSet()
    richards = lh.SoilModel(FT, domain=domain, energy_model=lh.PrescribedTemperatureModel(),
                            hydrology_model=lh.SoilHydrologyModel(FT), boundary_conditions=flux, earth_param_set=ep)
    heat = lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(),
                        hydrology_model=lh.PrescribedHydrologyModel(lambda z, t: 0.3 + 0 * z), boundary_conditions=flux,
                        earth_param_set=ep)
    factors = lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(),
                           hydrology_model=lh.SoilHydrologyModel(FT, viscosity_factor=lh.TemperatureDependentViscosity(FT)),
                           boundary_conditions=flux, earth_param_set=ep)
    atmos = lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                         boundary_conditions=lh.SoilColumnBC(top=lh.PrescribedAtmosForcing(
                             FT, u_atm=0.34, theta_atm=299.0, z_atm=0.05, theta_scale=299.0, rho_a_sfc=1.17,
                             q_atm=0.015), bottom=flux.bottom), earth_param_set=ep)
    words = [(richards, "coupled models only (SoilEnergyModel + SoilHydrologyModel)"),
             (heat, "coupled models only (SoilEnergyModel + SoilHydrologyModel)"),
             (factors, "conductivity factors other than NoEffect are not supported"),
             (atmos, "a prescribed-atmosphere top is not supported")]
    for model, msg in words:
        for marker in (lh.CoupledImplicitEuler(), lh.CoupledTRBDF2(tol=1e-9, max_iter=20)):
            with pytest.raises(NotImplementedError, match=type(marker).__name__ + ": " + msg.replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")):
                lh.Simulation(model, marker, Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
        with pytest.raises(NotImplementedError):
            lh.step_implicit_coupled(model, object(), None)
    with pytest.raises(ValueError):
        lh.step_implicit_coupled(richards, object(), None, method="rk4")


def _coupled_jl(lh, theta_l):
    """test/SoilModel/coupled.jl:1-89: its soil, its 20 levels on (-2, 0), zero-flux faces in both components, and
    its initial temperature 289 + 5 z; theta_l(z) is the initial liquid fraction.  Returns (model, Y, Ya)."""
    FT = np.float64
    sp, vg = pc.coupled_soil()
    msp = lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s, ν_ss_gravel=0.0, ν_ss_om=0.0, ν_ss_quartz=0.92, ρc_ds=sp.rho_c_ds,
                        κ_solid=sp.kappa_solid, κ_sat_unfrozen=sp.kappa_sat_unfrozen, κ_sat_frozen=sp.kappa_sat_frozen)
    hm = lh.vanGenuchten(FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                         bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-2.0, 0.0), nelements=20), energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm), boundary_conditions=bc,
                         soil_param_set=msp, earth_param_set=lh.EarthParameterSet())

    def ic(z, m):
        e = m.earth_param_set
        tl = theta_l(z)
        rho_c_s = m.soil_param_set.rho_c_ds + tl * (e.cp_l * e.rho_cloud_liq)
        return {"ϑ_l": tl, "θ_i": 0.0 * z, "ρe_int": rho_c_s * ((289.0 + 5.0 * z) - e.T_0)}

    Y, Ya = lh.initialize_states(model, ic, 0.0)
    return model, Y, Ya


def test_reference_coupled_model_through_simulation():
    """test/SoilModel/coupled.jl's model with CoupledTRBDF2() at dt = 30 stable steps and a saveat, against
    SSPRK33() at half a stable step to the same tf: the difference is within 4x the NumPy reference's own
    difference to that SSPRK33 run, and sol.t lands on tf.

    The initial water is 0.30 + 0.05 sin 3z, which stays unsaturated to tf.  coupled.jl's own initial state
    (0.495 everywhere) saturates the bottom cells on the way to its equilibrium, where the explicit stable step
    falls from 7600 s to 40 s: SSPRK33 at half the initial stable step overflows on it (the CPU oracle too), so it
    cannot be the yardstick there -- that state runs in test_reference_coupled_equilibrium_in_twelve_steps."""
    lh = g.load_package()
    n = 20
    theta_l = lambda z: 0.30 + 0.05 * np.sin(3.0 * z)
    model, Y0, Ya0 = _coupled_jl(lh, theta_l)
    sd = lh.stable_dt(model, Y0, Ya0)
    dt, nsteps = 30 * sd, 8
    tf = nsteps * dt
    vl0 = np.asarray(Y0.get("ϑ_l"), dtype=np.float64).reshape(1, n)
    re0 = np.asarray(Y0.get("ρe_int"), dtype=np.float64).reshape(1, n)

    def simulate(method, h, saveat):
        m, Y, Ya = _coupled_jl(lh, theta_l)
        sim = lh.Simulation(m, method, Y_init=Y, dt=h, tspan=(0.0, tf), Ya_init=Ya, saveat=saveat)
        return sim, lh.run(sim)

    sim, sol = simulate(lh.CoupledTRBDF2(), dt, 4 * dt)
    assert sim.integrator._nsteps_done == nsteps and len(sol.t) == 3 and sol.t[-1] == tf
    assert sim.integrator.implicit_stats[1] == 0
    _, ref = simulate(lh.SSPRK33(), sd / 2, None)
    sp, vg = pc.coupled_soil()
    om = M.CaseModel(M.MODEL_COUPLED, n, -2.0, 0.0, soil=sp, vg=vg, bc=pc._flux_bcs(energy=0.0, hydrology=0.0))
    vr, er, info = CR.coupled_implicit(om, vl0, np.zeros((1, n)), re0, dt, nsteps, "trbdf2")
    assert info["unconverged"] == 0
    for name, want in (("ϑ_l", vr), ("ρe_int", er)):
        ssp = np.asarray(ref.u[-1][name], dtype=np.float64).reshape(-1)
        dev = np.asarray(sol.u[-1][name], dtype=np.float64).reshape(-1)
        assert np.all(np.isfinite(ssp))
        d_dev, d_ref = float(np.max(np.abs(dev - ssp))), float(np.max(np.abs(want.reshape(-1) - ssp)))
        print(f"Simulation CoupledTRBDF2 {name}: device - SSPRK33 {d_dev:.3g}, reference - SSPRK33 {d_ref:.3g}")
        assert d_dev <= 4 * d_ref, (name, d_dev, d_ref)
        assert np.max(np.abs(dev - np.asarray(sol.u[0][name]).reshape(-1))) > 0


def test_reference_coupled_equilibrium_in_twelve_steps():
    """test/SoilModel/coupled.jl:1-120 ("Variably saturated equilibrium") with its own initial state and tf = 32
    days, in 12 CoupledTRBDF2 steps of 64 h instead of 138 240 SSPRK33 steps of 20 s, and the reference's own two
    assertions, verbatim.  (The NumPy reference: 2.3e-4 and 4.4e-4 against the 1e-3 of both.)"""
    lh = g.load_package()
    tf = 60.0 * 60 * 24 * 32
    model, Y, Ya = _coupled_jl(lh, lambda z: 0.495 + 0.0 * z)
    sim = lh.Simulation(model, lh.CoupledTRBDF2(), Y_init=Y, dt=tf / 12, tspan=(0.0, tf), Ya_init=Ya, saveat=tf / 3)
    sol = lh.run(sim)
    assert sim.integrator._nsteps_done == 12 and sol.t[-1] == tf and sim.integrator.implicit_stats[1] == 0
    z = np.asarray(Ya.zc, dtype=np.float64).reshape(-1)
    vlf = np.asarray(sol.u[-1]["ϑ_l"], dtype=np.float64).reshape(-1)
    e, sp = model.earth_param_set, model.soil_param_set
    temp = e.T_0 + np.asarray(sol.u[-1]["ρe_int"], dtype=np.float64).reshape(-1) / (sp.rho_c_ds + vlf * (e.cp_l * e.rho_cloud_liq))
    zi = -0.3
    expected = np.where(z < zi, -1e-3 * (z - zi) + 0.5, 0.5 * (1 + (2.6 * np.maximum(z - zi, 0.0)) ** 2.0) ** (-0.5))
    a, b = np.sqrt(np.mean(vlf - expected) ** 2.0), np.sqrt(np.mean(temp - 284.0) ** 2.0)
    print("coupled.jl in 12 CoupledTRBDF2 steps:", a, b)
    assert a < 1e-3 and b < 1e-3                                     # coupled.jl:117-118
    f = C.c_uint32()
    assert lh._ffi.lib().lh_get_status(model._backend().ctx, C.byref(f)) == 0 and f.value == 0


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("variant", ["plain", "ice", "percol"])
@pytest.mark.parametrize("kinds", CR.KINDS)
def test_residual_through_the_tendency_ldexp_form(kinds, variant, ldexp_form):
    test_residual_through_the_tendency(kinds, variant, np.float64)


@pytest.mark.parametrize("method", METHODS)
def test_parity_with_the_cpu_reference_ldexp_form(method, ldexp_form):
    test_parity_with_the_cpu_reference(method, np.float64)
