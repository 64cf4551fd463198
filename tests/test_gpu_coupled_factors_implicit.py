"""lh_step_coupled_factors_implicit / CoupledFactorsImplicitEuler / CoupledFactorsTRBDF2: implicit steps of the coupled
water and heat model with the IceImpedance factor on the device, checked through the library's
own tendency (lh_rhs of the same context), against lh_step_factors_implicit_euler on the Richards twin, against
lh_step_coupled_implicit where the factor is trivially 1, and against the NumPy reference
(tests/coupled_factors_implicit_ref.py over tests/coupled_implicit_ref.py).  The bounds are
tests/test_gpu_coupled_implicit.py's, restated."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import coupled_factors_implicit_ref as CF
import parity_cases as pc

CR = CF.CR
pytestmark = pytest.mark.gpu
STATUS_NONFINITE, STATUS_UNCONVERGED = 1, 8
METHODS, DTYPES, TOL, VL_BOUND = CF.METHODS, list(CF.DTYPES), CF.TOL, CF.VL_BOUND
NEW, PLAIN = "lh_step_coupled_factors_implicit", "lh_step_coupled_implicit"


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def flags_of(F, method):
    return F.LH_COUPLED_TRBDF2 if method == "trbdf2" else 0


def stats(gm):
    mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
    gm.F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
    gm.F.check(gm.L.lh_implicit_iterations(gm.ctx, C.byref(tot)), gm.ctx)
    return mi.value, un.value, tot.value


def device_steps(case, dt, nsteps, method="euler", bcv=None, tol=0.0, max_iter=0, math_mode=None, call=NEW):
    """(vl, rhoe, max iterations, unconverged, status) after one call of nsteps."""
    with pc.GpuModel(case, math_mode) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        b = None if bcv is None else np.ascontiguousarray(bcv, dtype=np.float64)
        F.check(getattr(gm.L, call)(gm.ctx, Y, Ya, 0.0, dt, nsteps, flags_of(F, method), ptr(b), tol, max_iter), gm.ctx)
        mi, un, _ = stats(gm)
        return (gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT), mi, un, gm.status())


def lh_rhs_of(case, vl, rhoe):
    """(d vl, d rhoe) = lh_rhs on the same context (the factor on) at (vl, rhoe), Float64 arrays of FT values."""
    c1 = dataclasses.replace(case, vl=np.ascontiguousarray(vl, dtype=case.dtype),
                             rhoe=np.ascontiguousarray(rhoe, dtype=case.dtype))
    with pc.GpuModel(c1) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        t = gm.tendencies(dY)
        return t["vl"].astype(np.float64), t["rhoe"].astype(np.float64)


# ------------------------------------------------------------------ 1. the residual through the tendency

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", CF.RESIDUAL_CASES)
def test_residual_through_the_tendency_of_the_same_context(which, dtype):
    """One backward-Euler step at 10x and 100x the stable step, R = Y1 - Yn - dt lh_rhs(Y1) with the factor on: the five
    boundary pairs with ice up to 0.04 and up to 0.15, and per-column parameters.  Water and energy rules of
    tests/test_gpu_coupled_implicit.py::test_residual_through_the_tendency; every column converged, status 0."""
    tol, eps = TOL[np.dtype(dtype)], float(np.finfo(dtype).eps)
    for label, kinds, case in [CF.residual_case(which, dtype)]:
        assert case.om.cf.impedance_kind == 1 and case.om.cf.viscosity_kind == 0
        vl0, ti, re0 = CR.f64(case)
        sd = CR.stable_dt(case)
        for mult in (10.0, 100.0):
            dt = mult * sd
            v1, e1, mi, un, st = device_steps(case, dt, 1)
            assert un == 0 and st == 0, (label, kinds, mult, mi, un, st)
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
            print(f"residual {label} {kinds} {np.dtype(dtype).name} {mult}x: iterations {mi}, water {rw.max():.3g} "
                  f"(bound {bound.min():.3g}), energy device {r_dev:.3g} reference {r_ref:.3g} floor {floor:.3g}")
            assert np.all(rw <= bound), (label, kinds, mult, float(np.max(rw / bound)))
            assert r_dev <= max(4 * r_ref, floor), (label, kinds, mult, r_dev, r_ref, floor)
            assert np.max(np.abs(v1 - case.vl)) > 0 and np.max(np.abs(e1 - case.rhoe)) > 0


# ------------------------------------------------------------------ 2. the water stage is the Richards factors call's

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kinds", [CR.KINDS[1], CR.KINDS[2]])
def test_the_water_stage_is_lh_step_factors_implicit_euler(kinds, dtype):
    """vartheta_l after 2 coupled backward-Euler steps at 30x is bitwise lh_step_factors_implicit_euler's on the
    Richards twin (same hydrology, ice and factor), with equal Newton statistics; 600 columns: more than one workgroup."""
    case = CF.factors_case(*kinds, dtype=dtype, ncols=600)
    twin = CF.factors_case(*kinds, dtype=dtype, ncols=600, model=M.MODEL_RICHARDS)
    np.testing.assert_array_equal(twin.vl, case.vl)
    np.testing.assert_array_equal(twin.ti, case.ti)
    assert twin.om.cf == case.om.cf
    dt = 30 * CR.stable_dt(case)
    with pc.GpuModel(case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        gm.F.check(gm.L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, 0.0, dt, 2, 0, None, 0.0, 0), gm.ctx)
        got, v1, st = stats(gm), gm.download(Y, gm.F.LH_VAR_VARTHETA_L), gm.status()
    with pc.GpuModel(twin) as gm:
        Y, Ya = gm.prognostic_and_aux()
        gm.F.check(gm.L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, dt, 2, None, 0.0, 0), gm.ctx)
        want, vr = stats(gm), gm.download(Y, gm.F.LH_VAR_VARTHETA_L)
    np.testing.assert_array_equal(v1, vr)
    assert got == want and got[1] == 0 and st == 0, (got, want, st)
    assert np.max(np.abs(v1 - case.vl)) > 0


# ------------------------------------------------------------------ 3. parity with the reference

def check_parity(name, dtype, nsteps, method):
    """tests/test_gpu_coupled_implicit.py::check_parity's rule: vartheta_l within VL_BOUND; rhoe_int within
    4 d + 64 eps ||rhoe_int||."""
    case, dt = CF.parity_case(name, dtype)
    (vr, er, info), d, scale = CF.parity_reference(name, dtype, nsteps, method)
    v1, e1, mi, un, st = device_steps(case, dt, nsteps, method)
    assert un == 0 and st == 0 and info["unconverged"] == 0, (mi, un, st, info)
    dv = float(np.max(np.abs(v1.astype(np.float64) - vr)))
    de = float(np.max(np.abs(e1.astype(np.float64) - er)))
    bound = CF.parity_bound(case, d, scale)
    print(f"parity {name} {method} {np.dtype(dtype).name} nsteps={nsteps}: vl {dv:.3g}, rhoe {de:.3g}, d {d:.3g}, "
          f"bound {bound:.3g}, ratio {de / bound:.3g}")
    assert dv <= VL_BOUND[np.dtype(dtype)], dv
    assert de <= bound, (de, d, bound)
    assert np.max(np.abs(e1 - case.rhoe)) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(CF.PARITY))
def test_parity_with_the_cpu_reference(name, method, dtype):
    """At 30x the stable step, both methods: 3 steps with a Dirichlet top over free drainage and over a Dirichlet
    bottom; ncols in {1, 67, 130} x nlev in {1, 2, 3, 16} with 1 and 5 steps; a Dirichlet energy face at the bottom."""
    for nsteps in CF.PARITY[name]["nsteps"]:
        check_parity(name, dtype, nsteps, method)


# ------------------------------------------------------------------ 4. the trivial factor

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_a_zero_ice_plane_is_the_plain_call(method, dtype):
    """With an all-zero theta_i plane the impedance is 1: both planes within the parity bound of lh_step_coupled_implicit
    on the same context with the factor off (3 steps at 30x)."""
    case = CF.factors_case(*CR.KINDS[1], dtype=dtype, zero_ice=True)
    plain = CF.factors_case(*CR.KINDS[1], dtype=dtype, zero_ice=True, impedance=False)
    assert not case.ti.any() and plain.om.cf.impedance_kind == 0
    dt = 30 * CR.stable_dt(plain)
    _, d, scale = CF.references(plain, dt, 3, method)
    v1, e1, mi, un, st = device_steps(case, dt, 3, method)
    v0, e0, m0, u0, s0 = device_steps(plain, dt, 3, method, call=PLAIN)
    assert (un, st, u0, s0) == (0, 0, 0, 0)
    dv = float(np.max(np.abs(v1.astype(np.float64) - v0)))
    de = float(np.max(np.abs(e1.astype(np.float64) - e0)))
    bound = CF.parity_bound(plain, d, scale)
    print(f"trivial factor {method} {np.dtype(dtype).name}: vl {dv:.3g} (bound {VL_BOUND[np.dtype(dtype)]:.3g}), rhoe {de:.3g} "
          f"(bound {bound:.3g}), relative {de / scale:.3g}")
    assert dv <= VL_BOUND[np.dtype(dtype)] and de <= bound
    assert np.max(np.abs(e1 - case.rhoe)) > 0


# ------------------------------------------------------------------ 5. bitwise properties

@pytest.mark.parametrize("dtype", DTYPES)
def test_n_steps_are_n_calls_and_a_sub_ensemble_is_its_columns(dtype):
    case = CF.factors_case(*CR.KINDS[3], dtype=dtype, ncols=130)
    dt, n = 30 * CR.stable_dt(case), 4
    v_call, e_call, mi, un, st = device_steps(case, dt, n)
    assert un == 0 and st == 0
    with pc.GpuModel(case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        for k in range(n):
            gm.F.check(gm.L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, k * dt, dt, 1, 0, None, 0.0, 0), gm.ctx)
        v_one, e_one = gm.download(Y, gm.F.LH_VAR_VARTHETA_L), gm.download(Y, gm.F.LH_VAR_RHOE_INT)
    np.testing.assert_array_equal(v_call, v_one)
    np.testing.assert_array_equal(e_call, e_one)
    # columns 64 .. 129 on their own: another lane, another wave, the same bits (both methods)
    sub = dataclasses.replace(case, ncols=66, vl=np.ascontiguousarray(case.vl[64:]), ti=np.ascontiguousarray(case.ti[64:]),
                              rhoe=np.ascontiguousarray(case.rhoe[64:]))
    for method in METHODS:
        vf, ef, *_ = device_steps(case, dt, 2, method)
        vs, es, *_ = device_steps(sub, dt, 2, method)
        np.testing.assert_array_equal(vs, vf[64:])
        np.testing.assert_array_equal(es, ef[64:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_boundary_values_in_time(dtype):
    """A ramped Dirichlet T and vartheta_l at the top through bcv over 4 steps: backward Euler is bitwise four one-step
    calls with lh_set_bc at the sampled times t_k+1; TR-BDF2 agrees with the reference reading the same table."""
    case = CF.factors_case(*CR.KINDS[3], dtype=dtype)
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
            F.check(gm.L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, k * dt, dt, 1, 0, None, 0.0, 0), gm.ctx)
        v_one, e_one = gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT)
    np.testing.assert_array_equal(v_call, v_one)
    np.testing.assert_array_equal(e_call, e_one)
    v_const, e_const, *_ = device_steps(case, dt, n, "euler")
    assert np.max(np.abs(e_call - e_const)) > 0 and np.max(np.abs(v_call - v_const)) > 0
    (vr, er, info), d, scale = CF.references(case, dt, n, "trbdf2", bcv=bcv)
    v2, e2, mi, un, st = device_steps(case, dt, n, "trbdf2", bcv=bcv)
    assert un == 0 and st == 0 and info["unconverged"] == 0
    assert np.max(np.abs(v2.astype(np.float64) - vr)) <= VL_BOUND[np.dtype(dtype)]
    assert np.max(np.abs(e2.astype(np.float64) - er)) <= CF.parity_bound(case, d, scale)


# ------------------------------------------------------------------ 6. order

@pytest.mark.parametrize("method", METHODS)
def test_order_on_the_device(method):
    """CR.order_ratios (T = 16 stable steps in 4, 8, 16 steps against oracle SSPRK33 at sd / 8) through the new call,
    4 columns of 16 levels with the factor on: inside CR.ORDER_BANDS, Float64."""
    solve = lambda case, dt, n: device_steps(case, dt, n, method)[:2]
    ratios, errs = CR.order_ratios(method, solve, CF.order_case())
    print(method, errs, ratios)
    lo, hi = CR.ORDER_BANDS[method]
    assert all(lo <= r <= hi for rs in ratios.values() for r in rs), (errs, ratios)


# ------------------------------------------------------------------ 7. conservation

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_conservation_with_flux_faces(method, dtype):
    """Flux faces in both components, 50 steps at 30x the stable step, under the bounds of
    tests/test_gpu_coupled_implicit.py::test_conservation_with_flux_faces."""
    fe_t, fe_b, fw_t, fw_b = -2.0, 3.0, -2e-9, -5e-10
    case = CF.factors_case(M.BC_FLUX, M.BC_FLUX, dtype=dtype, energy=((M.BC_FLUX, fe_t), (M.BC_FLUX, fe_b)))
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


# ------------------------------------------------------------------ 8. refusals and statistics

def _refused(gm, Y, Ya, rc, message, dt=1.0, nsteps=1, flags=0, call=NEW):
    got = getattr(gm.L, call)(gm.ctx, Y, Ya, 0.0, dt, nsteps, flags, None, 0.0, 0)
    assert got == rc, (got, rc, message)
    assert gm.L.lh_last_error(gm.ctx).decode() == call + ": " + message, gm.L.lh_last_error(gm.ctx)
    assert stats(gm) == (0, 0, 0)   # a refused call reports zeros


def _with(case, **changes):
    c = dataclasses.replace(case, om=copy.deepcopy(case.om))
    for k, v in changes.items():
        setattr(c.om, k, v)
    return c


VISCOSITY = ("a viscosity factor other than NoEffect is not supported: the water then reads the unknown T and the stage is "
             "no longer block triangular")
NO_IMPEDANCE = ("the context has no impedance factor (lh_set_conductivity_factors); lh_step_coupled_implicit steps a model "
                "without conductivity factors")
CLASS_MAP = ("lh_step_coupled_factors_implicit is not available with soil classes (a class map is set): lh_rhs, "
             "lh_ssprk33_stage, lh_step_ssprk33, lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are")


def test_refusals_in_order():
    case = CF.factors_case(*CR.KINDS[1], ncols=67, nlev=3)
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        # a call that runs, so that the statistics block holds numbers a refusal has to zero
        F.check(L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0), gm.ctx)
        assert stats(gm)[2] >= 67
        before = gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT)
        for dt, nsteps in ((0.0, 1), (-1.0, 1), (float("nan"), 1), (float("inf"), 1), (1.0, -1)):
            _refused(gm, Y, Ya, F.LH_EINVAL, "need nsteps >= 0 and a finite dt > 0", dt, nsteps)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x2", flags=2)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x80000001", flags=0x80000001)
        assert L.lh_step_coupled_factors_implicit(None, Y, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0) == F.LH_EINVAL
        for flags in (0, F.LH_COUPLED_TRBDF2):   # nsteps == 0 does nothing
            F.check(L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, 0.0, 1.0, 0, flags, None, 0.0, 0), gm.ctx)
        lacking = gm.state(0b0011)   # a state without rhoe_int
        assert L.lh_step_coupled_factors_implicit(gm.ctx, lacking, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0) == F.LH_ESTATE
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), before[0])   # no plane touched
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before[1])
        assert gm.status() == 0
        # the plain call still refuses the factor in its old words
        _refused(gm, Y, Ya, F.LH_EMODEL, "conductivity factors other than NoEffect are not supported", call=PLAIN)
    # bad arguments come before the model; the model before everything else
    for name in ("c2_richards_f64", "heat_dirichlet_f64"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            _refused(gm, Y, Ya, gm.F.LH_EINVAL, "need nsteps >= 0 and a finite dt > 0", dt=0.0)
            _refused(gm, Y, Ya, gm.F.LH_EMODEL, "coupled models only (SoilEnergyModel + SoilHydrologyModel)")
    # every context violates what its row names and everything after it
    base = CF.factors_case(*CR.KINDS[0], ncols=64, nlev=3)
    atm_om = copy.deepcopy(base.om)
    atm_om.atmos = M.AtmosForcing()
    for k in [k for k in atm_om.bc if k[0] == M.FACE_TOP]:
        del atm_om.bc[k]
    atm = lambda cf: _with(dataclasses.replace(base, om=atm_om), cf=cf)
    for c, msg in ((atm(M.default_cf(viscosity=True, impedance=True)), VISCOSITY),
                   (atm(M.default_cf(viscosity=True)), VISCOSITY),
                   (atm(M.default_cf()), NO_IMPEDANCE),
                   (atm(M.default_cf(impedance=True)), "a prescribed-atmosphere top is not supported")):
        with pc.GpuModel(c) as gm:
            Y, Ya = gm.prognostic_and_aux()
            _refused(gm, Y, Ya, gm.F.LH_EMODEL, msg)
            np.testing.assert_array_equal(gm.download(Y, gm.F.LH_VAR_RHOE_INT), c.rhoe)
    # a class map comes after the model and before the factors
    lay = _with(base, cf=M.default_cf(viscosity=True))
    with pc.GpuModel(lay) as gm:
        classes = [(3.0, 4.0, 0.03, 3e-5, 0.40, 1e-3), (1.3, 1.0, 0.08, 1e-7, 0.48, 1e-3)]   # (n, alpha, theta_r, Ksat, nu, S_s)
        gm.set_soil_classes(classes, np.zeros(3, dtype=np.uint8), thermal=[(1.0e6, 7.0, 2700.0, 2.0, 4.0, 0.0, 0.0, 0.9)] * 2)
        Y, Ya = gm.prognostic_and_aux()
        got = gm.L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0)
        assert got == gm.F.LH_EMODEL and gm.L.lh_last_error(gm.ctx).decode() == CLASS_MAP, gm.L.lh_last_error(gm.ctx)
        assert stats(gm) == (0, 0, 0)


def test_statistics_and_the_iteration_cap():
    case = CF.factors_case(*CR.KINDS[1], ncols=130)
    sd = CR.stable_dt(case)
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        F.check(L.lh_step_coupled_factors_implicit(gm.ctx, Y, Ya, 0.0, 30 * sd, 2, F.LH_COUPLED_TRBDF2, None, 0.0, 0), gm.ctx)
        mi, un, tot = stats(gm)
        assert mi >= 1 and un == 0 and gm.status() == 0
        assert 130 * 2 * 2 <= tot <= 130 * 2 * 2 * mi   # two water stages per step
    # max_iter = 1 at 100x: no column converges (bit 3), every one keeps its first iterate and gets its energy solve
    v1, e1, mi, un, st = device_steps(case, 100 * sd, 1, "euler", max_iter=1)
    assert mi == 1 and un == 130 and (st & STATUS_UNCONVERGED) and not (st & STATUS_NONFINITE)
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1))
    assert np.max(np.abs(e1 - case.rhoe)) > 0
    v2, e2, mi, un, st = device_steps(case, 100 * sd, 3, "trbdf2", max_iter=1)
    assert un == 130 * 3 * 2 and (st & STATUS_UNCONVERGED) and np.all(np.isfinite(e2))


def test_nonfinite_result_sets_status_bit_0():
    case = CF.factors_case(*CR.KINDS[0], ncols=67, nlev=3)
    case.rhoe = case.rhoe.copy()
    case.rhoe[5, 1] = np.nan
    *_, st = device_steps(case, 100.0, 1)
    assert st & STATUS_NONFINITE


def test_libm_math_and_per_column_parameters():
    """LH_MATH_LIBM and the per-column variants solve the same equations
    (tests/test_gpu_coupled_implicit.py::test_libm_math_and_per_column_parameters' bounds).  The per-column case has a
    free-drainage top over a Dirichlet bottom: with a per-column Dirichlet TOP the reference itself, under the device's
    stopping rule and iterated to round-off alike, leaves one column-stage of TR-BDF2 unconverged at 16 levels (its
    safeguard cycles in one column), so that pair can say nothing about the device; the reference's own convergence on
    the case is asserted first."""
    for percol, kinds in ((False, CR.KINDS[3]), (True, CR.KINDS[2])):
        case = CF.factors_case(*kinds, percol=percol)
        vl0, ti, re0 = CR.f64(case)
        dt = 10 * CR.stable_dt(case)
        for method in METHODS:
            vr, er, info = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1, method)
            stopped = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1, method, tol=TOL[np.dtype(np.float64)])[2]
            assert info["unconverged"] == 0 and stopped["unconverged"] == 0, (percol, method, info, stopped)
            v1, e1, mi, un, st = device_steps(case, dt, 1, method, math_mode=1)
            assert un == 0 and st == 0, (percol, method, mi, un, st)
            assert np.max(np.abs(v1 - vr)) <= 1e-10 and np.max(np.abs(e1 - er)) <= 1e-9 * np.max(np.abs(re0))


# ------------------------------------------------------------------ 9. through Simulation

FROZEN_BELOW, THETA_I = -1.0, 0.08


def _partly_frozen(lh):
    """tests/test_gpu_coupled_implicit.py::_coupled_jl's soil, 20 levels on (-2, 0) and zero-flux faces, with the
    impedance factor and theta_i = 0.08 below 1 m; theta_l = 0.25 + 0.04 sin 3z leaves every cell's pore space nu - theta_i
    unsaturated on the way.  Returns (model, Y, Ya)."""
    FT = np.float64
    sp, vg = pc.coupled_soil()
    msp = lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s, ν_ss_gravel=0.0, ν_ss_om=0.0, ν_ss_quartz=0.92, ρc_ds=sp.rho_c_ds,
                        κ_solid=sp.kappa_solid, κ_sat_unfrozen=sp.kappa_sat_unfrozen, κ_sat_frozen=sp.kappa_sat_frozen)
    hm = lh.vanGenuchten(FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                         bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-2.0, 0.0), nelements=20), energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm, impedance_factor=lh.IceImpedance(FT)),
                         boundary_conditions=bc, soil_param_set=msp, earth_param_set=lh.EarthParameterSet())

    def ic(z, m):
        e = m.earth_param_set
        tl = 0.25 + 0.04 * np.sin(3.0 * z)
        ti = np.where(z < FROZEN_BELOW, THETA_I, 0.0)
        rho_c_s = m.soil_param_set.rho_c_ds + tl * (e.cp_l * e.rho_cloud_liq) + ti * (e.cp_i * e.rho_cloud_ice)
        return {"ϑ_l": tl, "θ_i": ti, "ρe_int": rho_c_s * ((289.0 + 5.0 * z) - e.T_0) - ti * e.rho_cloud_ice * e.LH_f0}

    Y, Ya = lh.initialize_states(model, ic, 0.0)
    return model, Y, Ya


def test_partly_frozen_column_through_simulation():
    """A partly frozen coupled column (theta_i = 0.08 below 1 m, the impedance on) with CoupledFactorsTRBDF2() at
    dt = 30 stable steps and a saveat, against SSPRK33() at half a stable step to the same tf: the difference is within
    4x the NumPy reference's own difference to that SSPRK33 run
    (tests/test_gpu_coupled_implicit.py::test_reference_coupled_model_through_simulation's rule)."""
    lh = g.load_package()
    n = 20
    model, Y0, Ya0 = _partly_frozen(lh)
    sd = lh.stable_dt(model, Y0, Ya0)
    dt, nsteps = 30 * sd, 8
    tf = nsteps * dt
    field = lambda Y, name: np.asarray(Y.get(name), dtype=np.float64).reshape(1, n)
    vl0, ti0, re0 = field(Y0, "ϑ_l"), field(Y0, "θ_i"), field(Y0, "ρe_int")
    assert ti0.max() == THETA_I and ti0.min() == 0.0

    def simulate(method, h, saveat):
        m, Y, Ya = _partly_frozen(lh)
        sim = lh.Simulation(m, method, Y_init=Y, dt=h, tspan=(0.0, tf), Ya_init=Ya, saveat=saveat)
        return sim, lh.run(sim)

    sim, sol = simulate(lh.CoupledFactorsTRBDF2(), dt, 4 * dt)
    assert sim.integrator._nsteps_done == nsteps and len(sol.t) == 3 and sol.t[-1] == tf
    assert sim.integrator.implicit_stats[1] == 0
    _, ref = simulate(lh.SSPRK33(), sd / 2, None)
    sp, vg = pc.coupled_soil()
    om = M.CaseModel(M.MODEL_COUPLED, n, -2.0, 0.0, soil=sp, vg=vg, bc=pc._flux_bcs(energy=0.0, hydrology=0.0),
                     cf=M.default_cf(impedance=True))
    vr, er, info = CR.coupled_implicit(om, vl0, ti0, re0, dt, nsteps, "trbdf2")
    assert info["unconverged"] == 0
    assert np.all(vr < sp.nu - ti0)   # no cell saturates on the way
    for name, want in (("ϑ_l", vr), ("ρe_int", er)):
        ssp = np.asarray(ref.u[-1][name], dtype=np.float64).reshape(-1)
        dev = np.asarray(sol.u[-1][name], dtype=np.float64).reshape(-1)
        assert np.all(np.isfinite(ssp))
        d_dev, d_ref = float(np.max(np.abs(dev - ssp))), float(np.max(np.abs(want.reshape(-1) - ssp)))
        print(f"Simulation CoupledFactorsTRBDF2 {name}: device - SSPRK33 {d_dev:.3g}, reference - SSPRK33 {d_ref:.3g}")
        assert d_dev <= 4 * d_ref, (name, d_dev, d_ref)
        assert np.max(np.abs(dev - np.asarray(sol.u[0][name]).reshape(-1))) > 0
    # the plain marker refuses this model in the library's words
    with pytest.raises(NotImplementedError, match="CoupledTRBDF2: conductivity factors other than NoEffect are not supported"):
        lh.Simulation(model, lh.CoupledTRBDF2(), Y_init=Y0, dt=dt, tspan=(0.0, tf), Ya_init=Ya0)
