"""lh_step_factors_implicit_euler / lh_integrate_factors_trbdf2 (FactorsImplicitEuler / FactorsTRBDF2): backward Euler
and TR-BDF2 of Richards columns with conductivity factors (TemperatureDependentViscosity, IceImpedance) on the device,
through the C ABI: checked through the library's own tendency (lh_rhs), against the NumPy reference
(tests/factors_implicit_ref.py), against the plain calls where the factors are trivial, against the closed-form
Jacobian (tests/factors_jacobian_ref.py), bit for bit where the contract says so, and in the words of its refusals.

The cases (tests/factors_implicit_cases.py): 67 columns, 2 and 16 levels, loam, ice in every other column, T hashed per
cell in [270, 295] K; what the references alone say about them is tests/test_factors_implicit_reference.py's.

The Jacobian, read off the device as tests/test_gpu_newton_jacobian.py reads it: with max_iter = 1 one call returns one
Newton update d = Y1 - Y0 from Y0, and every cell satisfies
    |r_i| <= B max_i s_i + 64 eps(FT) sum_j |J_ref,ij| max(|Y1_j|, |dt f_j|),   r = J_ref d - dt f,
with J_ref the closed-form bands, f of lh_rhs, B = C q32 and q32 from the slopes evaluated in np.float32.  C
(test_factors_implicit_reference.C_BOUND = 8) is 4 x the largest Float64 ratio q / q32 measured on an MI355X, 1.57,
rounded up to a power of two (MEASURED below); the ceiling B <= q_1pc / 10 and the three mutants are the CPU module's.  Float32 guards
against gross errors only, as there.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import factors_implicit_cases as FC
import factors_implicit_ref as FR
import factors_jacobian_ref as FJ
import implicit_ref as IR
import parity_cases as pc
from test_factors_implicit_reference import PARITY, RESIDUAL, bound, residual_bound

pytestmark = pytest.mark.gpu
STATUS_NONFINITE, STATUS_UNCONVERGED, STATUS_FAILED = 1, 8, 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
EULER, TRBDF2 = "lh_step_factors_implicit_euler", "lh_integrate_factors_trbdf2"

# worst q / q32 over the columns and the cases of a type, measured on an MI355X (each test prints its own figure).
# Float32: the state is Float32, q is round-off of the state and not of the slopes, and the round-off term judges it.
MEASURED = {"f64": 1.57, "f32": 38.1}   # (2026-10-21; every Float64 case lies between 0.84 and 1.57)


def stats_of(gm):
    mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
    gm.F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
    gm.F.check(gm.L.lh_implicit_iterations(gm.ctx, C.byref(tot)), gm.ctx)
    return mi.value, un.value, tot.value


def trbdf2_stats_of(gm):
    st = (C.c_int64 * gm.F.LH_TRBDF2_NSTATS)()
    gm.F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    return dict(zip(KEYS, list(st)))


def euler_on_device(case, dt, nsteps, tol=0.0, max_iter=0, calls=1, math_mode=None, entry=EULER):
    """(vl after the steps, max iterations, unconverged, iterations, status) of `calls` calls of nsteps each."""
    with pc.GpuModel(case, math_mode) as gm:
        Y, Ya = gm.prognostic_and_aux()
        for _ in range(calls):
            gm.F.check(getattr(gm.L, entry)(gm.ctx, Y, Ya, 0.0, dt, nsteps, None, tol, max_iter), gm.ctx)
        return (gm.download(Y, gm.F.LH_VAR_VARTHETA_L),) + stats_of(gm) + (gm.status(),)


def trbdf2_on_device(case, t0, t1, dt, abstol=0.0, reltol=0.0, fixed=False, h0=None):
    """(vl at t1, stats dict, status, dt_cols after the call) of one lh_integrate_factors_trbdf2 call."""
    import torch
    with pc.GpuModel(case) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        ft = torch.float64 if case.dtype == np.float64 else torch.float32
        cols = torch.zeros(case.ncols, dtype=ft, device="cuda")
        if h0 is not None:
            cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
        torch.cuda.synchronize()
        F.check(gm.L.lh_integrate_factors_trbdf2(gm.ctx, Y, Ya, t0, t1, dt, abstol, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                                                 C.c_void_p(cols.data_ptr()), None), gm.ctx)
        st = trbdf2_stats_of(gm)
        vl = gm.download(Y, F.LH_VAR_VARTHETA_L)
        return vl, st, gm.status(), cols.cpu().numpy().astype(np.float64)


def device_tendency(case, vl):
    """lh_rhs of the case's context at the water state vl (Float64)"""
    with pc.GpuModel(dataclasses.replace(case, vl=np.ascontiguousarray(vl))) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        return gm.tendencies(dY)["vl"].astype(np.float64)


def columns(case, idx):
    idx = np.asarray(idx)
    return dataclasses.replace(case, ncols=len(idx), vl=np.ascontiguousarray(case.vl[idx]), ti=np.ascontiguousarray(case.ti[idx]),
                               T_aux=np.ascontiguousarray(case.T_aux[idx]))


# ------------------------------------------------------------------ residual through the tendency

@pytest.mark.parametrize("spec", RESIDUAL, ids=FC.IDS(RESIDUAL))
def test_residual_through_the_tendency(spec):
    """v1 - v0 - dt f(v1) with f = lh_rhs of the same context lies within 10 tol nu (1 + 4 dt / stable_dt) plus the
    suite's round_off term (64 eps(FT) times the largest of |v|, |dt f| of the column), in every column."""
    case, dt = FC.general(spec)
    tol = 1e-10 if spec.dtype == "f64" else 1e-5
    v1, mi, un, tot, status = euler_on_device(case, dt, 1)
    assert un == 0 and status == 0, (mi, un, status)
    assert np.all(np.isfinite(v1))
    f = device_tendency(case, v1)
    res = np.max(np.abs(v1 - case.vl - case.dtype(dt) * f.astype(case.dtype)), axis=1)
    round_off = 64 * np.finfo(case.dtype).eps * np.maximum(np.abs(v1).max(axis=1), dt * np.abs(f).max(axis=1))
    allowed = residual_bound(case, tol, spec.mult) + round_off
    print("factors residual %s: iterations <= %d, worst residual / bound %.3g" % (spec.id, mi, float(np.max(res / allowed))))
    assert np.all(res <= allowed), (float(np.max(res / allowed)), mi, np.flatnonzero(res > allowed).tolist())
    assert np.max(np.abs(v1 - case.vl)) > 0


def test_residual_with_per_column_parameters_and_libm_math():
    """Per-column parameter arrays and LH_MATH_LIBM are served as the plain calls serve them."""
    case, dt = FC.general(FC.Spec("f64", 16, FC.KINDS[3], "both", 10.0))
    c = np.arange(FC.NCOLS)
    om = dataclasses.replace(case.om, percol=dict(vg_n=1.4 + 0.4 * pc.uhash(c, 2, 16), vg_Ksat=case.om.vg.Ksat * (0.5 + pc.uhash(c, 4, 16)),
                                                  nu=0.42 + 0.05 * pc.uhash(c, 6, 16)))
    percol = dataclasses.replace(case, om=om)
    vl, ti, T = FC.f64(percol)
    dtp = 10 * pc.O.stable_dt(om, vl, ti, None, 0.5, T)
    for cs, step, mm in ((percol, dtp, None), (case, dt, 1), (percol, dtp, 1)):
        v1, mi, un, tot, status = euler_on_device(cs, step, 1, math_mode=mm)
        assert un == 0 and status == 0, (mm, mi, un, status)
        with pc.GpuModel(dataclasses.replace(cs, vl=v1), mm) as gm:
            Y, Ya = gm.prognostic_and_aux()
            dY = gm.state(0)
            gm.rhs(Y, Ya, dY)
            f = gm.tendencies(dY)["vl"]
        res = np.max(np.abs(v1 - cs.vl - step * f))
        assert res <= residual_bound(cs, 1e-10, 10.0) + 64 * np.finfo(np.float64).eps * 0.5, (mm, float(res))


# ------------------------------------------------------------------ parity with the NumPy reference

@pytest.mark.parametrize("spec", PARITY, ids=FC.IDS(PARITY))
def test_parity_with_the_cpu_reference(spec):
    """Three backward-Euler steps and three fixed TR-BDF2 steps at 10x the stable step against
    tests/factors_implicit_ref.py: 1e-10 in Float64, 2e-5 in Float32 (the suite's bounds for the same comparison
    without factors).  Measured on an MI355X (worst over the four cases): backward Euler 1.1e-16 (Float64) and 4.1e-8
    (Float32), TR-BDF2 3.9e-11 (Float64) and 8.1e-8 (Float32)."""
    case, dt = FC.general(spec)
    vl, ti, T = FC.f64(case)
    bnd = 1e-10 if spec.dtype == "f64" else 2e-5
    v1, mi, un, tot, status = euler_on_device(case, dt, 3)
    assert un == 0 and status == 0
    want, _, _ = FR.implicit_euler(case.om, vl, ti, T, dt, 3)
    e1 = float(np.max(np.abs(v1.astype(np.float64) - want)))
    v2, st, status, _ = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True)
    assert status == 0 and st["accepted"] == 3 * FC.NCOLS and st["rejected"] == 0 and st["unconverged"] == 0, st
    want2, _ = FR.trbdf2(case.om, vl, ti, T, 0.0, 3 * dt, dt, adaptive=False)
    e2 = float(np.max(np.abs(v2.astype(np.float64) - want2)))
    print("factors parity %s: backward Euler %.3g, TR-BDF2 %.3g" % (spec.id, e1, e2))
    assert e1 <= bnd and e2 <= bnd, (e1, e2)
    assert np.max(np.abs(want - vl)) > 1e3 * bnd   # (the steps move the state by far more than the bound)


def test_trivial_factors_reduce_to_the_plain_call():
    """Both kinds on with gamma = 0 and a zero theta_i plane: within 2e-10 of lh_step_implicit_euler on the same
    context with the factors off, each within 1e-10 of the same reference."""
    for nlev in (2, 16):
        on = FC.make_case(np.float64, nlev, FC.KINDS[1], "both", gamma=0.0, zero_ice=True)
        off = FC.make_case(np.float64, nlev, FC.KINDS[1], "none", zero_ice=True)
        vl, ti, T = FC.f64(off)
        dt = 10 * pc.O.stable_dt(off.om, vl, ti, None, 0.5, T)
        a = euler_on_device(on, dt, 3)
        b = euler_on_device(off, dt, 3, entry="lh_step_implicit_euler")
        assert a[2] == 0 and b[2] == 0 and a[4] == 0 and b[4] == 0
        want, _ = IR.implicit_euler(off.om, vl, ti, dt, 3)
        ea, eb, ab = (float(np.max(np.abs(x))) for x in (a[0] - want, b[0] - want, a[0] - b[0]))
        print("trivial factors n%d: factors call %.3g, plain call %.3g, between them %.3g" % (nlev, ea, eb, ab))
        assert ab <= 2e-10 and ea <= 1e-10 and eb <= 1e-10, (ea, eb, ab)


# ------------------------------------------------------------------ the Jacobian, read off the device

@pytest.mark.parametrize("spec", FC.JACOBIAN, ids=FC.IDS(FC.JACOBIAN))
def test_first_newton_update_satisfies_the_reference_jacobian(spec):
    p = FC.prepared(spec)
    with pc.GpuModel(p.obj) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        f = gm.tendencies(dY)["vl"].astype(np.float64)
        y0 = gm.download(Y, F.LH_VAR_VARTHETA_L).astype(np.float64)
        F.check(L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, p.dt, 1, None, 0.0, 1), gm.ctx)
        mi, un, tot = stats_of(gm)
        y1 = gm.download(Y, F.LH_VAR_VARTHETA_L).astype(np.float64)
        status = gm.status()
    np.testing.assert_array_equal(y0, p.pr.vl)
    assert np.all(np.isfinite(y1)) and np.all(np.isfinite(f))
    assert mi == 1 and tot == FC.NCOLS, (mi, tot)
    assert bool(status & STATUS_UNCONVERGED) == (un > 0) and (status & ~STATUS_UNCONVERGED) == 0, (status, un)
    d = y1 - y0
    dtf = float(spec.np_dtype(p.dt)) * f
    r, s = FJ.residual_and_scale(p.J, d, dtf)
    qdev = np.max(np.abs(r), axis=1) / np.max(s, axis=1)
    allowed = FJ.allowance(p.J, bound(p), d, y1, dtf, p.pr.eps)
    print("factors-jacobian %s: q %.3g, q32 %.3g, q/q32 %.3g, q_1pc %.3g, B %.3g, worst |r|/allowed %.3g, unconverged %d, |d|max %.3g"
          % (spec.id, qdev.max(), p.q32, qdev.max() / p.q32, p.q_1pc, bound(p), float(np.max(np.abs(r) / allowed)), un,
             float(np.max(np.abs(d)))))
    assert np.max(np.abs(d)) > 0
    bad = np.abs(r) > allowed
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist(), float(np.max(np.abs(r) / allowed)))


# ------------------------------------------------------------------ the adaptive integrator

# multiples of the stable step at which no column's E (the reference's, measured on the CPU) lies within 20 % of 1; at
# 4x of the 16-level case one column is rejected and 66 are accepted
ADAPTIVE_MULTS = {2: (1.0, 64.0), 16: (1.0, 4.0, 64.0)}


@pytest.mark.parametrize("nlev", [2, 16])
def test_one_adaptive_step_against_the_cpu_reference(nlev):
    """As tests/test_gpu_trbdf2.py's: a call that spans exactly one step.  A column the reference accepts (E <= 1)
    lands on the reference's Y_1 within 1e-5 and proposes h 0.9 E^(-1/3) within 5 %; a column the reference rejects
    is rejected (it then needs at least two accepted steps to reach t1)."""
    case, sd = FC.general(FC.Spec("f64", nlev, FC.KINDS[4], "both", 1.0))
    vl, ti, T = FC.f64(case)
    fn = FR.tendency(case.om, vl, ti, T)
    for mult in ADAPTIVE_MULTS[nlev]:
        h = mult * sd
        y1, _, e, _ = FR.attempt(case.om, vl, fn, ti, T, np.full(FC.NCOLS, h))
        E = FR.error_norm(e, vl, y1, 1e-6, 1e-3)
        assert not np.any((E > 0.8) & (E < 1.2)), (mult, E)
        acc = E <= 1.0
        v, st, status, cols = trbdf2_on_device(case, 0.0, h, h)
        assert status == 0 and st["failed"] == 0, (mult, st)
        nrej = int((~acc).sum())
        assert st["rejected"] >= nrej and st["accepted"] >= FC.NCOLS + nrej, (mult, nrej, st)
        if nrej == 0:
            assert st["rejected"] == 0 and st["accepted"] == FC.NCOLS, (mult, st)
        if acc.any():
            err = float(np.max(np.abs(v[acc] - y1[acc])))
            assert err <= 1e-5, (mult, err)
            want = h * np.clip(0.9 * E[acc] ** (-1.0 / 3.0), 0.2, 5.0)
            np.testing.assert_allclose(cols[acc], want, rtol=0.05, err_msg=f"x{mult}")
        if nrej:   # (a rejected column went on to t1 in smaller steps and proposes one)
            assert np.all(cols[~acc] > 0)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_adaptive_against_fixed(dtype):
    """An adaptive run at reltol = 1e-5 stays within 10 reltol nu of a fixed-step run at a sixteenth of its smallest
    step.  The run starts at the stable step sd, where E is below 1e-2 at this tolerance (the controller then grows
    the step; it shrinks one only above E = 0.73, reached at many times sd, and by at most 5), so sd bounds its
    smallest step from below: the fixed run steps by sd / 16.  The fixed run is the Float64 one for both types (of the
    Float32 case: its state, ice and T widened): 3200 steps in Float32 round the state 3200 times by up to
    eps(Float32) |v| / 2 = 2e-8 each, the size of the bound itself (measured: the Float32 fixed run lies 4.8e-5 from the
    Float32 adaptive one), so a Float32 fixed run is no reference for it.  Measured on an MI355X: 1.2e-5 in Float64."""
    case, sd = FC.general(FC.Spec(dtype, 16, FC.KINDS[4], "both", 1.0))
    rtol, T = 1e-5, 200 * sd
    v, st, status, cols = trbdf2_on_device(case, 0.0, T, sd, abstol=1e-8 if dtype == "f64" else 1e-6, reltol=rtol)
    assert status == 0 and st["failed"] == 0 and np.all(cols >= sd), st
    assert st["accepted"] < 200 * FC.NCOLS   # (it did grow its steps)
    wide = dataclasses.replace(case, dtype=np.float64, **dict(zip(("vl", "ti", "T_aux"), FC.f64(case))))
    ref, sf, status_f, _ = trbdf2_on_device(wide, 0.0, T, sd / 16, fixed=True)
    assert status_f == 0 and sf["unconverged"] == 0
    err = float(np.max(np.abs(v.astype(np.float64) - ref.astype(np.float64))))
    print("factors adaptive against fixed %s: %.3g (bound %.3g), %d accepted, %d rejected" % (dtype, err, 10 * rtol * case.om.soil.nu,
                                                                                          st["accepted"], st["rejected"]))
    assert err <= 10 * rtol * case.om.soil.nu, err


# ------------------------------------------------------------------ bitwise

@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_profile_equals_plane_bitwise(dtype):
    case, dt = FC.general(FC.Spec(dtype, 16, FC.KINDS[1], "both", 10.0))
    T = np.ascontiguousarray(np.broadcast_to(case.T_aux[:1], case.T_aux.shape))   # level-uniform: the first column's profile
    plane = dataclasses.replace(case, T_aux=T)
    prof = dataclasses.replace(plane, aux_profile=True)
    a, b = euler_on_device(plane, dt, 2), euler_on_device(prof, dt, 2)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:] and a[4] == 0
    assert np.max(np.abs(a[0] - euler_on_device(case, dt, 2)[0])) > 0   # (T matters)
    c, d = trbdf2_on_device(plane, 0.0, 20 * dt, dt), trbdf2_on_device(prof, 0.0, 20 * dt, dt)
    np.testing.assert_array_equal(c[0], d[0])
    np.testing.assert_array_equal(c[3], d[3])
    assert c[1] == d[1] and c[2] == d[2] == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_steps_calls_and_ensembles_bitwise(dtype):
    """One call of n steps equals n calls of one step; a column's result does not depend on which other columns are
    in the ensemble; LH_TRBDF2_FIXED ignores dt_cols."""
    case, dt = FC.general(FC.Spec(dtype, 16, FC.KINDS[3], "both", 10.0))
    one = euler_on_device(case, dt, 4)
    many = euler_on_device(case, dt, 1, calls=4)
    np.testing.assert_array_equal(one[0], many[0])
    idx = [3, 4, 20, 63, 64, 66]
    sub = euler_on_device(columns(case, idx), dt, 4)
    np.testing.assert_array_equal(sub[0], one[0][idx])
    T = 30 * dt
    full = trbdf2_on_device(case, 0.0, T, dt)
    part = trbdf2_on_device(columns(case, idx), 0.0, T, dt)
    np.testing.assert_array_equal(part[0], full[0][idx])
    np.testing.assert_array_equal(part[3], full[3][idx])
    f0 = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True)
    f1 = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True, h0=np.linspace(0.1 * dt, 7 * dt, FC.NCOLS))
    np.testing.assert_array_equal(f0[0], f1[0])
    assert f0[1] == f1[1] and f1[1]["accepted"] == 3 * FC.NCOLS
    np.testing.assert_array_equal(f1[3], np.full(FC.NCOLS, float(case.dtype(dt))))


# ------------------------------------------------------------------ refusals

def _refused(gm, rc, code, words):
    assert rc == code, (rc, gm.L.lh_last_error(gm.ctx))
    msg = gm.L.lh_last_error(gm.ctx).decode()
    assert msg == words, msg


def _both(gm, Y, Ya, code, words):
    L = gm.L
    _refused(gm, L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), code, words.format(who=EULER, plain="lh_step_implicit_euler"))
    assert stats_of(gm) == (0, 0, 0)
    _refused(gm, L.lh_integrate_factors_trbdf2(gm.ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), code,
             words.format(who=TRBDF2, plain="lh_integrate_trbdf2"))
    assert not any(trbdf2_stats_of(gm).values())


RICHARDS_ONLY = "{who}: Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)"
CLASS_MAP = ("{who} is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, lh_step_ssprk33, "
             "lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are, and lh_step_layered_implicit_euler and "
             "lh_integrate_layered_trbdf2 step implicitly")
NO_FACTORS = ("{who}: the context has no conductivity factor other than NoEffect (lh_set_conductivity_factors); "
              "{plain} steps a model without conductivity factors")
PLAIN_REFUSES = "{who}: conductivity factors other than NoEffect are not supported"


def test_refusals_in_order_and_words():
    case, dt = FC.general(FC.Spec("f64", 16, FC.KINDS[4], "both", 10.0))
    none = FC.make_case(np.float64, 16, FC.KINDS[4], "none")
    loam = (case.om.vg.n, case.om.vg.alpha, case.om.vg.theta_r, case.om.vg.Ksat, case.om.soil.nu, case.om.soil.S_s)
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        y0 = gm.download(Y, F.LH_VAR_VARTHETA_L)
        # a call that runs, so that the statistics blocks exist and hold numbers
        F.check(L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, dt, 1, None, 0.0, 0), gm.ctx)
        F.check(L.lh_integrate_factors_trbdf2(gm.ctx, Y, Ya, 0.0, dt, dt, 0.0, 0.0, 0, None, None), gm.ctx)
        assert stats_of(gm)[2] > 0 and trbdf2_stats_of(gm)["accepted"] >= FC.NCOLS
        y1 = gm.download(Y, F.LH_VAR_VARTHETA_L)
        assert np.max(np.abs(y1 - y0)) > 0
        # 1. the plain calls' argument checks, in their words under the new names
        _refused(gm, L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, 0.0, 1, None, 0.0, 0), F.LH_EINVAL,
                 EULER + ": need nsteps >= 0 and dt > 0")
        _refused(gm, L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, 1.0, -1, None, 0.0, 0), F.LH_EINVAL,
                 EULER + ": need nsteps >= 0 and dt > 0")
        assert stats_of(gm) == (0, 0, 0)
        for args, words in (((1.0, 0.0, 1.0, 0.0, 0.0, 0), "need finite t0 <= t1"), ((0.0, 1.0, 0.0, 0.0, 0.0, 0), "need a finite dt > 0"),
                            ((0.0, 1.0, 1.0, -1.0, 0.0, 0), "tolerances must be finite and >= 0"),
                            ((0.0, 1.0, 1.0, 0.0, 0.0, 2), "unknown flags 0x2")):
            _refused(gm, L.lh_integrate_factors_trbdf2(gm.ctx, Y, Ya, *args, None, None), F.LH_EINVAL, TRBDF2 + ": " + words)
            assert not any(trbdf2_stats_of(gm).values())
        # 3. a class map (before the factors are looked at: the same words with and without them)
        gm.set_soil_classes([loam, loam], np.zeros(16, dtype=np.uint8))
        _both(gm, Y, Ya, F.LH_EMODEL, CLASS_MAP)
        gm.set_soil_classes(None)
        # 6. stepping_preamble: a Ya without T
        rc = L.lh_step_factors_implicit_euler(gm.ctx, Y, None, 0.0, 10.0, 1, None, 0.0, 0)
        assert rc != F.LH_OK and "Ya" in L.lh_last_error(gm.ctx).decode(), L.lh_last_error(gm.ctx)
        # no refused call touched a plane
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), y1)
        # ... and the plain calls still refuse this context
        _refused(gm, L.lh_step_implicit_euler(gm.ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), F.LH_EMODEL,
                 PLAIN_REFUSES.format(who="lh_step_implicit_euler"))
        _refused(gm, L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), F.LH_EMODEL,
                 PLAIN_REFUSES.format(who="lh_integrate_trbdf2"))
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), y1)
        assert gm.status() == 0
    # 4. a context whose factors are both NoEffect -- before stepping_preamble (Ya = NULL), after the class map
    with pc.GpuModel(none) as gm:
        Y, Ya = gm.prognostic_and_aux()
        _both(gm, Y, Ya, gm.F.LH_EMODEL, NO_FACTORS)
        _both(gm, Y, None, gm.F.LH_EMODEL, NO_FACTORS)
        gm.set_soil_classes([loam, loam], np.zeros(16, dtype=np.uint8))
        _both(gm, Y, Ya, gm.F.LH_EMODEL, CLASS_MAP)
    # 2. any model but Richards -- after the argument checks, before everything else
    with pc.GpuModel(pc.make_case("coupled_f64_small")) as gm:
        Y, Ya = gm.prognostic_and_aux()
        _both(gm, Y, Ya, gm.F.LH_EMODEL, RICHARDS_ONLY)
        _refused(gm, gm.L.lh_step_factors_implicit_euler(gm.ctx, Y, Ya, 0.0, 0.0, 1, None, 0.0, 0), gm.F.LH_EINVAL,
                 EULER + ": need nsteps >= 0 and dt > 0")


# ------------------------------------------------------------------ the markers through Simulation

def test_markers_through_simulation():
    """A partly frozen column with a flux top and free drainage, both factors, a T profile: FactorsTRBDF2 ends within
    10 reltol nu of FactorsImplicitEuler at a step small enough that halving it changes the result by less than
    that."""
    lh = g.load_package()
    FT = np.float64
    nu, rtol = 0.45, 1e-4

    def run(method, dt):
        hm = lh.vanGenuchten(FT, n=1.56, α=3.6, Ksat=2.9e-7, θr=0.0)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-5e-8)),
                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage()))
        model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-0.5, 0.0), nelements=25, ncolumns=3),
                             energy_model=lh.PrescribedTemperatureModel(T_profile=lambda z, t: 271.0 + 20.0 * (z + 0.5)),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm,
                                                                   viscosity_factor=lh.TemperatureDependentViscosity(FT),
                                                                   impedance_factor=lh.IceImpedance(FT)),
                             boundary_conditions=bc, soil_param_set=lh.SoilParams(FT, ν=nu, S_s=1e-3),
                             earth_param_set=lh.EarthParameterSet())
        Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.22 + 0.0 * z, "θ_i": np.where(z < -0.3, 0.08, 0.0) + 0.0 * z}, 0.0)
        sim = lh.Simulation(model, method, Y_init=Y, dt=dt, tspan=(0.0, 7200.0), Ya_init=Ya, saveat=3600.0)
        sol = lh.run(sim)
        f = C.c_uint32()
        assert lh._ffi.lib().lh_get_status(model._backend().ctx, C.byref(f)) == 0 and f.value == 0
        return np.asarray(sol.u[-1]["ϑ_l"], dtype=np.float64)

    a = run(lh.FactorsImplicitEuler(), 10.0)
    b = run(lh.FactorsImplicitEuler(), 5.0)
    assert np.max(np.abs(a - b)) < 10 * rtol * nu, float(np.max(np.abs(a - b)))
    c = run(lh.FactorsTRBDF2(reltol=rtol), 10.0)
    assert np.max(np.abs(c - b)) <= 10 * rtol * nu, float(np.max(np.abs(c - b)))
    assert np.max(np.abs(c - 0.22)) > 100 * rtol * nu   # (water moved)
    with pytest.raises(NotImplementedError):
        run(lh.TRBDF2(), 10.0)
