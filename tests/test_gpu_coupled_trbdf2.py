"""lh_integrate_coupled_trbdf2 / CoupledAdaptiveTRBDF2: adaptive TR-BDF2 of the coupled water and heat model on the
device, every column with its own error-controlled step, against the NumPy reference
(tests/coupled_trbdf2_ref.py), oracle SSPRK33 and the boundary fluxes' budget."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import coupled_implicit_ref as CR
import coupled_trbdf2_ref as CT
import parity_cases as pc
from test_gpu_coupled_implicit import _coupled_jl

pytestmark = pytest.mark.gpu
STATUS_NONFINITE, STATUS_FAILED = 1, 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
DTYPES = [np.float64, np.float32]
ICED = (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE)
FLUX = (M.BC_FLUX, M.BC_FLUX)
WHO = "lh_integrate_coupled_trbdf2: "


def on_device(case, t0, t1, dt, abstol=0.0, abstol_e=0.0, reltol=0.0, bcv=None, h0=None, math_mode=None, flags=0):
    """(vl, rhoe at t1, stats dict, status, dt_cols after the call) of one lh_integrate_coupled_trbdf2 call."""
    import torch
    with pc.GpuModel(case, math_mode) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        ft = torch.float64 if case.dtype == np.float64 else torch.float32
        cols = torch.zeros(case.ncols, dtype=ft, device="cuda")
        if h0 is not None:
            cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
        torch.cuda.synchronize()
        p = None
        if bcv is not None:
            bcv = np.ascontiguousarray(bcv, dtype=np.float64)
            p = bcv.ctypes.data_as(C.POINTER(C.c_double))
        F.check(gm.L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags,
                                                 C.c_void_p(cols.data_ptr()), p), gm.ctx)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
        vl, rhoe = gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT)
        status = gm.status()
        return vl, rhoe, dict(zip(KEYS, list(st))), status, cols.cpu().numpy().astype(np.float64)


def build_case(kinds, dtype, ncols, ice=False, **kw):
    return CR.coupled_case(*kinds, dtype=dtype, ncols=ncols, ice=ice, **kw)


# ------------------------------------------------------------------ 1. one step against the reference

_ONE_STEP = {}   # per (dtype, step multiple, boundary table): the reference's attempts, computed once, never modified


def one_step_reference(case, h, bcv=None):
    """One step of h from the case's state by the reference: iterated to round-off (exact), stopped by the device's
    Newton rule (and, in Float32, with every stage output rounded to Float32), the error norms E of the exact one,
    and per variable d = max |other - exact|: what the device's stopping rule (and storing the state in FT) costs."""
    key = (case.name, np.dtype(case.dtype).name, case.ncols, repr(sorted(case.om.bc.items())), float(h),
           None if bcv is None else np.asarray(bcv).tobytes())
    if key not in _ONE_STEP:
        om = case.om
        v, ti, e = CR.f64(case)
        o0 = CT.TR._with_bc(om, bcv, 0.0, h, 0.0)
        fv, fe = CR.tendencies(o0, v, ti, e)
        exact = CT.attempt(om, v, e, fv, fe, ti, 0.0, h, bcv, 0.0, h)
        other = CT.attempt(om, v, e, fv, fe, ti, 0.0, h, bcv, 0.0, h, newton=CT.device_newton(),
                           round_to=None if case.dtype == np.float64 else np.float32)
        E = CT.error_norm(exact["ev"], exact["ee"], v, exact["v1"], e, exact["e1"], CT.ABSTOL, CT.abstol_e_default(om),
                          CT.RELTOL)
        d = (float(np.max(np.abs(other["v1"] - exact["v1"]))), float(np.max(np.abs(other["e1"] - exact["e1"]))))
        _ONE_STEP[key] = (exact, E, d)
    return _ONE_STEP[key]


def check_one_step(case, h, bcv=None, label=""):
    """A call that spans exactly one step.  Where the reference accepts in every column: the device accepts once per
    column, lands on the reference's Y_1 within 4 d + FLOOR eps ||Y|| per variable and proposes
    h clamp(0.9 E^(-1/3), 0.2, 5) within 5 %.  Where it rejects in every column: at least ncols rejected steps, and
    the call still reaches t1 (no failed column, at least ncols accepted steps).

    The bound has the form of check_parity's in tests/test_gpu_coupled_implicit.py: d (one_step_reference) is what
    the device's Newton rule and working in FT cost the reference itself, 4x the allowance, and FLOOR eps ||Y|| the
    rounding of two evaluations of the same formulas in FT.  The second term is needed: on these single steps the
    reference stopped by the device's rule takes the same iterations as the one iterated to round-off, so d is
    exactly 0 in Float64, a bound no second implementation meets.  FLOOR is check_parity's 64 in Float64, where d
    carries nothing (measured: vartheta_l 0 and 2.8e-17 against 5e-15, rhoe_int 1.9e-8 against 3.3e-7), and 8, the
    residual tests' figure, in Float32, where d already holds the roundings of the stage outputs (measured at 1x:
    rhoe_int 14.6 against 4 d = 7.8 plus 8 eps ||Y|| = 22)."""
    exact, E, (dv, de) = one_step_reference(case, h, bcv)
    v1, e1, st, status, cols = on_device(case, 0.0, h, h, bcv=bcv)
    assert status == 0 and st["failed"] == 0, (label, status, st)
    n = case.ncols
    eps = float(np.finfo(case.dtype).eps)
    if np.all(E <= 1.0):
        floor = 64 if case.dtype == np.float64 else 8
        bv = 4 * dv + floor * eps * float(np.max(np.abs(exact["v1"])))
        be = 4 * de + floor * eps * float(np.max(np.abs(exact["e1"])))
        gv = float(np.max(np.abs(v1.astype(np.float64) - exact["v1"])))
        ge = float(np.max(np.abs(e1.astype(np.float64) - exact["e1"])))
        want = h * CT.step_factor(E)
        print(f"one step {label} {np.dtype(case.dtype).name}: E {E.min():.3g}..{E.max():.3g}, vl {gv:.3g} (4 d = {4 * dv:.3g}, bound {bv:.3g}), "
              f"rhoe {ge:.3g} (4 d = {4 * de:.3g}, bound {be:.3g}), proposal / reference {np.min(cols / want):.4f}..{np.max(cols / want):.4f}")
        assert st["accepted"] == n and st["rejected"] == 0, (label, E, st)
        np.testing.assert_allclose(cols, want, rtol=0.05, err_msg=f"{label} E={E}")
        assert gv <= bv, (label, gv, dv, bv)
        assert ge <= be, (label, ge, de, be)
    else:
        print(f"one step {label} {np.dtype(case.dtype).name}: E {E.min():.3g}..{E.max():.3g}, {st}")
        assert np.all(E > 1.0) and st["rejected"] >= n and st["accepted"] >= n, (label, E, st)
        assert np.all(cols > 0)
    return v1, e1


@pytest.mark.parametrize("mult", [0.25, 1.0, 4.0, 16.0])
def test_one_step_against_the_cpu_reference(mult):
    """Float64, 8 columns x 64 levels, ice, Dirichlet top / free drainage: the reference measures E = 0.015 and 0.62
    at 0.25x and 1x the stable step (accepted), 11 and 56 at 4x and 16x (rejected).  check_one_step's bounds."""
    case = build_case(ICED, np.float64, 8, ice=True)
    check_one_step(case, mult * CR.stable_dt(case), label=f"{mult}x")


def test_one_step_in_float32():
    """The same step at 1x in Float32: d also holds the rounding of every stage output to Float32."""
    case = build_case(ICED, np.float32, 8, ice=True)
    check_one_step(case, CR.stable_dt(case), label="1x")


# ------------------------------------------------------------------ 2. integration

SPAN = 64.0
SUBSET = slice(0, 64, 8)   # the columns the NumPy integrator follows (columns are independent)
_INTEGRATED = {}


def integration_reference(kinds, ice, dtype, reltol):
    """(case, its stable step, the NumPy integrator's (vl, rhoe, info) on SUBSET with the device's Newton rule and,
    in Float32, everything the device keeps in a Float32 plane rounded to Float32 (coupled_trbdf2_ref.attempt's
    round_to: what working in FT costs.  In the flux case the water moves by 1e-6, 30 spacings of Float32 at 0.3, and
    the reference's error against SSPRK33 is 9.0e-8, 3.0e-8, 7.5e-9 in Float64 and 2.6e-7, 4.4e-7, 7.3e-7 in
    Float32 at the three reltols: more steps, more roundings), oracle SSPRK33 at sd / 8 on SUBSET); shared."""
    base = (kinds, ice, np.dtype(dtype).name)
    if base not in _INTEGRATED:
        case = build_case(kinds, dtype, 64, ice=ice)
        sd = CR.stable_dt(case)
        sub = dataclasses.replace(pc._w.reorder_columns(case, np.arange(64)[SUBSET]), ncols=8)
        vl, ti, re = (a.copy() for a in CR.f64(sub))
        pc.O.ssprk33(sub.om, sd / 8, int(8 * SPAN), vl, ti, re)
        _INTEGRATED[base] = (case, sub, sd, (vl, re))
    case, sub, sd, ssp = _INTEGRATED[base]
    key = base + (reltol,)
    if key not in _INTEGRATED:
        v, ti, e = CR.f64(sub)
        _INTEGRATED[key] = CT.integrate(sub.om, v, ti, e, 0.0, SPAN * sd, sd, reltol=reltol,
                                        newton=CT.device_newton(reltol=reltol),
                                        round_to=None if dtype == np.float64 else np.float32)
    return case, sd, _INTEGRATED[key], ssp


def unrounded_reference_error(kinds, ice, dtype, reltol):
    """max |vartheta_l - SSPRK33| on SUBSET of the NumPy integrator WITHOUT the Float32 roundings (the method's own
    error on the Float32 case's inputs), and the largest number of attempted steps of a column; shared."""
    case, sd, _, ssp = integration_reference(kinds, ice, dtype, reltol)
    key = (kinds, ice, np.dtype(dtype).name, reltol, "unrounded")
    if key not in _INTEGRATED:
        sub = _INTEGRATED[(kinds, ice, np.dtype(dtype).name)][1]
        v, ti, e = CR.f64(sub)
        vr, _, info = CT.integrate(sub.om, v, ti, e, 0.0, SPAN * sd, sd, reltol=reltol, newton=CT.device_newton(reltol=reltol))
        _INTEGRATED[key] = (float(np.max(np.abs(vr - ssp[0]))), int(np.max(info["accepted"] + info["rejected"])))
    return _INTEGRATED[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["iced", "flux"])
def test_integration_against_ssprk33_and_the_reference_integrator(name, dtype):
    """64 columns x 64 levels over 64 stable steps from h0 = the stable step, reltol 1e-3, 1e-4, 1e-5: status 0, no
    failed column; on columns 0::8 the error against oracle SSPRK33 at sd / 8 is within 1.5x the NumPy integrator's
    on the same columns (both variables) and, in Float64, falls with reltol; the accepted steps per column are within
    15 % of the NumPy integrator's mean count.  In Float32 the reference models the device's storage, so the device's
    vartheta_l error is also held against the method's own error (the reference without any rounding) plus one
    eps32 max |vartheta_l| per attempted step: a step forms w1, Y_g, w2, Y_1 and f_n+1 in Float32, a handful of
    roundings of half a spacing each, and one spacing per step is what they add up to when they all push one way
    (measured: 0.57 to 0.71 per step on the flux case, 0.13 to 0.23 on the iced one)."""
    kinds, ice = (ICED, True) if name == "iced" else (FLUX, False)
    last = None
    for reltol in (1e-3, 1e-4, 1e-5):
        case, sd, (vr, er, info), ssp = integration_reference(kinds, ice, dtype, reltol)
        v1, e1, st, status, cols = on_device(case, 0.0, SPAN * sd, sd, reltol=reltol)
        assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (reltol, status, st)
        assert not info["failed"].any()
        dev = [float(np.max(np.abs(a[SUBSET].astype(np.float64) - w))) for a, w in ((v1, ssp[0]), (e1, ssp[1]))]
        ref = [float(np.max(np.abs(a - w))) for a, w in ((vr, ssp[0]), (er, ssp[1]))]
        per_col, want = st["accepted"] / 64.0, float(np.mean(info["accepted"]))
        print(f"integration {name} {np.dtype(dtype).name} reltol {reltol}: errors device {dev[0]:.3g} {dev[1]:.3g}, reference "
              f"{ref[0]:.3g} {ref[1]:.3g}; accepted per column {per_col:.2f} (reference {want:.2f}), rejected "
              f"{st['rejected'] / 64.0:.2f} (reference {np.mean(info['rejected']):.2f}), Newton per stage "
              f"{st['newton_iterations'] / (2.0 * (st['accepted'] + st['rejected'])):.2f}")
        assert dev[0] <= 1.5 * ref[0] and dev[1] <= 1.5 * ref[1], (reltol, dev, ref)
        assert abs(per_col - want) <= 0.15 * want, (reltol, per_col, want)
        if dtype == np.float32:
            own, steps = unrounded_reference_error(kinds, ice, dtype, reltol)
            unit = float(np.finfo(np.float32).eps) * float(np.max(np.abs(case.vl)))
            print(f"  Float32 rounding: (device - unrounded reference) / (eps32 max|vl|) per attempted step "
                  f"{(dev[0] - own) / unit / steps:.2f} ({steps} steps)")
            assert dev[0] <= own + steps * unit, (reltol, dev[0], own, steps, unit)
        if dtype == np.float64 and last is not None:
            assert dev[0] < last[0] and dev[1] < last[1], (reltol, dev, last)
        last = dev


# ------------------------------------------------------------------ 3. shapes and independence

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nlev", [1, 2, 3, 64])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_shapes(ncols, nlev, dtype):
    """A ragged last wave, both faces on one cell, no interior face, one interior cell: 8 stable steps, every column
    reaches t1 finite with status 0, and each column is bitwise what it is in a call of its own."""
    case = build_case(ICED, dtype, ncols, ice=True, nlev=nlev)
    sd = CR.stable_dt(case)
    v1, e1, st, status, cols = on_device(case, 0.0, 8 * sd, sd)
    assert status == 0 and st["failed"] == 0 and st["accepted"] >= ncols, (status, st)
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1)) and np.all(cols > 0)
    assert np.max(np.abs(e1 - case.rhoe)) > 0
    assert st["wave_steps"] >= st["accepted"] + st["rejected"] and st["unconverged"] == 0
    k = ncols - 1
    one = dataclasses.replace(pc._w.reorder_columns(case, np.array([k])), ncols=1)
    v_k, e_k, _, _, c_k = on_device(one, 0.0, 8 * sd, sd)
    np.testing.assert_array_equal(v_k[0], v1[k])
    np.testing.assert_array_equal(e_k[0], e1[k])
    assert c_k[0] == cols[k]


def test_column_independence_with_per_column_parameters():
    """700 columns with per-column parameters and ice in every third: a permutation of the columns permutes both
    planes and dt_cols bitwise, a 128-column subset is bitwise its slice, and wave_steps (64 x each wave's largest
    step count) is at least the sum of the columns' counts."""
    case = build_case(ICED, np.float64, 700, percol=True)
    case.ti = np.where((np.arange(700) % 3 == 0)[:, None], 0.02, 0.0) * np.ones((1, case.om.nlev))
    sd = CR.stable_dt(case)
    T = 20 * sd
    v_a, e_a, st, status, cols = on_device(case, 0.0, T, sd)
    assert status == 0 and st["failed"] == 0, (status, st)
    assert np.all(np.isfinite(cols)) and np.all(cols > 0)
    order = np.random.default_rng(5).permutation(700)
    v_p, e_p, _, _, cols_p = on_device(pc._w.reorder_columns(case, order), 0.0, T, sd)
    np.testing.assert_array_equal(v_p, v_a[order])
    np.testing.assert_array_equal(e_p, e_a[order])
    np.testing.assert_array_equal(cols_p, cols[order])
    sub = dataclasses.replace(pc._w.reorder_columns(case, np.arange(100, 228)), ncols=128)
    v_s, e_s, *_ = on_device(sub, 0.0, T, sd)
    np.testing.assert_array_equal(v_s, v_a[100:228])
    np.testing.assert_array_equal(e_s, e_a[100:228])
    assert st["wave_steps"] >= st["accepted"] + st["rejected"]
    assert len(set(cols.tolist())) > 1   # the columns did choose their own steps


def test_dt_cols_carries_the_steps_across_calls():
    """Two calls over [0, T/2] and [T/2, T]: with dt_cols handed on, the second call starts from the first call's
    proposals (all above the stable step) and takes no more steps than one that starts from the stable step again,
    and another path."""
    case = build_case(ICED, np.float64, 67, ice=True)
    sd = CR.stable_dt(case)
    v1, e1, st1, status, cols = on_device(case, 0.0, 32 * sd, sd)
    assert status == 0 and np.all(cols > sd)
    mid = dataclasses.replace(case, vl=v1, rhoe=e1)
    _, _, st_carry, s1, _ = on_device(mid, 32 * sd, 64 * sd, sd, h0=cols)
    _, _, st_fresh, s2, _ = on_device(mid, 32 * sd, 64 * sd, sd)
    assert s1 == 0 and s2 == 0
    assert st_carry["accepted"] <= st_fresh["accepted"] and st_carry != st_fresh, (st_carry, st_fresh)


# ------------------------------------------------------------------ 4. failure

def test_a_tolerance_float32_cannot_meet_fails_every_column():
    """All three tolerances 1e-14 in Float32: h shrinks to the floor, every column fails (status bit 4) with nothing
    accepted, both planes are bitwise the initial state and dt_cols is 0."""
    case = build_case(FLUX, np.float32, 64)
    sd = CR.stable_dt(case)
    v, e, st, status, cols = on_device(case, 0.0, 10 * sd, sd, abstol=1e-14, abstol_e=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 64 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0 and st["rejected"] >= 64
    np.testing.assert_array_equal(v, case.vl)
    np.testing.assert_array_equal(e, case.rhoe)


def test_nonfinite_start_is_reported():
    """A NaN in rhoe_int: that column cannot accept a step (a NaN E rejects) and fails; the others finish."""
    case = build_case(FLUX, np.float64, 67, nlev=3)
    case.rhoe = case.rhoe.copy()
    case.rhoe[5, 1] = np.nan
    v, e, st, status, cols = on_device(case, 0.0, 100.0, 100.0)
    assert status & STATUS_FAILED and st["failed"] == 1 and cols[5] == 0 and np.all(np.delete(cols, 5) > 0), (status, st)
    assert np.all(np.isfinite(np.delete(e, 5, axis=0)))


# ------------------------------------------------------------------ 5. boundary values in time

def _bcv_of(case, t1_values=None):
    """[t0 | t1][face][component] from the case's scalar boundary values; t1_values: {(face, comp): value at t1}."""
    bcv = np.zeros((2, 2, 2))
    for (f, c), (kind, v) in case.om.bc.items():
        bcv[:, f, c] = v
    for (f, c), v in (t1_values or {}).items():
        bcv[1, f, c] = v
    return bcv


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_boundary_table_is_the_null_call(dtype):
    """A bcv whose two ends equal lh_set_bc's values is bitwise the bcv = NULL call."""
    case = build_case((M.BC_DIRICHLET, M.BC_DIRICHLET), dtype, 67, ice=True)
    sd = CR.stable_dt(case)
    v0, e0, st0, s0, c0 = on_device(case, 0.0, 16 * sd, sd)
    v1, e1, st1, s1, c1 = on_device(case, 0.0, 16 * sd, sd, bcv=_bcv_of(case))
    assert s0 == 0 and s1 == 0 and st0 == st1
    np.testing.assert_array_equal(v1, v0)
    np.testing.assert_array_equal(e1, e0)
    np.testing.assert_array_equal(c1, c0)


def test_ramped_dirichlet_top_against_the_reference():
    """Dirichlet T and vartheta_l at the top ramped over one step of half a stable step through bcv (the stage
    values at t + gamma h and t + h): check_one_step's bounds against the reference reading the same table, and
    another result than the constant table's."""
    case = build_case((M.BC_DIRICHLET, M.BC_DIRICHLET), np.float64, 8, ice=True)
    h = 0.5 * CR.stable_dt(case)
    bcv = _bcv_of(case, {(M.FACE_TOP, M.COMP_ENERGY): 276.5, (M.FACE_TOP, M.COMP_HYDROLOGY): 0.335})
    v1, e1 = check_one_step(case, h, bcv=bcv, label="ramp")
    v0, e0, *_ = on_device(case, 0.0, h, h, bcv=_bcv_of(case))
    assert np.max(np.abs(v1 - v0)) > 0 and np.max(np.abs(e1 - e0)) > 0


def test_dirichlet_energy_at_the_bottom():
    """A Dirichlet T at the bottom (its conductance in the pivot of cell 0, in the stage solves and in the
    homogeneous error solve), 280 K ramped to 280.5 K over half a stable step (the reference: E up to 0.36, every
    column accepts): check_one_step's bounds."""
    case = build_case(ICED, np.float64, 8, ice=True, energy=((M.BC_FLUX, -2.0), (M.BC_DIRICHLET, 280.0)))
    h = 0.5 * CR.stable_dt(case)
    bcv = _bcv_of(case, {(M.FACE_BOTTOM, M.COMP_ENERGY): 280.5})
    check_one_step(case, h, bcv=bcv, label="bottom Dirichlet")


# ------------------------------------------------------------------ 6. conservation

@pytest.mark.parametrize("dtype", DTYPES)
def test_conservation_with_flux_faces(dtype):
    """Flux faces in both components, ice, 64 stable steps at reltol 1e-3: per column sum_i rhoe_int and
    sum_i vartheta_l change by (t1 - t0) (F_b - F_t) / dz however the column chose its steps, to
    nlev 4 eps sum |rhoe_int| and nlev (4 eps sum |vartheta_l| + kappa (abstol + reltol nu)): the bound form of
    tests/test_gpu_coupled_implicit.py::test_conservation_with_flux_faces with the adaptive Newton test in the
    place of its tol nu.  Both expected changes are non-zero."""
    fe_t, fe_b, fw_t, fw_b = -2.0, 3.0, -2e-9, -5e-10
    case = CR.coupled_case(M.BC_FLUX, M.BC_FLUX, dtype=dtype, ncols=67, ice=True,
                           energy=((M.BC_FLUX, fe_t), (M.BC_FLUX, fe_b)))
    case.om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (M.BC_FLUX, fw_b)
    sd = CR.stable_dt(case)
    T = 64 * sd
    n, eps = case.om.nlev, float(np.finfo(dtype).eps)
    v1, e1, st, status, cols = on_device(case, 0.0, T, sd)
    assert status == 0 and st["failed"] == 0 and len(set(cols.tolist())) > 1, (status, st)
    vl0, ti, re0 = CR.f64(case)
    newton = CT.NEWTON_KAPPA * (CT.ABSTOL + CT.RELTOL * case.om.soil.nu)
    for name, got, was, fb, ft, extra in (("rhoe", e1, re0, fe_b, fe_t, 0.0), ("vl", v1, vl0, fw_b, fw_t, newton)):
        change = got.astype(np.float64).sum(axis=1) - was.sum(axis=1)
        want = T * (fb - ft) / CR.DZ
        allowed = n * (4 * eps * np.abs(was).sum(axis=1) + extra)
        print(f"conservation {name} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, "
              f"expected change {want:.3g}, steps per column {st['accepted'] / 67.0:.1f}")
        assert abs(want) > 0
        assert np.all(np.abs(change - want) <= allowed), (name, float(np.max(np.abs(change - want) / allowed)))


# ------------------------------------------------------------------ 7. tolerance defaults

def test_each_tolerance_defaults_on_its_own():
    """A tolerance of 0 takes its own default (abstol 1e-6, abstol_e 1e-6 rho_l c_l, reltol 1e-3), bit for bit, also
    beside tolerances that are not the defaults; the host mirror maps each None on its own."""
    case = build_case(ICED, np.float64, 64, ice=True)
    sd = CR.stable_dt(case)
    T = 16 * sd
    ae = CT.abstol_e_default(case.om)
    ref = on_device(case, 0.0, T, sd, abstol=1e-6, abstol_e=ae, reltol=1e-3)
    for a, b, r in ((0.0, ae, 1e-3), (1e-6, 0.0, 1e-3), (1e-6, ae, 0.0), (0.0, 0.0, 0.0)):
        got = on_device(case, 0.0, T, sd, abstol=a, abstol_e=b, reltol=r)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[4], ref[4])
    tight = on_device(case, 0.0, T, sd, abstol=1e-8, abstol_e=ae, reltol=1e-4)
    for a, b, r in ((1e-8, 0.0, 1e-4), ):
        got = on_device(case, 0.0, T, sd, abstol=a, abstol_e=b, reltol=r)
        np.testing.assert_array_equal(got[1], tight[1])
    assert np.max(np.abs(tight[1] - ref[1])) > 0 and tight[3] == 0
    loose_e = on_device(case, 0.0, T, sd, abstol_e=1e3 * ae)
    assert np.max(np.abs(loose_e[1] - ref[1])) > 0   # (the energy's tolerance is read)


# ------------------------------------------------------------------ 8. refusals

def _refused(gm, Y, Ya, rc, message, t0=0.0, t1=1.0, dt=1.0, abstol=0.0, abstol_e=0.0, reltol=0.0, flags=0):
    got = gm.L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, None, None)
    assert got == rc, (got, rc, message)
    assert gm.L.lh_last_error(gm.ctx).decode() == WHO + message, gm.L.lh_last_error(gm.ctx)
    st = (C.c_int64 * gm.F.LH_TRBDF2_NSTATS)(*([7] * gm.F.LH_TRBDF2_NSTATS))   # a refused call reports zeros
    gm.F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    assert list(st) == [0] * gm.F.LH_TRBDF2_NSTATS


def test_refusals_in_order():
    case = build_case(ICED, np.float64, 67, ice=True, nlev=3)
    nan, inf = float("nan"), float("inf")
    tols = "tolerances must be finite and >= 0"
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        _refused(gm, Y, Ya, F.LH_EINVAL, "need finite t0 <= t1", t0=1.0, t1=0.0)
        _refused(gm, Y, Ya, F.LH_EINVAL, "need finite t0 <= t1", t1=inf)
        for dt in (0.0, -1.0, nan, inf):
            _refused(gm, Y, Ya, F.LH_EINVAL, "need a finite dt > 0", dt=dt)
        for bad in (-1e-6, nan, inf):
            _refused(gm, Y, Ya, F.LH_EINVAL, tols, abstol=bad)
            _refused(gm, Y, Ya, F.LH_EINVAL, tols, abstol_e=bad)
            _refused(gm, Y, Ya, F.LH_EINVAL, tols, reltol=bad)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x1", flags=1)   # (fixed steps: lh_step_coupled_implicit)
        _refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x80000000", flags=0x80000000)
        assert L.lh_integrate_coupled_trbdf2(None, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
        bad_bcv = np.full(8, nan)
        assert L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None,
                                             bad_bcv.ctypes.data_as(C.POINTER(C.c_double))) == F.LH_EINVAL
        # t1 == t0 does nothing
        F.check(L.lh_integrate_coupled_trbdf2(gm.ctx, Y, Ya, 2.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0, None, None), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_VARTHETA_L), case.vl)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), case.rhoe)
        lacking = gm.state(0b0011)   # a state without rhoe_int
        assert L.lh_integrate_coupled_trbdf2(gm.ctx, lacking, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None, None) == F.LH_ESTATE
        assert gm.status() == 0
    # bad arguments come before the model
    for name in ("c2_richards_f64", "heat_dirichlet_f64"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            _refused(gm, Y, Ya, gm.F.LH_EINVAL, "need a finite dt > 0", dt=0.0)
            _refused(gm, Y, Ya, gm.F.LH_EMODEL, "coupled models only (SoilEnergyModel + SoilHydrologyModel)")
    # the model before the factors, the factors before the atmosphere
    fac = build_case(FLUX, np.float64, 64, nlev=3)
    fac.om = copy.deepcopy(fac.om)
    fac.om.cf = M.default_cf(viscosity=True)
    atm = build_case(FLUX, np.float64, 64, nlev=3)
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


def test_host_mirror_refuses_at_construction():
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
    coupled = lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                           boundary_conditions=flux, earth_param_set=ep)
    words = [(richards, "coupled models only (SoilEnergyModel + SoilHydrologyModel)"),
             (heat, "coupled models only (SoilEnergyModel + SoilHydrologyModel)"),
             (factors, "conductivity factors other than NoEffect are not supported"),
             (atmos, "a prescribed-atmosphere top is not supported")]
    esc = lambda s: s.replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")
    for model, msg in words:
        with pytest.raises(NotImplementedError, match="CoupledAdaptiveTRBDF2: " + esc(msg)):
            lh.Simulation(model, lh.CoupledAdaptiveTRBDF2(reltol=1e-4), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
        with pytest.raises(NotImplementedError, match="CoupledAdaptiveTRBDF2: " + esc(msg)):
            lh.integrate_coupled_trbdf2(model, object(), None, 0.0, 1.0, 1.0)
    with pytest.raises(NotImplementedError):   # TRBDF2() stays the Richards integrator
        lh.Simulation(coupled, lh.TRBDF2(), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)


# ------------------------------------------------------------------ 9. through Simulation

def test_reference_coupled_equilibrium_with_error_control():
    """test/SoilModel/coupled.jl:1-120 ("Variably saturated equilibrium") with its own model, initial state and
    tf = 32 days through Simulation(model, CoupledAdaptiveTRBDF2()) at the default tolerances, from an initial step
    of one hour, and the reference's own two assertions, verbatim.  The NumPy integrator on it: 19 accepted steps,
    none rejected, 2.3e-4 and 4.0e-4 against the 1e-3 of both (at reltol 1e-3: 1e-4 was not needed)."""
    lh = g.load_package()
    tf = 60.0 * 60 * 24 * 32
    model, Y, Ya = _coupled_jl(lh, lambda z: 0.495 + 0.0 * z)
    sim = lh.Simulation(model, lh.CoupledAdaptiveTRBDF2(), Y_init=Y, dt=3600.0, tspan=(0.0, tf), Ya_init=Ya, saveat=tf / 4)
    sol = lh.run(sim)
    stats = sim.integrator.trbdf2_stats
    assert sol.t[-1] == tf and len(sol.t) == 5 and stats["failed"] == 0, stats
    z = np.asarray(Ya.zc, dtype=np.float64).reshape(-1)
    vlf = np.asarray(sol.u[-1]["ϑ_l"], dtype=np.float64).reshape(-1)
    e, sp = model.earth_param_set, model.soil_param_set
    temp = e.T_0 + np.asarray(sol.u[-1]["ρe_int"], dtype=np.float64).reshape(-1) / (sp.rho_c_ds + vlf * (e.cp_l * e.rho_cloud_liq))
    zi = -0.3
    expected = np.where(z < zi, -1e-3 * (z - zi) + 0.5, 0.5 * (1 + (2.6 * np.maximum(z - zi, 0.0)) ** 2.0) ** (-0.5))
    a, b = np.sqrt(np.mean(vlf - expected) ** 2.0), np.sqrt(np.mean(temp - 284.0) ** 2.0)
    print(f"coupled.jl under CoupledAdaptiveTRBDF2: {a:.3g} {b:.3g}, accepted steps {stats['accepted']}, rejected {stats['rejected']}")
    assert a < 1e-3 and b < 1e-3                                     # coupled.jl:117-118
    assert 0 < stats["accepted"] < 138240   # (the reference's SSPRK33 steps of 20 s)
    f = C.c_uint32()
    assert lh._ffi.lib().lh_get_status(model._backend().ctx, C.byref(f)) == 0 and f.value == 0


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("mult", [0.25, 1.0, 4.0, 16.0])
def test_one_step_against_the_cpu_reference_ldexp_form(mult, ldexp_form):
    test_one_step_against_the_cpu_reference(mult)
