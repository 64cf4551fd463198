"""lh_integrate_heat_trbdf2 / HeatAdaptiveTRBDF2: adaptive TR-BDF2 of the heat-only model on the device, every column
with its own error-controlled step, against the NumPy reference (tests/heat_trbdf2_ref.py), the boundary fluxes'
budget and the reference's analytic problem (heat_test_interface.jl)."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import heat_implicit_ref as H
import heat_trbdf2_ref as T
import parity_cases as pc

pytestmark = pytest.mark.gpu
NAME = "lh_integrate_heat_trbdf2"
STATUS_NONFINITE, STATUS_FAILED = 1, 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
# ||rhoe_dev - rhoe_ref||_inf <= K eps(FT) cond_inf(I - d h A) ||rhoe||_inf per column: the bound and the K of
# tests/test_gpu_heat_implicit.py (4 x the worst ratio measured there on an MI355X, 10.36 in Float64 and 11.93 in
# Float32) -- an attempt here is that file's TR-BDF2 step with the same elimination.
K_BOUND = {np.dtype(np.float64): 4 * 10.36, np.dtype(np.float32): 4 * 11.93}
# the plain statistic next to it: the share of cells within PLAIN_REL of the field scale
PLAIN_REL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}
PLAIN_SHARE_MIN = 0.999
PROPOSAL_REL = 0.05   # dt_cols against the reference's proposal (tests/test_gpu_layered_coupled_trbdf2.py's bound)
MULTS = (0.25, 1.0)   # one attempt of this many stable steps
SPAN = 2000.0         # the integration tests' span in stable steps


def integrate_on(gm, Y, Ya, ncols, dtype, t0, t1, dt, abstol_e=0.0, reltol=0.0, bcv=None, h0=None, name=NAME, flags=0):
    """(rhoe at t1, stats dict, status, dt_cols after the call) of one call of `name` on the context gm."""
    import torch
    F = gm.F
    ft = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    cols = torch.zeros(ncols, dtype=ft, device="cuda")
    if h0 is not None:
        cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
    torch.cuda.synchronize()
    p = None
    if bcv is not None:
        bcv = np.ascontiguousarray(bcv, dtype=np.float64)
        p = bcv.ctypes.data_as(C.POINTER(C.c_double))
    F.check(getattr(gm.L, name)(gm.ctx, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, C.c_void_p(cols.data_ptr()), p), gm.ctx)
    st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
    F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    rhoe = gm.download(Y, F.LH_VAR_RHOE_INT)
    return rhoe, dict(zip(KEYS, list(st))), gm.status(), cols.cpu().numpy().astype(np.float64)


def on_device(case, t0, t1, dt, math_mode=None, **kw):
    with pc.GpuModel(case, math_mode) as gm:
        Y, Ya = gm.prognostic_and_aux()
        return integrate_on(gm, Y, Ya, case.ncols, case.dtype, t0, t1, dt, **kw)


def check_against_reference(label, dtype, P, y0, run, t1, dt, bcv=None, reltol=0.0):
    """One call over [0, t1] from h0 = dt against the reference integrator: the state under the bound and the plain
    statistic, dt_cols within PROPOSAL_REL of the reference's proposal (the reference with FT-rounded planes), the
    same accepted and rejected counts.  `run(t1, dt, bcv=, reltol=)` is the device.  Returns the device's result."""
    dt_ = np.dtype(dtype)
    eps = float(np.finfo(dtype).eps)
    ft = None if dt_ == np.float64 else np.float32
    want, _ = T.integrate(P, y0, 0.0, t1, dt, reltol=reltol, bcv=bcv)
    _, info = T.integrate(P, y0, 0.0, t1, dt, reltol=reltol, bcv=bcv, ft=ft)
    got, st, status, cols = run(t1, dt, bcv=bcv, reltol=reltol)
    g64 = got.astype(np.float64)
    assert status == 0 and st["failed"] == 0 and np.all(np.isfinite(g64)), (label, status, st)
    assert st["newton_iterations"] == 0 and st["unconverged"] == 0
    cond = H.cond_inf(P.bands, T.D * dt)
    scale = np.max(np.abs(want), axis=1)
    ratio = float(np.max(np.max(np.abs(g64 - want), axis=1) / (eps * cond * scale)))
    share = float(np.mean(np.abs(g64 - want) <= PLAIN_REL[dt_] * np.max(np.abs(want))))
    prop = float(np.max(np.abs(cols / info["dt_cols"] - 1.0)))
    print(f"{label} {dt_.name}: state ratio {ratio:.3g} of eps cond ||rhoe|| (K = {K_BOUND[dt_]:.1f}), plain share {share:.4f}, "
          f"proposal off by {prop:.3g}, accepted {st['accepted']} (reference {int(info['accepted'].sum())}), rejected "
          f"{st['rejected']} (reference {int(info['rejected'].sum())})")
    assert ratio <= K_BOUND[dt_], (label, ratio)
    assert share >= PLAIN_SHARE_MIN, (label, share)
    assert prop <= PROPOSAL_REL, (label, prop)
    assert st["accepted"] == int(info["accepted"].sum()) and st["rejected"] == int(info["rejected"].sum())
    return got, st, cols


def check_one_attempt(case, math_mode=None, label=""):
    P = T.problem(case)
    y0 = H.f64(case)[2]
    sd = H.stable_dt(case)
    run = lambda t1, dt, **kw: on_device(case, 0.0, t1, dt, math_mode=math_mode, **kw)
    for mult in MULTS:
        got, st, _ = check_against_reference(f"one attempt {label} {case.ncols}x{case.om.nlev} {mult} sd", case.dtype, P, y0, run,
                                             mult * sd, mult * sd)
        assert st["accepted"] + st["rejected"] >= case.ncols
    if case.om.nlev > 1:
        assert np.max(np.abs(got.astype(np.float64) - y0)) > 0


# ------------------------------------------------------------------ 1. one attempt against the reference

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 60])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_one_attempt_shapes(ncols, nlev, dtype):
    """Ragged last wave (67, 130 columns), both faces on one cell, no interior face, one interior cell, the reference's
    column; one attempt of 0.25 and 1 stable step."""
    check_one_attempt(H.heat_case(ncols, nlev, dtype), label="dirichlet")


VARIANTS = {
    "flux_flux": dict(bottom=M.BC_FLUX, top=M.BC_FLUX),
    "dirichlet_flux": dict(bottom=M.BC_DIRICHLET, top=M.BC_FLUX),
    "percol_dirichlet": dict(percol_bc=True),
    "ice": dict(ice=True),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_one_attempt_boundaries_and_ice(name, dtype):
    check_one_attempt(H.heat_case(67, 60, dtype, **VARIANTS[name]), label=name)


def percol_case(ncols, nlev, dtype):
    """a porosity per column (nu enters the liquid's cap and kappa's saturation)"""
    case = H.heat_case(ncols, nlev, dtype, ice=True)
    nu = case.om.soil.nu * (1.0 + 0.1 * pc.uhash(np.arange(ncols), 31, 1))
    # (rounded to the working type here, so that the device and the reference hold the same numbers)
    om = dataclasses.replace(case.om, percol={"nu": nu.astype(dtype).astype(np.float64)})
    return dataclasses.replace(case, om=om)


def test_one_attempt_libm_math():
    check_one_attempt(H.heat_case(67, 60, np.float64, ice=True), math_mode=1, label="libm")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_attempt_per_column_parameter(dtype):
    check_one_attempt(percol_case(67, 60, dtype), label="per-column nu")


# ------------------------------------------------------------------ 2. integration

_FINE = {}


def integration_case(faces, dtype):
    """(case, problem, state, stable step, fine fixed-step solution) of the CPU tests' 60-level cases at 8 columns"""
    key = (faces, np.dtype(dtype).name)
    if key not in _FINE:
        kw = dict(bottom=M.BC_FLUX, top=M.BC_FLUX) if faces == "flux" else {}
        case = H.heat_case(8, 60, dtype, **kw)
        P = T.problem(case)
        y0, sd = H.f64(case)[2], H.stable_dt(case)
        _FINE[key] = (case, P, y0, sd, T.fixed_trbdf2(P, y0, 0.0, SPAN * sd, 4000))
    return _FINE[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("faces", ["dirichlet", "flux"])
def test_integration_against_fine_fixed_steps(faces, dtype):
    """8 x 60 over 2000 stable steps from h0 = the stable step at reltol 1e-3, 1e-4, 1e-5: status 0, no failed column,
    the accepted steps per column within 8 % of the reference's mean, the error against fixed TR-BDF2 at span / 4000
    at most twice the reference's own.  In Float32 the reference keeps its planes in Float32, and the device is also
    held against the unrounded reference plus one eps32 max |rhoe| per attempted step."""
    case, P, y0, sd, fine = integration_case(faces, dtype)
    ft = None if dtype == np.float64 else np.float32
    for reltol in (1e-3, 1e-4, 1e-5):
        yr, info = T.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=reltol, ft=ft)
        got, st, status, cols = on_device(case, 0.0, SPAN * sd, sd, reltol=reltol)
        assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (reltol, status, st)
        assert not info["failed"].any()
        dev = float(np.max(np.abs(got.astype(np.float64) - fine)))
        ref = float(np.max(np.abs(yr - fine)))
        per_col, want = st["accepted"] / 8.0, float(np.mean(info["accepted"]))
        print(f"integration {faces} {np.dtype(dtype).name} reltol {reltol}: error device {dev:.4g}, reference {ref:.4g}; accepted "
              f"per column {per_col:.2f} (reference {want:.2f}), rejected {st['rejected'] / 8.0:.2f} (reference "
              f"{np.mean(info['rejected']):.2f}), max attempts {st['max_steps']}, wave_steps {st['wave_steps']}")
        assert abs(per_col - want) <= 0.08 * want, (reltol, per_col, want)
        assert dev <= 2.0 * ref, (reltol, dev, ref)
        assert st["wave_steps"] >= st["accepted"] + st["rejected"]
        if dtype == np.float32:
            yu, iu = T.integrate(P, y0, 0.0, SPAN * sd, sd, reltol=reltol)
            own, steps = float(np.max(np.abs(yu - fine))), int(np.max(iu["accepted"] + iu["rejected"]))
            unit = float(np.finfo(np.float32).eps) * float(np.max(np.abs(y0)))
            print(f"  Float32 rounding: (device - unrounded reference) / (eps32 max|rhoe|) per attempted step "
                  f"{(dev - own) / unit / steps:.2f} ({steps} steps)")
            assert dev <= own + steps * unit, (reltol, dev, own, steps, unit)


# ------------------------------------------------------------------ 3. columns and lanes

def differing_columns(ncols, dtype=np.float64):
    """columns that differ in water, ice, state and (per column) porosity and Dirichlet values"""
    case = percol_case(ncols, 60, dtype)
    c = np.arange(ncols)
    om = dataclasses.replace(case.om, percol_bc={k: (v[1] + 2.0 * (pc.uhash(c, 77 + k[0], 1) - 0.5)).astype(dtype).astype(np.float64)
                                                  for k, v in case.om.bc.items() if v[0] == M.BC_DIRICHLET})
    return dataclasses.replace(case, om=om)


def test_each_column_is_what_it_is_alone():
    case = differing_columns(130)
    sd = H.stable_dt(case)
    got, st, status, cols = on_device(case, 0.0, 300 * sd, sd)
    assert status == 0 and st["failed"] == 0
    for k in (0, 66, 129):
        one = dataclasses.replace(pc._w.reorder_columns(case, np.array([k])), ncols=1)
        g1, _, _, c1 = on_device(one, 0.0, 300 * sd, sd)
        np.testing.assert_array_equal(g1[0], got[k])
        assert c1[0] == cols[k]


def test_permutation_and_subset_of_differing_columns():
    """700 differing columns: a permutation permutes rhoe_int and dt_cols bitwise, a 128-column subset is its slice, and
    wave_steps (64 x each wave's largest attempt count) is at least the attempts."""
    case = differing_columns(700)
    sd = H.stable_dt(case)
    T1 = 300 * sd
    got, st, status, cols = on_device(case, 0.0, T1, sd)
    assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (status, st)
    order = np.random.default_rng(5).permutation(700)
    g_p, _, _, c_p = on_device(pc._w.reorder_columns(case, order), 0.0, T1, sd)
    np.testing.assert_array_equal(g_p, got[order])
    np.testing.assert_array_equal(c_p, cols[order])
    sub = dataclasses.replace(pc._w.reorder_columns(case, np.arange(100, 228)), ncols=128)
    g_s, _, _, c_s = on_device(sub, 0.0, T1, sd)
    np.testing.assert_array_equal(g_s, got[100:228])
    np.testing.assert_array_equal(c_s, cols[100:228])
    assert st["wave_steps"] >= st["accepted"] + st["rejected"]
    assert len(set(cols.tolist())) > 1   # the columns did choose their own steps


# ------------------------------------------------------------------ 4. reject and restore

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_first_step_of_the_whole_span_is_rejected(dtype):
    """h0 = the span: rejected first, and the column still lands on t1 exactly (the proposals are the reference's)."""
    case, P, y0, sd, _ = integration_case("dirichlet", dtype)
    run = lambda t1, dt, **kw: on_device(case, 0.0, t1, dt, **kw)
    got, st, cols = check_against_reference("h0 = span", dtype, P, y0, run, SPAN * sd, SPAN * sd)
    assert st["rejected"] >= 8 and st["accepted"] >= 8


def test_a_tolerance_float32_cannot_meet_fails_every_column():
    """Float32, both tolerances 1e-14: the estimate's rounding floor (about eps32 |rhoe| / d) is far above
    1e-14 |rhoe|, so h shrinks to the step floor: every column fails (status bit 4) with nothing accepted, rhoe_int is
    bitwise the initial state and dt_cols is 0.  The FT-rounded reference fails every column too (checked first)."""
    case = H.heat_case(64, 60, np.float32)
    P = T.problem(case)
    y0, sd = H.f64(case)[2], H.stable_dt(case)
    yr, info = T.integrate(P, y0, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14, ft=np.float32)
    assert info["failed"].all() and not info["accepted"].any() and np.array_equal(yr, y0)
    got, st, status, cols = on_device(case, 0.0, 30 * sd, sd, abstol_e=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 64 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0 and st["rejected"] >= 64
    np.testing.assert_array_equal(got, case.rhoe)


# ------------------------------------------------------------------ 5. boundary values in time

def bcv_of(case, t1_values=None):
    """[t0 | t1][face][component] from the case's scalar boundary values; t1_values: {(face, comp): value at t1}."""
    bcv = np.zeros((2, 2, 2))
    for (f, c), (kind, v) in case.om.bc.items():
        bcv[:, f, c] = v
    for (f, c), v in (t1_values or {}).items():
        bcv[1, f, c] = v
    return bcv


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_boundary_table_is_the_null_call(dtype):
    """A bcv whose two ends equal lh_set_bc's values is bitwise the bcv = NULL call; its hydrology entries change nothing."""
    case = H.heat_case(67, 60, dtype, ice=True)
    sd = H.stable_dt(case)
    g0, st0, s0, c0 = on_device(case, 0.0, 100 * sd, sd)
    bcv = bcv_of(case)
    g1, st1, s1, c1 = on_device(case, 0.0, 100 * sd, sd, bcv=bcv)
    bcv[:, :, M.COMP_HYDROLOGY] = [[0.3, -7.0], [1e9, 0.125]]
    g2, st2, s2, c2 = on_device(case, 0.0, 100 * sd, sd, bcv=bcv)
    assert s0 == 0 and s1 == 0 and s2 == 0 and st0 == st1 == st2
    for a, b in ((g1, c1), (g2, c2)):
        np.testing.assert_array_equal(a, g0)
        np.testing.assert_array_equal(b, c0)


@pytest.mark.parametrize("reltol", [1e-3, 1e-4])
def test_ramped_dirichlet_top_against_the_reference(reltol):
    """A Dirichlet top ramped from 280 K to 300 K over 500 stable steps through bcv, read at every stage time of every
    column's own steps: the reference reading the same table, under the one-attempt bound; another result than the
    constant table's."""
    case, P, y0, sd, _ = integration_case("dirichlet", np.float64)
    bcv = bcv_of(case, {(M.FACE_TOP, M.COMP_ENERGY): 300.0})
    assert bcv[0, M.FACE_TOP, M.COMP_ENERGY] == 280.0
    run = lambda t1, dt, **kw: on_device(case, 0.0, t1, dt, **kw)
    got, st, _ = check_against_reference(f"ramp reltol {reltol}", np.float64, P, y0, run, 500 * sd, sd, bcv=bcv, reltol=reltol)
    flat, *_ = on_device(case, 0.0, 500 * sd, sd, bcv=bcv_of(case), reltol=reltol)
    assert np.max(np.abs(got - flat)) > 0


# ------------------------------------------------------------------ 6. conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conservation_with_flux_faces(dtype):
    """sum_i rhoe_int changes by (t1 - t0) (F_bottom - F_top) / dz however a column chose its steps, to
    nlev 4 eps sum |rhoe_int| (tests/test_gpu_heat_implicit.py::test_conservation_with_flux_faces' bound)."""
    case = H.heat_case(67, 60, dtype, bottom=M.BC_FLUX, top=M.BC_FLUX, ice=True)
    fb, ft = H.BC_VALUES[M.BC_FLUX]
    sd = H.stable_dt(case)
    T1 = SPAN * sd
    dz = (case.om.zmax - case.om.zmin) / case.om.nlev
    got, st, status, cols = on_device(case, 0.0, T1, sd)
    assert status == 0 and st["failed"] == 0
    re = case.rhoe.astype(np.float64)
    change = got.astype(np.float64).sum(axis=1) - re.sum(axis=1)
    want = T1 * (fb - ft) / dz
    allowed = case.om.nlev * 4 * float(np.finfo(dtype).eps) * np.abs(re).sum(axis=1)
    print(f"conservation {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, expected "
          f"change {want:.3g}, steps per column {st['accepted'] / 67.0:.1f}")
    assert abs(want) > 0
    assert np.all(np.abs(change - want) <= allowed), float(np.max(np.abs(change - want) / allowed))


# ------------------------------------------------------------------ 7. defaults and refusals

def test_each_tolerance_defaults_on_its_own():
    """A tolerance of 0 takes its own default (abstol_e 1e-6 rho_l c_l, reltol 1e-3), bit for bit, also beside a
    tolerance that is not the default."""
    case = H.heat_case(64, 60, np.float64, ice=True)
    sd = H.stable_dt(case)
    T1 = 300 * sd
    ae = T.abstol_e_default(case.om)
    ref = on_device(case, 0.0, T1, sd, abstol_e=ae, reltol=1e-3)
    for a, r in ((0.0, 1e-3), (ae, 0.0), (0.0, 0.0)):
        got = on_device(case, 0.0, T1, sd, abstol_e=a, reltol=r)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[3], ref[3])
    tight = on_device(case, 0.0, T1, sd, abstol_e=ae, reltol=1e-5)
    got = on_device(case, 0.0, T1, sd, abstol_e=0.0, reltol=1e-5)
    np.testing.assert_array_equal(got[0], tight[0])
    assert np.max(np.abs(tight[0] - ref[0])) > 0 and tight[2] == 0
    loose = on_device(case, 0.0, T1, sd, abstol_e=1e6 * ae)
    assert np.max(np.abs(loose[0] - ref[0])) > 0   # (the absolute tolerance is read)


def refused(gm, Y, Ya, rc, message, name=NAME, t0=0.0, t1=1.0, dt=1.0, abstol_e=0.0, reltol=0.0, flags=0):
    got = getattr(gm.L, name)(gm.ctx, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, None, None)
    assert got == rc, (got, rc, message)
    assert gm.L.lh_last_error(gm.ctx).decode() == name + ": " + message, gm.L.lh_last_error(gm.ctx)
    st = (C.c_int64 * gm.F.LH_TRBDF2_NSTATS)(*([7] * gm.F.LH_TRBDF2_NSTATS))   # a refused call reports zeros
    gm.F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
    assert list(st) == [0] * gm.F.LH_TRBDF2_NSTATS


HEAT_ONLY = "heat-only models (SoilEnergyModel + PrescribedHydrologyModel)"


def test_refusals_in_order():
    case = H.heat_case(67, 3)
    nan, inf = float("nan"), float("inf")
    tols = "tolerances must be finite and >= 0"
    with pc.GpuModel(case) as gm:
        F, L = gm.F, gm.L
        Y, Ya = gm.prognostic_and_aux()
        # (after a call that counted)
        _, st, status, _ = integrate_on(gm, Y, Ya, 67, np.float64, 0.0, 100.0, 10.0)
        assert status == 0 and st["accepted"] >= 67
        refused(gm, Y, Ya, F.LH_EINVAL, "need finite t0 <= t1", t0=1.0, t1=0.0)
        refused(gm, Y, Ya, F.LH_EINVAL, "need finite t0 <= t1", t1=inf)
        for dt in (0.0, -1.0, nan, inf):
            refused(gm, Y, Ya, F.LH_EINVAL, "need a finite dt > 0", dt=dt)
        for bad in (-1e-6, nan, inf):
            refused(gm, Y, Ya, F.LH_EINVAL, tols, abstol_e=bad)
            refused(gm, Y, Ya, F.LH_EINVAL, tols, reltol=bad)
        refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x1", flags=1)   # (fixed steps: lh_step_heat_implicit)
        refused(gm, Y, Ya, F.LH_EINVAL, "unknown flags 0x80000000", flags=0x80000000)
        assert L.lh_integrate_heat_trbdf2(None, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
        bad_bcv = np.full(8, nan)
        assert L.lh_integrate_heat_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None,
                                          bad_bcv.ctypes.data_as(C.POINTER(C.c_double))) == F.LH_EINVAL
        # t1 == t0 does nothing
        before = gm.download(Y, F.LH_VAR_RHOE_INT)
        F.check(L.lh_integrate_heat_trbdf2(gm.ctx, Y, Ya, 2.0, 2.0, 1.0, 0.0, 0.0, 0, None, None), gm.ctx)
        np.testing.assert_array_equal(gm.download(Y, F.LH_VAR_RHOE_INT), before)
        lacking = gm.state(0b0001)   # Ya without theta_i
        assert L.lh_integrate_heat_trbdf2(gm.ctx, Y, lacking, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_ESTATE
        assert L.lh_integrate_heat_trbdf2(gm.ctx, Y, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_ESTATE
        assert gm.status() == 0
    # bad arguments come before the model
    for name in ("coupled_f64_small", "c2_richards_f64"):
        with pc.GpuModel(pc.make_case(name, ncols=64)) as gm:
            Y, Ya = gm.prognostic_and_aux()
            refused(gm, Y, Ya, gm.F.LH_EINVAL, "need a finite dt > 0", dt=0.0)
            refused(gm, Y, Ya, gm.F.LH_EMODEL, HEAT_ONLY)


def test_nonfinite_start_is_reported():
    """A NaN in rhoe_int: that column cannot accept a step (a NaN E rejects) and fails; the others finish."""
    case = H.heat_case(67, 3)
    case.rhoe = case.rhoe.copy()
    case.rhoe[5, 1] = np.nan
    got, st, status, cols = on_device(case, 0.0, 100.0, 100.0)
    assert status & STATUS_FAILED and st["failed"] == 1 and cols[5] == 0 and np.all(np.delete(cols, 5) > 0), (status, st)
    assert np.all(np.isfinite(np.delete(got, 5, axis=0)))


# ------------------------------------------------------------------ 8. the host mirror

def test_reference_analytic_case_through_simulation():
    """test/SoilModel/heat_test_interface.jl through Simulation(model, HeatAdaptiveTRBDF2(abstol_e = 1e-3 rho_c_ds),
    dt = 0.01): 200 library calls with the boundary sampled at the interval ends and the proposals carried, the
    reference's criterion MSE < 1e-6 (the CPU reference: 5.97e-7), no failed column."""
    lh = g.load_package()
    FT = np.float64
    msp = lh.SoilParams(FT, ν=0.495, ν_ss_gravel=0.1, ν_ss_om=0.1, ν_ss_quartz=0.1, ρc_ds=0.43314518988433487,
                        κ_solid=8.0, κ_sat_unfrozen=0.57, κ_sat_frozen=2.29)
    t0, tf, dt, n = 0.0, 2.0, 0.01, 60
    A, omega = 5.0, 2 * math.pi
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.Dirichlet(lambda t: 0.0)),
                         bottom=lh.SoilComponentBC(energy=lh.Dirichlet(lambda t: A * math.cos(omega * t))))
    param_set = lh.EarthParameterSet()
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(0.0, 1.0), nelements=n), energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.PrescribedHydrologyModel(), boundary_conditions=bc,
                         soil_param_set=msp, earth_param_set=param_set)
    ic = lambda z, m: {"ρe_int": m.soil_param_set.rho_c_ds * (0.0 - m.earth_param_set.T_0) + 0.0 * z}
    Y, Ya = lh.initialize_states(model, ic, t0)
    sim = lh.Simulation(model, lh.HeatAdaptiveTRBDF2(abstol_e=1e-3 * msp.rho_c_ds), Y_init=Y, dt=dt, tspan=(t0, tf),
                        Ya_init=Ya, saveat=50 * dt)
    sol = lh.run(sim)
    stats = sim.integrator.trbdf2_stats
    assert abs(sol.t[-1] - tf) < 1e-12 and stats["failed"] == 0 and stats["accepted"] >= 200
    z = np.asarray(Ya.zc, dtype=np.float64)
    s = math.sqrt(omega / 2) * (1 + 1j)
    analytic = np.real((np.exp(s * (1 - z)) - np.exp(-s * (1 - z))) * A * np.exp(1j * omega * tf)
                       / (np.exp(s) - np.exp(-s)))
    Tfinal = param_set.T_0 + np.asarray(sol.u[-1]["ρe_int"]).reshape(-1) / msp.rho_c_ds
    mse = float(np.mean((analytic - Tfinal) ** 2))
    print("analytic case, HeatAdaptiveTRBDF2 dt = 0.01: MSE", mse, stats)
    assert mse < 1e-6
    # the markers refuse what the library refuses, when the Simulation is built, and take no forcing
    domain = lh.Column(FT, zlim=(-1.0, 0.0), nelements=10)
    flux = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                           bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    coupled = lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                           boundary_conditions=flux, earth_param_set=param_set)
    for marker in (lh.HeatAdaptiveTRBDF2(), lh.LayeredHeatAdaptiveTRBDF2()):
        with pytest.raises(NotImplementedError, match="heat-only models"):
            lh.Simulation(coupled, marker, Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
    with pytest.raises(NotImplementedError, match="lh_integrate_heat_trbdf2 steps a model without soil classes"):
        lh.Simulation(model, lh.LayeredHeatAdaptiveTRBDF2(), Y_init=Y, dt=dt, tspan=(t0, tf), Ya_init=Ya)
    with pytest.raises(TypeError):
        lh.HeatAdaptiveTRBDF2(forcing=None)
