"""lh_integrate_trbdf2 / TRBDF2: adaptive TR-BDF2 of Richards columns on the device, against the NumPy
reference (tests/trbdf2_ref.py), SSPRK33 and backward Euler, with per-column step control."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import parity_cases as pc
import trbdf2_ref as R
from test_gpu_implicit import KINDS, bonan_case, implicit_on_device, richards_case, stable_dt

pytestmark = pytest.mark.gpu
STATUS_UNCONVERGED = 8
STATUS_FAILED = 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")


def trbdf2_on_device(case, t0, t1, dt, abstol=0.0, reltol=0.0, fixed=False, bcv=None, h0=None):
    """(vl at t1, stats dict, status, dt_cols after the call) of one lh_integrate_trbdf2 call."""
    import torch
    with pc.GpuModel(case) as gm:
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
        F.check(gm.L.lh_integrate_trbdf2(gm.ctx, Y, Ya, t0, t1, dt, abstol, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                                         C.c_void_p(cols.data_ptr()), p), gm.ctx)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
        vl = gm.download(Y, F.LH_VAR_VARTHETA_L)
        status = gm.status()
        return vl, dict(zip(KEYS, list(st))), status, cols.cpu().numpy().astype(np.float64)


def ssprk33_on_device(case, dt, nsteps):
    with pc.GpuModel(case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        gm.F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, 0.0, dt, int(nsteps), None), gm.ctx)
        return gm.download(Y, gm.F.LH_VAR_VARTHETA_L)


VARIANTS = [(k, v) for k in KINDS for v in ("plain", "ice", "percol")]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kinds,variant", VARIANTS)
def test_fixed_step_parity_with_the_cpu_reference(dtype, kinds, variant):
    case = richards_case(*kinds, dtype=dtype, ncols=64, ice=variant == "ice", percol=variant == "percol")
    dt = 10 * stable_dt(case)
    v1, st, status, _ = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True)
    assert status == 0 and st["accepted"] == 3 * 64 and st["rejected"] == 0 and st["unconverged"] == 0, st
    idx = np.arange(0, 64, 7)
    om = case.om
    if om.percol:
        om = copy.deepcopy(om)
        om.percol = {k: np.asarray(a)[idx] for k, a in om.percol.items()}
        om.percol_bc = {k: np.asarray(a)[idx] for k, a in om.percol_bc.items()}
    want, _ = R.trbdf2(om, case.vl[idx].astype(np.float64), case.ti[idx].astype(np.float64), 0.0, 3 * dt, dt,
                       adaptive=False)
    err = np.max(np.abs(v1[idx].astype(np.float64) - want))
    assert err <= (1e-10 if dtype == np.float64 else 2e-5), float(err)


def test_fixed_step_order_on_the_device():
    """Smooth wetting front, 40 stable steps: against a fixed-step run at dt/16, the error falls 3.5-4.5x per
    halving of dt (backward Euler: 1.7-2.3 in test_bonan_infiltration_first_order)."""
    case = pc.make_case("c2_richards_f64", ncols=128)
    sd = stable_dt(case)
    T = 40 * sd
    ref, *_ = trbdf2_on_device(case, 0.0, T, T / 640, fixed=True)
    errs = []
    for k in (10, 20, 40):
        v, st, status, _ = trbdf2_on_device(case, 0.0, T, T / k, fixed=True)
        assert status == 0 and st["accepted"] == k * 128
        errs.append(np.max(np.abs(v - ref)))
    r = [a / b for a, b in zip(errs, errs[1:])]
    assert all(3.5 <= x <= 4.5 for x in r), (errs, r)


def test_bonan_infiltration_adaptive():
    """test/SoilModel/richards_equation.jl:100-170 over 1200 s: every column reaches t1 with status 0, and at
    reltol 1e-4 the mean absolute error against SSPRK33 at 0.25 s is below backward Euler's at dt = 0.5 s."""
    case = bonan_case(ncols=4)
    T = 1200.0
    ref = ssprk33_on_device(case, 0.25, int(T / 0.25))
    v_ie, _, un, st_ie = implicit_on_device(case, 0.5, int(T / 0.5))
    assert un == 0 and st_ie == 0
    err_ie = np.mean(np.abs(v_ie - ref))
    for rtol in (1e-3, 1e-4):
        v, st, status, cols = trbdf2_on_device(case, 0.0, T, 1.0, reltol=rtol, abstol=1e-6)
        assert status == 0 and st["failed"] == 0, st
        assert np.all(np.isfinite(cols)) and np.all(cols > 0)
        err = np.mean(np.abs(v - ref))
        if rtol == 1e-4:
            assert err < err_ie, (err, err_ie, st)


def test_the_known_cycle_is_integrated():
    """Ice / free-drainage top / Dirichlet bottom over 100x its stable step: backward Euler flags column 182
    (status bit 3); TR-BDF2 brings every column to t1 with status 0, within 10 reltol nu of SSPRK33 at the
    stable step."""
    case = richards_case(M.BC_FREE_DRAINAGE, M.BC_DIRICHLET, ice=True)
    sd = stable_dt(case)
    _, _, un, st_ie = implicit_on_device(case, 100 * sd, 1)
    assert un >= 1 and st_ie & STATUS_UNCONVERGED
    rtol = 1e-3
    v, st, status, cols = trbdf2_on_device(case, 0.0, 100 * sd, 100 * sd, reltol=rtol, abstol=1e-6)
    assert status == 0 and st["failed"] == 0 and np.all(cols > 0), st
    ref = ssprk33_on_device(case, sd, 100)
    err = np.max(np.abs(v - ref), axis=1)
    assert err.max() <= 10 * rtol * case.om.soil.nu, (float(err.max()), int(err.argmax()), float(err[182]))


def test_reference_hydrostatic_case_through_simulation():
    """test/SoilModel/richards_equation.jl:1-98 through Simulation(model, TRBDF2()), with the reference's own
    assertion; fewer steps than the 31 104 SSPRK33 steps of the reference."""
    lh = g.load_package()
    FT = np.float64
    nu, S_s, vg_n, vg_a = 0.495, 1e-3, 2.0, 2.6
    msp = lh.SoilParams(FT, ν=nu, S_s=S_s)
    hm = lh.vanGenuchten(FT, n=vg_n, α=vg_a, Ksat=0.0443 / 3600 / 100, θr=0.0)
    domain = lh.Column(FT, zlim=(-10.0, 0.0), nelements=50)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0)),
                         bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0)))
    model = lh.SoilModel(FT, domain=domain, energy_model=lh.PrescribedTemperatureModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm),
                         boundary_conditions=bc, soil_param_set=msp, earth_param_set=lh.EarthParameterSet())
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.494 + 0 * z, "θ_i": 0.0 * z}, 0.0)
    sim = lh.Simulation(model, lh.TRBDF2(), Y_init=Y, dt=100.0, tspan=(0.0, 60 * 60 * 24 * 36.0),
                        Ya_init=Ya, saveat=60 * 3600.0)
    sol = lh.run(sim)
    assert sol.t[-1] == 60 * 60 * 24 * 36.0
    z = np.asarray(Ya.zc)
    zi = -0.56
    want = np.where(z < zi, -S_s * (z - zi) + nu, nu * (1 + (vg_a * (z - zi)) ** vg_n) ** (-0.5))
    got = np.asarray(sol.u[-1]["ϑ_l"]).reshape(-1)
    assert np.sqrt(np.mean(got - want) ** 2.0) < 1e-4     # the reference's expression, verbatim
    assert np.sqrt(np.mean((got - want) ** 2)) < 5e-3
    stats = sim.integrator.trbdf2_stats
    assert stats["failed"] == 0 and stats["accepted"] + stats["rejected"] < 31104, stats
    f = C.c_uint32()
    be = model._backend()
    assert lh._ffi.lib().lh_get_status(be.ctx, C.byref(f)) == 0 and f.value == 0


def test_boundary_values_linear_in_time():
    """A Dirichlet top that moves linearly over the call: parity with the CPU reference (fixed steps), and
    the value at t0 alone would give another result."""
    case = bonan_case(ncols=2)
    bcv = np.zeros((2, 2, 2))
    bcv[0, M.FACE_TOP, M.COMP_HYDROLOGY] = 0.20
    bcv[1, M.FACE_TOP, M.COMP_HYDROLOGY] = 0.267
    T, dt = 40.0, 4.0
    v, st, status, _ = trbdf2_on_device(case, 0.0, T, dt, fixed=True, bcv=bcv)
    assert status == 0 and st["unconverged"] == 0
    want, _ = R.trbdf2(case.om, case.vl[:1], case.ti[:1], 0.0, T, dt, adaptive=False, bcv=bcv)
    assert np.max(np.abs(v[0] - want[0])) < 1e-9
    flat = bcv.copy()
    flat[1] = flat[0]
    v_flat, *_ = trbdf2_on_device(case, 0.0, T, dt, fixed=True, bcv=flat)
    assert np.max(np.abs(v_flat - v)) > 1e-6
    # adaptive: every column reaches t1, closer to a fine solution than the fixed step of 4 s
    fine, *_ = trbdf2_on_device(case, 0.0, T, 0.25, fixed=True, bcv=bcv)
    rtol = 1e-4
    v_a, st_a, status_a, _ = trbdf2_on_device(case, 0.0, T, dt, bcv=bcv, reltol=rtol)
    assert status_a == 0 and st_a["failed"] == 0
    err_a, err_4 = np.max(np.abs(v_a - fine)), np.max(np.abs(v - fine))
    assert err_a < err_4 and err_a <= 10 * rtol * case.om.soil.nu, (err_a, err_4, st_a)


def test_column_independence_and_failed_columns():
    case = pc.make_case("c5_percol_f64", ncols=700)
    case.ti = np.where((np.arange(700) % 3 == 0)[:, None], 0.02, 0.0) * np.ones((1, case.om.nlev))
    sd = stable_dt(case)
    T = 20 * sd
    v_a, st, status, cols = trbdf2_on_device(case, 0.0, T, sd)
    assert status == 0 and st["failed"] == 0
    assert np.all(np.isfinite(cols)) and np.all(cols > 0)
    order = np.random.default_rng(5).permutation(700)
    perm = pc._w.reorder_columns(case, order)
    v_p, _, _, cols_p = trbdf2_on_device(perm, 0.0, T, sd)
    np.testing.assert_array_equal(v_p, v_a[order])
    np.testing.assert_array_equal(cols_p, cols[order])
    sub = dataclasses.replace(pc._w.reorder_columns(case, np.arange(100, 228)), ncols=128)
    v_s, *_ = trbdf2_on_device(sub, 0.0, T, sd)
    np.testing.assert_array_equal(v_s, v_a[100:228])
    # wave_steps: 64 x the largest step count of each wave, at least the sum of the columns' counts
    assert st["wave_steps"] >= st["accepted"] + st["rejected"]
    # a tolerance Float32 cannot meet: h shrinks to the floor, the column fails (bit 4), keeps its last
    # accepted state and reports dt_cols = 0
    c32 = richards_case(M.BC_FLUX, M.BC_FLUX, dtype=np.float32, ncols=64)
    sd32 = stable_dt(c32)
    v, st, status, cols = trbdf2_on_device(c32, 0.0, 10 * sd32, sd32, abstol=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 64 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0
    np.testing.assert_array_equal(v, c32.vl)


def test_refusals():
    for name in ("coupled_f64_small", "heat_dirichlet_f64"):
        case = pc.make_case(name, ncols=64)
        with pc.GpuModel(case) as gm:
            Y, Ya = gm.prognostic_and_aux()
            rc = gm.L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None)
            assert rc == gm.F.LH_EMODEL
    imp = richards_case(M.BC_FLUX, M.BC_FLUX, ncols=64)
    imp.om = copy.deepcopy(imp.om)
    imp.om.cf = M.default_cf(impedance=True)
    with pc.GpuModel(imp) as gm:
        Y, Ya = gm.prognostic_and_aux()
        assert gm.L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == gm.F.LH_EMODEL
    ok = richards_case(M.BC_FLUX, M.BC_FLUX, ncols=64)
    with pc.GpuModel(ok) as gm:
        Y, Ya = gm.prognostic_and_aux()
        L, F = gm.L, gm.F
        assert L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 1.0, 0.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
        assert L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, -1e-6, 0.0, 0, None, None) == F.LH_EINVAL
        assert L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, float("nan"), 0, None, None) == F.LH_EINVAL
        assert L.lh_integrate_trbdf2(gm.ctx, Y, Ya, 0.0, 1.0, 1.0, float("inf"), 0.0, 0, None, None) == F.LH_EINVAL
    # the host mirror refuses when the Simulation is built
    lh = g.load_package()
    FT = np.float64
    domain = lh.Column(FT, zlim=(-1.0, 0.0), nelements=10)
    flux = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                           bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    ep = lh.EarthParameterSet()
    models = [
        lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                     boundary_conditions=flux, earth_param_set=ep),
        lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(),
                     hydrology_model=lh.PrescribedHydrologyModel(lambda z, t: 0.3 + 0 * z), boundary_conditions=flux,
                     earth_param_set=ep),
        lh.SoilModel(FT, domain=domain, energy_model=lh.PrescribedTemperatureModel(),
                     hydrology_model=lh.SoilHydrologyModel(FT, impedance_factor=lh.IceImpedance(FT)),
                     boundary_conditions=flux, earth_param_set=ep),
        lh.SoilModel(FT, domain=domain, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                     boundary_conditions=lh.SoilColumnBC(top=lh.PrescribedAtmosForcing(
                         FT, u_atm=0.34, theta_atm=299.0, z_atm=0.05, theta_scale=299.0, rho_a_sfc=1.17,
                         q_atm=0.015), bottom=flux.bottom),
                     earth_param_set=ep),
    ]
    for model in models:
        with pytest.raises(NotImplementedError):
            lh.Simulation(model, lh.TRBDF2(), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
        with pytest.raises(NotImplementedError):
            lh.integrate_trbdf2(model, None, None, 0.0, 1.0, 1.0)


def test_scale_c2_1e6_columns():
    N = 1_000_000
    case = pc.make_case("c2_richards_f64", ncols=N)
    sub = pc.make_case("c2_richards_f64", ncols=2000)
    sd = stable_dt(sub)
    v1, st, status, cols = trbdf2_on_device(case, 0.0, 10 * sd, sd)
    assert status == 0 and st["failed"] == 0 and st["accepted"] >= N, st
    assert np.all(np.isfinite(v1)) and np.all(cols > 0)


def test_one_adaptive_step_against_the_cpu_reference():
    """The error estimate and the controller, pinned on single steps of a smooth C2 ensemble (a call that
    spans exactly one step): the reference measures E = 0.02 at the stable step, 0.24 at 4x (accepted) and
    1.3, 2.7 at 16x, 32x (rejected).  An accepted step lands on the reference's Y_1 and proposes
    h 0.9 E^(-1/3) within 5 % of the reference's; a step the reference rejects is rejected."""
    case = pc.make_case("c2_richards_f64", ncols=8)
    sd = stable_dt(case)
    y0, ti = case.vl.astype(np.float64), case.ti.astype(np.float64)
    fn = R.IR.tendency(case.om, y0, ti)
    for mult in (1.0, 4.0, 16.0, 32.0):
        h = mult * sd
        y1, _, e, _ = R.attempt(case.om, y0, fn, ti, np.zeros(8), np.full(8, h))
        E = R.error_norm(e, y0, y1, 1e-6, 1e-3)
        v, st, status, cols = trbdf2_on_device(case, 0.0, h, h)
        assert status == 0 and st["failed"] == 0, (mult, st)
        if np.all(E <= 1.0):
            assert st["accepted"] == 8 and st["rejected"] == 0, (mult, E, st)
            assert np.max(np.abs(v - y1)) <= 1e-5, (mult, float(np.max(np.abs(v - y1))))
            want = h * np.clip(0.9 * E ** (-1.0 / 3.0), 0.2, 5.0)
            np.testing.assert_allclose(cols, want, rtol=0.05, err_msg=f"x{mult} E={E}")
        else:
            assert np.all(E > 1.0) and st["rejected"] >= 8 and st["accepted"] >= 8, (mult, E, st)


def test_each_tolerance_defaults_on_its_own():
    """A tolerance of 0 takes its own default (abstol 1e-6, reltol 1e-3), bit for bit; the host mirror maps
    each None on its own: TRBDF2(abstol=1e-8) keeps reltol 1e-3 and succeeds in Float32."""
    case = pc.make_case("c2_richards_f64", ncols=64)
    sd = stable_dt(case)
    T = 20 * sd
    ref, *_ = trbdf2_on_device(case, 0.0, T, sd, abstol=1e-6, reltol=1e-3)
    for a, r in ((0.0, 1e-3), (1e-6, 0.0), (0.0, 0.0)):
        v, *_ = trbdf2_on_device(case, 0.0, T, sd, abstol=a, reltol=r)
        np.testing.assert_array_equal(v, ref)
    v8, st8, status8, _ = trbdf2_on_device(case, 0.0, T, sd, abstol=1e-8, reltol=1e-3)
    v80, *_ = trbdf2_on_device(case, 0.0, T, sd, abstol=1e-8, reltol=0.0)
    np.testing.assert_array_equal(v80, v8)
    assert status8 == 0
    lh = g.load_package()
    FT = np.float32
    sp = M.default_soil(nu=0.287, S_s=1e-3)
    vg = M.default_vg(n=3.96, alpha=2.7, Ksat=34 / 3600 / 100, theta_r=0.075)
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-1.5, 0.0), nelements=150, ncolumns=4),
                         energy_model=lh.PrescribedTemperatureModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(
                             FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)),
                         boundary_conditions=lh.SoilColumnBC(
                             top=lh.SoilComponentBC(hydrology=lh.Dirichlet(lambda t: 0.267)),
                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                         soil_param_set=lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s), earth_param_set=lh.EarthParameterSet())
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.1 + 0 * z, "θ_i": 0.0 * z}, 0.0)
    sim = lh.Simulation(model, lh.TRBDF2(abstol=1e-8), Y_init=Y, dt=60.0, tspan=(0.0, 600.0), Ya_init=Ya)
    sol = lh.run(sim)
    assert sim.integrator.trbdf2_stats["failed"] == 0, sim.integrator.trbdf2_stats
    f = C.c_uint32()
    assert lh._ffi.lib().lh_get_status(model._backend().ctx, C.byref(f)) == 0 and f.value == 0
    assert np.all(np.isfinite(np.asarray(sol.u[-1]["ϑ_l"])))


def test_fixed_mode_ignores_dt_cols():
    """LH_TRBDF2_FIXED steps by exactly dt whatever dt_cols holds, and leaves dt in it."""
    case = richards_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, ncols=64, ice=True)
    sd = stable_dt(case)
    dt = 10 * sd
    v0, st0, _, c0 = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True)
    junk = 0.1 * sd * (1.0 + np.arange(64))
    v1, st1, _, c1 = trbdf2_on_device(case, 0.0, 3 * dt, dt, fixed=True, h0=junk)
    np.testing.assert_array_equal(v1, v0)
    assert st1["accepted"] == st0["accepted"] == 3 * 64
    np.testing.assert_array_equal(c1, np.full(64, dt))


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("kinds,variant", VARIANTS)
def test_fixed_step_parity_with_the_cpu_reference_ldexp_form(kinds, variant, ldexp_form):
    test_fixed_step_parity_with_the_cpu_reference(np.float64, kinds, variant)


def test_one_adaptive_step_against_the_cpu_reference_ldexp_form(ldexp_form):
    test_one_adaptive_step_against_the_cpu_reference()
