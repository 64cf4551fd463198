"""lh_step_implicit_euler / ImplicitEuler: backward-Euler steps of Richards columns on the device,
checked through the library's own tendency (lh_rhs), against the NumPy reference
(tests/implicit_ref.py) and on the reference's two Richards cases."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import __graft_entry__ as g
import case_model as M
import implicit_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu
STATUS_UNCONVERGED = 8


def implicit_on_device(case, dt, nsteps, bcv=None, tol=0.0, max_iter=0, math_mode=None, calls=1):
    """(vl after the steps, max iterations, unconverged, status) of `calls` calls of nsteps each."""
    with pc.GpuModel(case, math_mode) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        p = None
        if bcv is not None:
            bcv = np.ascontiguousarray(bcv, dtype=np.float64)
            p = bcv.ctypes.data_as(C.POINTER(C.c_double))
        for _ in range(calls):
            F.check(gm.L.lh_step_implicit_euler(gm.ctx, Y, Ya, 0.0, dt, nsteps, p, tol, max_iter), gm.ctx)
        mi, un = C.c_int32(), C.c_int64()
        F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
        vl = gm.download(Y, F.LH_VAR_VARTHETA_L)
        return vl, mi.value, un.value, gm.status()


def device_residual(case, v1, dt, math_mode=None):
    """v1 - v0 - dt f(v1) with f = lh_rhs on the device."""
    c1 = dataclasses.replace(case, vl=np.ascontiguousarray(v1))
    with pc.GpuModel(c1, math_mode) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        f = gm.tendencies(dY)["vl"]
    return v1 - case.vl - case.dtype(dt) * f


def round_off(case, v1, dt):
    """Per column: what evaluating R in FT may leave besides Newton's own error -- 64 eps(FT) times the
    largest of |v|, |dt f| (the difference of two face fluxes of that size rounds in FT)."""
    c1 = dataclasses.replace(case, vl=np.ascontiguousarray(v1))
    with pc.GpuModel(c1) as gm:
        Y, Ya = gm.prognostic_and_aux()
        dY = gm.state(0)
        gm.rhs(Y, Ya, dY)
        f = gm.tendencies(dY)["vl"].astype(np.float64)
    big = np.maximum(np.abs(v1).max(axis=1), dt * np.abs(f).max(axis=1))
    return 64 * np.finfo(case.dtype).eps * big


def richards_case(top, bottom, dtype=np.float64, ncols=256, ice=False, consistent=False, percol=False):
    """A random Richards ensemble (64 levels, loam) with the given hydrology BC kinds."""
    n = 64
    vals = {M.BC_FLUX: -2e-9, M.BC_DIRICHLET: 0.34, M.BC_FREE_DRAINAGE: 0.0}
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (top, vals[top]),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (bottom, 0.2 if bottom == M.BC_DIRICHLET else vals[bottom])}
    om = M.CaseModel(M.MODEL_RICHARDS, n, -1.28, 0.0, bc=bc, consistent_bottom_sign=consistent)
    c = np.arange(ncols)
    if percol:
        om.percol = dict(vg_n=1.4 + 1.2 * pc.uhash(c, 2, n), vg_alpha=1.5 + 4.0 * pc.uhash(c, 3, n),
                         vg_Ksat=10.0 ** (-7.0 + 2.0 * pc.uhash(c, 4, n)), nu=0.35 + 0.15 * pc.uhash(c, 6, n))
        om.percol_bc = {k: v[1] * (1.0 + 0.05 * (pc.uhash(c, 77 + k[0], 1) - 0.5)) for k, v in bc.items()
                        if v[0] == M.BC_DIRICHLET}
    vl = pc.wetting_front(ncols, n, -1.28, 0.0, 0.35)
    ti = np.zeros((ncols, n))
    if ice:   # static ice in every other column, below the pore space left by the water
        ti = np.where((c % 2 == 0)[:, None], 0.04 * pc.uhash(c[:, None], np.arange(n)[None, :] + 5, 1000), 0.0)
    return pc.Case("implicit", om, dtype, ncols, vl=vl.astype(dtype), ti=ti.astype(dtype))


def stable_dt(case):
    return pc.O.stable_dt(case.om, case.vl.astype(np.float64), case.ti.astype(np.float64), None, 0.5)


KINDS = [(M.BC_FLUX, M.BC_FLUX), (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET),
         (M.BC_DIRICHLET, M.BC_DIRICHLET), (M.BC_FLUX, M.BC_FREE_DRAINAGE)]


# Residual bound: Newton stops once no Newton step exceeds tol max(|v|, nu) (tol = 1e-10 in Float64, 1e-5
# in Float32).  The residual left is about J times that last step, and the rows of J = I - dt df/dv sum to
# at most about 1 + 4 dt / stable_dt (the stable step is courant 1/2 of the diffusive bound): stated bound
# 10 tol nu (1 + 4 dt / stable_dt) plus the round-off of evaluating R in FT (round_off).  (Measured: Float32
# at 100x leaves 1e-3 in a converged column, above a flat 100 tol.)
VARIANTS = [(k, v) for k in KINDS for v in ("plain", "ice", "percol", "consistent")
            if v != "consistent" or k[1] == M.BC_DIRICHLET]   # (the bottom-sign opt-out needs a Dirichlet bottom)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kinds,variant", VARIANTS)
def test_residual_through_the_tendency(dtype, kinds, variant):
    case = richards_case(*kinds, dtype=dtype, ice=variant == "ice", percol=variant == "percol",
                         consistent=variant == "consistent")
    tol = 1e-10 if dtype == np.float64 else 1e-5
    sd = stable_dt(case)
    # One column of one ensemble is the exception: with ice, free drainage at the top and a Dirichlet
    # bottom, column 182 at 100x the stable step is a Newton cycle that the safeguard does not break --
    # the CPU reference (finite-difference Jacobian, the same safeguard) cycles on it too, for 200
    # iterations.  It is counted, flagged by status bit 3, and only it may miss the
    # residual bound.
    cycling = {182} if (kinds == (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET) and variant == "ice") else set()
    for mult in (10.0, 100.0):
        v1, mi, un, st = implicit_on_device(case, mult * sd, 1)
        allowed = len(cycling) if mult == 100.0 else 0
        assert un <= allowed and bool(st & STATUS_UNCONVERGED) == (un > 0), (mult, mi, un, st)
        assert np.all(np.isfinite(v1))
        res = np.max(np.abs(device_residual(case, v1, mult * sd)), axis=1)
        bound = 10 * tol * case.om.soil.nu * (1 + 4 * mult) + round_off(case, v1, mult * sd)
        bad = set(np.flatnonzero(res > bound).tolist())
        assert bad <= (cycling if un else set()), (mult, float(res.max()), mi, sorted(bad))
        assert np.max(np.abs(v1 - case.vl)) > 0


def test_residual_c5_and_libm_math():
    case = pc.make_case("c5_percol_f64", ncols=512)
    sd = stable_dt(case)
    for mm in (None, 1):   # production math and LH_MATH_LIBM
        v1, mi, un, st = implicit_on_device(case, 10 * sd, 1, math_mode=mm)
        assert un == 0 and st == 0
        assert np.max(np.abs(device_residual(case, v1, 10 * sd, math_mode=mm))) <= 1e-8


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_parity_with_the_cpu_reference(dtype):
    case = richards_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, dtype=dtype, ncols=128, ice=True)
    sd = stable_dt(case)
    dt = 30 * sd
    v1, mi, un, st = implicit_on_device(case, dt, 3)
    assert un == 0
    idx = np.arange(0, 128, 9)
    om = case.om
    want, _ = R.implicit_euler(om, case.vl[idx].astype(np.float64), case.ti[idx].astype(np.float64), dt, 3)
    err = np.max(np.abs(v1[idx].astype(np.float64) - want))
    # Float32: the state, the closures and the tendency round to 24 bits (measured ~1e-6)
    assert err <= (1e-10 if dtype == np.float64 else 2e-5), float(err)


def test_reference_hydrostatic_case_through_simulation():
    """test/SoilModel/richards_equation.jl:1-98 with ImplicitEuler at dt = 3600 s (864 steps
    instead of 31 104 SSPRK33 steps of 100 s), and the reference's own assertion."""
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
    sim = lh.Simulation(model, lh.ImplicitEuler(), Y_init=Y, dt=3600.0, tspan=(0.0, 60 * 60 * 24 * 36.0),
                        Ya_init=Ya, saveat=60 * 3600.0)
    assert lh.step(sim) is None
    sol = lh.run(sim)
    assert sim.integrator._nsteps_done == 864
    z = np.asarray(Ya.zc)
    zi = -0.56
    want = np.where(z < zi, -S_s * (z - zi) + nu, nu * (1 + (vg_a * (z - zi)) ** vg_n) ** (-0.5))
    got = np.asarray(sol.u[-1]["ϑ_l"]).reshape(-1)
    assert np.sqrt(np.mean(got - want) ** 2.0) < 1e-4     # the reference's expression, verbatim
    assert np.sqrt(np.mean((got - want) ** 2)) < 5e-3
    # every step converged
    f = C.c_uint32()
    be = model._backend()
    assert lh._ffi.lib().lh_get_status(be.ctx, C.byref(f)) == 0 and f.value == 0


def bonan_case(ncols=2):
    sp = M.default_soil(nu=0.287, S_s=1e-3)
    vg = M.default_vg(n=3.96, alpha=2.7, Ksat=34 / 3600 / 100, theta_r=0.075)
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.267),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    om = M.CaseModel(M.MODEL_RICHARDS, 150, -1.5, 0.0, soil=sp, vg=vg, bc=bc)
    return pc.Case("bonan", om, np.float64, ncols, vl=np.full((ncols, 150), 0.1), ti=np.zeros((ncols, 150)))


def test_bonan_infiltration_first_order():
    """test/SoilModel/richards_equation.jl:100-170 over 1200 s: dt = 0.5, 1, 2 s against the device's
    SSPRK33 at 0.25 s.  The mean-absolute error grows 1.7-2.3x per doubling of dt, the CPU test's window
    (the CPU reference measures 1.717 and 1.711 here; at dt = 4 s the sharp wetting front is no longer
    resolved in time and the ratio drops to 1.69).  Every column-step converges."""
    case = bonan_case()
    T = 1200.0
    with pc.GpuModel(case) as gm:
        Y, Ya = gm.prognostic_and_aux()
        gm.F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, 0.0, 0.25, int(T / 0.25), None), gm.ctx)
        ref = gm.download(Y, gm.F.LH_VAR_VARTHETA_L)
    errs = []
    for dt in (0.5, 1.0, 2.0):
        v, mi, un, st = implicit_on_device(case, dt, int(T / dt))
        assert un == 0 and st == 0, (dt, mi, un)
        errs.append(np.mean(np.abs(v - ref)))
    r = [errs[1] / errs[0], errs[2] / errs[1]]
    assert all(1.7 <= x <= 2.3 for x in r), (errs, r)
    # the same scheme as the CPU reference
    want, _ = R.implicit_euler(case.om, case.vl[:1], case.ti[:1], 4.0, 10)
    v, *_ = implicit_on_device(case, 4.0, 10)
    assert np.max(np.abs(v[0] - want[0])) < 1e-9


def test_boundary_values_at_the_new_time_level():
    """bcv: the Dirichlet top of step k is the value of t_{k+1}.  One call of n steps with bcv equals n
    one-step calls with that value set by lh_set_bc, bit for bit; Simulation(ImplicitEuler()) with a
    time-dependent Dirichlet closure equals the same."""
    case = bonan_case(ncols=3)
    top = lambda t: 0.20 + 0.06 * (1.0 - np.exp(-t / 30.0))
    dt, n = 4.0, 12
    bcv = np.zeros((n, 2, 2))
    bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = [top((k + 1) * dt) for k in range(n)]
    v_call, mi, un, st = implicit_on_device(case, dt, n, bcv=bcv)
    assert un == 0 and st == 0
    with pc.GpuModel(case) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        for k in range(n):
            F.check(gm.L.lh_set_bc(gm.ctx, M.FACE_TOP, M.COMP_HYDROLOGY, M.BC_DIRICHLET, top((k + 1) * dt), None),
                    gm.ctx)
            F.check(gm.L.lh_step_implicit_euler(gm.ctx, Y, Ya, k * dt, dt, 1, None, 0.0, 0), gm.ctx)
        v_one = gm.download(Y, F.LH_VAR_VARTHETA_L)
    np.testing.assert_array_equal(v_call, v_one)
    # t_n instead of t_{n+1} would differ: the value changes by 10 % over the first step
    v_old, *_ = implicit_on_device(case, dt, n, bcv=np.concatenate([bcv[:1] * 0 + [[0, 0], [0, 0.20]], bcv[:-1]]))
    assert np.max(np.abs(v_old - v_call)) > 1e-6
    # the host mirror evaluates the closure at t_{n+1}
    lh = g.load_package()
    FT = np.float64
    sp, vg = case.om.soil, case.om.vg
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-1.5, 0.0), nelements=150, ncolumns=3),
                         energy_model=lh.PrescribedTemperatureModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(
                             FT, n=vg.n, α=vg.alpha, Ksat=vg.Ksat, θr=vg.theta_r)),
                         boundary_conditions=lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.Dirichlet(top)),
                                                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage())),
                         soil_param_set=lh.SoilParams(FT, ν=sp.nu, S_s=sp.S_s), earth_param_set=lh.EarthParameterSet())
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.1 + 0 * z, "θ_i": 0.0 * z}, 0.0)
    sim = lh.Simulation(model, lh.ImplicitEuler(), Y_init=Y, dt=dt, tspan=(0.0, n * dt), Ya_init=Ya)
    sol = lh.run(sim)
    np.testing.assert_array_equal(np.asarray(sol.u[-1]["ϑ_l"]).reshape(3, 150), v_call)


def test_column_independence_and_call_splitting():
    case = pc.make_case("c5_percol_f64", ncols=700)
    case.ti = np.where((np.arange(700) % 3 == 0)[:, None], 0.02, 0.0) * np.ones((1, case.om.nlev))
    sd = stable_dt(case)
    dt = 20 * sd
    v_a, *_ = implicit_on_device(case, dt, 4)
    order = np.random.default_rng(5).permutation(700)
    perm = pc._w.reorder_columns(case, order)
    v_p, *_ = implicit_on_device(perm, dt, 4)
    np.testing.assert_array_equal(v_p, v_a[order])
    v_2, *_ = implicit_on_device(case, dt, 2, calls=2)
    np.testing.assert_array_equal(v_2, v_a)


def test_scale_c2_1e6_columns():
    N = 1_000_000
    case = pc.make_case("c2_richards_f64", ncols=N)
    sub = pc.make_case("c2_richards_f64", ncols=2000)
    sd = stable_dt(sub)
    v1, mi, un, st = implicit_on_device(case, 10 * sd, 2)
    assert un == 0 and st == 0 and mi >= 1
    assert np.all(np.isfinite(v1))


def test_refusals():
    for name in ("coupled_f64_small", "heat_dirichlet_f64"):
        case = pc.make_case(name, ncols=64)
        with pc.GpuModel(case) as gm:
            Y, Ya = gm.prognostic_and_aux()
            rc = gm.L.lh_step_implicit_euler(gm.ctx, Y, Ya, 0.0, 1.0, 1, None, 0.0, 0)
            assert rc == gm.F.LH_EMODEL
    imp = richards_case(M.BC_FLUX, M.BC_FLUX, ncols=64)
    imp.om = copy.deepcopy(imp.om)
    imp.om.cf = M.default_cf(impedance=True)
    with pc.GpuModel(imp) as gm:
        Y, Ya = gm.prognostic_and_aux()
        assert gm.L.lh_step_implicit_euler(gm.ctx, Y, Ya, 0.0, 1.0, 1, None, 0.0, 0) == gm.F.LH_EMODEL
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
    # (a prescribed atmosphere exists for the coupled model only -- lh_set_atmos_forcing and validate_model
    # refuse it on a Richards model -- so its model here is refused as coupled, before the atmosphere check)
    for model in models:
        with pytest.raises(NotImplementedError):
            lh.Simulation(model, lh.ImplicitEuler(), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("kinds,variant", VARIANTS)
def test_residual_through_the_tendency_ldexp_form(kinds, variant, ldexp_form):
    test_residual_through_the_tendency(np.float64, kinds, variant)


def test_parity_with_the_cpu_reference_ldexp_form(ldexp_form):
    test_parity_with_the_cpu_reference(np.float64)
