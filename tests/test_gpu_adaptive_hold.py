"""lh_step_ssprk33_adaptive_hold: adaptive SSPRK33 with the step size held over chunks of `hold` steps.

The call is DEFINED by a sequence of existing calls (include/landhydro.h): per chunk, copy Y to Z,
lh_step_ssprk33_adaptive(Z, nsteps = 1, dtbuf) for the chunk's dt, then `hold` x
lh_step_ssprk33_device_dt(Y, dtbuf).  Y, every chunk's dt and the elapsed time must be those bits on
both engines: one launch of the persistent column stepper per chunk, which also leaves the bound of the
state it ends on (<= 128 levels), and the fused stages (everything else).  About 200 columns: not a
multiple of 64, nor of the 4 / 8 / 12 columns of a stepper workgroup; two cases at 4100 columns for the
workgroup shapes of large ensembles.
"""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import case_model as M
import parity_cases as pc

pytestmark = pytest.mark.gpu

NCOLS, NCHUNKS, COURANT = 200, 3, 0.3
STEPPER, FUSED = 1, 0   # LH_ENGINE_COLUMN_STEPPER / LH_ENGINE_FUSED_STAGES


def _c5_percol_dirichlet():
    """c5_percol_f64 (per-column van Genuchten parameters and porosity) under a per-column Dirichlet top."""
    case = pc.make_case("c5_percol_f64", ncols=NCOLS)
    om = copy.deepcopy(case.om)
    top = (M.FACE_TOP, M.COMP_HYDROLOGY)
    th_r, nu = om.percol["vg_theta_r"], om.percol["nu"]
    om.bc[top] = (M.BC_DIRICHLET, 0.3)
    om.percol_bc = {top: th_r + 0.6 * (nu - th_r)}
    return dataclasses.replace(case, om=om, name="c5_percol_f64_dirichlet")


def _ice_every_other_column():
    import test_gpu_implicit as ti
    return ti.richards_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, ncols=NCOLS, ice=True)


def _atmosphere(n=24):
    """A coupled Float64 ensemble under a prescribed atmosphere (the soil and forcing of the reference's
    surface-flux experiment), insulated below, initial moisture and temperature varied per column."""
    nu = 0.55
    sp = dataclasses.replace(pc.coupled_soil()[0], nu=nu, nu_ss_quartz=0.4, rho_c_ds=(1 - nu) * 1.926e06)
    vg = M.default_vg(n=1.68, alpha=5.0, Ksat=1.31 / 100 / 3600 / 1000, theta_r=0.084)
    atm = M.AtmosForcing(u_atm=0.34, theta_atm=299.0, z_atm=0.05, theta_scale=299.0, rho_a_sfc=1.17, q_atm=0.015)
    om = M.CaseModel(M.MODEL_COUPLED, n, -0.55, 0.0, soil=sp, vg=vg,
                     bc={(M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_FLUX, 0.0),
                         (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FLUX, 0.0)}, atmos=atm, percol_atmos={})
    c = np.arange(NCOLS)
    zc, _ = pc.grid_np(-0.55, 0.0, n)
    vl = 0.25 + 0.25 * pc.uhash(c, 34, n)[:, None] + 0.05 * np.sin(9.0 * zc)[None, :]
    T = 296.0 + 6.0 * pc.uhash(c, 35, n)[:, None] + 2.0 * zc[None, :]
    rhoe = (sp.rho_c_ds + vl * (om.earth.cp_l * om.earth.rho_liq)) * (T - om.earth.T_0)
    return pc.Case("atmos_hold", om, np.float64, NCOLS, vl=vl, ti=np.zeros((NCOLS, n)), rhoe=rhoe)


# name -> (builder, engine the call must report, math mode (None: default), dt_max as a fraction of the first bound)
CASES = {
    "richards_f64_n5": (lambda: pc.make_case("c2_richards_f64_n5", ncols=NCOLS), STEPPER, None, 0.0),
    "richards_f64_n64": (lambda: pc.make_case("c2_richards_f64", ncols=NCOLS), STEPPER, None, 0.0),
    "richards_f64_n65": (lambda: pc.make_case("c2_richards_f64_n65", ncols=NCOLS), STEPPER, None, 0.0),   # CW = 2, ragged top lane
    "richards_f64_n128": (lambda: pc.make_case("c4_richards_f64_128", ncols=NCOLS), STEPPER, None, 0.0),
    "richards_f64_n160": (lambda: pc.make_case("c2_richards_f64_n160", ncols=NCOLS), FUSED, None, 0.0),
    "coupled_f32_n64": (lambda: pc.make_case("c3_coupled_f32", ncols=NCOLS), STEPPER, None, 0.0),
    "coupled_f64_n64": (lambda: pc.make_case("c3_coupled_f64", ncols=NCOLS), STEPPER, None, 0.0),
    "heat_dirichlet_f64": (lambda: pc.make_case("heat_dirichlet_f64", ncols=NCOLS), STEPPER, None, 0.0),
    "richards_ice_alternating": (_ice_every_other_column, STEPPER, None, 0.0),
    "c5_percol_dirichlet": (_c5_percol_dirichlet, STEPPER, None, 0.0),
    "c1_dirichlet_f64": (lambda: pc.make_case("c1_dirichlet_f64", ncols=NCOLS), STEPPER, None, 0.0),
    "richards_f64_n64_libm": (lambda: pc.make_case("c2_richards_f64", ncols=NCOLS), STEPPER, "libm", 0.0),
    "richards_f64_n64_capped": (lambda: pc.make_case("c2_richards_f64", ncols=NCOLS), STEPPER, None, 0.25),
    "coupled_atmosphere_f64": (_atmosphere, FUSED, None, 0.0),
    # 4096 columns and more: the stepper's workgroups take 8 or 12 columns instead of 4 (wave_stepper_columns),
    # as on the 1e6-column workloads; 4100 is a multiple of neither, so the last workgroup has spare waves
    "richards_f64_n64_4100cols": (lambda: pc.make_case("c2_richards_f64", ncols=4100), STEPPER, None, 0.0),
    "richards_f64_n128_4100cols": (lambda: pc.make_case("c4_richards_f64_128", ncols=4100), STEPPER, None, 0.0),
}


def _tdtype(case):
    import torch
    return torch.float64 if case.dtype == np.float64 else torch.float32


def _prognostic(g, Y):
    F, m = g.F, g.case.om.model
    out = {}
    if m != M.MODEL_HEAT:
        out["vl"] = g.download(Y, F.LH_VAR_VARTHETA_L)
    if m != M.MODEL_RICHARDS:
        out["rhoe"] = g.download(Y, F.LH_VAR_RHOE_INT)
    return out


def _copy_into(g, Z, Y):
    """Z := Y (the prognostic planes that move; theta_i never does)."""
    F = g.F
    for k, a in _prognostic(g, Y).items():
        g.upload(Z, F.LH_VAR_VARTHETA_L if k == "vl" else F.LH_VAR_RHOE_INT, a)


def _word(case):
    import torch
    w = torch.zeros(1, device="cuda", dtype=_tdtype(case))
    torch.cuda.synchronize()   # (the library works on its own stream)
    return w


def _first_bound(g, Y, Ya, courant):
    b = _word(g.case)
    dY = g.state(0)
    g.F.check(g.L.lh_rhs_stable_dt(g.ctx, 0.0, Y, Ya, dY, courant, b.data_ptr()), g.ctx)
    g.F.check(g.L.lh_synchronize(g.ctx), g.ctx)
    return float(b.item())


def reference_sequence(g, Y, Ya, courant, dt_max, nchunks, hold, end_bounds=None):
    """The defining sequence, from existing calls only.  Returns (dt of every chunk, elapsed in FT).
    end_bounds: a list that receives lh_rhs_stable_dt of the state every chunk ends on."""
    F, L, ctx = g.F, g.L, g.ctx
    Z, _ = g.prognostic_and_aux()
    dY = g.state(0) if end_bounds is not None else None
    dtbuf, b = _word(g.case), _word(g.case)
    dts, elapsed = [], np.zeros(1, dtype=g.case.dtype)
    for _ in range(nchunks):
        _copy_into(g, Z, Y)
        F.check(L.lh_step_ssprk33_adaptive(ctx, Z, Ya, 0.0, courant, dt_max, 1, dtbuf.data_ptr(), None), ctx)
        for _ in range(hold):
            F.check(L.lh_step_ssprk33_device_dt(ctx, Y, Ya, 0.0, dtbuf.data_ptr(), None), ctx)
        F.check(L.lh_synchronize(ctx), ctx)
        dts.append(float(dtbuf.item()))
        for _ in range(hold):
            elapsed += g.case.dtype(dts[-1])
        if end_bounds is not None:
            F.check(L.lh_rhs_stable_dt(ctx, 0.0, Y, Ya, dY, courant, b.data_ptr()), ctx)
            F.check(L.lh_synchronize(ctx), ctx)
            end_bounds.append(float(b.item()))
    return dts, float(elapsed[0])


def _model(name):
    build, engine, math, cap = CASES[name]
    case = build()
    g = pc.GpuModel(case, math_mode=None if math is None else pc._pkg()._ffi.LH_MATH_LIBM)
    return case, g, engine, cap


@pytest.mark.parametrize("hold", [1, 3, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_the_reference_sequence(name, hold):
    case, g, engine, cap = _model(name)
    with g:
        F, L, ctx = g.F, g.L, g.ctx
        assert L.lh_adaptive_hold_engine(ctx, hold) == engine
        Yr, Ya = g.prognostic_and_aux()
        dt_max = cap * _first_bound(g, Yr, Ya, COURANT)
        dts, elapsed = reference_sequence(g, Yr, Ya, COURANT, dt_max, NCHUNKS, hold)
        want = _prognostic(g, Yr)
        g.status()
        # one call of NCHUNKS chunks
        Y1, _ = g.prognostic_and_aux()
        t, el = _word(case), _word(case)
        F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y1, Ya, 0.0, COURANT, dt_max, NCHUNKS, hold, t.data_ptr(), el.data_ptr()), ctx)
        F.check(L.lh_synchronize(ctx), ctx)
        got1 = _prognostic(g, Y1)
        assert float(t.item()) == dts[-1] and float(el.item()) == elapsed
        # NCHUNKS calls of one chunk: every chunk's dt
        Y2, _ = g.prognostic_and_aux()
        el.zero_()
        import torch
        torch.cuda.synchronize()
        each = []
        for _ in range(NCHUNKS):
            F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y2, Ya, 0.0, COURANT, dt_max, 1, hold, t.data_ptr(), el.data_ptr()), ctx)
            F.check(L.lh_synchronize(ctx), ctx)
            each.append(float(t.item()))
        got2 = _prognostic(g, Y2)
        assert each == dts and float(el.item()) == elapsed
        assert not (g.status() & 4)
    assert all(d > 0 for d in dts)
    if cap:
        assert all(d == float(case.dtype(dt_max)) for d in dts)        # the cap bites in every chunk
    for k in want:
        assert np.array_equal(want[k], got1[k]), (name, hold, k, "one call")
        assert np.array_equal(want[k], got2[k]), (name, hold, k, "chunk by chunk")
    assert any(not np.array_equal(want[k], getattr(case, k)) for k in want), "the state never moved"


@pytest.mark.parametrize("name", ["richards_f64_n64", "coupled_f32_n64", "richards_f64_n160", "coupled_atmosphere_f64"])
def test_hold_one_is_the_adaptive_call(name):
    """hold = 1: bitwise lh_step_ssprk33_adaptive(nsteps = nchunks), elapsed included."""
    case, g, _, _ = _model(name)
    with g:
        F, L, ctx = g.F, g.L, g.ctx
        Ya = None
        out = []
        for which in range(2):
            Y, Ya = g.prognostic_and_aux()
            t, el = _word(case), _word(case)
            if which == 0:
                F.check(L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, COURANT, 0.0, 5, t.data_ptr(), el.data_ptr()), ctx)
            else:
                F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, COURANT, 0.0, 5, 1, t.data_ptr(), el.data_ptr()), ctx)
            F.check(L.lh_synchronize(ctx), ctx)
            out.append((_prognostic(g, Y), float(t.item()), float(el.item())))
    assert out[0][1:] == out[1][1:] and out[0][1] > 0
    for k in out[0][0]:
        assert np.array_equal(out[0][0][k], out[1][0][k]), (name, k)


# ------------------------------------------------------------------ the overrun flag (status bit 5)

def _hydrostatic_case():
    """A still column: hydrostatic, both Dirichlet face values hydrostatic, the consistent bottom sign."""
    import __graft_entry__ as ge
    lh = ge.load_package()
    P = lh.parameterizations
    n, zmin, zmax, zi = 64, -1.28, 0.0, -2.0
    hm = lh.vanGenuchten(np.float64)
    nu, S_s = 0.43, 1e-3
    zc, _ = pc.grid_np(zmin, zmax, n)
    vl = np.repeat(P.hydrostatic_profile(hm, zc, zi, nu, S_s)[None, :], NCOLS, axis=0)
    top = float(P.hydrostatic_profile(hm, np.float64(zmax), zi, nu, S_s))
    bot = float(P.hydrostatic_profile(hm, np.float64(zmin), zi, nu, S_s))
    om = M.CaseModel(M.MODEL_RICHARDS, n, zmin, zmax,
                     bc={(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, top),
                         (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, bot)}, consistent_bottom_sign=True)
    return pc.Case("hydrostatic", om, np.float64, NCOLS, vl=vl, ti=np.zeros((NCOLS, n)))


def _wetting_front_case(nlev):
    """test_gpu_implicit.bonan_case (a dry sand column under a nearly saturated Dirichlet top: a sharp
    wetting front), at its own 150 levels (the fused stages) or fewer (the stepper)."""
    import test_gpu_implicit as ti
    case = ti.bonan_case(ncols=NCOLS)
    if nlev != case.om.nlev:
        om = dataclasses.replace(case.om, nlev=nlev, zmin=-0.01 * nlev)
        case = dataclasses.replace(case, om=om, vl=np.full((NCOLS, nlev), 0.1), ti=np.zeros((NCOLS, nlev)))
    return case


# (builder, hold, courant, nchunks, engine, the per-step path must say).  The wetting front: hold = 64 and
# courant = 0.5 as first proposed; see the docstring of the test for what they measured.
OVERRUN = {
    "still_hydrostatic": (_hydrostatic_case, 16, 0.5, 3, STEPPER, False),
    "wetting_front_n150": (lambda: _wetting_front_case(150), 64, 0.5, 2, FUSED, True),
    "wetting_front_n120": (lambda: _wetting_front_case(120), 64, 0.5, 2, STEPPER, True),
}


@pytest.mark.parametrize("name", list(OVERRUN))
def test_overrun_flag_is_what_the_per_step_path_says(name):
    """Bit 5 of the status: some chunk's dt exceeded the stable-step bound of the state the chunk ended on
    (or that bound was no positive finite number).  The expectation comes from existing calls only
    (lh_rhs_stable_dt on the state the reference sequence reaches after every chunk) and is itself
    asserted, so that neither input can pass vacuously.
    Measured (MI355X): the wetting front trips with the values first proposed, hold = 64 and courant = 0.5 --
    chunk dt 0.04141, 0.17752 s against end-state bounds 0.17752, 0.15458 s (the second chunk overruns), the
    same figures at 150 levels (fused stages) and 120 levels (stepper); the hydrostatic column keeps
    dt = bound = 13699.859 s through every chunk."""
    build, hold, courant, nchunks, engine, expect = OVERRUN[name]
    case = build()
    with pc.GpuModel(case) as g:
        F, L, ctx = g.F, g.L, g.ctx
        assert L.lh_adaptive_hold_engine(ctx, hold) == engine
        Yr, Ya = g.prognostic_and_aux()
        ends = []
        dts, _ = reference_sequence(g, Yr, Ya, courant, 0.0, nchunks, hold, end_bounds=ends)
        per_step = any(not (b > 0 and np.isfinite(b)) or b < d for b, d in zip(ends, dts))
        print(name, "hold", hold, "courant", courant, "dt", dts, "end bounds", ends, "per-step path:", per_step)
        g.status()
        Y, _ = g.prognostic_and_aux()
        t = _word(case)
        F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, courant, 0.0, nchunks, hold, t.data_ptr(), None), ctx)
        flags = g.status()
    assert per_step == expect
    assert bool(flags & 32) == per_step
    assert not (flags & 4)


# ------------------------------------------------------------------ error paths, the host mirror, a communicator

def test_error_paths_and_the_zero_step_fallback():
    case = pc.make_case("c2_richards_f64", ncols=NCOLS)
    with pc.GpuModel(case) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        t = _word(case)
        assert L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 0, t.data_ptr(), None) == F.LH_EINVAL
        assert L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, -1, 4, t.data_ptr(), None) == F.LH_EINVAL
        assert L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 4, None, None) == F.LH_EINVAL
        assert L.lh_step_ssprk33_adaptive_hold(None, Y, Ya, 0.0, 0.3, 0.0, 1, 4, t.data_ptr(), None) == F.LH_EINVAL
        assert L.lh_adaptive_hold_engine(ctx, 0) == F.LH_EINVAL and L.lh_adaptive_hold_engine(None, 4) == F.LH_EINVAL
        # the longest chunk is 2^20 steps (the header names the range)
        assert L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, 1, (1 << 20) + 1, t.data_ptr(), None) == F.LH_EINVAL
        assert L.lh_adaptive_hold_engine(ctx, (1 << 20) + 1) == F.LH_EINVAL and L.lh_adaptive_hold_engine(ctx, 1 << 20) >= 0
        F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, 0, 4, t.data_ptr(), None), ctx)   # no chunk: nothing happens
        assert np.array_equal(g.download(Y, F.LH_VAR_VARTHETA_L), case.vl)
    # no positive finite bound and no cap (Ksat = 0 under flux boundaries: no positive diffusivity anywhere,
    # the minimum stays +inf): the chunk is taken with dt = 0 and bit 2 is set, as in lh_step_ssprk33_adaptive
    bad = dataclasses.replace(case, om=dataclasses.replace(case.om, vg=dataclasses.replace(case.om.vg, Ksat=0.0)))
    seen = []
    with pc.GpuModel(bad) as g:
        F, L, ctx = g.F, g.L, g.ctx
        for which in range(2):
            Y, Ya = g.prognostic_and_aux()
            t, el = _word(case), _word(case)
            t.fill_(7.0)
            import torch
            torch.cuda.synchronize()
            if which == 0:
                F.check(L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, 0.3, 0.0, 2, t.data_ptr(), el.data_ptr()), ctx)
            else:
                F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.3, 0.0, 2, 4, t.data_ptr(), el.data_ptr()), ctx)
            flags = g.status()
            seen.append((flags & 4, float(t.item()), float(el.item())))
            assert which == 0 or flags & 32       # ... and such a bound after a chunk is an overrun
    assert seen[0] == seen[1] == (4, 0.0, 0.0)


def test_host_mirror_hold_keyword():
    """step_adaptive(hold=4, nsteps=3) is the C call with nchunks = 3; hold=1 is today's step_adaptive."""
    import torch

    import __graft_entry__ as ge
    lh = ge.load_package()
    F, L = lh._ffi, lh._ffi.lib()
    FT, N = np.float64, NCOLS
    hm = lh.vanGenuchten(FT, n=2.0, α=2.6, Ksat=0.0443 / 3600 / 100, θr=0.0)
    c = np.arange(N)[:, None]
    ic = lambda z, m: {"ϑ_l": 0.2 + 0.2 * (1.0 + z) + 0.05 * pc.uhash(c, 3, 7) + 0.0 * z, "θ_i": 0.0 * z}

    def fresh():
        domain = lh.Column(FT, zlim=(-1.0, 0.0), nelements=40, ncolumns=N)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0)),
                             bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0)))
        model = lh.SoilModel(FT, domain=domain, energy_model=lh.PrescribedTemperatureModel(),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm),
                             boundary_conditions=bc, soil_param_set=lh.SoilParams(FT, ν=0.495, S_s=1e-3),
                             earth_param_set=lh.EarthParameterSet())
        return (model,) + tuple(lh.initialize_states(model, ic, 0.0))

    model, Y, Ya = fresh()
    elapsed, dt = lh.step_adaptive(model, Y, Ya, t=0.0, courant=0.3, nsteps=3, hold=4)
    v_mirror = np.array(Y.soil.ϑ_l)
    model.close()
    model, Y, Ya = fresh()
    be = model._backend()
    be.set_bcs(model, 0.0)
    buf = torch.zeros(2, device=torch.device("cuda", be.device_index()), dtype=torch.float64)
    torch.cuda.synchronize()
    ya = Ya.handle if hasattr(Ya, "handle") else None
    F.check(L.lh_step_ssprk33_adaptive_hold(be.ctx, Y.handle, ya, 0.0, 0.3, 0.0, 3, 4, C.c_void_p(buf.data_ptr()),
                                            C.c_void_p(buf.data_ptr() + 8)), be.ctx)
    F.check(L.lh_synchronize(be.ctx), be.ctx)
    assert (elapsed, dt) == (float(buf[1].item()), float(buf[0].item())) and dt > 0 and elapsed > 0
    assert np.array_equal(v_mirror, np.array(Y.soil.ϑ_l))
    model.close()
    # hold = 1 (also the default) is the call as it was
    res = []
    for kw in ({}, {"hold": 1}):
        model, Y, Ya = fresh()
        res.append((lh.step_adaptive(model, Y, Ya, t=0.0, courant=0.3, nsteps=6, **kw), np.array(Y.soil.ϑ_l)))
        model.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
    model, Y, Ya = fresh()
    with pytest.raises(ValueError):
        lh.step_adaptive(model, Y, Ya, nsteps=1, hold=0)
    model.close()


def test_one_rank_communicator_all_reduces_once_per_chunk():
    """With a communicator attached the min all-reduce is enqueued once per chunk (where
    lh_step_ssprk33_adaptive enqueues it once per step): over a one-rank communicator the result is the
    result without one."""
    case = pc.make_case("c2_richards_f64", ncols=NCOLS)
    out = []
    for attach in (False, True):
        with pc.GpuModel(case) as g:
            F, L, ctx = g.F, g.L, g.ctx
            if attach:
                ident = (C.c_ubyte * F.LH_COMM_ID_BYTES)()
                F.check(L.lh_comm_unique_id(ident), None)
                F.check(L.lh_comm_init(ctx, 0, 1, ident), ctx)
            Y, Ya = g.prognostic_and_aux()
            t, el = _word(case), _word(case)
            F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, COURANT, 0.0, 3, 5, t.data_ptr(), el.data_ptr()), ctx)
            F.check(L.lh_synchronize(ctx), ctx)
            out.append((g.download(Y, F.LH_VAR_VARTHETA_L), float(t.item()), float(el.item())))
            if attach:
                F.check(L.lh_comm_destroy(ctx), ctx)
    assert out[0][1:] == out[1][1:] and out[0][1] > 0
    assert np.array_equal(out[0][0], out[1][0])
