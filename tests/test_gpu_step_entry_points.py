"""The stepping entry points of the C ABI as a family: every SSPRK33 entry point takes the same fused
three-stage step, and every stepping call refuses in the same order with the same words.

Characterisation tests of the host-side driver code in lh_api.hip (the stage sequence, the shared
opening of the calls); the refusals all come before any launch."""
import ctypes as C

import numpy as np
import pytest

import case_model as M
import parity_cases as pc

pytestmark = pytest.mark.gpu


def _fields(g, st):
    F, m = g.F, g.case.om.model
    vars_ = {M.MODEL_RICHARDS: (F.LH_VAR_VARTHETA_L, F.LH_VAR_THETA_I), M.MODEL_HEAT: (F.LH_VAR_RHOE_INT,)}.get(
        m, (F.LH_VAR_VARTHETA_L, F.LH_VAR_THETA_I, F.LH_VAR_RHOE_INT))
    return {v: g.download(st, v) for v in vars_}


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _distinct_bcv(case):
    """[1][3][2][2]: the case's boundary values, moved by a different amount in every entry."""
    base = np.zeros((2, 2))
    for (f, comp), (kind, v) in case.om.bc.items():
        base[f, comp] = v
    k = np.arange(1.0, 13.0).reshape(1, 3, 2, 2)
    small = np.array([1e-3, 1e-10])          # energy (K or W/m^2), hydrology (m^3/m^3 or m/s)
    return np.ascontiguousarray(base * (1.0 + 1e-3 * k) + small * k)


@pytest.mark.parametrize("use_bcv", [False, True])
@pytest.mark.parametrize("tune", [b"persist=0,seg=-1", b"persist=0,seg=5"])   # seg=5: U2 is a state of its own
@pytest.mark.parametrize("name,ncols", [("heat_dirichlet_f64", 64), ("c3_coupled_f64", 200)])
def test_every_ssprk33_entry_point_takes_the_same_fused_step(name, ncols, tune, use_bcv):
    """One step by lh_step_ssprk33, by three lh_ssprk33_stage calls and by lh_step_ssprk33_device_dt: the
    same bits in every prognostic plane, with the context's boundary values and with per-stage ones."""
    import torch
    case = pc.make_case(name, ncols=ncols)
    bcv = _distinct_bcv(case) if use_bcv else None
    tdtype = torch.float64 if case.dtype == np.float64 else torch.float32

    def route(step):
        with pc.GpuModel(case) as g:
            g.F.check(g.L.lh_set_tuning(g.ctx, tune), g.ctx)
            Y, Ya = g.prognostic_and_aux()
            out = C.c_double()
            g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, 0.5, C.byref(out)), g.ctx)
            dt = float(case.dtype(out.value))     # in FT: the by-value and the device-word routes see one number
            step(g, Y, Ya, dt)
            res = _fields(g, Y)
            assert g.status() == 0
            return dt, res

    def by_stepper(g, Y, Ya, dt):
        g.F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, dt, 1, _dp(bcv)), g.ctx)

    def by_stages(g, Y, Ya, dt):
        U = g.state({M.MODEL_HEAT: 0b0100}.get(case.om.model, 0b0101))   # the stage state: no theta_i plane
        for stage in (1, 2, 3):
            g.F.check(g.L.lh_ssprk33_stage(g.ctx, stage, Y, U, Ya, dt, _dp(bcv[0, stage - 1]) if use_bcv else None),
                      g.ctx)

    def by_device_dt(g, Y, Ya, dt):
        word = torch.full((1,), dt, device="cuda", dtype=tdtype)
        torch.cuda.synchronize()              # (written on torch's stream, read on the library's)
        g.F.check(g.L.lh_step_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, C.c_void_p(word.data_ptr()), _dp(bcv)), g.ctx)
        g.F.check(g.L.lh_synchronize(g.ctx), g.ctx)

    dt0, ref = route(by_stepper)
    assert dt0 > 0
    for other in (by_stages, by_device_dt):
        dt, got = route(other)
        assert dt == dt0
        for v in ref:
            np.testing.assert_array_equal(got[v], ref[v], err_msg=f"{name} {tune.decode()} {other.__name__} var {v}")


# ---- refusals: 8 columns x 4 levels, every call wrong in two ways at once, the first refusal asserted

NCOLS, NLEV = 8, 4
FREE_DRAINAGE_TEXT = "FreeDrainage is a hydrology boundary condition (top energy)"
Y_TEXT = "Y state lacks a required variable (has mask 0x1, needs 0x%x)"


def _ctx(model, broken=False, viscosity=False):
    """A small context; broken: a boundary condition validate_model refuses (LH_EMODEL)."""
    energy = None if model == M.MODEL_RICHARDS else 0.0
    hydrology = None if model == M.MODEL_HEAT else 0.0
    bc = pc._flux_bcs(energy=energy, hydrology=hydrology)
    if broken:
        bc[(M.FACE_TOP, M.COMP_ENERGY)] = (M.BC_FREE_DRAINAGE, 0.0)
    om = M.CaseModel(model, NLEV, -0.4, 0.0, bc=bc, cf=M.default_cf(viscosity=viscosity))
    return pc.GpuModel(pc.Case("refusals", om, np.float64, NCOLS))


def _refused(g, rc, want_rc, want_text):
    text = g.L.lh_last_error(g.ctx)
    assert (rc, text.decode() if text else None) == (want_rc, want_text)


def _explicit_calls():
    """name -> (call(g, Y, Ya, bad_args), the text of its argument refusal)"""
    import torch
    word = torch.zeros(2, device="cuda", dtype=torch.float64)
    torch.cuda.synchronize()
    p0, p1 = C.c_void_p(word.data_ptr()), C.c_void_p(word.data_ptr() + 8)

    def ssprk33(g, Y, Ya, bad):
        return g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, 0.0 if bad else 1.0, 1, None)

    def device_dt(g, Y, Ya, bad):
        return g.L.lh_step_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, None if bad else p0, None)

    def adaptive(g, Y, Ya, bad):
        return g.L.lh_step_ssprk33_adaptive(g.ctx, Y, Ya, 0.0, 0.0 if bad else 0.5, 0.0, 1, p0, p1)

    def adaptive_hold(g, Y, Ya, bad):
        return g.L.lh_step_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.5, 0.0, 1, 0 if bad else 4, p0, p1)

    return {
        "lh_step_ssprk33": (ssprk33, "lh_step_ssprk33: need nsteps >= 0 and dt > 0"),
        "lh_step_ssprk33_device_dt": (device_dt, "lh_step_ssprk33_device_dt: NULL argument"),
        "lh_step_ssprk33_adaptive": (adaptive, "lh_step_ssprk33_adaptive: need nsteps >= 0 and courant > 0"),
        "lh_step_ssprk33_adaptive_hold": (adaptive_hold, "lh_step_ssprk33_adaptive_hold: need nchunks >= 0, "
                                                         "1 <= hold <= 1048576 and courant > 0"),
    }, word


@pytest.mark.parametrize("entry", ["lh_step_ssprk33", "lh_step_ssprk33_device_dt", "lh_step_ssprk33_adaptive",
                                   "lh_step_ssprk33_adaptive_hold"])
def test_explicit_stepping_calls_refuse_in_order(entry):
    F = pc._pkg()._ffi
    calls, keep = _explicit_calls()
    call, arg_text = calls[entry]
    with _ctx(M.MODEL_RICHARDS) as g:                       # a bad argument and a bad Y: the argument
        _refused(g, call(g, g.state(0b0001), None, True), F.LH_EINVAL, arg_text)
    with _ctx(M.MODEL_RICHARDS, broken=True) as g:          # a refused model and a bad Y: the model
        _refused(g, call(g, g.state(0b0001), None, False), F.LH_EMODEL, FREE_DRAINAGE_TEXT)
    with _ctx(M.MODEL_HEAT) as g:                           # a bad Y and no Ya: Y
        _refused(g, call(g, g.state(0b0001), None, False), F.LH_ESTATE, Y_TEXT % 0x4)
        # a Ya of another context and of the wrong planes: the context
        with _ctx(M.MODEL_HEAT) as g2:
            _refused(g, call(g, g.state(0), g2.state(0b0100), False), F.LH_EINVAL, "Ya state belongs to another context")
        _refused(g, call(g, g.state(0), None, False), F.LH_ESTATE, "Ya state is NULL but the model reads it")
    del keep


def test_implicit_euler_refuses_in_order():
    F = pc._pkg()._ffi
    who = "lh_step_implicit_euler"

    def call(g, Y, dt=1.0):
        return g.L.lh_step_implicit_euler(g.ctx, Y, None, 0.0, dt, 1, None, 0.0, 0)

    with _ctx(M.MODEL_HEAT) as g:
        _refused(g, call(g, g.state(0b0001), dt=0.0), F.LH_EINVAL, who + ": need nsteps >= 0 and dt > 0")
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL,
                 who + ": Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)")
    with _ctx(M.MODEL_RICHARDS, broken=True, viscosity=True) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL,
                 who + ": conductivity factors other than NoEffect are not supported")
    with _ctx(M.MODEL_RICHARDS, broken=True) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL, FREE_DRAINAGE_TEXT)
    with _ctx(M.MODEL_RICHARDS) as g:
        with _ctx(M.MODEL_RICHARDS) as g2:                  # a Y of another context that also lacks a plane
            _refused(g, call(g, g2.state(0b0001)), F.LH_EINVAL, "Y state belongs to another context")
        _refused(g, call(g, g.state(0b0001)), F.LH_ESTATE, Y_TEXT % 0x3)


def test_trbdf2_refuses_in_order():
    F = pc._pkg()._ffi
    who = "lh_integrate_trbdf2"

    def call(g, Y, t0=0.0, dt=1.0, reltol=0.0, flags=0):
        return g.L.lh_integrate_trbdf2(g.ctx, Y, None, t0, 1.0, dt, 0.0, reltol, flags, None, None)

    with _ctx(M.MODEL_HEAT) as g:
        Y = g.state(0b0001)
        _refused(g, call(g, Y, t0=float("nan"), dt=0.0), F.LH_EINVAL, who + ": need finite t0 <= t1")
        _refused(g, call(g, Y, dt=0.0, reltol=-1.0), F.LH_EINVAL, who + ": need a finite dt > 0")
        _refused(g, call(g, Y, reltol=-1.0, flags=0x8), F.LH_EINVAL, who + ": tolerances must be finite and >= 0")
        _refused(g, call(g, Y, flags=0x8), F.LH_EINVAL, who + ": unknown flags 0x8")
        _refused(g, call(g, Y), F.LH_EMODEL,
                 who + ": Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)")
    with _ctx(M.MODEL_RICHARDS, broken=True, viscosity=True) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL,
                 who + ": conductivity factors other than NoEffect are not supported")
    with _ctx(M.MODEL_RICHARDS, broken=True) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL, FREE_DRAINAGE_TEXT)
    with _ctx(M.MODEL_RICHARDS) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_ESTATE, Y_TEXT % 0x3)


def test_heat_implicit_refuses_in_order():
    F = pc._pkg()._ffi
    who = "lh_step_heat_implicit"

    def call(g, Y, Ya=None, nsteps=1, flags=0):
        return g.L.lh_step_heat_implicit(g.ctx, Y, Ya, 0.0, 1.0, nsteps, flags, None)

    with _ctx(M.MODEL_RICHARDS) as g:
        Y = g.state(0b0001)
        _refused(g, call(g, Y, nsteps=-1, flags=0x8), F.LH_EINVAL, who + ": need nsteps >= 0 and a finite dt > 0")
        _refused(g, call(g, Y, flags=0x8), F.LH_EINVAL, who + ": unknown flags 0x8")
        _refused(g, call(g, Y), F.LH_EMODEL,
                 who + ": heat-only models (SoilEnergyModel + PrescribedHydrologyModel)")
    with _ctx(M.MODEL_HEAT, broken=True) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_EMODEL, FREE_DRAINAGE_TEXT)
    with _ctx(M.MODEL_HEAT) as g:
        _refused(g, call(g, g.state(0b0001)), F.LH_ESTATE, Y_TEXT % 0x4)
        # the states are checked before a call of no steps returns
        _refused(g, call(g, g.state(0b0001), nsteps=0), F.LH_ESTATE, Y_TEXT % 0x4)
        _refused(g, call(g, g.state(0), nsteps=0), F.LH_ESTATE, "Ya state is NULL but the model reads it")
        assert call(g, g.state(0), g.state(0b0011), nsteps=0) == F.LH_OK
