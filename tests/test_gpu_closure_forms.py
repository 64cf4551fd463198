"""The v_ldexp (clay-like, VGF = false) form of the Float64 water kernels, on every entry point.

Two legs.  A: the form FORCED (`vgfast=0`) on the project's ordinary, well-conditioned cases, where the
tolerance model of tests/parity_cases.py and its plain statistic have teeth -- the same assertions and
bounds as the tests of the default form.  B: true clay-like parameters (n in [1.03, 1.07]), where the host
must choose the form itself, on moist states for which the reference alone is well conditioned
(tests/clay_cases.py, asserted on the CPU by tests/test_clay_cases_cpu.py), plus the bone-dry behaviour
the form exists for and the edges of the host's interval test.

Every test asserts lh_closure_form, so that a test that silently runs the other form fails.  Run with -s
for the use of the tolerance model (profiles/closure_forms_tolerance_use.txt).
"""
import ctypes as C

import numpy as np
import pytest

import case_model as M
import clay_cases as cc
import closure_form as CF
import coupled_implicit_ref as CR
import implicit_ref as IR
import layered_implicit_ref as LI
import parity_cases as pc
import trbdf2_ref as TR
# the default form's tests: their case lists, constants, helpers and, under the ldexp_form fixture, themselves
import test_gpu_adaptive_hold as TA
import test_gpu_boundary_fluxes as TB
import test_gpu_coupled_implicit as TCI
import test_gpu_coupled_trbdf2 as TCT
import test_gpu_implicit as TI
import test_gpu_layered as TL
import test_gpu_layered_implicit as TLI
import test_gpu_parity as TP
import test_gpu_stepper as TS
import test_gpu_trbdf2 as TT
from closure_form import host_chosen_ldexp_form, ldexp_form  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
O = pc.O


def _water_f64(names):
    def keep(name):
        return "f32" not in name and not name.startswith("heat")
    return [n for n in names if keep(n)]


RHS_NAMES = _water_f64(TP.CASES)
DIAG_NAMES = ["c2_richards_f64", "mixed_factors_f64", "c5_percol_f64"]   # test_closures_match_oracle's Float64 cases


class Ctx(pc.GpuModel):
    """A context with a tuning string, whose closure form is asserted before anything is launched."""

    def __init__(self, case, tune=None, want=None, math_mode=None):
        super().__init__(case, math_mode)
        if tune is not None:
            self.F.check(self.L.lh_set_tuning(self.ctx, tune), self.ctx)
        if want is not None:
            assert self.L.lh_closure_form(self.ctx) == want, (case.name, tune, self.L.lh_closure_form(self.ctx), want)


def gpu_rhs(case, tune, want, check_status=True):
    with Ctx(case, tune, want) as g:
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        out = g.tendencies(dY)
        status = g.status()
    if check_status:
        assert status == 0, "non-finite tendency flagged"
        return out
    return out, status


def gpu_diag(case, tune, want):
    with Ctx(case, tune, want) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        D = g.state(0b1111)
        F.check(g.L.lh_diagnostics(g.ctx, Y, Ya, D), g.ctx)
        out = dict(K=g.download(D, F.LH_DIAG_K), psi=g.download(D, F.LH_DIAG_PSI),
                   kappa=g.download(D, F.LH_DIAG_KAPPA), T=g.download(D, F.LH_DIAG_T))
        return out, g.status()


def diag_keys(case):
    return ("K", "psi") if case.om.model == M.MODEL_RICHARDS else ("K", "psi", "T", "kappa")


def closure_use(case, got, want, Cw):
    """{field: worst |got - want| / tolerance} against closure_tolerances at Cw."""
    tol = pc.closure_tolerances(case, want, Cw)
    return {k: float(np.max(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)) / tol[k]))
            for k in diag_keys(case)}


def fmt(d):
    return " ".join(f"{k}={v:.3g}" for k, v in d.items())


# =============================================================== A. the forced form on the ordinary cases

@pytest.mark.parametrize("name", RHS_NAMES)
def test_forced_rhs_matches_oracle(name):
    """A1: lh_rhs under vgfast=0, exactly as test_gpu_parity.test_rhs_matches_oracle (Cw = 2, plain statistic)."""
    case = pc.make_case(name)
    want = pc.run_oracle_rhs(case)
    got = gpu_rhs(case, b"vgfast=0", CF.LDEXP)
    ref = gpu_rhs(case, None, CF.INTEGER_EXPONENT)
    print(f"A1 {name}: use of the model at Cw=4: ldexp {fmt(pc.error_summary(case, got, want, 4.0))} | "
          f"integer {fmt(pc.error_summary(case, ref, want, 4.0))} | plain share ldexp {fmt(pc.plain_statistic(case, got, want))}")
    pc.assert_tendencies_close(case, got, want, TP.CW, label="[vgfast=0]", plain=True)


@pytest.mark.parametrize("name", DIAG_NAMES)
def test_forced_closures_match_oracle_and_the_default_form(name):
    """A2: each form inside closure_tolerances at Cw = 2; between the forms psi, T and kappa bit for bit (the two
    2^(.) forms agree bit for bit on normal results, lh_closures.hpp: one kernel, a run-time flag) -- K may differ
    by the rounded product of ex2_prod, which the oracle bound covers; the same status."""
    case = pc.make_case(name)
    want = O.diagnostics(case.om, case.vl, case.ti, case.rhoe, case.T_aux)
    a, sa = gpu_diag(case, b"vgfast=0", CF.LDEXP)
    b, sb = gpu_diag(case, None, CF.INTEGER_EXPONENT)
    ua, ub = closure_use(case, a, want, TP.CW), closure_use(case, b, want, TP.CW)
    nK = int(np.sum(a["K"] != b["K"]))
    print(f"A2 {name}: use at Cw=2: ldexp {fmt(ua)} | integer {fmt(ub)} | K differs in {nK} of {a['K'].size} cells")
    assert sa == sb
    for u in (ua, ub):
        assert all(v <= 1.0 for v in u.values()), u
    for k in ("psi", "T", "kappa"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")


@pytest.mark.parametrize("name", _water_f64(TB.CASES))
def test_forced_boundary_fluxes(name, ldexp_form):
    """A3: the assertions and bounds of test_boundary_fluxes_match_the_oracle, every context under vgfast=0."""
    TB.test_boundary_fluxes_match_the_oracle(name)


def test_forced_stable_dt_and_device_dt_stepping(ldexp_form):
    """A3: test_stable_dt_matches_oracle_and_device_dt_stepping under vgfast=0 (its Float32 and heat cases have
    one form only and run as they are)."""
    TS.test_stable_dt_matches_oracle_and_device_dt_stepping()


@pytest.mark.parametrize("name", ["c2_richards_f64", "c3_coupled_f64", "mixed_smooth_f64", "c1_dirichlet_f64",
                                  "c5_percol_f64", "richards_viscosity_f64", "single_cell_f64"])
def test_forced_fused_rhs_stable_dt(name, ldexp_form):
    """A3: lh_rhs_stable_dt (rhs_kernel mode 4) under vgfast=0, the assertions of test_fused_rhs_stable_dt."""
    TS.test_fused_rhs_stable_dt(name)


ENGINES = [b"vgfast=0,persist=0,seg=-1", b"vgfast=0,persist=2"]


def gpu_steps(case, dt, nsteps, tune, want_form, engine=None):
    with Ctx(case, tune, want_form) as g:
        F = g.F
        if engine is not None:
            assert g.L.lh_step_engine(g.ctx, nsteps, 0) == engine
        Y, Ya = g.prognostic_and_aux()
        F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, dt, nsteps, None), g.ctx)
        out = {"vl": g.download(Y, F.LH_VAR_VARTHETA_L), "ti": g.download(Y, F.LH_VAR_THETA_I)}
        if case.om.model == M.MODEL_COUPLED:
            out["rhoe"] = g.download(Y, F.LH_VAR_RHOE_INT)
        return out, g.status()


@pytest.mark.parametrize("model", [M.MODEL_COUPLED, M.MODEL_RICHARDS], ids=["coupled", "richards"])
def test_forced_engines_are_bitwise_equal_on_random_states(model):
    """A4: test_randomised_states_step_bitwise_equal_in_both_engines in the v_ldexp form: three steps of the
    random ensembles by the fused stages (unsegmented, and as the host segments them) and by the persistent
    stepper give the same bits, NaNs and status."""
    import test_gpu_fuzz  # noqa: F401  (puts tools/ on the path)
    import fuzz_closures
    F = pc._pkg()._ffi
    for factors in (False, True):
        for percol in (False, True):
            case = fuzz_closures.fuzz_case(9007, np.float64, factors, percol, model)
            res = [gpu_steps(case, 1e-4, 3, tune, CF.LDEXP, eng) for tune, eng in
                   ((ENGINES[0], F.LH_ENGINE_FUSED_STAGES), (ENGINES[1], F.LH_ENGINE_COLUMN_STEPPER),
                    (b"vgfast=0,persist=0", F.LH_ENGINE_FUSED_STAGES))]
            for other in res[1:]:
                assert res[0][1] == other[1], (model, factors, percol)
                for k in res[0][0]:
                    np.testing.assert_array_equal(res[0][0][k], other[0][k], err_msg=f"{model} {factors} {percol} {k}")


@pytest.mark.parametrize("name", ["c2_richards_f64_n16", "c2_richards_f64_n96", "c2_richards_f64_n130", "c3_coupled_f64"])
def test_forced_theta_zt_matches_oracle(name):
    """A4: theta(z, t) after 20 steps against the oracle's SSPRK33, 1e-11 of the field scale, in both engines
    (16, 96, 130 levels: one and two cells per lane of the wave stepper, one thread per cell)."""
    F = pc._pkg()._ffi
    case = pc.make_case(name, ncols=67)
    dt = TS.stable_dt(case)
    want = TS.cpu_steps(case, dt, 20)
    for tune, eng in zip(ENGINES, (F.LH_ENGINE_FUSED_STAGES, F.LH_ENGINE_COLUMN_STEPPER)):
        got, status = gpu_steps(case, dt, 20, tune, CF.LDEXP, eng)
        assert status == 0
        err = {k: float(np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k]))) for k in want if k != "ti"}
        print(f"A4 {name} {tune.decode()}: theta(z,t) error / field scale {fmt(err)}")
        TS.assert_state_close(case, got, want, 1e-11)
    assert np.max(np.abs(want["vl"] - case.vl)) > 0




@pytest.mark.parametrize("tune", [b"vgfast=0", b"vgfast=0,persist=0"], ids=["stepper", "fused"])
@pytest.mark.parametrize("name", ["c2_richards_f64_n16", "c2_richards_f64_n96", "c2_richards_f64_n130", "c3_coupled_f64"])
def test_forced_adaptive_entry_points_end_on_the_reference_sequence(name, tune):
    """A4: lh_step_ssprk33_adaptive_hold (hold = 4) ends on the bits of its defining call sequence
    (test_gpu_adaptive_hold.reference_sequence), and hold = 1 on those of lh_step_ssprk33_adaptive -- the
    equalities between entry points that hold in the default form, in the v_ldexp form."""
    case = pc.make_case(name, ncols=67)
    hold, nchunks = 4, 3
    with Ctx(case, tune, CF.LDEXP) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Yr, Ya = g.prognostic_and_aux()
        dts, elapsed = TA.reference_sequence(g, Yr, Ya, TA.COURANT, 0.0, nchunks, hold)
        want = TA._prognostic(g, Yr)
        Y1, _ = g.prognostic_and_aux()
        t, el = TA._word(case), TA._word(case)
        F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y1, Ya, 0.0, TA.COURANT, 0.0, nchunks, hold, t.data_ptr(), el.data_ptr()), ctx)
        F.check(L.lh_synchronize(ctx), ctx)
        got = TA._prognostic(g, Y1)
        assert float(t.item()) == dts[-1] and float(el.item()) == elapsed and all(d > 0 for d in dts)
        for k in want:
            assert np.array_equal(want[k], got[k]), (name, k)
            assert not np.array_equal(want[k], getattr(case, k)), "the state never moved"
        out = []
        for which in range(2):
            Y, _ = g.prognostic_and_aux()
            t, el = TA._word(case), TA._word(case)
            if which == 0:
                F.check(L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, TA.COURANT, 0.0, 5, t.data_ptr(), el.data_ptr()), ctx)
            else:
                F.check(L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, TA.COURANT, 0.0, 5, 1, t.data_ptr(), el.data_ptr()), ctx)
            F.check(L.lh_synchronize(ctx), ctx)
            out.append((TA._prognostic(g, Y), float(t.item()), float(el.item())))
        assert out[0][1:] == out[1][1:] and out[0][1] > 0
        for k in out[0][0]:
            assert np.array_equal(out[0][0][k], out[1][0][k]), (name, k)
        assert g.L.lh_closure_form(ctx) == CF.LDEXP and not (g.status() & 4)


@pytest.mark.parametrize("name", ["c2_richards_f32", "heat_dirichlet_f64"])
def test_forced_form_does_not_apply_to_float32_and_heat(name):
    """A5: one form only -- lh_closure_form says so, and vgfast=0 leaves lh_rhs bitwise unchanged."""
    case = pc.make_case(name)
    a = gpu_rhs(case, None, CF.NOT_APPLICABLE)
    b = gpu_rhs(case, b"vgfast=0", CF.NOT_APPLICABLE)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
    F = pc._pkg()._ffi
    with Ctx(pc.make_case("c2_richards_f64", ncols=8), b"vgfast=0", CF.NOT_APPLICABLE, math_mode=F.LH_MATH_LIBM):
        pass                                   # LH_MATH_LIBM has one form, too
    assert F.lib().lh_closure_form(None) == F.LH_EINVAL


# =============================================================== B. clay-like ensembles: the host decides

def _id(spec):
    return "-".join(str(x) for x in spec)


@pytest.mark.parametrize("spec", cc.RHS_CASES, ids=_id)
def test_clay_rhs_and_closures_match_oracle(spec):
    """B1: five variants x two models, 200 x 16, the host's own decision; Cw = 4 (the randomised test's constant)
    with NO masked cell, status 0, the plain statistic with the project's floors."""
    case = cc.clay_case(*spec)
    want = pc.run_oracle_rhs(case)
    got = gpu_rhs(case, None, CF.LDEXP)
    dwant = O.diagnostics(case.om, case.vl, case.ti, case.rhoe, case.T_aux)
    dgot, status = gpu_diag(case, None, CF.LDEXP)
    use = closure_use(case, dgot, dwant, 4.0)
    print(f"B1 {case.name}: use at Cw=4: tendencies {fmt(pc.error_summary(case, got, want, 4.0))} | closures {fmt(use)} | "
          f"plain share {fmt(pc.plain_statistic(case, got, want))}")
    assert status == 0
    for k in diag_keys(case):
        assert np.all(np.isfinite(dgot[k])), k
    assert all(v <= 1.0 for v in use.values()), use
    pc.assert_tendencies_close(case, got, want, 4.0, label="[clay]", plain=True)


@pytest.mark.parametrize("model", cc.MODELS, ids=["richards", "coupled"])
def test_clay_decision_reaches_every_column_and_columns_stay_independent(model):
    """B2: two clay columns (17 and ncols - 3) among ordinary ones switch the whole launch: the ordinary columns
    are bitwise what they give, without the two, under vgfast=0; the two are bitwise what they give alone."""
    full = cc.clay_case(model, "mixed", 200, 16, cc.SEED)
    clay = list(cc.mixed_clay_columns(full.ncols))
    rest = [c for c in range(full.ncols) if c not in clay]
    a = gpu_rhs(full, None, CF.LDEXP)
    with Ctx(cc.take_columns(full, rest), None, CF.INTEGER_EXPONENT):
        pass                                   # (without the two, the host chooses the other form)
    b = gpu_rhs(cc.take_columns(full, rest), b"vgfast=0", CF.LDEXP)
    c = gpu_rhs(cc.take_columns(full, clay), None, CF.LDEXP)
    for k in a:
        np.testing.assert_array_equal(a[k][rest], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k][clay], c[k], err_msg=k)


@pytest.mark.parametrize("spec", cc.STEP_CASES, ids=_id)
def test_clay_steppers_and_step_bound(spec):
    """B3: 67 columns at 16, 96 and 130 levels (the three stepper kernels), dt = lh_stable_dt at Courant 0.5,
    20 steps: both engines bitwise equal, theta(z, t) within 1e-11 of the field scale of the oracle's SSPRK33,
    lh_stable_dt within 1e-6 of the oracle's."""
    F = pc._pkg()._ffi
    case = cc.clay_case(*spec)
    want_dt = O.stable_dt(case.om, case.vl, case.ti, case.rhoe, cc.STEP_COURANT, case.T_aux)
    with Ctx(case, None, CF.LDEXP) as g:
        Y, Ya = g.prognostic_and_aux()
        out = C.c_double()
        g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, cc.STEP_COURANT, C.byref(out)), g.ctx)
        dt = out.value
    assert abs(dt - want_dt) <= 1e-6 * want_dt, (dt, want_dt)
    want = TS.cpu_steps(case, dt, cc.STEP_COUNT)
    res = []
    for tune, eng in ((b"persist=0,seg=-1", F.LH_ENGINE_FUSED_STAGES), (b"persist=2", F.LH_ENGINE_COLUMN_STEPPER)):
        got, status = gpu_steps(case, dt, cc.STEP_COUNT, tune, CF.LDEXP, eng)
        assert status == 0
        res.append(got)
        err = {k: float(np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k]))) for k in want if k != "ti"}
        print(f"B3 {case.name} {tune.decode()}: theta(z,t) error / field scale {fmt(err)}; lh_stable_dt rel. error "
              f"{abs(dt - want_dt) / want_dt:.3g}")
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)
    for got in res:
        TS.assert_state_close(case, got, want, cc.STEP_BOUND)


@pytest.mark.parametrize("moist", [0, 46], ids=["alone", "among_moist_columns"])
def test_bone_dry_clay_saturates(moist):
    """B4: n in {1.03, 1.05, 1.07} x S in {1e-15 ... 0.1}, whole columns at that S -- what the v_ldexp form exists
    for (the integer-exponent form would leave the normal range and return garbage).  K is exactly 0 wherever the
    oracle's is; psi is inside closure_tolerances at Cw = 4 where the oracle's is finite; where the oracle's psi is
    -Inf because S^(-1/m) overflowed, the device may return the finite log-domain value (2^(x/n) has no such
    intermediate) or -Inf: exactly that case is masked (deviations).  Non-finite tendencies
    only where the oracle's are non-finite; the status flag says what the device returned; the moist columns are
    bitwise what they are without the dry ones."""
    case, nd = cc.dry_clay_columns(moist=moist)
    want = O.diagnostics(case.om, case.vl, case.ti)
    got, _ = gpu_diag(case, None, CF.LDEXP)
    assert nd == 18 and np.all(want["K"][:nd] == 0.0)
    assert np.all(got["K"][want["K"] == 0.0] == 0.0)
    tol = pc.closure_tolerances(case, want, 4.0)
    wpsi, gpsi = want["psi"], got["psi"]
    fin = np.isfinite(wpsi)
    overflow = np.isneginf(wpsi)
    assert np.all(fin | overflow) and overflow[:nd].any() and not overflow[nd:].any()
    assert np.all(np.isfinite(gpsi[fin]))
    with np.errstate(all="ignore"):
        use = np.where(fin, np.abs(gpsi - wpsi) / tol["psi"], 0.0)
    assert np.all((np.isfinite(gpsi) & (gpsi < 0)) | np.isneginf(gpsi) | ~overflow), "psi where the reference overflowed"
    kfin = np.isfinite(want["K"])
    useK = float(np.max(np.abs(got["K"] - want["K"])[kfin] / tol["K"][kfin]))
    print(f"B4 {case.name}: psi use at Cw=4 {use.max():.3g} (dry columns {use[:nd].max():.3g}), K use {useK:.3g}; the reference's psi "
          f"overflowed in {int(overflow.sum())} cells, the device's is finite in {int((overflow & np.isfinite(gpsi)).sum())} of them "
          f"(largest |psi| {np.abs(gpsi[np.isfinite(gpsi)]).max():.3g})")
    assert use.max() <= 1.0 and useK <= 1.0
    # the tendency
    twant = pc.run_oracle_rhs(case)
    tgot, status = gpu_rhs(case, None, CF.LDEXP, check_status=False)
    bad_w, bad_g = ~np.isfinite(twant["vl"]), ~np.isfinite(tgot["vl"])
    assert not np.any(bad_g & ~bad_w), "a non-finite tendency where the reference's is finite"
    # finite where the reference has NaN: only in columns whose psi is the masked overflow
    cols = np.flatnonzero((bad_w & ~bad_g).any(axis=1))
    assert all(overflow[c].any() and np.isfinite(gpsi[c]).all() for c in cols), cols
    print(f"B4 {case.name}: tendencies finite on the device where the reference has NaN (its psi overflowed): columns "
          f"{[(float(case.om.percol['vg_n'][c]), float(case.vl[c, 0] / case.om.soil.nu)) for c in cols]} as (n, S)")
    assert (status & 1) == int(bad_g.any()), (status, int(bad_g.sum()))
    assert np.all(tgot["ti"] == 0)
    ok = ~bad_w & ~bad_g
    tolt = pc.tendency_tolerance(case, 4.0)["vl"]
    with np.errstate(all="ignore"):
        allowed = tolt + 4.0 * float(np.finfo(np.float64).eps) * np.abs(twant["vl"])
        assert np.all(np.abs(tgot["vl"] - twant["vl"])[ok] <= allowed[ok])
    if moist:
        rest = list(range(nd, case.ncols))
        alone = gpu_rhs(cc.take_columns(case, rest), b"vgfast=0", CF.LDEXP)
        np.testing.assert_array_equal(tgot["vl"][rest], alone["vl"])
        assert np.all(np.isfinite(alone["vl"]))


def _uniform_ctx(n=1.56, alpha=3.6, theta_r=0.0, nu=0.43, ncols=8, nlev=4):
    om = M.CaseModel(M.MODEL_RICHARDS, nlev, -0.05 * nlev, 0.0, soil=M.default_soil(nu=nu),
                     vg=M.default_vg(n=n, alpha=alpha, theta_r=theta_r), bc=pc._flux_bcs(hydrology=0.0))
    S = 0.5 + 0.6 * pc.uhash(np.arange(ncols)[:, None], np.arange(nlev)[None, :], 1000)      # [0.5, 1.1)
    vl = theta_r + (nu - theta_r) * S
    return pc.Case("edge", om, np.float64, ncols, vl=vl, ti=np.zeros((ncols, nlev)))


M_EDGE = 0.07 * 1.001
N_OF_M = lambda m: 1.0 / (1.0 - m)   # noqa: E731
EDGES = [
    # (keyword arguments of the uniform context, the form the host must choose)
    (dict(n=N_OF_M(M_EDGE * (1 + 1e-6))), CF.INTEGER_EXPONENT),
    (dict(n=N_OF_M(M_EDGE * (1 - 1e-6))), CF.LDEXP),
    (dict(nu=1.01e-5 * (1 + 1e-6)), CF.INTEGER_EXPONENT),
    (dict(nu=1.01e-5 * (1 - 1e-6)), CF.LDEXP),
    (dict(nu=1.0 * (1 - 1e-6)), CF.INTEGER_EXPONENT),
    (dict(nu=1.0 * (1 + 1e-6)), CF.LDEXP),
    (dict(alpha=1.01e-20 * (1 + 1e-6)), CF.INTEGER_EXPONENT),
    (dict(alpha=1.01e-20 * (1 - 1e-6)), CF.LDEXP),
    (dict(alpha=0.99e20 * (1 - 1e-6)), CF.INTEGER_EXPONENT),
    (dict(alpha=0.99e20 * (1 + 1e-6)), CF.LDEXP),
]


def test_interval_test_edges():
    """B5: the host's interval test, one uniform context per row (nothing is launched on these), then the ways
    the decision moves: a NaN in a per-column n, removing the array, a class table with and without its map,
    and vgfast=0 over everything."""
    for kw, want in EDGES:
        with Ctx(_uniform_ctx(**kw), None, want) as g:
            g.F.check(g.L.lh_set_tuning(g.ctx, b"vgfast=0"), g.ctx)
            assert g.L.lh_closure_form(g.ctx) == CF.LDEXP, kw
            g.F.check(g.L.lh_set_tuning(g.ctx, b""), g.ctx)
            assert g.L.lh_closure_form(g.ctx) == want, kw
    case = _uniform_ctx()
    with Ctx(case, None, CF.INTEGER_EXPONENT) as g:
        F, L, ctx = g.F, g.L, g.ctx
        form = lambda: L.lh_closure_form(ctx)   # noqa: E731
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        arr = np.full(case.ncols, 2.0)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["vg_n"], dp(arr)), ctx)
        assert form() == CF.INTEGER_EXPONENT
        arr[5] = np.nan
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["vg_n"], dp(arr)), ctx)
        assert form() == CF.LDEXP                                   # every comparison is false for a NaN
        arr[5] = 1.05
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["vg_n"], dp(arr)), ctx)
        assert form() == CF.LDEXP
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["vg_n"], None), ctx)
        assert form() == CF.INTEGER_EXPONENT                        # the scalar decision again
        # 16 classes, one of them clay: the table alone decides nothing, the map does
        classes = [(1.3 + 0.1 * k, 3.6, 0.0, 2.9e-7, 0.43, 1e-3) for k in range(16)]
        classes[11] = (1.05,) + classes[11][1:]
        g.set_soil_classes(classes)
        assert form() == CF.INTEGER_EXPONENT
        g.set_soil_class_map(np.arange(case.om.nlev) % 16)
        assert form() == CF.LDEXP
        classes[11] = (1.4,) + classes[11][1:]
        g.set_soil_classes(classes)
        assert form() == CF.INTEGER_EXPONENT
        F.check(L.lh_set_tuning(ctx, b"vgfast=0"), ctx)
        assert form() == CF.LDEXP
        F.check(L.lh_set_tuning(ctx, b"vgfast=1"), ctx)
        assert form() == CF.INTEGER_EXPONENT
        classes[11] = (1.05,) + classes[11][1:]
        g.set_soil_classes(classes)
        assert form() == CF.LDEXP
        g.set_soil_class_map(None)
        assert form() == CF.INTEGER_EXPONENT


def test_both_sides_of_the_m_edge_match_the_oracle():
    """B5: moist states (S in [0.5, 1.1]) with n a relative 1e-6 of m on either side of the edge: each side, in
    the form the host chooses for it, matches the oracle at Cw = 4; and at the edge the two forms give the same
    psi bit for bit -- compared on the upper side's n, which both forms can run (the two sides' n differ by
    1e-6 of m, far more than a rounding, so their psi cannot be compared with each other)."""
    for sign, want_form in ((+1, CF.INTEGER_EXPONENT), (-1, CF.LDEXP)):
        case = _uniform_ctx(n=N_OF_M(M_EDGE * (1 + sign * 1e-6)), ncols=200, nlev=16)
        want = pc.run_oracle_rhs(case)
        got = gpu_rhs(case, None, want_form)
        dwant = O.diagnostics(case.om, case.vl, case.ti)
        dgot, status = gpu_diag(case, None, want_form)
        use = closure_use(case, dgot, dwant, 4.0)
        print(f"B5 m = 0.07007 (1 {'+' if sign > 0 else '-'} 1e-6): use at Cw=4: tendencies {fmt(pc.error_summary(case, got, want, 4.0))} | closures {fmt(use)}")
        assert status == 0 and all(v <= 1.0 for v in use.values()), use
        pc.assert_tendencies_close(case, got, want, 4.0, label="[m edge]", plain=True)
        if sign > 0:
            forced, _ = gpu_diag(case, b"vgfast=0", CF.LDEXP)
            np.testing.assert_array_equal(forced["psi"], dgot["psi"])


# =============================================================== the implicit and layered families on clay-like soils
# One step of FAMILY_STEP stable steps (lh_stable_dt at Courant 0.5) from a moist state; every column converges; the
# family's residual-through-the-tendency bound and, against its NumPy reference, its parity bound.

STATUS_UNCONVERGED, STATUS_FAILED = 8, 16


def device_stable_dt(g, Y, Ya, courant=0.5):
    out = C.c_double()
    g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, courant, C.byref(out)), g.ctx)
    return out.value


def family_step(case):
    with Ctx(case, None, CF.LDEXP) as g:
        Y, Ya = g.prognostic_and_aux()
        sd = device_stable_dt(g, Y, Ya)
    assert np.isfinite(sd) and sd > 0
    return cc.FAMILY_STEP * sd


def test_clay_implicit_euler_and_trbdf2(host_chosen_ldexp_form):
    """lh_step_implicit_euler: the residual bound of test_gpu_implicit (10 tol nu (1 + 4 mult) + round-off, nu the
    column's own) and 1e-10 against implicit_ref; lh_integrate_trbdf2 (one fixed step): 1e-10 against trbdf2_ref."""
    case = cc.family_case(M.MODEL_RICHARDS)
    dt = family_step(case)
    v1, mi, un, st = TI.implicit_on_device(case, dt, 1)
    assert un == 0 and st == 0, (mi, un, st)
    res = np.max(np.abs(TI.device_residual(case, v1, dt)), axis=1)
    bound = 10 * 1e-10 * case.om.percol["nu"] * (1 + 4 * cc.FAMILY_STEP) + TI.round_off(case, v1, dt)
    want, iters = IR.implicit_euler(case.om, case.vl, case.ti, dt, 1)
    err = float(np.max(np.abs(v1 - want)))
    print(f"clay backward Euler: iterations {mi} (reference {iters.max()}), residual / bound {float(np.max(res / bound)):.3g}, "
          f"against the reference {err:.3g}")
    assert iters.max() < 120 and np.all(res <= bound), float(np.max(res / bound))
    assert err <= 1e-10 and np.max(np.abs(v1 - case.vl)) > 1e-6
    v2, stats, status, _ = TT.trbdf2_on_device(case, 0.0, dt, dt, fixed=True)
    assert status == 0 and stats["accepted"] == case.ncols and stats["rejected"] == 0 and stats["unconverged"] == 0, stats
    want2, _ = TR.trbdf2(case.om, case.vl, case.ti, 0.0, dt, dt, adaptive=False)
    err2 = float(np.max(np.abs(v2 - want2)))
    print(f"clay fixed TR-BDF2 against the reference: {err2:.3g}")
    assert err2 <= 1e-10


def test_clay_coupled_implicit(host_chosen_ldexp_form):
    """lh_step_coupled_implicit: the residual bounds of test_gpu_coupled_implicit for backward Euler, its parity
    bounds (check_parity) for backward Euler and fixed TR-BDF2."""
    case = cc.family_case(M.MODEL_COUPLED)
    dt = family_step(case)
    mult = cc.FAMILY_STEP
    vl0, ti, re0 = CR.f64(case)
    eps = float(np.finfo(np.float64).eps)
    v1, e1, mi, un, st = TCI.device_steps(case, dt, 1)
    assert un == 0 and st == 0, (mi, un, st)

    def res(v, e):
        fv, fe = TCI.lh_rhs_of(case, v, e)
        big = np.maximum(np.abs(v).max(axis=1), dt * np.abs(fv).max(axis=1))
        return np.max(np.abs(v - vl0 - dt * fv), axis=1), 64 * eps * big, float(np.max(np.abs(e - re0 - dt * fe)))

    rw, round_off, r_dev = res(v1, e1)
    bound = 10 * 1e-10 * case.om.percol["nu"] * (1 + 4 * mult) + round_off
    vr, er, info = CR.coupled_implicit(case.om, vl0, ti, re0, dt, 1)
    _, _, r_ref = res(vr, er)
    floor = 8 * eps * np.max(np.abs(re0))
    print(f"clay coupled backward Euler: iterations {mi}, water residual / bound {float(np.max(rw / bound)):.3g}, energy device "
          f"{r_dev:.3g} reference {r_ref:.3g} floor {floor:.3g}")
    assert info["unconverged"] == 0
    assert np.all(rw <= bound), float(np.max(rw / bound))
    assert r_dev <= max(4 * r_ref, floor), (r_dev, r_ref, floor)
    for method in TCI.METHODS:
        TCI.check_parity(case, dt, 1, method, label="clay")


def test_clay_coupled_adaptive_trbdf2(host_chosen_ldexp_form):
    """lh_integrate_coupled_trbdf2, a call that spans one step: no failed column, and every column the reference
    accepts with E <= 0.9 (a column within 10 % of E = 1 may go either way and one beyond is re-stepped: neither is
    compared) lands on the reference's Y_1 within check_one_step's bound, 4 d + 64 eps ||Y|| per variable."""
    case = cc.family_case(M.MODEL_COUPLED)
    h = family_step(case)
    exact, E, (dv, de) = TCT.one_step_reference(case, h)
    v1, e1, st, status, cols = TCT.on_device(case, 0.0, h, h)
    assert status == 0 and st["failed"] == 0 and st["unconverged"] == 0, (status, st)
    ok = E <= 0.9
    assert ok.sum() >= case.ncols // 2 and st["accepted"] >= case.ncols and st["rejected"] >= int(np.sum(E >= 1.1)), (E, st)
    eps = float(np.finfo(np.float64).eps)
    bv = 4 * dv + 64 * eps * float(np.max(np.abs(exact["v1"])))
    be = 4 * de + 64 * eps * float(np.max(np.abs(exact["e1"])))
    gv = float(np.max(np.abs(v1 - exact["v1"])[ok]))
    ge = float(np.max(np.abs(e1 - exact["e1"])[ok]))
    print(f"clay coupled adaptive TR-BDF2: E {E.min():.3g}..{E.max():.3g}, {int(ok.sum())} columns compared, vl {gv:.3g} (bound {bv:.3g}), "
          f"rhoe {ge:.3g} (bound {be:.3g}), {st}")
    assert gv <= bv and ge <= be, (gv, bv, ge, be)


def test_clay_layered_tendency_and_integrators(host_chosen_ldexp_form):
    """Layered soils with two clay classes (3 and 11 of 16, n = 1.05): the class table switches the launches to the
    v_ldexp form.  lh_rhs against layered_ref at the plain statistic's floors; lh_step_layered_implicit_euler: the
    residual bound of test_gpu_layered_implicit and its parity bound against layered_implicit_ref;
    lh_integrate_layered_trbdf2 (one fixed step): the parity bound."""
    lay = cc.layered_clay_case()
    assert {3, 11} <= set(np.unique(lay.class_map).tolist())
    got = TL.gpu_rhs(lay)["vl"]
    want = TL.R.rhs(lay)
    share = pc.plain_statistic(lay.case, dict(vl=got), dict(vl=want))["vl"]
    print(f"clay layered tendency: worst cell / field scale {TL.worst_cell(got, want):.3g}, share within 1e-13: {share:.4f}")
    assert share >= pc.PLAIN_SHARE_MIN[np.dtype(np.float64)], share
    with TL.layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        dt = cc.FAMILY_STEP * TL.stable_dt(g, Y, Ya)
    r = TLI.euler(lay, dt, 1, want_rhs=True)
    assert r["unconverged"] == 0 and r["status"] == 0, (r["max_iters"], r["unconverged"], r["status"])
    res = np.max(np.abs(r["vl"] - lay.case.vl - dt * r["f"]), axis=1)
    bound, _ = TLI.residual_bound(lay, r, dt, cc.FAMILY_STEP)
    want1, iters = LI.implicit_euler(lay, dt, 1)
    err = float(np.max(np.abs(r["vl"] - want1)))
    print(f"clay layered backward Euler: iterations {r['max_iters']} (reference {np.max(iters)}), residual / bound "
          f"{float(np.max(res / bound)):.3g}, against the reference {err:.3g}")
    assert np.all(res <= bound), float(np.max(res / bound))
    assert err <= TLI.PARITY[np.dtype(np.float64)] and np.max(np.abs(r["vl"] - lay.case.vl)) > 1e-6
    v2, st, status, _ = TLI.trbdf2(lay, 0.0, dt, dt, fixed=True)
    assert status == 0 and st["accepted"] == lay.case.ncols and st["rejected"] == 0 and st["unconverged"] == 0, st
    want2, _ = LI.trbdf2(lay, 0.0, dt, dt, adaptive=False)
    err2 = float(np.max(np.abs(v2 - want2)))
    print(f"clay layered fixed TR-BDF2 against the reference: {err2:.3g}")
    assert err2 <= TLI.PARITY[np.dtype(np.float64)]
