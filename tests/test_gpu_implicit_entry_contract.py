"""The host contract of the seven implicit entry points, on contexts of 3 columns x 2 levels: the exact words of
every refusal of lh_step_implicit_euler, lh_integrate_trbdf2 and lh_step_heat_implicit (the coupled and the layered
calls have theirs pinned in their own files), arguments before the model before the states for all seven, a refused
call reporting zero statistics, calls with nothing to do, and the layered Richards pair against the scalar pair on
classes that equal the scalar parameters.  Every case is a refused call, an early return or one tiny step."""
import ctypes as C

import numpy as np
import pytest

import case_model as M
import coupled_implicit_ref as CR
import heat_implicit_ref as H
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc
from test_gpu_layered import layered_gpu
from test_gpu_layered_heat import heat_gpu
from test_gpu_layered_implicit import PARITY

pytestmark = pytest.mark.gpu

E, T = "lh_step_implicit_euler", "lh_integrate_trbdf2"
LE, LT = "lh_step_layered_implicit_euler", "lh_integrate_layered_trbdf2"
HI, CE, CT = "lh_step_heat_implicit", "lh_step_coupled_implicit", "lh_integrate_coupled_trbdf2"
SEVEN = (E, T, LE, LT, HI, CE, CT)
NEWTON, ADAPTIVE = (E, LE, CE), (T, LT, CT)      # the calls that write lh_implicit_stats / lh_trbdf2_stats
NCOLS, NLEV = 3, 2
FLUX = (M.BC_FLUX, M.BC_FLUX)

RICHARDS_ONLY = "Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)"
COUPLED_ONLY = "coupled models only (SoilEnergyModel + SoilHydrologyModel)"
HEAT_ONLY = "heat-only models (SoilEnergyModel + PrescribedHydrologyModel)"
WITH_CLASSES = (" is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, lh_step_ssprk33, "
                "lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are")
STEP_IMPLICITLY = ", and lh_step_layered_implicit_euler and lh_integrate_layered_trbdf2 step implicitly"
WITH_CLASSES_ON_THIS_MODEL = (" is not available with soil classes (a class map is set) on this model: it steps "
                              "Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)")
NO_CLASS_MAP = ": the context has no class map (lh_set_soil_class_map); %s steps a model without soil classes"
FACTORS = "conductivity factors other than NoEffect are not supported"
BAD_DT = {E: "need nsteps >= 0 and dt > 0", LE: "need nsteps >= 0 and dt > 0",
          HI: "need nsteps >= 0 and a finite dt > 0", CE: "need nsteps >= 0 and a finite dt > 0",
          T: "need a finite dt > 0", LT: "need a finite dt > 0", CT: "need a finite dt > 0"}
WRONG_MODEL = {E: RICHARDS_ONLY, T: RICHARDS_ONLY, LE: RICHARDS_ONLY, LT: RICHARDS_ONLY, HI: HEAT_ONLY,
               CE: COUPLED_ONLY, CT: COUPLED_ONLY}


def scalar_classes():
    """two classes, both the parameters a scalar Richards context has by default"""
    om = M.CaseModel(M.MODEL_RICHARDS, NLEV, -0.02 * NLEV, 0.0)
    k = [om.vg.n, om.vg.alpha, om.vg.theta_r, om.vg.Ksat, om.soil.nu, om.soil.S_s]
    return np.array([k, k], dtype=np.float64)


def richards_pair(dtype=np.float64, factors=False):
    """A Richards case whose column c has class c mod 2 at every level, the two classes equal to the scalar
    parameters of the case itself: lay.case alone is the scalar context, with its map the layered one."""
    return R.make_layered(dtype, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), classes=scalar_classes(), bc="dirichlet",
                          factors=factors)


def layered_heat_only():
    return LH.make_layered_heat(np.float64, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), model=M.MODEL_HEAT,
                                classes=R.texture_classes()[:2], bc="dirichlet")


# The four kinds of context and the step each is stepped by: ten layered stable steps for the Richards ones, 100 s
# for the heat-only (an exact linear solve at any step) and the coupled one (half its diffusive bound at dz = 0.02).
def context(kind):
    if kind == "richards":
        return pc.GpuModel(richards_pair().case)
    if kind == "layered":
        return layered_gpu(richards_pair())
    if kind == "heat":
        return pc.GpuModel(H.heat_case(NCOLS, NLEV))
    return pc.GpuModel(CR.coupled_case(*FLUX, ncols=NCOLS, nlev=NLEV))


def step_of(kind):
    return 10 * R.stable_dt(richards_pair()) if kind in ("richards", "layered") else 100.0


HOME = {E: "richards", T: "richards", LE: "layered", LT: "layered", HI: "heat", CE: "coupled", CT: "coupled"}
# a context of another model (the layered calls: without a class map too), and the call of that context that writes
# the same statistics block
FOREIGN = {E: "coupled", T: "coupled", LE: "coupled", LT: "coupled", HI: "richards", CE: "richards", CT: "richards"}
OWN = {("coupled", NEWTON): CE, ("coupled", ADAPTIVE): CT, ("richards", NEWTON): E, ("richards", ADAPTIVE): T}


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def call(g, name, Y, Ya, dt, nsteps=1, flags=0, bcv=None, t0=0.0, t1=None, abstol=0.0, reltol=0.0):
    """One call of `name`: nsteps steps of dt for the fixed-step calls, [t0, t1 = nsteps dt] from dt for the adaptive."""
    f = getattr(g.L, name)
    t1 = nsteps * dt if t1 is None else t1
    if name in (E, LE):
        return f(g.ctx, Y, Ya, 0.0, dt, nsteps, _dptr(bcv), 0.0, 0)
    if name == HI:
        return f(g.ctx, Y, Ya, 0.0, dt, nsteps, flags, _dptr(bcv))
    if name == CE:
        return f(g.ctx, Y, Ya, 0.0, dt, nsteps, flags, _dptr(bcv), 0.0, 0)
    if name in (T, LT):
        return f(g.ctx, Y, Ya, t0, t1, dt, abstol, reltol, flags, None, _dptr(bcv))
    return f(g.ctx, Y, Ya, t0, t1, dt, abstol, 0.0, reltol, flags, None, _dptr(bcv))


def refused(g, rc, code, message):
    assert rc == code, (rc, code, g.L.lh_last_error(g.ctx))
    assert g.L.lh_last_error(g.ctx).decode() == message, g.L.lh_last_error(g.ctx)


def statistics(g):
    """((max_iters, unconverged, iterations), the seven lh_trbdf2_stats counters); every output starts non-zero"""
    mi, un, it = C.c_int32(7), C.c_int64(7), C.c_int64(7)
    st = (C.c_int64 * g.F.LH_TRBDF2_NSTATS)(*([7] * g.F.LH_TRBDF2_NSTATS))
    g.F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
    g.F.check(g.L.lh_implicit_iterations(g.ctx, C.byref(it)), g.ctx)
    g.F.check(g.L.lh_trbdf2_stats(g.ctx, st), g.ctx)
    return (mi.value, un.value, it.value), tuple(st)


def all_zero(g):
    return statistics(g) == ((0, 0, 0), (0,) * g.F.LH_TRBDF2_NSTATS)


def counted(g, name):
    """whether the statistics block of `name` holds a call that did something"""
    (mi, _, it), st = statistics(g)
    return (mi > 0 and it > 0) if name in NEWTON else st[0] > 0


def planes(g, Y):
    """every plane of the prognostic state, as the context's model names them"""
    F, m = g.F, g.case.om.model
    v = {M.MODEL_RICHARDS: (F.LH_VAR_VARTHETA_L, F.LH_VAR_THETA_I), M.MODEL_HEAT: (F.LH_VAR_RHOE_INT,),
         M.MODEL_COUPLED: (F.LH_VAR_VARTHETA_L, F.LH_VAR_THETA_I, F.LH_VAR_RHOE_INT)}[m]
    return [g.download(Y, k) for k in v]


# ------------------------------------------------------------ messages

def test_messages_of_lh_step_implicit_euler():
    nan = float("nan")
    with context("richards") as g:
        Y, Ya = g.prognostic_and_aux()
        for dt, nsteps in ((0.0, 1), (-1.0, 1), (nan, 1), (1.0, -1)):
            refused(g, call(g, E, Y, Ya, dt, nsteps), g.F.LH_EINVAL, E + ": need nsteps >= 0 and dt > 0")
        assert g.L.lh_step_implicit_euler(None, Y, Ya, 0.0, 1.0, 1, None, 0.0, 0) == g.F.LH_EINVAL
        # the layered calls on a context without a class map name the scalar call
        refused(g, call(g, LE, Y, Ya, 1.0), g.F.LH_EMODEL, LE + NO_CLASS_MAP % E)
        refused(g, call(g, LT, Y, Ya, 1.0), g.F.LH_EMODEL, LT + NO_CLASS_MAP % T)
    for kind in ("coupled", "heat"):
        with context(kind) as g:
            Y, Ya = g.prognostic_and_aux()
            refused(g, call(g, E, Y, Ya, 1.0), g.F.LH_EMODEL, E + ": " + RICHARDS_ONLY)
    # the scalar call on a layered context names the layered calls
    with context("layered") as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, E, Y, Ya, 1.0), g.F.LH_EMODEL, E + WITH_CLASSES + STEP_IMPLICITLY)
    with pc.GpuModel(richards_pair(factors=True).case) as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, E, Y, Ya, 1.0), g.F.LH_EMODEL, E + ": " + FACTORS)


def test_messages_of_lh_integrate_trbdf2():
    nan, inf = float("nan"), float("inf")
    with context("richards") as g:
        Y, Ya = g.prognostic_and_aux()
        EINVAL = g.F.LH_EINVAL
        for t0, t1 in ((1.0, 0.0), (0.0, inf), (nan, 1.0), (-inf, 0.0)):
            refused(g, call(g, T, Y, Ya, 1.0, t0=t0, t1=t1), EINVAL, T + ": need finite t0 <= t1")
        for dt in (0.0, -1.0, nan, inf):
            refused(g, call(g, T, Y, Ya, dt, t1=1.0), EINVAL, T + ": need a finite dt > 0")
        for bad in (-1e-6, nan, inf):
            refused(g, call(g, T, Y, Ya, 1.0, abstol=bad), EINVAL, T + ": tolerances must be finite and >= 0")
            refused(g, call(g, T, Y, Ya, 1.0, reltol=bad), EINVAL, T + ": tolerances must be finite and >= 0")
        refused(g, call(g, T, Y, Ya, 1.0, flags=2), EINVAL, T + ": unknown flags 0x2")
        refused(g, call(g, T, Y, Ya, 1.0, flags=0x80000001), EINVAL, T + ": unknown flags 0x80000001")
        for k in (0, 7):
            bcv = np.full(8, 0.3)
            bcv[k] = nan if k else inf
            refused(g, call(g, T, Y, Ya, 1.0, bcv=bcv), EINVAL, T + ": non-finite boundary value")
        assert g.L.lh_integrate_trbdf2(None, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == EINVAL
    for kind in ("coupled", "heat"):
        with context(kind) as g:
            Y, Ya = g.prognostic_and_aux()
            refused(g, call(g, T, Y, Ya, 1.0), g.F.LH_EMODEL, T + ": " + RICHARDS_ONLY)
    with context("layered") as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, T, Y, Ya, 1.0), g.F.LH_EMODEL, T + WITH_CLASSES + STEP_IMPLICITLY)
    with pc.GpuModel(richards_pair(factors=True).case) as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, T, Y, Ya, 1.0), g.F.LH_EMODEL, T + ": " + FACTORS)


def test_messages_of_lh_step_heat_implicit():
    nan, inf = float("nan"), float("inf")
    with context("heat") as g:
        Y, Ya = g.prognostic_and_aux()
        for dt, nsteps in ((0.0, 1), (-1.0, 1), (nan, 1), (inf, 1), (1.0, -1)):
            refused(g, call(g, HI, Y, Ya, dt, nsteps), g.F.LH_EINVAL, HI + ": need nsteps >= 0 and a finite dt > 0")
        refused(g, call(g, HI, Y, Ya, 1.0, flags=2), g.F.LH_EINVAL, HI + ": unknown flags 0x2")
        refused(g, call(g, HI, Y, Ya, 1.0, flags=0x80000001), g.F.LH_EINVAL, HI + ": unknown flags 0x80000001")
        assert g.L.lh_step_heat_implicit(None, Y, Ya, 0.0, 1.0, 1, 0, None) == g.F.LH_EINVAL
    for kind in ("coupled", "richards", "layered"):
        with context(kind) as g:
            Y, Ya = g.prognostic_and_aux()
            refused(g, call(g, HI, Y, Ya, 1.0), g.F.LH_EMODEL, HI + ": " + HEAT_ONLY)
    # its own order on a heat-only context with a class map: the model, the states, then the class map
    with heat_gpu(layered_heat_only()) as g:
        Y, Ya = g.prognostic_and_aux()
        assert call(g, HI, Y, None, 1.0) == g.F.LH_ESTATE
        refused(g, call(g, HI, Y, Ya, 1.0), g.F.LH_EMODEL, HI + WITH_CLASSES)
        # the Richards calls there: the scalar ones by the model, the layered ones by the model with a map
        for name in (E, T):
            refused(g, call(g, name, Y, Ya, 1.0), g.F.LH_EMODEL, name + ": " + RICHARDS_ONLY)
        for name in (LE, LT):
            refused(g, call(g, name, Y, Ya, 1.0), g.F.LH_EMODEL, name + WITH_CLASSES_ON_THIS_MODEL)


# ------------------------------------------------------------ order

@pytest.mark.parametrize("name", SEVEN)
def test_arguments_before_the_model_before_the_states(name):
    with context(FOREIGN[name]) as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, name, Y, Ya, 0.0), g.F.LH_EINVAL, name + ": " + BAD_DT[name])
        refused(g, call(g, name, None, Ya, 1.0), g.F.LH_EMODEL, name + ": " + WRONG_MODEL[name])
        refused(g, call(g, name, Y, Ya, 1.0), g.F.LH_EMODEL, name + ": " + WRONG_MODEL[name])


# ------------------------------------------------------------ statistics

@pytest.mark.parametrize("name", NEWTON + ADAPTIVE)
def test_a_refused_call_reports_zeros(name):
    group = NEWTON if name in NEWTON else ADAPTIVE
    # by a bad argument, after its own step has left counters
    with context(HOME[name]) as g:
        Y, Ya = g.prognostic_and_aux()
        g.F.check(call(g, name, Y, Ya, step_of(HOME[name])), g.ctx)
        assert counted(g, name), statistics(g)
        assert call(g, name, Y, Ya, 0.0) == g.F.LH_EINVAL
        assert all_zero(g), statistics(g)
    # by the model, after the step of the context's own call has left counters in the same block
    with context(FOREIGN[name]) as g:
        Y, Ya = g.prognostic_and_aux()
        own = OWN[(FOREIGN[name], group)]
        g.F.check(call(g, own, Y, Ya, step_of(FOREIGN[name])), g.ctx)
        assert counted(g, own), statistics(g)
        assert call(g, name, Y, Ya, 1.0) == g.F.LH_EMODEL
        assert all_zero(g), statistics(g)


# ------------------------------------------------------------ calls with nothing to do

EMPTY = [(E, 0), (LE, 0), (T, 0), (T, 1), (LT, 0), (LT, 1), (HI, 0), (HI, 1), (CE, 0), (CE, 1), (CT, 0)]


@pytest.mark.parametrize("name,flags", EMPTY, ids=["%s-%d" % e for e in EMPTY])
def test_nothing_to_do(name, flags):
    """nsteps == 0 (t1 == t0) on a fresh context returns LH_OK, leaves every plane of Y as uploaded and the
    statistics at zero; the step after it works and is counted; and the same again after that step."""
    dt = step_of(HOME[name])

    def nothing(g, Y, Ya):
        if name in ADAPTIVE:
            return call(g, name, Y, Ya, dt, flags=flags, t0=3.0, t1=3.0)
        return call(g, name, Y, Ya, dt, 0, flags=flags)

    with context(HOME[name]) as g:
        Y, Ya = g.prognostic_and_aux()
        before = planes(g, Y)
        g.F.check(nothing(g, Y, Ya), g.ctx)
        for a, b in zip(planes(g, Y), before):
            np.testing.assert_array_equal(a, b)
        assert all_zero(g), statistics(g)
        g.F.check(call(g, name, Y, Ya, dt, flags=flags), g.ctx)
        after = planes(g, Y)
        assert any(np.any(a != b) for a, b in zip(after, before)) and all(np.all(np.isfinite(a)) for a in after)
        assert name == HI or counted(g, name), statistics(g)
        g.F.check(nothing(g, Y, Ya), g.ctx)
        for a, b in zip(planes(g, Y), after):
            np.testing.assert_array_equal(a, b)
        assert all_zero(g), statistics(g)
        assert g.status() == 0


# ------------------------------------------------------------ the layered pair is the scalar pair

@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_layered_pair_is_the_scalar_pair(dtype):
    """Classes equal to the scalar parameters: one backward-Euler step and one fixed TR-BDF2 step of the layered
    calls against the scalar calls, within the bound of tests/test_gpu_layered_implicit.py's comparison of the
    layered with the per-column kernels (not bitwise: rhs_kernel folds Ksat into the gradient factor)."""
    lay = richards_pair(dtype)
    om = lay.case.om
    assert [list(k) for k in lay.classes] == [[om.vg.n, om.vg.alpha, om.vg.theta_r, om.vg.Ksat, om.soil.nu, om.soil.S_s]] * 2
    assert sorted(set(lay.class_map[:, 0])) == [0, 1] and np.all(lay.class_map == lay.class_map[:, :1])
    dt = 10 * R.stable_dt(lay)
    for scalar, layered, flags in ((E, LE, 0), (T, LT, 1)):
        got = {}
        for name, g in ((scalar, pc.GpuModel(lay.case)), (layered, layered_gpu(lay))):
            with g:
                Y, Ya = g.prognostic_and_aux()
                g.F.check(call(g, name, Y, Ya, dt, flags=flags), g.ctx)
                got[name] = g.download(Y, g.F.LH_VAR_VARTHETA_L).astype(np.float64)
                assert g.status() == 0 and counted(g, name), (name, statistics(g))
        err = float(np.max(np.abs(got[layered] - got[scalar])))
        moved = float(np.max(np.abs(got[scalar] - lay.case.vl)))
        print("%s against %s: %.3g (moved %.3g)" % (layered, scalar, err, moved))
        assert err <= PARITY[np.dtype(dtype)], (layered, err)
        assert moved > 0
