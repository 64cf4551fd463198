"""lh_step_layered_heat_implicit / LayeredHeatImplicitEuler / LayeredHeatTRBDF2: implicit steps of a heat-only model
with per-cell soil classes on the device, against the NumPy reference (tests/layered_heat_implicit_ref.py), through
the library's own layered tendency (lh_rhs of the same context), against lh_step_heat_implicit where every column
has one class, and its host contract.  Mirrors tests/test_gpu_heat_implicit.py."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest

import case_model as M
import heat_implicit_ref as H
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu

NAME, SCALAR = "lh_step_layered_heat_implicit", "lh_step_heat_implicit"
METHODS = ("euler", "trbdf2")
MULTS = (1.0, 30.0, 1000.0)        # step sizes in units of the explicit engines' stable step
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
# ||rhoe_dev - rhoe_ref||_inf <= K eps(FT) cond_inf(M) ||rhoe||_inf per column, M = I - c A the stage matrix of the
# reference.  K started as tests/test_gpu_heat_implicit.py's K_BOUND, 4 x 10.36 and 4 x 11.93 (the elimination and the
# time loop are the scalar kernel's arithmetic).  Measured on an MI355X over the cases of this file (DESIGN section
# 4.24) the worst ratios are 14.25 in Float64 (67 x 12, a class per cell, Dirichlet faces) and 41.06 in Float32 (ice
# between two flux faces; 17.02 with Dirichlet faces, at most 9.55 without ice), every one of them TR-BDF2 after 5
# steps of 1x the stable step, where the scalar file has its worst too: cond is 2 to 3 there, so the bound is a few
# eps, and what is measured is not the solve but the few ulp by which kappa and rho_c_s of the production closures
# differ from the Float64 host closures of the reference, carried through 10 solves and 5 tendencies; a map with
# another class in every cell has a conductivity jump at every face.  4 x the measurement exceeds the scalar K in both
# types, so K is 4 x the measurement.
K_BOUND = {np.dtype(np.float64): 4 * 14.25, np.dtype(np.float32): 4 * 41.06}
PLAIN_REL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}
PLAIN_SHARE_MIN = 0.999
WORST = {}                          # dtype -> the worst ratio this session has seen (printed by every parity test)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def heat_gpu(lay, **kw):
    """A context with the case's classes, their thermal supplement and its class map."""
    g = pc.GpuModel(lay.case, **kw)
    g.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    return g


class Device:
    """One layered context for several runs from the case's own state."""

    def __init__(self, lay):
        self.lay = lay
        self.g = heat_gpu(lay)
        self.Y, self.Ya = self.g.prognostic_and_aux()
        self.dY = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.g.close()

    def steps(self, dt, nsteps, method, bcv=None, calls=1, name=NAME):
        """rhoe_int after `calls` calls of nsteps each from the case's state; bcv [calls * nsteps + 1][2][2] is split
        at the seams."""
        g, F = self.g, self.g.F
        g.upload(self.Y, F.LH_VAR_RHOE_INT, self.lay.case.rhoe)
        flags = F.LH_HEAT_TRBDF2 if method == "trbdf2" else 0
        for k in range(calls):
            b = None if bcv is None else np.ascontiguousarray(bcv[k * nsteps:(k + 1) * nsteps + 1], dtype=np.float64)
            F.check(getattr(g.L, name)(g.ctx, self.Y, self.Ya, k * nsteps * dt, dt, nsteps, flags, ptr(b)), g.ctx)
        out = g.download(self.Y, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
        return out

    def rhs(self, rhoe):
        """lh_rhs of this context at the state rhoe"""
        g = self.g
        if self.dY is None:
            self.dY, self.Y2 = g.state(0), g.state(0)
        g.upload(self.Y2, g.F.LH_VAR_RHOE_INT, np.ascontiguousarray(rhoe, dtype=self.lay.case.dtype))
        g.rhs(self.Y2, self.Ya, self.dY)
        return g.tendencies(self.dY)["rhoe"].astype(np.float64)


def coef_of(method, dt):
    return LI.D * dt if method == "trbdf2" else dt


@functools.lru_cache(maxsize=None)
def parity_figures(dtype, ncols, nlev, kind="cells", bc="dirichlet", percol_bc=False, ice=False):
    """Per (method, multiple, nsteps): the largest err / (eps cond ||rhoe||) over the columns and the share of cells
    within PLAIN_REL of the field scale; and whether one stable step moved the state.  One context, one set of
    bands and one reference per case, shared by the tests that read them."""
    lay = LI.layered_case(dtype, ncols, nlev, kind=kind, bc=bc, percol_bc=percol_bc, ice=ice)
    re = LI.state64(lay)
    bands, _ = LI.affine_parts(lay)
    sd = LI.stable_dt(lay)
    eps = float(np.finfo(dtype).eps)
    out = {}
    with Device(lay) as d:
        for method in METHODS:
            for mult in MULTS:
                dt = mult * sd
                cond = LI.cond_inf(bands, coef_of(method, dt))
                for nsteps in (1, 5):
                    want = LI.heat_implicit(lay, re, dt, nsteps, method, bands=bands)
                    got = d.steps(dt, nsteps, method).astype(np.float64)
                    assert np.all(np.isfinite(got))
                    scale = np.max(np.abs(want), axis=1)
                    ratio = np.max(np.abs(got - want), axis=1) / (eps * cond * scale)
                    share = float(np.mean(np.abs(got - want) <= PLAIN_REL[np.dtype(dtype)] * np.max(np.abs(want))))
                    out[(method, mult, nsteps)] = (float(np.max(ratio)), share, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
        moved = float(np.max(np.abs(d.steps(sd, 1, "euler") - lay.case.rhoe)))
    return out, moved


def check_parity(dtype, ncols, nlev, plain=True, **kw):
    """The bound and, beside it (plain), the plain statistic, over both methods, 1 and 5 steps, three step sizes; the
    figures are printed before they are asserted."""
    res, moved = parity_figures(dtype, ncols, nlev, **kw)
    dt = np.dtype(dtype)
    worst = max(v[0] for v in res.values())
    share = min(v[1] for v in res.values())
    WORST[dt] = max(WORST.get(dt, 0.0), worst)
    at = max(res, key=lambda k: res[k][0])
    print(f"parity {dt.name} ncols={ncols} nlev={nlev} {kw}: worst ratio {worst:.4g} at {at} (this session, {dt.name}: "
          f"{WORST[dt]:.4g}), smallest plain share {share:.4f} at {min(res, key=lambda k: res[k][1])}, "
          f"worst cell {max(v[2] for v in res.values()):.3g} of the field scale")
    bad = {k: v for k, v in res.items() if v[0] > K_BOUND[dt]}
    assert not bad, (K_BOUND[dt], bad)
    if plain:
        assert share >= PLAIN_SHARE_MIN, {k: v for k, v in res.items() if v[1] < PLAIN_SHARE_MIN}
    if nlev > 1:   # (the steps did something)
        assert moved > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 12])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_parity_shapes(ncols, nlev, dtype):
    """A different class in every cell (5 classes, two of them organic: any_om is on).  Ragged last workgroup (67,
    130 columns: the lanes past the last column must reach all three table stagings), both faces on one cell, no
    interior face, one interior cell; 1 and 5 steps at 1x, 30x and 1000x the stable step, both methods."""
    check_parity(dtype, ncols, nlev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_parity_three_horizons_60_levels(dtype):
    check_parity(dtype, 67, 60, kind="horizons")


VARIANTS = {
    "flux_flux": dict(bc="flux"),
    "dirichlet_bottom_flux_top": dict(bc="mixed"),
    "percol_dirichlet": dict(percol_bc=True),
    "ice": dict(ice=True),
    "ice_flux_flux": dict(bc="flux", ice=True),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_parity_boundaries_and_ice(name, dtype):
    """Flux / flux, Dirichlet bottom with a flux top, per-column Dirichlet values and static ice, each with the bound
    and the plain statistic.  Ice between two flux faces (a combination of this file's own) is held to the bound
    alone: measured in Float32, backward Euler, 5 steps of 1000x, 2 of its 804 cells are more than 1e-5 of the
    field scale off (the worst 1.08e-5, share 0.9975) at 0.29 of the bound; Float64 1.0000.  Between flux faces the column's mean is not damped by the
    solve, so what the forward sweep rounds in c k_i (c 1e3 rho_c_s, the beta of neighbouring cells 6 K apart where
    one holds ice) stays in the result in proportion to cond (2.0e3 here), which the bound carries and a fixed 1e-5
    does not; and 804 cells leave the share no cell to spare where the scalar file's 4020 leave four."""
    check_parity(dtype, 67, 12, plain=(name != "ice_flux_flux"), **VARIANTS[name])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["dirichlet", "flux_flux", "ice"])
def test_residual_through_the_tendency(name, dtype):
    """R = Y1 - Yn - dt f(Y1) with f = lh_rhs of the same layered context: at most 4x the same quantity of the
    reference solution rounded to FT (floor 8 eps ||rhoe||)."""
    kw = {} if name == "dirichlet" else VARIANTS[name]
    lay = LI.layered_case(dtype, 67, 12, **kw)
    re = LI.state64(lay)
    bands, _ = LI.affine_parts(lay)
    eps = float(np.finfo(dtype).eps)
    sd = LI.stable_dt(lay)
    with Device(lay) as d:
        for mult in MULTS:
            dt = mult * sd
            got = d.steps(dt, 1, "euler")
            want = LI.heat_implicit(lay, re, dt, 1, "euler", bands=bands).astype(dtype)
            res = lambda y1: np.max(np.abs(y1.astype(np.float64) - re - dt * d.rhs(y1)))
            r_dev, r_ref = res(got), res(want)
            floor = 8 * eps * np.max(np.abs(re))
            print(f"residual {name} {np.dtype(dtype).name} {mult}x: device {r_dev:.3g} reference {r_ref:.3g} floor {floor:.3g}")
            assert r_dev <= max(4 * r_ref, floor), (mult, r_dev, r_ref, floor)


# ------------------------------------------------------------ column-uniform maps against the scalar call

def scalar_steps(case, dt, nsteps, method):
    with pc.GpuModel(case) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        F.check(gm.L.lh_step_heat_implicit(gm.ctx, Y, Ya, 0.0, dt, nsteps, F.LH_HEAT_TRBDF2 if method == "trbdf2" else 0, None), gm.ctx)
        out = gm.download(Y, F.LH_VAR_RHOE_INT)
        assert gm.status() == 0
        return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_column_uniform_map_against_the_scalar_call(method, dtype):
    """67 columns x 12 levels, 3 classes, every column one class: the layered call against lh_step_heat_implicit on
    the per-class scalar contexts (the class's numbers as the context's scalars), 5 steps of 30x the stable step.
    Each side is inside the parity bound of its own reference; their difference is printed.

    Measured on an MI355X: bitwise equal, both methods, both types -- kappa_closure_cls and
    temperature_closure_cls are the scalar closures operation for operation, and the class's table entry holds the
    numbers make_params gives the scalars.  That is what is asserted."""
    dt_ = np.dtype(dtype)
    lay = LI.layered_case(dtype, 67, 12, kind="columns")
    re = LI.state64(lay)
    bands, _ = LI.affine_parts(lay)
    dt, nsteps = 30.0 * LI.stable_dt(lay), 5
    eps = float(np.finfo(dtype).eps)
    cond = LI.cond_inf(bands, coef_of(method, dt))
    with Device(lay) as d:
        layered = d.steps(dt, nsteps, method)
    want = LI.heat_implicit(lay, re, dt, nsteps, method, bands=bands)
    bound = K_BOUND[dt_] * eps * cond * np.max(np.abs(want), axis=1)
    assert np.all(np.max(np.abs(layered - want), axis=1) <= bound)
    scalar = np.zeros_like(layered)
    for cols, case in LH.per_class_cases(lay):
        got = scalar_steps(case, dt, nsteps, method)
        vl, ti, r0 = H.f64(case)
        ref = H.heat_implicit(case.om, vl, ti, r0, dt, nsteps, method)
        c1 = H.cond_inf(H.affine_parts(case.om, vl, ti)[0], coef_of(method, dt))
        assert np.all(np.max(np.abs(got - ref), axis=1) <= K_BOUND[dt_] * eps * c1 * np.max(np.abs(ref), axis=1))
        scalar[cols] = got
    gap = np.max(np.abs(layered.astype(np.float64) - scalar), axis=1)
    print(f"layered against scalar {method} {dt_.name}: largest difference {np.max(gap):.3g} "
          f"({np.max(gap / (eps * cond * np.max(np.abs(want), axis=1))):.3g} eps cond ||rhoe||), bitwise equal: "
          f"{np.array_equal(layered, scalar)}")
    np.testing.assert_array_equal(layered, scalar)
    assert np.max(np.abs(layered.astype(np.float64) - re)) > 0


# ------------------------------------------------------------ bitwise properties

def _table(dt, n):
    bcv = np.zeros((n + 1, 2, 2))
    t = dt * np.arange(n + 1)
    bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = 281.0 + 4.0 * np.sin(t / (3 * dt))
    bcv[:, M.FACE_TOP, M.COMP_ENERGY] = 287.0 - 3.0 * np.cos(t / (2 * dt))
    return bcv


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_splitting_a_call_columns_and_repeats(method, dtype):
    """2N steps in one call are bitwise N + N in two, with constant boundary values and with a time-dependent table
    split at the seam; a repeated call gives the same bits; the first 67 columns of a 130-column run are the
    67-column run; and the table means what the reference says it means."""
    lay = LI.layered_case(dtype, 130, 12, ice=True)
    small = LI.layered_case(dtype, 67, 12, ice=True)
    for a, b in ((lay.case.rhoe, small.case.rhoe), (lay.case.vl, small.case.vl), (lay.case.ti, small.case.ti),
                 (lay.class_map, small.class_map)):
        assert np.array_equal(a[:67], b)
    dt, N = 30 * LI.stable_dt(lay), 3
    bcv = _table(dt, 2 * N)
    with Device(lay) as d:
        one = d.steps(dt, 2 * N, method)
        np.testing.assert_array_equal(d.steps(dt, N, method, calls=2), one)
        np.testing.assert_array_equal(d.steps(dt, 2 * N, method), one)
        one_b = d.steps(dt, 2 * N, method, bcv=bcv)
        np.testing.assert_array_equal(d.steps(dt, N, method, bcv=bcv, calls=2), one_b)
    assert np.max(np.abs(one_b.astype(np.float64) - one)) > 0
    with Device(small) as d:
        np.testing.assert_array_equal(d.steps(dt, 2 * N, method), one[:67])
        np.testing.assert_array_equal(d.steps(dt, 2 * N, method, bcv=bcv), one_b[:67])
    bands, _ = LI.affine_parts(small)
    want = LI.heat_implicit(small, LI.state64(small), dt, 2 * N, method, bcv=bcv, bands=bands)
    eps = float(np.finfo(dtype).eps)
    cond = LI.cond_inf(bands, coef_of(method, dt))
    ratio = np.max(np.abs(one_b[:67] - want), axis=1) / (eps * cond * np.max(np.abs(want), axis=1))
    print(f"bcv parity {method} {np.dtype(dtype).name}: worst ratio {np.max(ratio):.3g}")
    assert np.max(ratio) <= K_BOUND[np.dtype(dtype)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_conservation_with_flux_faces(method, dtype):
    """sum_i rhoe_int changes by nsteps dt (F_bottom - F_top) / dz, to nlev 4 eps sum |rhoe_int|: 50 steps of 30x the
    stable step on the per-cell map, 67 x 60 as in tests/test_gpu_heat_implicit.py.

    The shape matters to this bound.  Read from the figures below, not traced: the stage matrix is factored once per
    call, so the few ulp by which the stored multipliers miss a zero column sum are the same in every solve, and the
    defect grows with the number of solves (50
    for backward Euler, 100 for TR-BDF2) and not with the number of levels, while the bound is nlev 4 eps for the
    whole call.  Measured on an MI355X at 12 levels, where the bound is 48 eps sum |rhoe_int|: 1.41 (backward Euler)
    and 2.61 (TR-BDF2) of it in Float64, 1.50 and 2.28 in Float32, i.e. 68 to 125 eps after 50 steps, 1.1 to 1.4 eps
    per solve.  That is what the scalar kernel's arithmetic gives (a column-uniform map is bitwise the scalar call);
    the bound was written for the scalar file's 60 levels, 240 eps, and is taken at that shape here."""
    lay = LI.layered_case(dtype, 67, 60, bc="flux")
    om = lay.case.om
    (_, fb), (_, ft) = LH.ENERGY_BC["flux"]
    nsteps, dt = 50, 30 * LI.stable_dt(lay)
    dz = (om.zmax - om.zmin) / om.nlev
    with Device(lay) as d:
        got = d.steps(dt, nsteps, method).astype(np.float64)
    re = LI.state64(lay)
    change = got.sum(axis=1) - re.sum(axis=1)
    want = nsteps * dt * (fb - ft) / dz
    allowed = om.nlev * 4 * float(np.finfo(dtype).eps) * np.abs(re).sum(axis=1)
    print(f"conservation {method} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound")
    assert np.all(np.abs(change - want) <= allowed), float(np.max(np.abs(change - want) / allowed))
    assert abs(want) > 0


# ------------------------------------------------------------ the host contract, on 3 columns x 2 levels

NCOLS, NLEV = 3, 2
HEAT_ONLY = ": heat-only models (SoilEnergyModel + PrescribedHydrologyModel)"
NO_CLASS_MAP = ": the context has no class map (lh_set_soil_class_map); lh_step_heat_implicit steps a model without soil classes"
BAD_ARGS = ": need nsteps >= 0 and a finite dt > 0"
PERCOL = ": soil classes (a class map is set) cannot be combined with per-column parameter arrays (lh_set_percol_param)"
LIBM = ": soil classes (a class map is set) have no LH_MATH_LIBM kernels"
SCALAR_WITH_CLASSES = (" is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, lh_step_ssprk33, "
                       "lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are")


def tiny():
    return LH.make_layered_heat(np.float64, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), model=M.MODEL_HEAT,
                                classes=R.texture_classes()[:2], thermal=LH.thermal_classes()[:2], bc="dirichlet")


def call(g, Y, Ya, dt=100.0, nsteps=1, flags=0, name=NAME):
    return getattr(g.L, name)(g.ctx, Y, Ya, 0.0, dt, nsteps, flags, None)


def refused(g, rc, code, message):
    assert rc == code, (rc, code, g.L.lh_last_error(g.ctx))
    assert g.L.lh_last_error(g.ctx).decode() == message, g.L.lh_last_error(g.ctx)


def test_refusals_in_their_order():
    nan, inf = float("nan"), float("inf")
    lay = tiny()
    # 1. the arguments, before the model; 2. the model, before the states
    for case in (R.make_layered(np.float64, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), classes=R.texture_classes()[:2]).case,
                 pc.make_case("coupled_f64_small", ncols=NCOLS)):
        with pc.GpuModel(case) as g:
            Y, Ya = g.prognostic_and_aux()
            for dt, nsteps in ((0.0, 1), (-1.0, 1), (nan, 1), (inf, 1), (1.0, -1)):
                refused(g, call(g, Y, Ya, dt, nsteps), g.F.LH_EINVAL, NAME + BAD_ARGS)
            refused(g, call(g, Y, Ya, flags=2), g.F.LH_EINVAL, NAME + ": unknown flags 0x2")
            refused(g, call(g, Y, Ya, flags=0x80000001), g.F.LH_EINVAL, NAME + ": unknown flags 0x80000001")
            refused(g, call(g, None, Ya), g.F.LH_EMODEL, NAME + HEAT_ONLY)
            refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + HEAT_ONLY)
            assert g.L.lh_step_layered_heat_implicit(None, Y, Ya, 0.0, 1.0, 1, 0, None) == g.F.LH_EINVAL
    # 3. the states, before 4. the class map: a heat-only context without one
    with pc.GpuModel(lay.case) as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, Y, Ya, 0.0), g.F.LH_EINVAL, NAME + BAD_ARGS)
        assert call(g, Y, None) == g.F.LH_ESTATE
        assert call(g, Y, g.state(0b0001)) == g.F.LH_ESTATE      # Ya without theta_i
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        refused(g, call(g, Y, Ya, flags=g.F.LH_HEAT_TRBDF2), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        # classes and their supplement alone are not a map
        g.set_soil_classes(lay.classes, None, thermal=lay.thermal)
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        g.F.check(call(g, Y, Ya, name=SCALAR), g.ctx)             # (the scalar call steps it)
        assert g.status() == 0
    # 5. what every layered call refuses, after the states; and the scalar call's old words on the same context
    with heat_gpu(lay) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        assert call(g, Y, None) == F.LH_ESTATE
        arr = np.full(NCOLS, 0.45)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), ctx)
        assert call(g, Y, None) == F.LH_ESTATE
        refused(g, call(g, Y, Ya), F.LH_EMODEL, NAME + PERCOL)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], None), ctx)
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        refused(g, call(g, Y, Ya), F.LH_EMODEL, NAME + LIBM)
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        assert call(g, Y, None, name=SCALAR) == F.LH_ESTATE
        refused(g, call(g, Y, Ya, name=SCALAR), F.LH_EMODEL, SCALAR + SCALAR_WITH_CLASSES)
        # nothing above moved the state, and the call works
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), lay.case.rhoe)
        F.check(call(g, Y, Ya), ctx)
        assert np.any(g.download(Y, F.LH_VAR_RHOE_INT) != lay.case.rhoe) and g.status() == 0


@pytest.mark.parametrize("flags", [0, 1])
def test_nothing_to_do(flags):
    """nsteps == 0 returns LH_OK and leaves Y as uploaded, on a fresh context and after a step."""
    lay = tiny()
    with heat_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        F.check(call(g, Y, Ya, nsteps=0, flags=flags), g.ctx)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), lay.case.rhoe)
        F.check(call(g, Y, Ya, flags=flags), g.ctx)
        after = g.download(Y, F.LH_VAR_RHOE_INT)
        assert np.any(after != lay.case.rhoe) and np.all(np.isfinite(after))
        F.check(call(g, Y, Ya, nsteps=0, flags=flags), g.ctx)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), after)
        assert g.status() == 0


@pytest.mark.parametrize("flags", [0, 1])
def test_nonfinite_result_sets_status_bit_0_and_nothing_else(flags):
    lay = tiny()
    rhoe = lay.case.rhoe.copy()
    rhoe[1, 1] = np.nan
    with heat_gpu(LH.LayeredHeat(dataclasses.replace(lay.case, rhoe=rhoe), lay.classes, lay.thermal, lay.class_map)) as g:
        Y, Ya = g.prognostic_and_aux()
        g.F.check(call(g, Y, Ya, flags=flags), g.ctx)
        assert g.status() == 1
        out = g.download(Y, g.F.LH_VAR_RHOE_INT)
        assert np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))      # (columns are independent)


# ------------------------------------------------------------ the host mirror

def test_host_mirror_three_horizons_through_simulation():
    """A three-horizon heat-only SoilModel with a diurnal sine as its Dirichlet top through
    Simulation(model, LayeredHeatTRBDF2(), saveat=...): bitwise the direct C calls, one per saveat chunk, with the
    table sampled at the same times.  The markers refuse a model without classes and a coupled model."""
    lh = pc._pkg()
    FT = np.float64
    n, N = 12, 5
    lay = LI.layered_case(FT, N, n, kind="horizons")
    om = lay.case.om
    vl_row = np.ascontiguousarray(lay.case.vl[0])
    case = dataclasses.replace(lay.case, vl=np.ascontiguousarray(np.repeat(vl_row[None, :], N, axis=0)))
    lay = LH.LayeredHeat(case, lay.classes, lay.thermal, lay.class_map)
    bottom, day = 281.0, 86400.0
    top = lambda t: 287.0 + 4.0 * math.sin(2.0 * math.pi * t / day)
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(LH.THERMAL_FIELDS, t))))
                         for k, t in zip(lay.classes, lay.thermal)], lay.class_map[0].astype(np.int64))
    dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.Dirichlet(top)), bottom=lh.SoilComponentBC(energy=lh.Dirichlet(bottom)))
    kw = dict(domain=dom, boundary_conditions=bc, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet())
    model = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.PrescribedHydrologyModel(vartheta_l_profile=lambda z, t: vl_row + 0.0 * z),
                         soil_classes=sc, **kw)
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ρe_int": 1e7 + 0.0 * z}, 0.0)
    Y.soil.ρe_int = case.rhoe
    dt, total, chunk = 3600.0, 12, 4
    sim = lh.Simulation(model, lh.LayeredHeatTRBDF2(), Y_init=Y, dt=dt, tspan=(0.0, total * dt), Ya_init=Ya, saveat=chunk * dt)
    sol = lh.run(sim)
    got = np.array(sim.integrator.u.soil.ρe_int)
    assert sim.integrator._nsteps_done == total and len(sol.t) == total // chunk + 1
    with heat_gpu(lay) as g:
        F = g.F
        Yc, Yac = g.prognostic_and_aux()
        t = 0.0
        for _ in range(total // chunk):
            times = [t + k * dt for k in range(chunk + 1)]
            bcv = np.zeros((chunk + 1, 2, 2))
            bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = bottom
            bcv[:, M.FACE_TOP, M.COMP_ENERGY] = [top(x) for x in times]
            F.check(g.L.lh_step_layered_heat_implicit(g.ctx, Yc, Yac, t, dt, chunk, F.LH_HEAT_TRBDF2, ptr(bcv)), g.ctx)
            t = t + chunk * dt
        want = g.download(Yc, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    np.testing.assert_array_equal(got, want)
    assert np.max(np.abs(want - case.rhoe)) > 1e-3 * np.max(np.abs(case.rhoe))
    # ... and step_implicit_layered_heat is the same call
    Y2, Ya2 = lh.initialize_states(model, lambda z, m: {"ρe_int": 1e7 + 0.0 * z}, 0.0)
    Y2.soil.ρe_int = case.rhoe
    for k in range(total // chunk):
        lh.step_implicit_layered_heat(model, Y2, Ya2, k * chunk * dt, dt, chunk, "trbdf2")
    np.testing.assert_array_equal(np.array(Y2.soil.ρe_int), want)
    # the scalar markers keep refusing this model; the layered ones refuse a model without classes and a coupled one
    for marker in (lh.HeatImplicitEuler(), lh.HeatTRBDF2()):
        with pytest.raises(NotImplementedError, match="soil classes"):
            lh.Simulation(model, marker, Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    plain = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.PrescribedHydrologyModel(), **kw)
    flux = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)),
                           bottom=lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0), energy=lh.VerticalFlux(0.0)))
    coupled = lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT),
                           boundary_conditions=flux, earth_param_set=lh.EarthParameterSet())
    for other in (plain, coupled):
        for marker in (lh.LayeredHeatImplicitEuler(), lh.LayeredHeatTRBDF2()):
            with pytest.raises(NotImplementedError, match=type(marker).__name__):
                lh.Simulation(other, marker, Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
    model.close()
