"""Layered soils for the coupled and the heat-only model on the device: per-cell soil classes with their thermal
supplement through lh_set_soil_classes / lh_set_soil_class_thermal / lh_set_soil_class_map, the layered tendency,
its fused SSPRK33 stages, the step bound, the diagnostics and the boundary fluxes -- against the CPU oracle
called once per class where every column has one class, and against the NumPy restatement
(tests/layered_heat_ref.py) where it cannot.  Mirrors tests/test_gpu_layered.py."""
import copy
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import case_model as M
import layered_heat_ref as H
import layered_ref as R
import parity_cases as pc
from layered_heat_checks import CW, assert_close_per_class, check_conservation, oracle_per_class

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
MODELS = [M.MODEL_COUPLED, M.MODEL_HEAT]
MODEL_IDS = ["coupled", "heat"]
FIELDS = {M.MODEL_COUPLED: ("vl", "rhoe"), M.MODEL_HEAT: ("rhoe",)}


def heat_gpu(lay, class_map="own", **kw):
    """A context with the case's classes, their thermal supplement and (unless class_map is None) its class map."""
    g = pc.GpuModel(lay.case, **kw)
    g.set_soil_classes(lay.classes, lay.class_map if isinstance(class_map, str) else class_map, thermal=lay.thermal)
    return g


def upload_state(g, Y, Ya, vl=None, rhoe=None):
    F = g.F
    if vl is not None:
        g.upload(Ya if g.case.om.model == M.MODEL_HEAT else Y, F.LH_VAR_VARTHETA_L, vl)
    if rhoe is not None:
        g.upload(Y, F.LH_VAR_RHOE_INT, rhoe)


def state_of(g, Y):
    F = g.F
    out = dict(rhoe=g.download(Y, F.LH_VAR_RHOE_INT))
    if g.case.om.model != M.MODEL_HEAT:
        out["vl"] = g.download(Y, F.LH_VAR_VARTHETA_L)
    return out


def gpu_rhs(lay, class_map="own", vl=None, rhoe=None):
    with heat_gpu(lay, class_map) as g:
        Y, Ya = g.prognostic_and_aux()
        upload_state(g, Y, Ya, vl, rhoe)
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        out = g.tendencies(dY)
        assert g.status() == 0, "non-finite tendency flagged"
        return out


def gpu_fluxes(g, Y, Ya, face):
    n = g.case.ncols
    fe, fw = np.empty(n), np.empty(n)
    g.F.check(g.L.lh_boundary_fluxes(g.ctx, Y, Ya, 0.0, face, fe.ctypes.data_as(C.POINTER(C.c_double)),
                                     fw.ctypes.data_as(C.POINTER(C.c_double))), g.ctx)
    return fe, fw


def stable_dt(g, Y, Ya, courant=0.5):
    out = C.c_double()
    g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, courant, C.byref(out)), g.ctx)
    return out.value


@functools.lru_cache(maxsize=None)
def uniform_case(dtype, model, bc, factors, ice):
    return H.make_layered_heat(dtype, 700, 64, R.uniform_map(700, 64), model=model, bc=bc, factors=factors, ice=ice)


@functools.lru_cache(maxsize=None)
def horizon_case(dtype, model, bc=None):
    return H.make_layered_heat(dtype, 130, 64, R.horizon_map(130, 64), model=model, bc=bc or H.PER_CELL_BC[model])


def worst_cell(got, want):
    """the worst cell in units of the field's largest value"""
    w = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - w)) / np.max(np.abs(w)))


# ------------------------------------------------------------ column-uniform maps against the oracle

UNIFORM = ([(M.MODEL_COUPLED, bc, f, i) for bc in ("flux", "flux_drain", "dirichlet", "dirichlet_consistent")
            for f, i in ((False, False), (False, True), (True, False), (True, True))] +
           [(M.MODEL_HEAT, bc, False, i) for bc in ("flux", "dirichlet") for i in (False, True)])
UNIFORM_IDS = ["%s-%s-%s" % (MODEL_IDS[MODELS.index(m)], bc, {(False, False): "plain", (False, True): "ice", (True, False): "factors",
                                                                (True, True): "factors_ice"}[(f, i)]) for m, bc, f, i in UNIFORM]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model,bc,factors,ice", UNIFORM, ids=UNIFORM_IDS)
def test_column_uniform_maps_match_the_oracle(dtype, model, bc, factors, ice):
    """700 columns, column c of class c mod 16 at every level: the layered kernels must give the oracle's tendency
    called once per class with that class's hydraulic and thermal numbers as the scalar parameters (energy
    Dirichlet in the Dirichlet cases; the heat-only model has no hydrology faces and no conductivity factors)."""
    lay = uniform_case(dtype, model, bc, factors, ice)
    used, share = assert_close_per_class(lay, gpu_rhs(lay), plain=True)
    print("share of the model used at Cw = %g: %s; plain share %s" % (CW[np.dtype(dtype)], used, share))


# ------------------------------------------------------------ per-cell maps against the NumPy reference

def layered_figures(dtype, model):
    """per field: (worst cell of the layered run against the NumPy reference, worst cell of its column-uniform twin
    against the oracle, share of cells within PLAIN_REL), in units of the field's largest tendency.  The twin is
    the same state and tables with every column's map set to its bottom class."""
    lay = horizon_case(dtype, model)
    got, want = gpu_rhs(lay), H.rhs(lay)
    twin = H.LayeredHeat(lay.case, lay.classes, lay.thermal, R.bottom_class_map(lay.class_map))
    twin_got = gpu_rhs(twin)
    _, twin_want = oracle_per_class(twin)
    share = pc.plain_statistic(lay.case, got, want)
    return {k: (worst_cell(got[k], want[k]), worst_cell(twin_got[k], twin_want[k]), share[k]) for k in FIELDS[model]}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_layered_matches_the_numpy_reference(dtype, model):
    """130 x 64, 16 classes, horizons of unequal thickness that differ per column.  Per field the worst cell may be
    4 x the worst cell of the column-uniform twin against the oracle in the same run (floor PLAIN_REL), and the
    share within PLAIN_REL is at least PLAIN_SHARE_MIN: test_layered_matches_the_numpy_reference's rule."""
    dt = np.dtype(dtype)
    for k, (worst, twin_worst, share) in layered_figures(dtype, model).items():
        print("%s: layered worst cell %.3g, column-uniform twin %.3g, share within %g: %.4f" % (k, worst, twin_worst, pc.PLAIN_REL[dt], share))
        assert share >= pc.PLAIN_SHARE_MIN[dt], (k, share)
        assert worst <= 4.0 * max(twin_worst, pc.PLAIN_REL[dt]), (k, worst, twin_worst)


# ------------------------------------------------------------ at rest, and conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_isothermal_hydrostatic_column_is_at_rest_on_the_device(dtype, model):
    """the device's tendency of the column at rest, against the scale the NumPy REFERENCE gives for the same state
    with the map one level off its horizons (as test_layered_hydrostatic_column_is_at_rest_on_the_device takes it)"""
    rest = gpu_rhs(H.isothermal_hydrostatic(dtype, model))
    shifted = H.rhs(H.isothermal_hydrostatic(dtype, model, shift=1))
    for k in FIELDS[model]:
        r, s = np.abs(rest[k]).max(), np.abs(shifted[k]).max()
        print("%s: max|d| at rest %.3g, one level off its horizons %.3g, ratio %.3g" % (k, r, s, r / s))
        assert r <= 1e-6 * s, (k, r, s)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model,bc", [(M.MODEL_COUPLED, "flux"), (M.MODEL_COUPLED, "flux_drain"), (M.MODEL_COUPLED, "dirichlet"),
                                      (M.MODEL_HEAT, "flux"), (M.MODEL_HEAT, "dirichlet")])
def test_conservation_with_the_faces_lh_boundary_fluxes_returns(dtype, model, bc):
    lay = horizon_case(dtype, model, bc)
    with heat_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        d = g.tendencies(dY)
        faces = {f: gpu_fluxes(g, Y, Ya, f) for f in (M.FACE_BOTTOM, M.FACE_TOP)}
    print("conservation: worst column uses %s of the bound" % check_conservation(lay, {k: d[k] for k in FIELDS[model]}, faces))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model,bc", [(M.MODEL_COUPLED, "flux_drain"), (M.MODEL_COUPLED, "dirichlet"),
                                      (M.MODEL_COUPLED, "dirichlet_consistent"), (M.MODEL_HEAT, "dirichlet")])
def test_boundary_fluxes_are_bitwise_the_faces_of_the_tendency(dtype, model, bc):
    """One-level columns: both faces are boundary faces, so each tendency is f_bottom / dz - f_top / dz of the two
    returned fluxes, formed as the kernel forms it.  In the Dirichlet cases the energy face takes kappa from the
    boundary cell's own class, which differs from the context's scalars in kappa_sat_*, nu and nu_ss_om: the
    returned flux is the reference's with the class's numbers and not the one with the scalars'."""
    FT = np.dtype(dtype).type
    lay = H.make_layered_heat(dtype, 67, 1, R.horizon_map(67, 1, 16), model=model, bc=bc, zmin=-0.05)
    with heat_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        d = g.tendencies(dY)
        bot, top = gpu_fluxes(g, Y, Ya, M.FACE_BOTTOM), gpu_fluxes(g, Y, Ya, M.FACE_TOP)
    inv_dz = FT(1) / ((FT(0.0) - FT(-0.05)) / FT(1))
    for k, j in (("rhoe", 0), ("vl", 1)):
        if k in FIELDS[model]:
            assert np.array_equal(d[k][:, 0], bot[j].astype(dtype) * inv_dz - top[j].astype(dtype) * inv_dz), k
            assert np.any(d[k] != 0)
    if bc != "flux_drain":
        _, want = H.rhs(lay, faces=True)
        scalars = [getattr(lay.case.om.soil, n) for n in H.THERMAL_FIELDS]
        _, other = H.rhs(H.LayeredHeat(lay.case, lay.classes, np.repeat(np.array([scalars]), 16, axis=0), lay.class_map), faces=True)
        for face, got in ((M.FACE_BOTTOM, bot), (M.FACE_TOP, top)):
            w = want[face][0].astype(np.float64)
            gap = float(np.max(np.abs(got[0] - w)) / np.max(np.abs(w)))
            off = float(np.max(np.abs(other[face][0].astype(np.float64) - w)) / np.max(np.abs(w)))
            print("energy Dirichlet face %d: against the reference %.3g, the scalars' kappa would be off by %.3g" % (face, gap, off))
            # kappa to 8 Cw eps (parity_cases.closure_tolerances), T_face - T_c a difference of 285 K numbers over 5 K
            assert gap <= (8 + 2 * 285 / 4) * CW[np.dtype(dtype)] * np.finfo(dtype).eps, gap
            assert off > 1e-2


# ------------------------------------------------------------ shapes

def _one_column_runner(lay1):
    """rhs of single columns through ONE one-column context: state and map replaced per column"""
    g = heat_gpu(lay1)
    Y, Ya = g.prognostic_and_aux()
    dY = g.state(0)

    def run(vl, rhoe, cmap):
        upload_state(g, Y, Ya, vl, rhoe)
        g.set_soil_class_map(cmap)
        g.rhs(Y, Ya, dY)
        return g.tendencies(dY)
    return g, run


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 64])
@pytest.mark.parametrize("ncls", [1, 3, 16])
def test_shapes_columns_are_independent(dtype, model, nlev, ncls):
    """ncols in {1, 67, 130}: each column is bitwise what it is alone, a column permutation permutes the result
    bitwise, and a map given as [nelements] equals its broadcast."""
    classes, thermal = R.texture_classes()[:ncls], H.thermal_classes()[:ncls]
    mk = lambda ncols: H.make_layered_heat(dtype, ncols, nlev, R.horizon_map(ncols, nlev, ncls), model=model, classes=classes,
                                           thermal=thermal, bc="dirichlet")
    g1, run1 = _one_column_runner(mk(1))
    try:
        for ncols in (1, 67, 130):
            lay = mk(ncols)
            got = gpu_rhs(lay)
            for k in FIELDS[model]:
                assert np.all(np.isfinite(got[k]))
            for c in range(ncols):
                alone = run1(lay.case.vl[c:c + 1], lay.case.rhoe[c:c + 1], lay.class_map[c:c + 1])
                for k in FIELDS[model]:
                    assert np.array_equal(alone[k], got[k][c:c + 1]), (ncols, c, k)
            perm = np.random.default_rng(ncols).permutation(ncols)
            take = lambda a: np.ascontiguousarray(a[perm])
            plan = H.LayeredHeat(lay.case, classes, thermal, take(lay.class_map))
            moved = gpu_rhs(plan, vl=take(lay.case.vl), rhoe=take(lay.case.rhoe))
            row = np.ascontiguousarray(lay.class_map[0])
            same = H.LayeredHeat(lay.case, classes, thermal, np.ascontiguousarray(np.repeat(row[None, :], ncols, axis=0)))
            by_row, by_plane = gpu_rhs(lay, class_map=row), gpu_rhs(same)
            for k in FIELDS[model]:
                assert np.array_equal(moved[k], got[k][perm]), (ncols, k)
                assert np.array_equal(by_row[k], by_plane[k]), (ncols, k)
    finally:
        g1.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_known_zero_theta_i_equals_an_uploaded_zero_plane(dtype, model):
    """a theta_i plane the library knows to be zero (a fill: the NOICE kernels) gives bitwise the result of an
    uploaded all-zero one (the kernels that read it): the tendency and the three stages"""
    lay = horizon_case(dtype, model, "dirichlet")
    res = []
    for known in (True, False):
        with heat_gpu(lay) as g:
            F = g.F
            Y, Ya = g.prognostic_and_aux()      # (an all-zero theta_i goes up as a fill)
            if not known:
                z = np.zeros_like(lay.case.vl)
                F.check(g.L.lh_upload(g.ctx, Ya if model == M.MODEL_HEAT else Y, F.LH_VAR_THETA_I, z.ctypes.data, 1, lay.case.om.nlev), g.ctx)
            dY, U = g.state(0), g.state(0)
            g.rhs(Y, Ya, dY)
            out = [g.tendencies(dY)]
            dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
            for stage in (1, 2, 3):
                F.check(g.L.lh_ssprk33_stage(g.ctx, stage, Y, U, Ya, dt, None), g.ctx)
            out.append(state_of(g, Y))
            res.append(out)
    for k in FIELDS[model]:
        assert np.array_equal(res[0][0][k], res[1][0][k]) and np.array_equal(res[0][1][k], res[1][1][k]), k
    assert np.any(res[0][1]["rhoe"] != lay.case.rhoe)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_level_uniform_profiles_are_broadcast_before_a_layered_launch(dtype):
    """heat-only: the prescribed vartheta_l and theta_i handed over as level-uniform profiles (lh_upload_profile)
    give bitwise the tendency, the step bound and the stepped state of the same values uploaded as planes"""
    ncols, nlev = 67, 16
    lay = H.make_layered_heat(dtype, ncols, nlev, R.horizon_map(ncols, nlev), model=M.MODEL_HEAT, bc="dirichlet")
    lev = np.arange(nlev)
    vl = np.repeat((0.2 + 0.1 * np.sin(0.7 * lev))[None, :], ncols, axis=0).astype(dtype)     # inside every class's (theta_r, nu)
    ti = np.repeat(np.where(lev % 5 == 2, 0.02, 0.0)[None, :], ncols, axis=0).astype(dtype)
    om = lay.case.om
    zc, _ = R.grid_np(om.zmin, om.zmax, nlev)
    rhoe = H.rhoe_from_T(lay.classes, lay.thermal, lay.class_map, om, vl, ti.astype(np.float64), H._temperature_field(ncols, nlev, zc, False), dtype)
    res = []
    for profile in (True, False):
        case = dataclasses.replace(lay.case, vl=vl, ti=ti, rhoe=rhoe, aux_profile=profile)
        with heat_gpu(H.LayeredHeat(case, lay.classes, lay.thermal, lay.class_map)) as g:
            Y, Ya = g.prognostic_and_aux()
            dY = g.state(0)
            g.rhs(Y, Ya, dY)
            dt = stable_dt(g, Y, Ya, 0.5)
            g.F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, 0.5 * dt, 2, None), g.ctx)
            res.append((g.tendencies(dY)["rhoe"], dt, state_of(g, Y)["rhoe"]))
            assert g.status() == 0
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and np.array_equal(res[0][2], res[1][2])
    assert np.any(res[0][0] != 0) and np.any(res[0][2] != rhoe)


# ------------------------------------------------------------ stepping and the step bound

STEP_BOUND = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 3e-6}    # DESIGN.md section 2, of the field scale


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_step_ssprk33_matches_the_reference_and_is_reproducible(dtype, model):
    lay = horizon_case(dtype, model)
    nsteps = 20
    with heat_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        assert g.L.lh_step_engine(g.ctx, nsteps, 0) == F.LH_ENGINE_FUSED_STAGES
        dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
        F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, dt, nsteps, None), g.ctx)
        got = state_of(g, Y)
        Y1, _ = g.prognostic_and_aux()
        for _ in range(nsteps):
            F.check(g.L.lh_step_ssprk33(g.ctx, Y1, Ya, 0.0, dt, 1, None), g.ctx)
        one_by_one = state_of(g, Y1)
        assert g.status() == 0
    want = H.ssprk33(lay, dt, nsteps)
    want64 = H.ssprk33(H.as64(lay), dt, nsteps) if np.dtype(dtype) == np.float32 else None
    for k in FIELDS[model]:
        assert np.array_equal(got[k], one_by_one[k]), k
        start = getattr(lay.case, k).astype(np.float64)
        moved = float(np.max(np.abs(want[k].astype(np.float64) - start)) / np.max(np.abs(start)))
        err = worst_cell(got[k], want[k])
        print("%s after %d steps of %.3g s: %.3g of the field scale (the state moved by %.3g of it)" % (k, nsteps, dt, err, moved))
        if want64 is not None:   # the Float32 reference itself stays within the bound of the Float64 one here
            ref_gap = worst_cell(want[k], want64[k])
            print("%s: Float32 reference against the Float64 one: %.3g" % (k, ref_gap))
            assert ref_gap <= STEP_BOUND[np.dtype(dtype)], (k, ref_gap)
        assert moved > 1e-6, (k, moved)
        assert err <= STEP_BOUND[np.dtype(dtype)], (k, err)


def _column(lay, k):
    c = lay.case
    case = dataclasses.replace(c, ncols=1, vl=c.vl[k:k + 1], ti=c.ti[k:k + 1], rhoe=c.rhoe[k:k + 1])
    return H.LayeredHeat(case, lay.classes, lay.thermal, lay.class_map[k:k + 1])


def heat_governed_case(dtype, model):
    """low rho_c_ds, high kappa_sat, near-dry water: the heat term sets the bound (in the coupled model too).
    The classes' van Genuchten n is narrowed to 2.0 .. 2.4: the water rule takes the mean K of a face times the
    LARGER slope of its two cells, and between a class with n = 1.25 (slope 5e8 when dry) and one with n = 3.2 that
    product governs however dry the column is."""
    thermal = H.thermal_classes()
    thermal[:, 0] *= 0.2
    thermal[:, 3:5] *= 2.0
    classes = R.texture_classes()
    classes[:, 0] = 2.0 + 0.4 * ((np.arange(16) * 0.37) % 1.0)
    lay = H.make_layered_heat(dtype, 130, 64, R.horizon_map(130, 64), model=model, classes=classes, thermal=thermal, bc="flux")
    cls = lay.classes[lay.class_map]
    vl = (cls[..., 2] + 0.03 * (cls[..., 4] - cls[..., 2])).astype(dtype)
    om = lay.case.om
    zc, _ = R.grid_np(om.zmin, om.zmax, om.nlev)
    T = H._temperature_field(130, 64, zc, False)
    rhoe = H.rhoe_from_T(lay.classes, thermal, lay.class_map, om, vl, np.zeros(vl.shape), T, dtype)
    return H.LayeredHeat(dataclasses.replace(lay.case, vl=vl, rhoe=rhoe), lay.classes, thermal, lay.class_map)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model,which", [(M.MODEL_COUPLED, "water"), (M.MODEL_COUPLED, "heat"), (M.MODEL_HEAT, "heat")],
                         ids=["coupled-water", "coupled-heat", "heat-heat"])
def test_stable_dt_is_the_references_bound(dtype, model, which):
    """lh_stable_dt against the reference's bound, where the water governs and where the heat does; in the
    heat-governed case after ONE cell's class is swapped for the thermally most diffusive one (a cell of the
    column that sets the bound, the first for which the reference's bound falls and stays the heat's).  A cell has
    one class byte, so the swap replaces the WHOLE class, its hydraulic numbers included."""
    lay = horizon_case(dtype, model, "dirichlet") if which == "water" else heat_governed_case(dtype, model)
    want, w_water, w_heat = H.stable_dt(lay, 0.5, parts=True)
    assert (w_water < w_heat) == (which == "water"), (w_water, w_heat)
    swapped = want2 = None
    if which == "heat":
        percol = [H.stable_dt(_column(lay, k), 0.5) for k in range(lay.case.ncols)]
        k = int(np.argmin(percol))
        assert abs(percol[k] - want) <= 1e-12 * want
        d = H.diagnostics(lay)
        diffusivity = [np.max((d["kappa"] / d["rcs"])[lay.class_map == q], initial=0.0) for q in range(16)]
        best = int(np.argmax(diffusivity))
        for i in np.flatnonzero(lay.class_map[k] != best):
            m = lay.class_map.copy()
            m[k, i] = best
            w2, _, h2 = H.stable_dt(lay, 0.5, class_map=m, parts=True)
            if w2 < want and h2 == w2:
                swapped, want2 = m, w2
                break
        assert swapped is not None
    with heat_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        got = stable_dt(g, Y, Ya, 0.5)
        print("lh_stable_dt %.9g, reference %.9g (water %.6g, heat %.6g), relative difference %.3g" % (got, want, w_water, w_heat, abs(got - want) / want))
        assert abs(got - want) <= 1e-6 * want
        if swapped is not None:
            g.set_soil_class_map(swapped)
            got2 = stable_dt(g, Y, Ya, 0.5)
            print("one cell swapped: lh_stable_dt %.9g, reference %.9g, relative difference %.3g" % (got2, want2, abs(got2 - want2) / want2))
            assert abs(got2 - want2) <= 1e-6 * want2
            assert got2 < got and want2 < want


# ------------------------------------------------------------ diagnostics

def gpu_diagnostics(g):
    F = g.F
    Y, Ya = g.prognostic_and_aux()
    D = g.state(0b1111)
    F.check(g.L.lh_diagnostics(g.ctx, Y, Ya, D), g.ctx)
    return dict(K=g.download(D, F.LH_DIAG_K), psi=g.download(D, F.LH_DIAG_PSI), kappa=g.download(D, F.LH_DIAG_KAPPA),
                T=g.download(D, F.LH_DIAG_T))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_diagnostics_are_the_reference_closures_per_cell(dtype, model):
    """lh_diagnostics K, psi, T and kappa of every cell against the host closures with the cell's numbers, within
    the closure tolerances of the tendency model at the fixed cases' Cw (every cell taken as a one-level column
    with its own per-column parameters, which is what parity_cases.closure_tolerances reads)."""
    lay = H.make_layered_heat(dtype, 130, 64, R.horizon_map(130, 64), model=model, bc="flux", ice=True)
    with heat_gpu(lay) as g:
        got = gpu_diagnostics(g)
    want = H.diagnostics(lay)
    cells = lay.case.vl.size
    om = copy.deepcopy(lay.case.om)
    p = R.cell_params(lay)
    om.percol = {k2: p[k1].astype(np.float64).reshape(cells) for k1, k2 in
                 zip(R.CLASS_FIELDS, ("vg_n", "vg_alpha", "vg_theta_r", "vg_Ksat", "nu", "S_s"))}
    flat = dataclasses.replace(lay.case, om=om, ncols=cells, vl=lay.case.vl.reshape(cells, 1), ti=lay.case.ti.reshape(cells, 1))
    water = model != M.MODEL_HEAT
    zero = np.zeros((cells, 1))
    diag = dict(K=want["K"].reshape(cells, 1) if water else zero, psi=want["psi"].reshape(cells, 1) if water else zero,
                T=want["T"].reshape(cells, 1), kappa=want["kappa"].reshape(cells, 1))
    tol = pc.closure_tolerances(flat, diag, CW[np.dtype(dtype)])
    for name in (("K", "psi", "T", "kappa") if water else ("T", "kappa")):
        err = np.abs(got[name].astype(np.float64) - want[name].astype(np.float64)).reshape(cells, 1)
        print("%s: worst cell uses %.3g of the closure tolerance" % (name, float(np.max(err / tol[name]))))
        assert np.all(err <= tol[name]), name
    # a figure, not an assertion: T and kappa of a one-class map against the scalar launch with that class's numbers
    one = H.make_layered_heat(dtype, 130, 64, np.zeros((130, 64), np.uint8), model=model, classes=R.texture_classes()[3:4],
                              thermal=H.thermal_classes()[4:5], bc="flux", ice=True)
    with heat_gpu(one) as g:
        layered = gpu_diagnostics(g)
    with pc.GpuModel(H.class_scalar_case(one, 0, np.arange(130))) as g:
        scalar = gpu_diagnostics(g)
    print("one-class map against the scalar launch, bit for bit: T %s, kappa %s" % (np.array_equal(layered["T"], scalar["T"]),
                                                                                   np.array_equal(layered["kappa"], scalar["kappa"])))


# ------------------------------------------------------------ refusals and unchanged behaviour

def _refused(g, rc, code, *words):
    assert rc == code, (rc, g.L.lh_last_error(g.ctx))
    msg = g.L.lh_last_error(g.ctx).decode()
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_refusals(model):
    lay = H.make_layered_heat(np.float64, 67, 8, R.horizon_map(67, 8, 3), model=model, classes=R.texture_classes()[:3],
                              thermal=H.thermal_classes()[:3], bc="flux")
    F = pc._pkg()._ffi
    L = F.lib()
    sc = "soil classes"
    with pc.GpuModel(lay.case) as g:
        ctx = g.ctx
        Y, Ya = g.prognostic_and_aux()
        dY, U = g.state(0), g.state(0)
        g.rhs(Y, Ya, dY)
        before = g.tendencies(dY)["rhoe"]
        has = C.c_int32(-1)
        cmap = np.ascontiguousarray(lay.class_map)
        mp = cmap.ctypes.data_as(C.POINTER(C.c_uint8))
        cls = (F.lh_soil_class * 3)(*[F.lh_soil_class(*k) for k in lay.classes])
        th = (F.lh_soil_class_thermal * 3)(*[F.lh_soil_class_thermal(*k) for k in lay.thermal])
        # a count mismatch (before and after classes are set) and a NULL array
        _refused(g, L.lh_set_soil_class_thermal(ctx, 3, th), F.LH_EINVAL, "3 thermal classes", "0 soil classes")
        F.check(L.lh_set_soil_classes(ctx, 3, cls), ctx)
        _refused(g, L.lh_set_soil_class_thermal(ctx, 2, th), F.LH_EINVAL, "2 thermal classes", "3 soil classes")
        _refused(g, L.lh_set_soil_class_thermal(ctx, 3, None), F.LH_EINVAL, "NULL")
        F.check(L.lh_soil_class_thermal_info(ctx, C.byref(has)), ctx)
        assert has.value == 0
        # a map without the supplement: the old message
        _refused(g, L.lh_set_soil_class_map(ctx, mp, 1, 8), F.LH_EMODEL, sc, "LH_MODEL_RICHARDS")
        F.check(L.lh_set_soil_class_thermal(ctx, 3, th), ctx)
        F.check(L.lh_soil_class_thermal_info(ctx, C.byref(has)), ctx)
        assert has.value == 1
        # lh_set_soil_classes drops the supplement
        F.check(L.lh_set_soil_classes(ctx, 3, cls), ctx)
        F.check(L.lh_soil_class_thermal_info(ctx, C.byref(has)), ctx)
        assert has.value == 0
        _refused(g, L.lh_set_soil_class_map(ctx, mp, 1, 8), F.LH_EMODEL, sc, "LH_MODEL_RICHARDS")
        F.check(L.lh_set_soil_class_thermal(ctx, 3, th), ctx)
        F.check(L.lh_set_soil_class_map(ctx, mp, 1, 8), ctx)
        # ... so neither it nor removing the supplement is possible under a map
        _refused(g, L.lh_set_soil_classes(ctx, 3, cls), F.LH_EMODEL, "class map in place needs thermal properties")
        _refused(g, L.lh_set_soil_classes(ctx, 0, None), F.LH_EMODEL, "class map in place needs thermal properties")
        _refused(g, L.lh_set_soil_class_thermal(ctx, 0, None), F.LH_EMODEL, "class map in place")
        # the entry points without layered kernels
        dev = g.state(0)      # (any device word: the calls are refused before they read it)
        dptr, ls, cs = C.c_void_p(), C.c_int64(), C.c_int64()
        F.check(L.lh_state_device_ptr(ctx, dev, F.LH_VAR_RHOE_INT, C.byref(dptr), C.byref(ls), C.byref(cs)), ctx)
        _refused(g, L.lh_rhs_stable_dt(ctx, 0.0, Y, Ya, dY, 0.5, dptr), F.LH_EMODEL, sc, "lh_rhs_stable_dt")
        _refused(g, L.lh_step_ssprk33_device_dt(ctx, Y, Ya, 0.0, dptr, None), F.LH_EMODEL, sc, "lh_step_ssprk33_device_dt")
        _refused(g, L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, 0.5, 0.0, 1, dptr, None), F.LH_EMODEL, sc, "lh_step_ssprk33_adaptive")
        _refused(g, L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.5, 0.0, 1, 2, dptr, None), F.LH_EMODEL, sc,
                 "lh_step_ssprk33_adaptive_hold")
        _refused(g, L.lh_tune_placement(ctx, Y, Ya, dY, 0, 0, None, None), F.LH_EMODEL, sc, "lh_tune_placement")
        _refused(g, L.lh_step_layered_implicit_euler(ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), F.LH_EMODEL, sc,
                 "lh_step_layered_implicit_euler")
        _refused(g, L.lh_integrate_layered_trbdf2(ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), F.LH_EMODEL, sc,
                 "lh_integrate_layered_trbdf2")
        if model == M.MODEL_HEAT:
            _refused(g, L.lh_step_heat_implicit(ctx, Y, Ya, 0.0, 10.0, 1, 0, None), F.LH_EMODEL, sc, "lh_step_heat_implicit")
        else:
            _refused(g, L.lh_step_coupled_implicit(ctx, Y, Ya, 0.0, 10.0, 1, 0, None, 0.0, 0), F.LH_EMODEL, sc, "lh_step_coupled_implicit")
            _refused(g, L.lh_integrate_coupled_trbdf2(ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0.0, 0, None, None), F.LH_EMODEL, sc,
                     "lh_integrate_coupled_trbdf2")
        # a per-column parameter array together with the map, at every entry point that takes the layered kernels
        out, fw = C.c_double(), np.empty(lay.case.ncols)
        D = g.state(0b1111)

        def layered_calls():
            return (L.lh_rhs(ctx, 0.0, Y, Ya, dY), L.lh_ssprk33_stage(ctx, 1, Y, U, Ya, 1.0, None),
                    L.lh_step_ssprk33(ctx, Y, Ya, 0.0, 1.0, 1, None), L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(out)),
                    L.lh_diagnostics(ctx, Y, Ya, D),
                    L.lh_boundary_fluxes(ctx, Y, Ya, 0.0, 0, None, fw.ctypes.data_as(C.POINTER(C.c_double))))
        arr = np.full(lay.case.ncols, 0.45)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), ctx)
        for rc in layered_calls():
            _refused(g, rc, F.LH_EMODEL, sc, "per-column")
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], None), ctx)
        # LH_MATH_LIBM
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        _refused(g, L.lh_rhs(ctx, 0.0, Y, Ya, dY), F.LH_EMODEL, sc, "LH_MATH_LIBM")
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        # a prescribed-atmosphere top (the coupled model: the heat-only one has no such method)
        if model == M.MODEL_COUPLED:
            a = M.AtmosForcing()
            f = F.lh_atmos_forcing(a.u_atm, a.theta_atm, a.z_atm, a.theta_scale, a.rho_a_sfc, a.q_atm, 0.001, 0.001, a.R_v, a.R_d,
                                   a.grav, a.cp_d, a.cp_v, a.LH_v0, a.T_triple, a.press_triple, a.von_karman)
            F.check(L.lh_set_atmos_forcing(ctx, C.byref(f), None), ctx)
            for rc in layered_calls():
                _refused(g, rc, F.LH_EMODEL, sc, "prescribed-atmosphere")
            F.check(L.lh_set_atmos_forcing(ctx, None, None), ctx)
        # the layered tendency differs from the scalar one; without the map the scalar one is back, bitwise
        g.rhs(Y, Ya, dY)
        assert np.any(g.tendencies(dY)["rhoe"] != before)
        F.check(L.lh_set_soil_class_map(ctx, None, 0, 0), ctx)
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["rhoe"], before)
        # without the map the supplement and the classes may go
        F.check(L.lh_set_soil_class_thermal(ctx, 0, None), ctx)
        F.check(L.lh_set_soil_classes(ctx, 0, None), ctx)
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["rhoe"], before)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_the_class_tables_follow_the_contexts_scalars(dtype, model):
    """The Kersten exponent of a class reads the context's `a`, its k_dry the context's kappa_dry_parameter and the
    air's conductivity (lh_set_earth_params): classes, supplement and map set FIRST and lh_set_soil_params /
    lh_set_earth_params afterwards give bitwise the tendency, the step bound and kappa of the other order."""
    lay = H.make_layered_heat(dtype, 67, 16, R.horizon_map(67, 16), model=model, bc="dirichlet")
    om = lay.case.om
    om2 = dataclasses.replace(om, soil=dataclasses.replace(om.soil, a=0.4, kappa_dry_parameter=0.08),
                              earth=dataclasses.replace(om.earth, K_therm=0.03))
    late = H.LayeredHeat(dataclasses.replace(lay.case, om=om2), lay.classes, lay.thermal, lay.class_map)

    def run(first, then=None):
        with heat_gpu(first) as g:
            F, L, ctx = g.F, g.L, g.ctx
            if then is not None:      # the scalars change under the classes, the supplement and the map
                e, sp = then.earth, then.soil
                F.check(L.lh_set_soil_params(ctx, C.byref(F.lh_soil_params(*[getattr(sp, n[0]) for n in F.lh_soil_params._fields_]))), ctx)
                F.check(L.lh_set_earth_params(ctx, C.byref(F.lh_earth_params(e.rho_liq, e.rho_ice, e.cp_l, e.cp_i, e.T_0, e.LH_f0, e.K_therm))), ctx)
            Y, Ya = g.prognostic_and_aux()
            dY, D = g.state(0), g.state(0b1111)
            g.rhs(Y, Ya, dY)
            F.check(L.lh_diagnostics(ctx, Y, Ya, D), ctx)
            return g.tendencies(dY)["rhoe"], stable_dt(g, Y, Ya, 0.5), g.download(D, F.LH_DIAG_KAPPA)

    want, before, got = run(late), run(lay), run(lay, then=om2)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2])
    assert np.any(before[2] != want[2]) and np.any(before[0] != want[0])       # (the three scalars matter here)
    ref = H.diagnostics(late)["kappa"].astype(np.float64)
    print("kappa after the late setters against the reference: %.3g" % float(np.max(np.abs(got[2] - ref) / ref)))
    assert np.all(np.abs(got[2] - ref) <= 8 * CW[np.dtype(dtype)] * np.finfo(dtype).eps * ref)   # closure_tolerances' kappa


def test_a_richards_context_ignores_the_supplement():
    lay = R.make_layered(np.float64, 67, 8, R.horizon_map(67, 8, 3), classes=R.texture_classes()[:3])
    with pc.GpuModel(lay.case) as g:
        g.set_soil_classes(lay.classes, lay.class_map)
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        without = g.tendencies(dY)["vl"]
        g.set_soil_class_thermal(H.thermal_classes()[:3])
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["vl"], without)
        g.set_soil_class_thermal(None)     # (a Richards context may drop it under a map)
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["vl"], without) and np.any(without != 0)


# ------------------------------------------------------------ the host mirror

def test_host_mirror_three_horizons_through_simulation():
    """A three-horizon coupled SoilModel through Simulation(model, SSPRK33()) ends bitwise on the state of the same
    run through the C ABI; make_rhs, stable_dt and boundary_fluxes agree with the direct calls; everything else
    refuses in its check_scope."""
    lh = pc._pkg()
    FT = np.float64
    n, N = 48, 70
    classes, thermal = R.texture_classes()[[0, 5, 2]], H.thermal_classes()[[0, 4, 2]]
    horizons = np.zeros(n, dtype=np.int64)
    horizons[15:] = 1
    horizons[33:] = 2
    lay = H.make_layered_heat(FT, N, n, np.repeat(horizons[None, :], N, axis=0), classes=classes, thermal=thermal, bc="flux_drain")
    om = lay.case.om
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(H.THERMAL_FIELDS, t))))
                         for k, t in zip(classes, thermal)], horizons)
    e_bot, e_top = om.bc[(M.FACE_BOTTOM, M.COMP_ENERGY)][1], om.bc[(M.FACE_TOP, M.COMP_ENERGY)][1]
    dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(e_top), hydrology=lh.VerticalFlux(-2e-8)),
                         bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(e_bot), hydrology=lh.FreeDrainage()))
    model = lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT)), boundary_conditions=bc,
                         soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet(), soil_classes=sc)
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z, "ρe_int": 1e7 + 0.0 * z}, 0.0)
    Y.soil.ϑ_l = lay.case.vl
    Y.soil.ρe_int = lay.case.rhoe
    dt_stable = lh.stable_dt(model, Y, Ya)
    assert abs(dt_stable - H.stable_dt(lay, 0.5)) <= 1e-6 * dt_stable
    dY = Y.similar()
    lh.make_rhs(model)(dY, Y, Ya, 0.0)
    direct = gpu_rhs(lay)
    assert np.array_equal(np.array(dY.soil.ϑ_l), direct["vl"]) and np.array_equal(np.array(dY.soil.ρe_int), direct["rhoe"])
    with heat_gpu(lay) as g:
        Yc, Yac = g.prognostic_and_aux()
        fe, fw = gpu_fluxes(g, Yc, Yac, M.FACE_BOTTOM)
        fb = lh.boundary_fluxes((Y, Ya), model.boundary_conditions.bottom, "bottom", model)
        assert np.array_equal(np.asarray(fb["fϑ_l"], np.float64), fw) and np.array_equal(np.asarray(fb["fρe_int"], np.float64), fe)
        dt, nsteps = 0.5 * dt_stable, 12
        g.F.check(g.L.lh_step_ssprk33(g.ctx, Yc, Yac, 0.0, dt, nsteps, None), g.ctx)
        want = state_of(g, Yc)
    sim = lh.Simulation(model, lh.SSPRK33(), Y_init=Y, dt=dt, tspan=(0.0, nsteps * dt), Ya_init=Ya)
    lh.run(sim)
    assert np.array_equal(np.array(sim.integrator.u.soil.ϑ_l), want["vl"])
    assert np.array_equal(np.array(sim.integrator.u.soil.ρe_int), want["rhoe"]) and np.any(want["rhoe"] != lay.case.rhoe)
    for method in (lh.CoupledImplicitEuler(), lh.CoupledTRBDF2(), lh.CoupledAdaptiveTRBDF2()):
        with pytest.raises(NotImplementedError, match="soil classes"):
            lh.Simulation(model, method, Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.step_adaptive(model, Y, Ya)
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.tune_placement(model, Y, Ya, dY)
    model.close()


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 coupled only: Float32 and the heat-only model have one form.  ldexp_form: every context of the test is
# created under `vgfast=0` and asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left.)
from closure_form import ldexp_form  # noqa: E402,F401

COUPLED_UNIFORM = [u for u in UNIFORM if u[0] == M.MODEL_COUPLED]


@pytest.mark.parametrize("model,bc,factors,ice", COUPLED_UNIFORM, ids=[i for u, i in zip(UNIFORM, UNIFORM_IDS) if u[0] == M.MODEL_COUPLED])
def test_column_uniform_maps_match_the_oracle_ldexp_form(model, bc, factors, ice, ldexp_form):
    test_column_uniform_maps_match_the_oracle(np.float64, model, bc, factors, ice)


def test_layered_matches_the_numpy_reference_ldexp_form(ldexp_form):
    test_layered_matches_the_numpy_reference(np.float64, M.MODEL_COUPLED)


def test_step_ssprk33_matches_the_reference_and_is_reproducible_ldexp_form(ldexp_form):
    test_step_ssprk33_matches_the_reference_and_is_reproducible(np.float64, M.MODEL_COUPLED)
