"""Layered soils on the device: per-cell soil classes through lh_set_soil_classes / lh_set_soil_class_map, the
layered tendency, its fused SSPRK33 stages, the step bound, the diagnostics and the boundary fluxes -- against
the CPU oracle where a map can be written as per-column parameters, and against the NumPy restatement of the
layered tendency (tests/layered_ref.py) where it cannot."""
import ctypes as C
import functools

import numpy as np
import pytest

import case_model as M
import layered_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
CW = {np.dtype(np.float64): 2.0, np.dtype(np.float32): 4.0}   # the fixed cases' constants (tests/test_gpu_parity.py)


def layered_gpu(lay, class_map="own", **kw):
    """A context with the case's classes and (unless class_map is None) its class map set."""
    g = pc.GpuModel(lay.case, **kw)
    g.set_soil_classes(lay.classes, lay.class_map if isinstance(class_map, str) else class_map)
    return g


def gpu_rhs(lay, class_map="own", vl=None):
    with layered_gpu(lay, class_map) as g:
        Y, Ya = g.prognostic_and_aux()
        if vl is not None:
            g.upload(Y, g.F.LH_VAR_VARTHETA_L, vl)
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
def uniform_case(dtype, bc, factors, ice):
    return R.make_layered(dtype, 700, 64, R.uniform_map(700, 64), bc=bc, factors=factors, ice=ice)


@functools.lru_cache(maxsize=None)
def horizon_case(dtype, bc="flux_drain"):
    return R.make_layered(dtype, 130, 64, R.horizon_map(130, 64), bc=bc)


def worst_cell(got, want):
    """the worst cell in units of the field's largest tendency"""
    w = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - w)) / np.max(np.abs(w)))


# ------------------------------------------------------------ column-uniform maps against the oracle

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
@pytest.mark.parametrize("factors,ice", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "ice", "factors", "factors_ice"])
def test_column_uniform_maps_match_the_oracle(dtype, bc, factors, ice):
    """700 columns, column c of class c mod 16 at every level: the layered kernels must give the oracle's
    tendency with the matching per-column parameters (the regrouped face, true conductivities summed, differs
    from rhs_kernel's by rounding, so this is not bitwise the per-column launch)."""
    lay = uniform_case(dtype, bc, factors, ice)
    case = R.with_percol(lay)
    want = pc.O.rhs(case.om, case.vl, case.ti, None, case.T_aux)
    got = gpu_rhs(lay)
    print("share of the model used at Cw = %g: %s" % (CW[np.dtype(dtype)], pc.error_summary(case, got, want, CW[np.dtype(dtype)])))
    pc.assert_tendencies_close(case, got, want, Cw=CW[np.dtype(dtype)], plain=True)


# ------------------------------------------------------------ layered against the NumPy reference

def layered_figures(dtype):
    """(worst cell of the layered run against the NumPy reference, worst cell of its column-uniform twin
    against the oracle, share of cells within PLAIN_REL), all in units of the field's largest tendency.  The
    twin is the same state and table with every column's map set to its bottom class."""
    lay = horizon_case(dtype)
    got = gpu_rhs(lay)["vl"]
    want = R.rhs(lay)
    twin = R.Layered(lay.case, lay.classes, R.bottom_class_map(lay.class_map))
    tcase = R.with_percol(twin)
    twin_got = gpu_rhs(twin)["vl"]
    twin_want = pc.O.rhs(tcase.om, tcase.vl, tcase.ti, None, tcase.T_aux)["vl"]
    share = pc.plain_statistic(lay.case, dict(vl=got), dict(vl=want))["vl"]
    return worst_cell(got, want), worst_cell(twin_got, twin_want), share


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layered_matches_the_numpy_reference(dtype):
    """130 x 64, 16 classes, horizons of unequal thickness that differ per column, every interface a Ksat jump
    >= 100.  The worst cell may be 4 x the worst cell of the column-uniform twin against the oracle in the same
    run (floor PLAIN_REL): the 4 covers the interface faces, where one side's rounding is weighted by the other
    side's Ksat."""
    dt = np.dtype(dtype)
    worst, twin_worst, share = layered_figures(dtype)
    print("layered worst cell %.3g, column-uniform twin %.3g, share within %g: %.4f" % (worst, twin_worst, pc.PLAIN_REL[dt], share))
    assert share >= pc.PLAIN_SHARE_MIN[dt], share
    assert worst <= 4.0 * max(twin_worst, pc.PLAIN_REL[dt]), (worst, twin_worst)


# ------------------------------------------------------------ hydrostatic and conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layered_hydrostatic_column_is_at_rest_on_the_device(dtype):
    rest = np.abs(gpu_rhs(R.hydrostatic(dtype))["vl"]).max()
    shifted = np.abs(R.rhs(R.hydrostatic(dtype, shift=1))).max()
    print("hydrostatic: max|d| %.3g, one level off its horizons %.3g" % (rest, shifted))
    assert rest <= 1e-6 * shifted, (rest, shifted)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux", "flux_drain", "dirichlet"])
def test_conservation_with_the_faces_lh_boundary_fluxes_returns(dtype, bc):
    lay = horizon_case(dtype, bc)
    om = lay.case.om
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        d = g.tendencies(dY)["vl"].astype(np.float64)
        f_bot = gpu_fluxes(g, Y, Ya, M.FACE_BOTTOM)[1]
        f_top = gpu_fluxes(g, Y, Ya, M.FACE_TOP)[1]
    dz = (om.zmax - om.zmin) / om.nlev
    eps = float(np.finfo(dtype).eps)
    bound = om.nlev * 4 * eps * np.abs(d).sum(axis=1) * dz
    err = np.abs(d.sum(axis=1) * dz - (f_bot - f_top))
    print("conservation: worst column uses %.3g of the bound" % float(np.max(err / bound)))
    assert np.all(err <= bound)


# ------------------------------------------------------------ shapes

def _one_column_runner(lay1):
    """rhs of single columns through ONE one-column context: state, map and boundary values replaced per column"""
    g = layered_gpu(lay1)
    Y, Ya = g.prognostic_and_aux()
    dY = g.state(0)

    def run(vl, cmap):
        g.upload(Y, g.F.LH_VAR_VARTHETA_L, vl)
        g.set_soil_class_map(cmap)
        g.rhs(Y, Ya, dY)
        return g.download(dY, g.F.LH_VAR_VARTHETA_L)
    return g, run


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 64])
@pytest.mark.parametrize("ncls", [1, 3, 16])
def test_shapes_columns_are_independent(dtype, nlev, ncls):
    """ncols in {1, 67, 130}: each column is bitwise what it is alone, a column permutation permutes the result
    bitwise, and a map given as [nelements] equals its broadcast."""
    classes = R.texture_classes()[:ncls]
    alone = R.make_layered(dtype, 1, nlev, R.horizon_map(1, nlev, ncls), classes=classes, bc="dirichlet")
    g1, run1 = _one_column_runner(alone)
    try:
        for ncols in (1, 67, 130):
            lay = R.make_layered(dtype, ncols, nlev, R.horizon_map(ncols, nlev, ncls), classes=classes, bc="dirichlet")
            got = gpu_rhs(lay)["vl"]
            assert np.all(np.isfinite(got))
            for c in range(ncols):
                assert np.array_equal(run1(lay.case.vl[c:c + 1], lay.class_map[c:c + 1]), got[c:c + 1]), (ncols, c)
            perm = np.random.default_rng(ncols).permutation(ncols)
            plan = R.Layered(lay.case, classes, np.ascontiguousarray(lay.class_map[perm]))
            assert np.array_equal(gpu_rhs(plan, vl=np.ascontiguousarray(lay.case.vl[perm]))["vl"], got[perm]), ncols
            row = np.ascontiguousarray(lay.class_map[0])
            same = R.Layered(lay.case, classes, np.ascontiguousarray(np.repeat(row[None, :], ncols, axis=0)))
            assert np.array_equal(gpu_rhs(lay, class_map=row)["vl"], gpu_rhs(same)["vl"]), ncols
    finally:
        g1.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_known_zero_theta_i_equals_an_uploaded_zero_plane(dtype):
    """a theta_i plane the library knows to be zero (a fill: the NOICE kernels) gives bitwise the result of an
    uploaded all-zero one (the kernels that read it)"""
    lay = horizon_case(dtype, "dirichlet")
    res = []
    for known in (True, False):
        with layered_gpu(lay) as g:
            F = g.F
            Y, Ya = g.prognostic_and_aux()      # (an all-zero theta_i goes up as a fill)
            if not known:
                z = np.zeros_like(lay.case.vl)
                F.check(g.L.lh_upload(g.ctx, Y, F.LH_VAR_THETA_I, z.ctypes.data, 1, lay.case.om.nlev), g.ctx)
            dY, U = g.state(0), g.state(0)
            g.rhs(Y, Ya, dY)
            out = [g.tendencies(dY)["vl"]]
            for stage in (1, 2, 3):
                F.check(g.L.lh_ssprk33_stage(g.ctx, stage, Y, U, Ya, 50.0, None), g.ctx)
            out.append(g.download(Y, F.LH_VAR_VARTHETA_L))
            res.append(out)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.any(res[0][1] != lay.case.vl)


# ------------------------------------------------------------ stepping and the step bound

STEP_BOUND = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 3e-6}    # DESIGN.md section 2, of the field scale


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_step_ssprk33_matches_the_reference_and_is_reproducible(dtype):
    lay = horizon_case(dtype)
    nsteps = 20
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        assert g.L.lh_step_engine(g.ctx, nsteps, 0) == F.LH_ENGINE_FUSED_STAGES
        dt = 0.5 * stable_dt(g, Y, Ya, 0.5)
        F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, dt, nsteps, None), g.ctx)
        got = g.download(Y, F.LH_VAR_VARTHETA_L)
        Y1, _ = g.prognostic_and_aux()
        for _ in range(nsteps):
            F.check(g.L.lh_step_ssprk33(g.ctx, Y1, Ya, 0.0, dt, 1, None), g.ctx)
        one_by_one = g.download(Y1, F.LH_VAR_VARTHETA_L)
        assert g.status() == 0
    assert np.array_equal(got, one_by_one)
    want = R.ssprk33(lay, dt, nsteps)
    moved = float(np.max(np.abs(want.astype(np.float64) - lay.case.vl)))
    err = worst_cell_of_state(got, want)
    print("theta(z, t) after %d steps of %.3g s: %.3g of the field scale (the state moved by %.3g)" % (nsteps, dt, err, moved))
    if np.dtype(dtype) == np.float32:   # the Float32 reference itself stays within the bound of the Float64 one here
        lay64 = R.Layered(_as64(lay.case), lay.classes, lay.class_map)
        ref_gap = worst_cell_of_state(want, R.ssprk33(lay64, dt, nsteps))
        print("Float32 reference against the Float64 one: %.3g" % ref_gap)
        assert ref_gap <= STEP_BOUND[np.dtype(dtype)], ref_gap
    assert moved > 1e-6
    assert err <= STEP_BOUND[np.dtype(dtype)], err


def worst_cell_of_state(got, want):
    w = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - w)) / np.max(np.abs(w)))


def _as64(case):
    import dataclasses
    return dataclasses.replace(case, dtype=np.float64, vl=case.vl.astype(np.float64), ti=case.ti.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet"])
def test_stable_dt_is_the_references_bound(dtype, bc):
    """lh_stable_dt against the reference's bound, and after ONE cell's class is swapped for the most conductive
    one (a cell of the column that sets the bound, the first for which the reference's bound falls)."""
    lay = horizon_case(dtype, bc)
    want = R.stable_dt(lay, 0.5)
    best = int(np.argmax(lay.classes[:, 3]))
    percol = [R.stable_dt(R.Layered(_column(lay.case, k), lay.classes, lay.class_map[k:k + 1]), 0.5)
              for k in range(lay.case.ncols)]
    k = int(np.argmin(percol))
    assert abs(percol[k] - want) <= 1e-12 * want
    swapped = want2 = None
    for i in np.flatnonzero(lay.class_map[k] != best):
        m = lay.class_map.copy()
        m[k, i] = best
        w2 = R.stable_dt(lay, 0.5, class_map=m)
        if w2 < want:
            swapped, want2 = m, w2
            break
    assert swapped is not None
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        got = stable_dt(g, Y, Ya, 0.5)
        print("lh_stable_dt %.9g, reference %.9g, relative difference %.3g" % (got, want, abs(got - want) / want))
        assert abs(got - want) <= 1e-6 * want
        g.set_soil_class_map(swapped)
        got2 = stable_dt(g, Y, Ya, 0.5)
        print("one cell swapped: lh_stable_dt %.9g, reference %.9g" % (got2, want2))
        assert abs(got2 - want2) <= 1e-6 * want2
        assert got2 < got


def _column(case, k):
    import dataclasses
    return dataclasses.replace(case, ncols=1, vl=case.vl[k:k + 1], ti=case.ti[k:k + 1],
                               T_aux=None if case.T_aux is None else case.T_aux[k:k + 1])


# ------------------------------------------------------------ diagnostics and boundary fluxes

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_diagnostics_are_the_reference_closures_per_cell(dtype):
    """lh_diagnostics K and psi of every cell against the host closures with the cell's parameters, within the
    closure tolerances of the tendency model at the fixed cases' Cw (every cell taken as a one-level column
    with its own per-column parameters, which is what parity_cases.closure_tolerances reads)."""
    lay = R.make_layered(dtype, 130, 64, R.horizon_map(130, 64), bc="flux_drain", ice=True)
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        D = g.state(0b1111)
        F.check(g.L.lh_diagnostics(g.ctx, Y, Ya, D), g.ctx)
        K, psi = g.download(D, F.LH_DIAG_K), g.download(D, F.LH_DIAG_PSI)
    want = R.diagnostics(lay)
    import copy
    import dataclasses
    cells = lay.case.vl.size
    om = copy.deepcopy(lay.case.om)
    p = R.cell_params(lay)
    om.percol = {k2: p[k1].astype(np.float64).reshape(cells) for k1, k2 in
                 zip(R.CLASS_FIELDS, ("vg_n", "vg_alpha", "vg_theta_r", "vg_Ksat", "nu", "S_s"))}
    flat = dataclasses.replace(lay.case, om=om, ncols=cells, vl=lay.case.vl.reshape(cells, 1), ti=lay.case.ti.reshape(cells, 1))
    diag = dict(K=want["K"].reshape(cells, 1), psi=want["psi"].reshape(cells, 1), T=np.full((cells, 1), 288.0),
                kappa=np.zeros((cells, 1)))
    tol = pc.closure_tolerances(flat, diag, CW[np.dtype(dtype)])
    for name, got in (("K", K), ("psi", psi)):
        err = np.abs(got.astype(np.float64) - want[name].astype(np.float64)).reshape(cells, 1)
        print("%s: worst cell uses %.3g of the closure tolerance" % (name, float(np.max(err / tol[name]))))
        assert np.all(err <= tol[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent"])
def test_boundary_fluxes_are_bitwise_the_faces_of_the_tendency(dtype, bc):
    """One-level columns: both faces are boundary faces, so the tendency is f_bottom / dz - f_top / dz of the
    two returned fluxes, formed as the kernel forms it (each flux times 1/dz, then the difference)."""
    FT = np.dtype(dtype).type
    lay = R.make_layered(dtype, 67, 1, R.horizon_map(67, 1, 16), bc=bc, zmin=-0.05)
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        d = g.tendencies(dY)["vl"][:, 0]
        f_bot = gpu_fluxes(g, Y, Ya, M.FACE_BOTTOM)[1].astype(dtype)
        f_top = gpu_fluxes(g, Y, Ya, M.FACE_TOP)[1].astype(dtype)
    inv_dz = FT(1) / ((FT(0.0) - FT(-0.05)) / FT(1))
    assert np.array_equal(d, f_bot * inv_dz - f_top * inv_dz)
    assert np.any(d != 0)


# ------------------------------------------------------------ refusals

def _refused(g, rc, code, *words):
    assert rc == code, (rc, g.L.lh_last_error(g.ctx))
    msg = g.L.lh_last_error(g.ctx).decode()
    for w in words:
        assert w in msg, msg


def test_refusals():
    lay = R.make_layered(np.float64, 67, 8, R.horizon_map(67, 8, 3), classes=R.texture_classes()[:3])
    F = pc._pkg()._ffi
    L = F.lib()
    with pc.GpuModel(lay.case) as g:
        ctx = g.ctx
        Y, Ya = g.prognostic_and_aux()
        dY, U = g.state(0), g.state(0)
        g.rhs(Y, Ya, dY)
        before = g.tendencies(dY)["vl"]
        n, has = C.c_int32(-1), C.c_int32(-1)
        F.check(L.lh_soil_class_info(ctx, C.byref(n), C.byref(has)), ctx)
        assert (n.value, has.value) == (0, 0)
        cmap = np.ascontiguousarray(lay.class_map)
        mp = cmap.ctypes.data_as(C.POINTER(C.c_uint8))
        # no classes yet; class counts outside 0 .. 16; a NULL array
        _refused(g, L.lh_set_soil_class_map(ctx, mp, 1, 8), F.LH_EMODEL, "no soil classes")
        cls = (F.lh_soil_class * 17)(*[F.lh_soil_class(*R.texture_classes()[k % 16]) for k in range(17)])
        _refused(g, L.lh_set_soil_classes(ctx, 17, cls), F.LH_EINVAL, "0 .. 16")
        _refused(g, L.lh_set_soil_classes(ctx, -1, cls), F.LH_EINVAL, "0 .. 16")
        _refused(g, L.lh_set_soil_classes(ctx, 2, None), F.LH_EINVAL, "NULL")
        # an index >= nclasses, with the first offending (column, level)
        F.check(L.lh_set_soil_classes(ctx, 3, cls), ctx)
        bad = cmap.copy()
        bad[5, 2] = 3
        bad[9, 1] = 7
        _refused(g, L.lh_set_soil_class_map(ctx, bad.ctypes.data_as(C.POINTER(C.c_uint8)), 1, 8), F.LH_EINVAL,
                 "class 3", "column 5, level 2")
        F.check(L.lh_soil_class_info(ctx, C.byref(n), C.byref(has)), ctx)
        assert (n.value, has.value) == (3, 0)
        F.check(L.lh_set_soil_class_map(ctx, mp, 1, 8), ctx)
        F.check(L.lh_soil_class_info(ctx, C.byref(n), C.byref(has)), ctx)
        assert (n.value, has.value) == (3, 1)
        # fewer classes than the map in place uses
        assert cmap.max() == 2
        _refused(g, L.lh_set_soil_classes(ctx, int(cmap.max()), cls), F.LH_EINVAL, "class map in place")
        # the entry points without layered kernels
        dev = g.state(0)      # (any device word: the calls are refused before they read it)
        dptr, ls, cs = C.c_void_p(), C.c_int64(), C.c_int64()
        F.check(L.lh_state_device_ptr(ctx, dev, F.LH_VAR_VARTHETA_L, C.byref(dptr), C.byref(ls), C.byref(cs)), ctx)
        sc = "soil classes"
        _refused(g, L.lh_rhs_stable_dt(ctx, 0.0, Y, Ya, dY, 0.5, dptr), F.LH_EMODEL, sc, "lh_rhs_stable_dt")
        _refused(g, L.lh_step_ssprk33_device_dt(ctx, Y, Ya, 0.0, dptr, None), F.LH_EMODEL, sc, "lh_step_ssprk33_device_dt")
        _refused(g, L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, 0.5, 0.0, 1, dptr, None), F.LH_EMODEL, sc, "lh_step_ssprk33_adaptive")
        _refused(g, L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, 0.5, 0.0, 1, 2, dptr, None), F.LH_EMODEL, sc,
                 "lh_step_ssprk33_adaptive_hold")
        _refused(g, L.lh_step_implicit_euler(ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), F.LH_EMODEL, sc, "lh_step_implicit_euler")
        _refused(g, L.lh_integrate_trbdf2(ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), F.LH_EMODEL, sc, "lh_integrate_trbdf2")
        _refused(g, L.lh_tune_placement(ctx, Y, Ya, dY, 0, 0, None, None), F.LH_EMODEL, sc, "lh_tune_placement")
        # a per-column parameter array together with the map, at every entry point that takes the layered kernels
        arr = np.full(lay.case.ncols, 0.45)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), ctx)
        out, fw = C.c_double(), np.empty(lay.case.ncols)
        D = g.state(0b1111)
        for rc in (L.lh_rhs(ctx, 0.0, Y, Ya, dY), L.lh_ssprk33_stage(ctx, 1, Y, U, Ya, 1.0, None),
                   L.lh_step_ssprk33(ctx, Y, Ya, 0.0, 1.0, 1, None), L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(out)),
                   L.lh_diagnostics(ctx, Y, Ya, D),
                   L.lh_boundary_fluxes(ctx, Y, Ya, 0.0, 0, None, fw.ctypes.data_as(C.POINTER(C.c_double)))):
            _refused(g, rc, F.LH_EMODEL, sc, "per-column")
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], None), ctx)
        # LH_MATH_LIBM
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        _refused(g, L.lh_rhs(ctx, 0.0, Y, Ya, dY), F.LH_EMODEL, sc, "LH_MATH_LIBM")
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        # lh_stream_probe is untouched
        ms = C.c_float()
        F.check(L.lh_stream_probe(ctx, Y, 0b01, dY, 0b01, 1, C.byref(ms)), ctx)
        # the layered tendency differs from the scalar one; without the map the scalar one is back, bitwise
        g.rhs(Y, Ya, dY)
        assert np.any(g.tendencies(dY)["vl"] != before)
        F.check(L.lh_set_soil_class_map(ctx, None, 0, 0), ctx)
        F.check(L.lh_soil_class_info(ctx, C.byref(n), C.byref(has)), ctx)
        assert (n.value, has.value) == (3, 0)
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["vl"], before)
        # nclasses = 0 removes the classes and the map
        F.check(L.lh_set_soil_class_map(ctx, mp, 1, 8), ctx)
        F.check(L.lh_set_soil_classes(ctx, 0, None), ctx)
        F.check(L.lh_soil_class_info(ctx, C.byref(n), C.byref(has)), ctx)
        assert (n.value, has.value) == (0, 0)
        g.rhs(Y, Ya, dY)
        assert np.array_equal(g.tendencies(dY)["vl"], before)
    # any model but Richards
    heat = pc.make_case("heat_dirichlet_f64", ncols=4)
    with pc.GpuModel(heat) as g:
        F.check(L.lh_set_soil_classes(g.ctx, 3, cls), g.ctx)
        m = np.zeros((4, heat.om.nlev), dtype=np.uint8)
        _refused(g, L.lh_set_soil_class_map(g.ctx, m.ctypes.data_as(C.POINTER(C.c_uint8)), 1, heat.om.nlev), F.LH_EMODEL,
                 "soil classes", "LH_MODEL_RICHARDS")


# ------------------------------------------------------------ the host mirror

def test_host_mirror_three_horizons_through_simulation():
    """A three-horizon SoilModel through Simulation(model, SSPRK33()) ends on the state of the same run through
    the C ABI; make_rhs, stable_dt and boundary_fluxes go through the layered kernels; everything else refuses."""
    lh = pc._pkg()
    FT = np.float64
    n, N = 48, 70
    classes = R.texture_classes()[[0, 5, 2]]
    horizons = np.zeros(n, dtype=np.int64)
    horizons[15:] = 1
    horizons[33:] = 2
    lay = R.make_layered(FT, N, n, np.repeat(horizons[None, :], N, axis=0), classes=classes, bc="flux_drain")
    om = lay.case.om

    def build(soil_classes, **kw):
        dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-2e-8)),
                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage()))
        args = dict(domain=dom, energy_model=lh.PrescribedTemperatureModel(),
                    hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT)),
                    boundary_conditions=bc, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet(),
                    soil_classes=soil_classes)
        args.update(kw)
        return lh.SoilModel(FT, **args)

    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3]), ν=k[4], S_s=k[5])
                         for k in classes], horizons)
    model = build(sc)
    vl0 = lay.case.vl
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z}, 0.0)
    Y.soil.ϑ_l = vl0
    dt_stable = lh.stable_dt(model, Y, Ya)
    assert abs(dt_stable - R.stable_dt(lay, 0.5)) <= 1e-6 * dt_stable
    dY = Y.similar()
    lh.make_rhs(model)(dY, Y, Ya, 0.0)
    d = np.array(dY.soil.ϑ_l)
    assert np.array_equal(d, gpu_rhs(lay)["vl"])
    fb = lh.boundary_fluxes((Y, Ya), model.boundary_conditions.bottom, "bottom", model)["fϑ_l"]
    assert np.all(fb < 0) and np.all(np.isfinite(fb))
    dt, nsteps = 0.5 * dt_stable, 12
    sim = lh.Simulation(model, lh.SSPRK33(), Y_init=Y, dt=dt, tspan=(0.0, nsteps * dt), Ya_init=Ya)
    lh.run(sim)
    got = np.array(sim.integrator.u.soil.ϑ_l)
    with layered_gpu(lay) as g:
        Yc, Yac = g.prognostic_and_aux()
        g.F.check(g.L.lh_step_ssprk33(g.ctx, Yc, Yac, 0.0, dt, nsteps, None), g.ctx)
        want = g.download(Yc, g.F.LH_VAR_VARTHETA_L)
    assert np.array_equal(got, want) and np.any(got != vl0)
    # what has no layered kernels refuses in its check_scope; what the library would refuse, at construction
    for method in (lh.ImplicitEuler(), lh.TRBDF2()):
        with pytest.raises(NotImplementedError, match="soil classes"):
            lh.Simulation(model, method, Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.step_adaptive(model, Y, Ya)
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.tune_placement(model, Y, Ya, dY)
    with pytest.raises(lh.ModelError, match="soil classes"):
        build(sc, energy_model=lh.SoilEnergyModel())
    with pytest.raises(lh.ModelError, match="per-column"):
        build(sc, soil_param_set=lh.SoilParams(FT, ν=np.full(N, 0.45)))
    with pytest.raises(lh.ModelError, match="class 3"):
        lh.SoilClasses(sc.classes, np.array([0, 1, 3]))
    with pytest.raises(ValueError, match="class_map has shape"):
        build(lh.SoilClasses(sc.classes, horizons[:-1]))
    # [ncolumns, nelements] is the same model
    model2 = build(lh.SoilClasses(sc.classes, np.repeat(horizons[None, :], N, axis=0)))
    Y2, Ya2 = lh.initialize_states(model2, lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z}, 0.0)
    Y2.soil.ϑ_l = vl0
    dY2 = Y2.similar()
    lh.make_rhs(model2)(dY2, Y2, Ya2, 0.0)
    assert np.array_equal(np.array(dY2.soil.ϑ_l), d)
    model.close()
    model2.close()


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
@pytest.mark.parametrize("factors,ice", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "ice", "factors", "factors_ice"])
def test_column_uniform_maps_match_the_oracle_ldexp_form(bc, factors, ice, ldexp_form):
    test_column_uniform_maps_match_the_oracle(np.float64, bc, factors, ice)


def test_layered_matches_the_numpy_reference_ldexp_form(ldexp_form):
    test_layered_matches_the_numpy_reference(np.float64)


def test_step_ssprk33_matches_the_reference_and_is_reproducible_ldexp_form(ldexp_form):
    test_step_ssprk33_matches_the_reference_and_is_reproducible(np.float64)
