"""lh_step_layered_coupled_implicit: implicit steps of the coupled water and heat model with per-cell soil classes on
the device, checked through the library's own layered tendency (lh_rhs of the same context), against
lh_step_layered_implicit_euler on the Richards twin, against the NumPy reference
(tests/layered_coupled_implicit_ref.py), and its host contract.  Mirrors tests/test_gpu_coupled_implicit.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu

NAME, SCALAR = "lh_step_layered_coupled_implicit", "lh_step_coupled_implicit"
METHODS = ("euler", "trbdf2")
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}          # the library's defaults
VL_BOUND = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 2e-5}     # tests/test_gpu_coupled_implicit.py's
HYDS = {"flux": (M.BC_FLUX, M.BC_FLUX), "dirichlet_drain": (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE),
        "drain_dirichlet": (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET), "dirichlet": (M.BC_DIRICHLET, M.BC_DIRICHLET)}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def flags_of(F, method):
    return F.LH_COUPLED_TRBDF2 if method == "trbdf2" else 0


def coupled_gpu(lay, **kw):
    """A context with the case's classes, their thermal supplement and its class map (heat_gpu of
    tests/test_gpu_layered_heat_implicit.py)."""
    g = pc.GpuModel(lay.case, **kw)
    g.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    return g


class Device:
    """One layered coupled context for several runs from the case's own state."""

    def __init__(self, lay):
        self.lay = lay
        self.g = coupled_gpu(lay)
        self.Y, self.Ya = self.g.prognostic_and_aux()
        self.dY = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.g.close()

    def restore(self):
        g, F = self.g, self.g.F
        g.upload(self.Y, F.LH_VAR_VARTHETA_L, self.lay.case.vl)
        g.upload(self.Y, F.LH_VAR_RHOE_INT, self.lay.case.rhoe)

    def stats(self):
        g = self.g
        mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
        g.F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        g.F.check(g.L.lh_implicit_iterations(g.ctx, C.byref(tot)), g.ctx)
        return mi.value, un.value, tot.value

    def steps(self, dt, nsteps, method="euler", bcv=None, calls=1, tol=0.0, max_iter=0, restore=True):
        """(vl, rhoe, (max iterations, unconverged, iterations) of the last call, status) after `calls` calls of
        nsteps each; bcv [calls * nsteps + 1][2][2] is split at the seams."""
        g, F = self.g, self.g.F
        if restore:
            self.restore()
        for k in range(calls):
            b = None if bcv is None else np.ascontiguousarray(bcv[k * nsteps:(k + 1) * nsteps + 1], dtype=np.float64)
            F.check(getattr(g.L, NAME)(g.ctx, self.Y, self.Ya, k * nsteps * dt, dt, nsteps, flags_of(F, method), ptr(b),
                                       tol, max_iter), g.ctx)
        st = self.stats()
        return g.download(self.Y, F.LH_VAR_VARTHETA_L), g.download(self.Y, F.LH_VAR_RHOE_INT), st, g.status()

    def rhs(self, vl, rhoe):
        """lh_rhs of this context at (vl, rhoe): Float64 arrays of FT values"""
        g, dt = self.g, self.lay.case.dtype
        if self.dY is None:
            self.dY = g.state(0)
            self.Y2, _ = g.prognostic_and_aux()
        g.upload(self.Y2, g.F.LH_VAR_VARTHETA_L, np.ascontiguousarray(vl, dtype=dt))
        g.upload(self.Y2, g.F.LH_VAR_RHOE_INT, np.ascontiguousarray(rhoe, dtype=dt))
        g.rhs(self.Y2, self.Ya, self.dY)
        t = g.tendencies(self.dY)
        return t["vl"].astype(np.float64), t["rhoe"].astype(np.float64)


def richards_twin(lay):
    """The Richards case with the same classes, map, water state, ice and hydrology faces."""
    om = dataclasses.replace(lay.case.om, model=M.MODEL_RICHARDS,
                             bc={k: v for k, v in lay.case.om.bc.items() if k[1] == M.COMP_HYDROLOGY})
    om.percol_bc = {k: v for k, v in lay.case.om.percol_bc.items() if k[1] == M.COMP_HYDROLOGY}
    return R.Layered(dataclasses.replace(lay.case, om=om, rhoe=None), lay.classes, lay.class_map)


# ------------------------------------------------------------------ 1. the residual through the tendency

def check_residual(lay, label, mults=(10.0, 100.0)):
    """One backward-Euler step at 10x and 100x the stable step (mults), R = Y1 - Yn - dt lh_rhs(Y1) of the same layered
    context.  Water: <= 10 tol nu (1 + 4 mult) + the round-off of evaluating R, nu the largest class porosity, every
    column converged.  Energy: <= max(4 r_ref, 8 eps ||rhoe_int||), r_ref the same residual of the reference solution
    rounded to FT (tests/test_gpu_coupled_implicit.py::test_residual_through_the_tendency's rules)."""
    dtype = lay.case.dtype
    vl0, re0 = LC.state64(lay)
    tol, eps = TOL[np.dtype(dtype)], float(np.finfo(dtype).eps)
    nu = float(lay.classes[:, 4].max())
    sd = LC.stable_dt(lay)
    with Device(lay) as d:
        for mult in mults:
            dt = mult * sd
            v1, e1, (mi, un, _), st = d.steps(dt, 1)
            assert un == 0 and st == 0, (mult, mi, un, st)
            assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1))

            def res(v, e):
                fv, fe = d.rhs(v, e)
                v, e = v.astype(np.float64), e.astype(np.float64)
                big = np.maximum(np.abs(v).max(axis=1), dt * np.abs(fv).max(axis=1))
                return np.max(np.abs(v - vl0 - dt * fv), axis=1), 64 * eps * big, float(np.max(np.abs(e - re0 - dt * fe)))

            rw, round_off, r_dev = res(v1, e1)
            bound = 10 * tol * nu * (1 + 4 * mult) + round_off
            vr, er, _ = LC.coupled_implicit(lay, vl0, re0, dt, 1)
            _, _, r_ref = res(vr.astype(dtype), er.astype(dtype))
            floor = 8 * eps * np.max(np.abs(re0))
            print(f"residual {label} {np.dtype(dtype).name} {mult}x: iterations {mi}, water {rw.max():.3g} "
                  f"(bound {bound.min():.3g}), energy device {r_dev:.3g} reference {r_ref:.3g} floor {floor:.3g}")
            assert np.all(rw <= bound), (mult, float(np.max(rw / bound)))
            assert r_dev <= max(4 * r_ref, floor), (mult, r_dev, r_ref, floor)
            assert np.max(np.abs(v1 - lay.case.vl)) > 0 and np.max(np.abs(e1 - lay.case.rhoe)) > 0
        return d.g.L.lh_closure_form(d.g.ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
@pytest.mark.parametrize("hyd", ["flux", "dirichlet_drain", "drain_dirichlet"])
@pytest.mark.parametrize("shape", [(130, 24, "horizons"), (67, 12, "cells")], ids=["130x24_horizons", "67x12_cells"])
def test_residual_through_the_tendency(shape, hyd, ice, dtype):
    """check_residual on 130 x 24 with three horizons and on 67 x 12 with a class per cell (5 classes, two organic),
    hydrology pairs flux/flux, Dirichlet/free drainage and free drainage/Dirichlet, with and without ice."""
    ncols, nlev, kind = shape
    # The three horizons under a free-draining top and a Dirichlet bottom are classes 2, 5, 0 bottom to top, not the
    # 0, 5, 2 of the other cases: with class 0 (n = 1.25) on the wetted Dirichlet face the safeguarded Newton of the
    # NumPy reference itself leaves columns unconverged at 100x (3 to 7 of 130 under the device's rule and cap of 50,
    # 2 after 400 iterations to round-off), so "every column converged" would test the method's reach, not the kernel.
    # tests/test_layered_coupled_implicit_reference.py asserts that fact about the reference.
    classes = R.texture_classes()[[2, 5, 0]] if (kind == "horizons" and hyd == "drain_dirichlet") else None
    lay = LC.layered_case(dtype, ncols, nlev, kind=kind, hyd=HYDS[hyd], energy="dirichlet" if hyd != "flux" else "flux", ice=ice,
                          classes=classes)
    check_residual(lay, f"{shape} {hyd} ice={ice}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
def test_residual_on_the_map_set_aside_at_10x(ice, dtype):
    """The map the case above set aside -- 130 x 24, classes 0, 5, 2 bottom to top, a free-draining top over a
    Dirichlet bottom -- at 10x the stable step, where the reference's Newton converges in every column (CPU test):
    the same rules."""
    lay = LC.layered_case(dtype, 130, 24, kind="horizons", hyd=HYDS["drain_dirichlet"], energy="dirichlet", ice=ice)
    check_residual(lay, f"horizons 0,5,2 drain_dirichlet ice={ice}", mults=(10.0,))


# ------------------------------------------------------------------ 2. the water stage is the layered Richards call

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
@pytest.mark.parametrize("hyd", ["dirichlet_drain", "drain_dirichlet"])
def test_the_water_stage_is_lh_step_layered_implicit_euler(hyd, ice, dtype):
    """vartheta_l after 2 coupled backward-Euler steps at 30x is bitwise lh_step_layered_implicit_euler's on the
    Richards context with the same classes, map, ice and hydrology faces; 600 columns (more than one workgroup, a
    ragged last wave); the Newton statistics are equal too."""
    lay = LC.layered_case(dtype, 600, 12, kind="cells", hyd=HYDS[hyd], energy="dirichlet", ice=ice)
    dt = 30 * LC.stable_dt(lay)
    with Device(lay) as d:
        v1, e1, stats, st = d.steps(dt, 2)
    twin = richards_twin(lay)
    with pc.GpuModel(twin.case) as g:
        g.set_soil_classes(twin.classes, twin.class_map)
        Y, Ya = g.prognostic_and_aux()
        g.F.check(g.L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, dt, 2, None, 0.0, 0), g.ctx)
        mr, ur, tr = C.c_int32(), C.c_int64(), C.c_int64()
        g.F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mr), C.byref(ur)), g.ctx)
        g.F.check(g.L.lh_implicit_iterations(g.ctx, C.byref(tr)), g.ctx)
        vr = g.download(Y, g.F.LH_VAR_VARTHETA_L)
        assert g.status() == 0
    np.testing.assert_array_equal(v1, vr)
    assert stats == (mr.value, ur.value, tr.value) and stats[1] == 0 and st == 0, (stats, st)
    assert np.max(np.abs(v1 - lay.case.vl)) > 0 and np.max(np.abs(e1 - lay.case.rhoe)) > 0


# ------------------------------------------------------------------ 3. parity with the NumPy reference

_REFERENCES = {}   # computed once per (case, step, method, table), shared, never modified


def _references(key, lay, dt, nsteps, method, bcv):
    """(the reference iterated to round-off, d, ||rhoe_int||): d is what the device's stopping rule alone costs
    (Float64) or what storing the state in Float32 alone costs -- from the reference alone."""
    key = key + (np.dtype(lay.case.dtype).name, float(dt), nsteps, method, None if bcv is None else bcv.tobytes())
    if key not in _REFERENCES:
        vl, re = LC.state64(lay)
        run = lambda **kw: LC.coupled_implicit(lay, vl, re, dt, nsteps, method, bcv=bcv, **kw)
        exact = run()
        other = run(tol=TOL[np.dtype(np.float64)]) if lay.case.dtype == np.float64 else run(round_to=np.float32)
        _REFERENCES[key] = (exact, float(np.max(np.abs(other[1] - exact[1]))), float(np.max(np.abs(re))))
    return _REFERENCES[key]


def check_parity(d, key, dt, nsteps, method, bcv=None, label="", got=None):
    """tests/test_gpu_coupled_implicit.py::check_parity's rule: vartheta_l within VL_BOUND, rhoe_int within
    4 d + 64 eps ||rhoe_int||; the ratio is printed before it is asserted."""
    lay = d.lay
    (vr, er, info), dd, scale = _references(key, lay, dt, nsteps, method, bcv)
    v1, e1, (mi, un, _), st = got if got is not None else d.steps(dt, nsteps, method, bcv=bcv)
    assert un == 0 and st == 0 and info["unconverged"] == 0, (mi, un, st, info)
    eps = float(np.finfo(lay.case.dtype).eps)
    dv = float(np.max(np.abs(v1.astype(np.float64) - vr)))
    de = float(np.max(np.abs(e1.astype(np.float64) - er)))
    bound = 4 * dd + 64 * eps * scale
    print(f"parity {label} {method} {np.dtype(lay.case.dtype).name} {key} nsteps={nsteps}: vl {dv:.3g}, rhoe {de:.3g}, "
          f"d {dd:.3g}, bound {bound:.3g}, ratio {de / bound:.3g}")
    assert dv <= VL_BOUND[np.dtype(lay.case.dtype)], dv
    assert de <= bound, (de, dd, bound)
    return v1, e1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("nlev", [1, 2, 3, 12])
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_parity_shapes(ncols, nlev, dtype):
    """A class per cell; a ragged last wave (67, 130 columns), both faces on one cell, no interior face, one interior
    cell; one and five steps of both methods at 30x the stable step."""
    lay = LC.layered_case(dtype, ncols, nlev, kind="cells", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)
    dt = 30 * LC.stable_dt(lay)
    with Device(lay) as d:
        for method in METHODS:
            for nsteps in (1, 5):
                check_parity(d, ("shapes", ncols, nlev), dt, nsteps, method, label="shapes")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["horizons_67x60", "bottom_dirichlet", "bottom_dirichlet_flux_top", "percol"])
def test_parity_cases(case, dtype):
    """67 x 60 with three horizons; Dirichlet energy at the bottom with a Dirichlet and with a flux top (G_b in the
    pivot of cell 0, in the right-hand side and in TR-BDF2's tendency sweep); per-column Dirichlet values.  3 steps of
    both methods at 30x."""
    kw = {"horizons_67x60": dict(ncols=67, nlev=60, kind="horizons", energy="dirichlet"),
          "bottom_dirichlet": dict(ncols=67, nlev=12, kind="cells", energy="dirichlet"),
          "bottom_dirichlet_flux_top": dict(ncols=67, nlev=12, kind="cells", energy="mixed"),
          "percol": dict(ncols=67, nlev=12, kind="cells", energy="dirichlet", percol_bc=True)}[case]
    hyd = HYDS["dirichlet" if case == "percol" else "drain_dirichlet" if case.startswith("bottom") else "dirichlet_drain"]
    lay = LC.layered_case(dtype, hyd=hyd, ice=True, **kw)
    dt = 30 * LC.stable_dt(lay)
    with Device(lay) as d:
        for method in METHODS:
            v1, e1 = check_parity(d, (case,), dt, 3, method, label=case)
            assert np.max(np.abs(e1 - lay.case.rhoe)) > 0


# ------------------------------------------------------------------ 8. the clay form

LDEXP, NOT_APPLICABLE = 0, 2      # lh_closure_form (tests/closure_form.py)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
def test_clay_form(ice, dtype):
    """67 x 12, a class per cell from a table whose fifth class has n = 1.06 (layered_adaptive_cases.clay_table's class
    5: m < 0.07, so the host chooses the v_ldexp closure form for the whole table, and in Float64 the VGF = false
    kernels run; lh_closure_form is asserted, Float32 has one form).  Rule 1 (the residual at 10x and 100x) and
    rule 3 (parity, 1 and 5 steps of both methods at 30x)."""
    import layered_adaptive_cases as AC
    classes = AC.clay_table()[[0, 1, 2, 3, AC.CLAY_CLASS]]
    assert classes[4, 0] == 1.06
    lay = LC.layered_case(dtype, 67, 12, kind="cells", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=ice, classes=classes)
    assert np.any(lay.class_map == 4)
    want = LDEXP if dtype == np.float64 else NOT_APPLICABLE
    assert check_residual(lay, f"clay ice={ice}") == want
    dt = 30 * LC.stable_dt(lay)
    with Device(lay) as d:
        for method in METHODS:
            for nsteps in (1, 5):
                check_parity(d, ("clay", ice), dt, nsteps, method, label="clay")
        assert d.g.L.lh_closure_form(d.g.ctx) == want


# ------------------------------------------------------------------ 5. bitwise invariances

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_bitwise_invariances(method, dtype):
    """2N steps in one call against N + N with bcv split at the seam; the first 67 columns of a 130-column run against
    the 67-column run; a repeated call from the same state.  TR-BDF2 recomputes f_n at the seam (one tendency sweep
    per call, where the one-call run carries f_n+1 = z_1 / h): its split run is held to rule 3's bound instead."""
    N = 3
    mk = lambda ncols: LC.layered_case(dtype, ncols, 12, kind="cells", hyd=HYDS["dirichlet"], energy="dirichlet", ice=True)
    lay = mk(130)
    dt = 30 * LC.stable_dt(lay)
    bcv = np.zeros((2 * N + 1, 2, 2))
    k = np.arange(2 * N + 1)
    bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY], bcv[:, M.FACE_TOP, M.COMP_ENERGY] = 281.0 + 0.3 * k, 287.0 - 0.4 * k
    bcv[:, M.FACE_BOTTOM, M.COMP_HYDROLOGY], bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = 0.26 + 0.002 * k, 0.30 - 0.003 * k
    with Device(lay) as d:
        one = d.steps(dt, 2 * N, method, bcv=bcv)
        again = d.steps(dt, 2 * N, method, bcv=bcv)
        two = d.steps(dt, N, method, bcv=bcv, calls=2)
        np.testing.assert_array_equal(one[0], again[0])
        np.testing.assert_array_equal(one[1], again[1])
        assert one[3] == 0 and np.max(np.abs(one[1] - lay.case.rhoe)) > 0
        if method == "euler":
            np.testing.assert_array_equal(one[0], two[0])
            np.testing.assert_array_equal(one[1], two[1])
        else:
            check_parity(d, ("seam",), dt, 2 * N, method, bcv=bcv, label="split at the seam", got=two)
    small = mk(67)
    np.testing.assert_array_equal(small.case.vl, lay.case.vl[:67])
    np.testing.assert_array_equal(small.class_map, lay.class_map[:67])
    with Device(small) as d:
        part = d.steps(dt, 2 * N, method, bcv=bcv)
    np.testing.assert_array_equal(part[0], one[0][:67])
    np.testing.assert_array_equal(part[1], one[1][:67])


# ------------------------------------------------------------------ 6. conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_conservation_with_flux_faces(method, dtype):
    """Flux faces in both components, ice, 50 steps at 30x the stable step, 67 x 60: sum_i rhoe_int changes by
    nsteps dt (F_b - F_t) / dz to nlev 4 eps sum |rhoe_int|, sum_i vartheta_l by the same expression to
    nlev 4 eps sum |vartheta_l| -- the same bound for both, without the scalar file's tol nu allowance for the Newton's
    stopping rule (DESIGN sections 4.16, 4.24).  Each ratio to the bound is printed before it is asserted."""
    fe_t, fe_b, fw_t, fw_b = -2.0, 3.0, -2e-9, -5e-10
    lay = LC.layered_case(dtype, 67, 60, kind="horizons", hyd=HYDS["flux"], energy="flux", ice=True)
    om = lay.case.om
    om.bc[(M.FACE_TOP, M.COMP_ENERGY)], om.bc[(M.FACE_BOTTOM, M.COMP_ENERGY)] = (M.BC_FLUX, fe_t), (M.BC_FLUX, fe_b)
    om.bc[(M.FACE_TOP, M.COMP_HYDROLOGY)], om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (M.BC_FLUX, fw_t), (M.BC_FLUX, fw_b)
    nsteps, dt = 50, 30 * LC.stable_dt(lay)
    n, eps = om.nlev, float(np.finfo(dtype).eps)
    with Device(lay) as d:
        v1, e1, (mi, un, _), st = d.steps(dt, nsteps, method)
    assert un == 0 and st == 0
    vl0, re0 = LC.state64(lay)
    dz = (om.zmax - om.zmin) / om.nlev
    for name, got, was, fb, ft in (("rhoe", e1, re0, fe_b, fe_t), ("vl", v1, vl0, fw_b, fw_t)):
        change = got.astype(np.float64).sum(axis=1) - was.sum(axis=1)
        want = nsteps * dt * (fb - ft) / dz
        allowed = n * 4 * eps * np.abs(was).sum(axis=1)
        print(f"conservation {name} {method} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} "
              f"of the bound, expected change {want:.3g}")
        assert abs(want) > 0
        assert np.all(np.abs(change - want) <= allowed), (name, float(np.max(np.abs(change - want) / allowed)))


# ------------------------------------------------------------------ 7. boundary values in time

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_boundary_values_in_time(dtype):
    """A ramped Dirichlet T and vartheta_l at the top through bcv over 4 steps: backward Euler is bitwise four
    lh_set_bc + one-step calls at the sampled times t_k+1; TR-BDF2 is within rule 3's bound of the reference reading
    the same table."""
    lay = LC.layered_case(dtype, 67, 12, kind="cells", hyd=HYDS["dirichlet"], energy="dirichlet", ice=True)
    n, dt = 4, 30 * LC.stable_dt(lay)
    bcv = np.zeros((n + 1, 2, 2))
    k = np.arange(n + 1)
    bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY], bcv[:, M.FACE_BOTTOM, M.COMP_HYDROLOGY] = 281.0, 0.26
    bcv[:, M.FACE_TOP, M.COMP_ENERGY], bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = 287.0 - 0.75 * k, 0.30 - 0.004 * k
    with Device(lay) as d:
        g, F = d.g, d.g.F
        v1, e1, _, st = d.steps(dt, n, "euler", bcv=bcv)
        assert st == 0
        d.restore()
        for s in range(1, n + 1):
            for face in (M.FACE_BOTTOM, M.FACE_TOP):
                for comp in (M.COMP_ENERGY, M.COMP_HYDROLOGY):
                    F.check(g.L.lh_set_bc(g.ctx, face, comp, F.LH_BC_DIRICHLET, float(bcv[s, face, comp]), None), g.ctx)
            F.check(getattr(g.L, NAME)(g.ctx, d.Y, d.Ya, (s - 1) * dt, dt, 1, 0, None, 0.0, 0), g.ctx)
        np.testing.assert_array_equal(g.download(d.Y, F.LH_VAR_VARTHETA_L), v1)
        np.testing.assert_array_equal(g.download(d.Y, F.LH_VAR_RHOE_INT), e1)
        assert g.status() == 0
        for face in (M.FACE_BOTTOM, M.FACE_TOP):      # back to the case's own values
            for comp in (M.COMP_ENERGY, M.COMP_HYDROLOGY):
                F.check(g.L.lh_set_bc(g.ctx, face, comp, F.LH_BC_DIRICHLET, float(lay.case.om.bc[(face, comp)][1]), None), g.ctx)
        check_parity(d, ("ramp",), dt, n, "trbdf2", bcv=bcv, label="ramp")
        # the table is read: another ramp gives another state
        other = d.steps(dt, n, "euler", bcv=bcv[::-1].copy())
        assert np.max(np.abs(other[1] - e1)) > 0


# ------------------------------------------------------------------ 9. the host contract

NCOLS, NLEV = 5, 6
COUPLED_ONLY = ": coupled models only (SoilEnergyModel + SoilHydrologyModel)"
LAYERED_OTHER_MODEL = " is not available with soil classes (a class map is set) on this model: it steps coupled models only (SoilEnergyModel + SoilHydrologyModel)"
NO_CLASS_MAP = ": the context has no class map (lh_set_soil_class_map); lh_step_coupled_implicit steps a model without soil classes"
PERCOL = ": soil classes (a class map is set) cannot be combined with per-column parameter arrays (lh_set_percol_param)"
LIBM = ": soil classes (a class map is set) have no LH_MATH_LIBM kernels"
ATMOS = ": soil classes (a class map is set) cannot be combined with a prescribed-atmosphere top (lh_set_atmos_forcing)"
FACTORS = ": conductivity factors other than NoEffect are not supported"
SCALAR_WITH_CLASSES = (" is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, "
                       "lh_step_ssprk33, lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are")


def tiny(**kw):
    return LH.make_layered_heat(np.float64, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), model=M.MODEL_COUPLED,
                                classes=R.texture_classes()[:2], thermal=LH.thermal_classes()[:2], bc="dirichlet", **kw)


def call(g, Y, Ya, dt=100.0, nsteps=1, flags=0, name=NAME, tol=0.0, max_iter=0):
    return getattr(g.L, name)(g.ctx, Y, Ya, 0.0, dt, nsteps, flags, None, tol, max_iter)


def refused(g, rc, code, message):
    assert rc == code, (rc, code, g.L.lh_last_error(g.ctx))
    assert g.L.lh_last_error(g.ctx).decode() == message, g.L.lh_last_error(g.ctx)


def test_refusals_in_their_order():
    lay = tiny()
    # the arguments, then the wrong model: a Richards context with a map, a heat-only context with one, a heat-only
    # context without
    rich = R.make_layered(np.float64, NCOLS, NLEV, R.uniform_map(NCOLS, NLEV, 2), classes=R.texture_classes()[:2])
    with pc.GpuModel(rich.case) as g:
        g.set_soil_classes(rich.classes, rich.class_map)
        Y, Ya = g.prognostic_and_aux()
        for dt, nsteps in ((0.0, 1), (-1.0, 1), (float("nan"), 1), (1.0, -1)):
            assert call(g, Y, Ya, dt, nsteps) == g.F.LH_EINVAL
        refused(g, call(g, Y, Ya, flags=2), g.F.LH_EINVAL, NAME + ": unknown flags 0x2")
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + LAYERED_OTHER_MODEL)
        assert getattr(g.L, NAME)(None, Y, Ya, 0.0, 1.0, 1, 0, None, 0.0, 0) == g.F.LH_EINVAL
    with pc.GpuModel(rich.case) as g:                                 # (the same model without a map)
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + COUPLED_ONLY)
    # a coupled context without a map: the scalar call is named, and steps it
    with pc.GpuModel(lay.case) as g:
        Y, Ya = g.prognostic_and_aux()
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        refused(g, call(g, Y, Ya, flags=g.F.LH_COUPLED_TRBDF2), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        g.set_soil_classes(lay.classes, None, thermal=lay.thermal)     # classes alone are not a map
        refused(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + NO_CLASS_MAP)
        g.F.check(call(g, Y, Ya, name=SCALAR), g.ctx)
        assert g.status() == 0
    # layered_check (a prescribed atmosphere, per-column arrays, LH_MATH_LIBM, in its order), then conductivity factors,
    # then the states -- every refusal before the states is shown with Y = NULL; and the scalar call's old words on the
    # same context.  (implicit_refusals' own atmosphere line comes after the factors and is not reachable with a map:
    # layered_check refuses the atmosphere first, which is the order the header gives.)
    with coupled_gpu(lay) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        arr = np.full(NCOLS, 0.45)
        a = M.AtmosForcing()
        f = F.lh_atmos_forcing(a.u_atm, a.theta_atm, a.z_atm, a.theta_scale, a.rho_a_sfc, a.q_atm, 0.001, 0.001, a.R_v, a.R_d,
                               a.grav, a.cp_d, a.cp_v, a.LH_v0, a.T_triple, a.press_triple, a.von_karman)
        F.check(L.lh_set_atmos_forcing(ctx, C.byref(f), None), ctx)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), ctx)
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        refused(g, call(g, None, Ya), F.LH_EMODEL, NAME + ATMOS)          # all three set: the atmosphere first
        refused(g, call(g, None, Ya, flags=F.LH_COUPLED_TRBDF2), F.LH_EMODEL, NAME + ATMOS)
        F.check(L.lh_set_atmos_forcing(ctx, None, None), ctx)
        refused(g, call(g, None, Ya), F.LH_EMODEL, NAME + PERCOL)         # then the per-column arrays
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], None), ctx)
        refused(g, call(g, None, Ya), F.LH_EMODEL, NAME + LIBM)           # then LH_MATH_LIBM
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        assert call(g, None, Ya) == F.LH_ESTATE
        refused(g, call(g, Y, Ya, name=SCALAR), F.LH_EMODEL, SCALAR + SCALAR_WITH_CLASSES)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), lay.case.rhoe)
        F.check(call(g, Y, Ya), ctx)
        assert np.any(g.download(Y, F.LH_VAR_RHOE_INT) != lay.case.rhoe) and g.status() == 0
    fac = tiny(factors=True)
    with coupled_gpu(fac) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        refused(g, call(g, None, Ya), F.LH_EMODEL, NAME + LIBM)           # layered_check before the factors
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        refused(g, call(g, None, Ya), F.LH_EMODEL, NAME + FACTORS)        # the factors before the states


@pytest.mark.parametrize("flags", [0, 1])
def test_nothing_to_do(flags):
    """nsteps == 0 returns LH_OK and leaves Y as uploaded, on a fresh context and after a step."""
    lay = tiny()
    with coupled_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        F.check(call(g, Y, Ya, nsteps=0, flags=flags), g.ctx)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), lay.case.rhoe)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_VARTHETA_L), lay.case.vl)
        F.check(call(g, Y, Ya, flags=flags), g.ctx)
        after = g.download(Y, F.LH_VAR_RHOE_INT)
        assert np.any(after != lay.case.rhoe) and np.all(np.isfinite(after))
        F.check(call(g, Y, Ya, nsteps=0, flags=flags), g.ctx)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), after)
        assert g.status() == 0


@pytest.mark.parametrize("flags", [0, 1])
def test_max_iter_one_sets_status_bit_3_and_counts(flags):
    """max_iter = 1 at 1000 stable steps: status bit 3 and nothing else, the largest count is 1, the number of
    unconverged column-stages is the one the NumPy reference counts under the same rule and cap (every column-stage:
    ncols x stages), and the energy solve at the last iterate is finite."""
    lay = tiny()
    dt = 1000 * LC.stable_dt(lay)
    method = "trbdf2" if flags else "euler"
    want = LC.coupled_implicit(lay, *LC.state64(lay), dt, 1, method, tol=TOL[np.dtype(np.float64)], max_iter=1)[2]["unconverged"]
    assert want == NCOLS * (2 if flags else 1)
    with coupled_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        g.F.check(call(g, Y, Ya, dt=dt, flags=flags, max_iter=1), g.ctx)
        mi, un = C.c_int32(), C.c_int64()
        g.F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        assert g.status() == 8 and mi.value == 1
        assert un.value == want
        assert np.all(np.isfinite(g.download(Y, g.F.LH_VAR_RHOE_INT)))


@pytest.mark.parametrize("flags", [0, 1])
def test_nonfinite_energy_sets_status_bit_0(flags):
    lay = tiny()
    rhoe = lay.case.rhoe.copy()
    rhoe[1, 1] = np.nan
    with coupled_gpu(LH.LayeredHeat(dataclasses.replace(lay.case, rhoe=rhoe), lay.classes, lay.thermal, lay.class_map)) as g:
        Y, Ya = g.prognostic_and_aux()
        g.F.check(call(g, Y, Ya, flags=flags), g.ctx)
        assert g.status() == 1
        out = g.download(Y, g.F.LH_VAR_RHOE_INT)
        assert np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))      # (columns are independent)
        assert np.all(np.isfinite(g.download(Y, g.F.LH_VAR_VARTHETA_L)))            # (the water does not read rhoe_int)


# ------------------------------------------------------------------ 4. against the scalar call

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("method", METHODS)
def test_column_uniform_classes_against_the_scalar_call(method, dtype):
    """67 x 12 with every column one of 3 classes, split by per_class_cases into scalar contexts stepped by
    lh_step_coupled_implicit, 3 steps at 30x: within rule 3's bounds (not bitwise: the layered water path carries
    true conductivities K_r Ksat, the scalar one relative ones with Ksat folded into the gradient's factor)."""
    lay = LC.layered_case(dtype, 67, 12, kind="columns", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)
    dt = 30 * LC.stable_dt(lay)
    with Device(lay) as d:
        v1, e1 = check_parity(d, ("columns",), dt, 3, method, label="columns")
    (_, er, _), dd, scale = _references(("columns",), lay, dt, 3, method, None)
    eps = float(np.finfo(dtype).eps)
    bound = 4 * dd + 64 * eps * scale
    worst_v = worst_e = 0.0
    for cols, case in LH.per_class_cases(lay):
        with pc.GpuModel(case) as g:
            Y, Ya = g.prognostic_and_aux()
            g.F.check(getattr(g.L, SCALAR)(g.ctx, Y, Ya, 0.0, dt, 3, flags_of(g.F, method), None, 0.0, 0), g.ctx)
            vs, es = g.download(Y, g.F.LH_VAR_VARTHETA_L), g.download(Y, g.F.LH_VAR_RHOE_INT)
            assert g.status() == 0
        worst_v = max(worst_v, float(np.max(np.abs(vs.astype(np.float64) - v1[cols]))))
        worst_e = max(worst_e, float(np.max(np.abs(es.astype(np.float64) - e1[cols]))))
    print(f"layered against scalar {method} {np.dtype(dtype).name}: vl {worst_v:.3g}, rhoe {worst_e:.3g} "
          f"({worst_e / scale:.3g} of ||rhoe_int||), bound {bound:.3g}, ratio {worst_e / bound:.3g}")
    assert worst_v <= VL_BOUND[np.dtype(dtype)] and worst_e <= bound


# ------------------------------------------------------------------ 10. the host mirror

def test_host_mirror_three_horizons_through_simulation():
    """A three-horizon coupled SoilModel with a diurnal sine as its Dirichlet top temperature through
    Simulation(model, LayeredCoupledTRBDF2(), saveat=...): bitwise the direct C calls, one per saveat chunk, with the
    table sampled at the same times.  The markers on a model without soil_classes, or on a heat-only model, raise in
    the library's words."""
    import math
    lh = pc._pkg()
    FT = np.float64
    n, N = 12, 5
    lay = LC.layered_case(FT, N, n, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    om, case = lay.case.om, lay.case
    bottom, day, fw = 281.0, 86400.0, -2e-9
    top = lambda t: 287.0 + 4.0 * math.sin(2.0 * math.pi * t / day)
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(LH.THERMAL_FIELDS, t))))
                         for k, t in zip(lay.classes, lay.thermal)], lay.class_map[0].astype(np.int64))
    dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.Dirichlet(top), hydrology=lh.VerticalFlux(fw)),
                         bottom=lh.SoilComponentBC(energy=lh.Dirichlet(bottom), hydrology=lh.FreeDrainage()))
    model = lh.SoilModel(FT, domain=dom, boundary_conditions=bc, soil_param_set=lh.SoilParams(FT),
                         earth_param_set=lh.EarthParameterSet(), energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT), soil_classes=sc)

    def start():
        Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.2 + 0.0 * z, "θ_i": 0.0 * z, "ρe_int": 1e7 + 0.0 * z}, 0.0)
        Y.soil.ϑ_l, Y.soil.ρe_int = case.vl, case.rhoe
        return Y, Ya

    Y, Ya = start()
    dt, total, chunk = 30 * LC.stable_dt(lay), 12, 4
    sim = lh.Simulation(model, lh.LayeredCoupledTRBDF2(), Y_init=Y, dt=dt, tspan=(0.0, total * dt), Ya_init=Ya, saveat=chunk * dt)
    sol = lh.run(sim)
    got_v, got_e = np.array(sim.integrator.u.soil.ϑ_l), np.array(sim.integrator.u.soil.ρe_int)
    assert sim.integrator._nsteps_done == total and len(sol.t) == total // chunk + 1
    assert sim.integrator.implicit_stats[1] == 0
    with Device(lay) as d:
        g, F = d.g, d.g.F
        t = 0.0
        for _ in range(total // chunk):
            times = [t + k * dt for k in range(chunk + 1)]
            bcv = np.zeros((chunk + 1, 2, 2))
            bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY], bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = bottom, fw
            bcv[:, M.FACE_TOP, M.COMP_ENERGY] = [top(x) for x in times]
            F.check(getattr(g.L, NAME)(g.ctx, d.Y, d.Ya, t, dt, chunk, F.LH_COUPLED_TRBDF2, ptr(bcv), 0.0, 0), g.ctx)
            t = t + chunk * dt
        want_v, want_e = g.download(d.Y, F.LH_VAR_VARTHETA_L), g.download(d.Y, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_e, want_e)
    assert np.max(np.abs(want_e - case.rhoe)) > 1e-3 * np.max(np.abs(case.rhoe)) and np.max(np.abs(want_v - case.vl)) > 0
    # ... and step_implicit_layered_coupled is the same call
    Y2, Ya2 = start()
    for k in range(total // chunk):
        assert lh.step_implicit_layered_coupled(model, Y2, Ya2, k * chunk * dt, dt, chunk, "trbdf2")[1] == 0
    np.testing.assert_array_equal(np.array(Y2.soil.ρe_int), want_e)
    # the scalar markers keep refusing this model; the layered ones refuse a model without classes and a heat-only one
    for marker in (lh.CoupledImplicitEuler(), lh.CoupledTRBDF2()):
        with pytest.raises(NotImplementedError, match="soil classes"):
            lh.Simulation(model, marker, Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    kw = dict(domain=dom, earth_param_set=lh.EarthParameterSet())
    plain = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT), boundary_conditions=bc, **kw)
    ebc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)), bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)))
    heat = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.PrescribedHydrologyModel(), boundary_conditions=ebc, **kw)
    for other, words in ((plain, "the context has no class map"), (heat, "coupled models only")):
        for marker in (lh.LayeredCoupledImplicitEuler(), lh.LayeredCoupledTRBDF2()):
            with pytest.raises(NotImplementedError, match=type(marker).__name__ + ": " + words):
                lh.Simulation(other, marker, Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
    model.close()


# ------------------------------------------------------------------ 11. a sand-over-clay column, end to end

def test_sand_over_clay_against_ssprk33():
    """8 x 60 with three horizons (conductive, tight, conductive: Ksat jumps of more than 100 at both interfaces), a
    flux top and a free-draining bottom, Dirichlet temperatures; the start is layered_ref.make_layered's wetting front
    in psi (-0.25 m at its wettest: no cell saturates).  4 TR-BDF2 steps of 30 stable steps each against lh_step_ssprk33
    at half a stable step over the same span on the same layered context: the device-minus-SSPRK33 distance in
    vartheta_l and in rhoe_int is at most 4x the NumPy reference's own distance to layered_heat_ref.ssprk33."""
    FT = np.float64
    lay = LC.layered_case(FT, 8, 60, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    sd = LC.stable_dt(lay)
    nsteps, per = 4, 30
    vl0, re0 = LC.state64(lay)
    assert np.all(vl0 < lay.classes[lay.class_map, 4])
    with Device(lay) as d:
        g, F = d.g, d.g.F
        v1, e1, (mi, un, _), st = d.steps(per * sd, nsteps, "trbdf2")
        assert un == 0 and st == 0
        d.restore()
        F.check(g.L.lh_step_ssprk33(g.ctx, d.Y, d.Ya, 0.0, 0.5 * sd, 2 * per * nsteps, None), g.ctx)
        vs, es = g.download(d.Y, F.LH_VAR_VARTHETA_L), g.download(d.Y, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    vr, er, info = LC.coupled_implicit(lay, vl0, re0, per * sd, nsteps, "trbdf2")
    ex = LH.ssprk33(LH.as64(lay), 0.5 * sd, 2 * per * nsteps)
    dev = (float(np.max(np.abs(v1 - vs))), float(np.max(np.abs(e1 - es))))
    ref = (float(np.max(np.abs(vr - ex["vl"]))), float(np.max(np.abs(er - ex["rhoe"]))))
    print(f"sand over clay: device - SSPRK33 vl {dev[0]:.3g}, rhoe {dev[1]:.3g}; reference - SSPRK33 vl {ref[0]:.3g}, rhoe {ref[1]:.3g}; "
          f"Newton iterations at most {mi}; the state moved by vl {np.max(np.abs(vs - vl0)):.3g}, rhoe {np.max(np.abs(es - re0)):.3g}")
    assert info["unconverged"] == 0 and ref[0] > 0 and ref[1] > 0
    assert dev[0] <= 4 * ref[0] and dev[1] <= 4 * ref[1]
