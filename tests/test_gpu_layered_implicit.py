"""lh_step_layered_implicit_euler / lh_integrate_layered_trbdf2 (LayeredImplicitEuler, LayeredTRBDF2): backward
Euler and adaptive TR-BDF2 of Richards columns with per-cell soil classes on the device -- through the library's
own layered tendency (lh_rhs), against the NumPy reference (tests/layered_implicit_ref.py), against the
per-column kernels on column-uniform maps, and against SSPRK33."""
import ctypes as C
import functools

import numpy as np
import pytest

import case_model as M
import layered_implicit_ref as LI
import layered_ref as R
import parity_cases as pc
from test_gpu_implicit import implicit_on_device
from test_gpu_layered import gpu_fluxes, layered_gpu

pytestmark = pytest.mark.gpu
STATUS_UNCONVERGED = 8
STATUS_FAILED = 16
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}        # the library's Newton defaults
PARITY = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 2e-5}     # tests/test_gpu_implicit.py, test_gpu_trbdf2.py


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def euler(lay, dt, nsteps, tol=0.0, max_iter=0, calls=1, bcv=None, upload_zero_ti=False, want_rhs=False):
    """`calls` lh_step_layered_implicit_euler calls of nsteps each.  A dict: vl, max_iters, unconverged, iterations,
    status and, with want_rhs, f = lh_rhs at the new state in the same context."""
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        if upload_zero_ti:
            z = np.zeros_like(lay.case.vl)
            F.check(g.L.lh_upload(g.ctx, Y, F.LH_VAR_THETA_I, z.ctypes.data, 1, lay.case.om.nlev), g.ctx)
        b = None if bcv is None else np.ascontiguousarray(bcv, dtype=np.float64)
        for _ in range(calls):
            F.check(g.L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, dt, nsteps, _dptr(b), tol, max_iter), g.ctx)
        mi, un, total = C.c_int32(), C.c_int64(), C.c_int64()
        F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        F.check(g.L.lh_implicit_iterations(g.ctx, C.byref(total)), g.ctx)
        out = dict(vl=g.download(Y, F.LH_VAR_VARTHETA_L), max_iters=mi.value, unconverged=un.value,
                   iterations=total.value, status=g.status())
        if want_rhs:
            dY = g.state(0)
            g.rhs(Y, Ya, dY)
            out["f"] = g.tendencies(dY)["vl"]
            out["f_bot"] = gpu_fluxes(g, Y, Ya, M.FACE_BOTTOM)[1]
            out["f_top"] = gpu_fluxes(g, Y, Ya, M.FACE_TOP)[1]
        return out


def trbdf2(lay, t0, t1, dt, abstol=0.0, reltol=0.0, fixed=False, h0=None):
    """(vl at t1, stats dict, status, dt_cols after the call) of one lh_integrate_layered_trbdf2 call."""
    import torch
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        ft = torch.float64 if lay.case.dtype == np.float64 else torch.float32
        cols = torch.zeros(lay.case.ncols, dtype=ft, device="cuda")
        if h0 is not None:
            cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
        torch.cuda.synchronize()
        F.check(g.L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, t0, t1, dt, abstol, reltol, F.LH_TRBDF2_FIXED if fixed else 0,
                                                C.c_void_p(cols.data_ptr()), None), g.ctx)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(g.L.lh_trbdf2_stats(g.ctx, st), g.ctx)
        vl = g.download(Y, F.LH_VAR_VARTHETA_L)
        return vl, dict(zip(KEYS, list(st))), g.status(), cols.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def horizon_case(dtype, ncols, bc="flux_drain", ice=False):
    return R.make_layered(dtype, ncols, 64, R.horizon_map(ncols, 64), bc=bc, ice=ice)


@functools.lru_cache(maxsize=None)
def order_case():
    """the case of tests/test_layered_implicit_reference.py's order test, its stable step and SSPRK33 at a quarter of
    it over 200 stable steps (computed once, shared, never written)"""
    lay = R.make_layered(np.float64, 24, 64, R.horizon_map(24, 64), bc="flux_drain")
    sd = R.stable_dt(lay)
    ref = R.ssprk33(lay, sd / 4, 800)
    ref.setflags(write=False)
    return lay, sd, ref


def nu_max(lay):
    return float(np.asarray(lay.classes)[:, 4].max())


def residual_bound(lay, r, dt, mult):
    """tests/test_gpu_implicit.py's stated bound per column, 10 tol nu (1 + 4 mult) + round_off, with nu the largest
    class porosity and round_off = 64 eps(FT) max(|v|, dt |f|)."""
    dt_ = np.dtype(lay.case.dtype)
    v1, f = r["vl"].astype(np.float64), r["f"].astype(np.float64)
    big = np.maximum(np.abs(v1).max(axis=1), dt * np.abs(f).max(axis=1))
    return 10 * TOL[dt_] * nu_max(lay) * (1 + 4 * mult) + 64 * np.finfo(dt_).eps * big, big


# ------------------------------------------------------------ solved, by the library's own tendency

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["plain", "ice"])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
def test_residual_through_the_tendency(dtype, bc, ice):
    """One step at 10x and at 100x the layered stable step, 48 x 64, four horizons per column with Ksat jumps
    >= 150: every column converges (the NumPy reference does, in at most 11 iterations) and every column's
    max |v1 - v0 - dt lh_rhs(v1)| is within the bound.  No column is left out."""
    lay = horizon_case(dtype, 48, bc, ice)
    sd = R.stable_dt(lay)
    for mult in (10.0, 100.0):
        dt = mult * sd
        r = euler(lay, dt, 1, want_rhs=True)
        assert r["unconverged"] == 0 and not (r["status"] & STATUS_UNCONVERGED), (mult, r["max_iters"], r["unconverged"], r["status"])
        v1 = r["vl"]
        assert np.all(np.isfinite(v1))
        res = np.max(np.abs(v1 - lay.case.vl - lay.case.dtype(dt) * r["f"]), axis=1)
        bound, _ = residual_bound(lay, r, dt, mult)
        print("x%g: max iterations %d, worst residual / bound %.3g" % (mult, r["max_iters"], float(np.max(res / bound))))
        assert np.all(res <= bound), (mult, float(res.max()), r["max_iters"], np.flatnonzero(res > bound).tolist())
        assert np.max(np.abs(v1 - lay.case.vl)) > 0


# ------------------------------------------------------------ parity with the NumPy reference

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet"])
def test_parity_with_the_numpy_reference(dtype, bc):
    """Three steps at 30x the stable step, 128 columns with ice, every ninth column against the reference."""
    lay = horizon_case(dtype, 128, bc, True)
    dt = 30 * R.stable_dt(lay)
    r = euler(lay, dt, 3)
    assert r["unconverged"] == 0
    idx = np.arange(0, 128, 9)
    want, _ = LI.implicit_euler(LI.columns(lay, idx), dt, 3)
    err = np.max(np.abs(r["vl"][idx].astype(np.float64) - want))
    print("backward Euler against the reference: %.3g" % err)
    assert err <= PARITY[np.dtype(dtype)], float(err)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["plain", "ice"])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet"])
def test_fixed_step_trbdf2_parity_with_the_numpy_reference(dtype, bc, ice):
    lay = horizon_case(dtype, 64, bc, ice)
    dt = 10 * R.stable_dt(lay)
    v1, st, status, _ = trbdf2(lay, 0.0, 3 * dt, dt, fixed=True)
    assert status == 0 and st["accepted"] == 3 * 64 and st["rejected"] == 0 and st["unconverged"] == 0, st
    idx = np.arange(0, 64, 7)
    want, _ = LI.trbdf2(LI.columns(lay, idx), 0.0, 3 * dt, dt, adaptive=False)
    err = np.max(np.abs(v1[idx].astype(np.float64) - want))
    print("fixed TR-BDF2 against the reference: %.3g" % err)
    assert err <= PARITY[np.dtype(dtype)], float(err)


def test_one_adaptive_step_against_the_numpy_reference():
    """The error estimate and the controller on single steps (a call that spans exactly one step), as
    tests/test_gpu_trbdf2.py pins them: a column the reference accepts lands on the reference's Y_1 (1e-5) and
    proposes h 0.9 E^(-1/3) within 5 %; a column the reference rejects is rejected.  The device's Jacobian is
    analytic and the reference's a finite difference, so a column within 10 % of E = 1 may go either way and is
    judged on neither side."""
    lay = LI.columns(horizon_case(np.float64, 48), np.arange(0, 48, 6))
    n = lay.case.ncols
    sd = R.stable_dt(lay)
    y0 = lay.case.vl
    fn = LI.tendency(lay, y0)
    seen = set()
    for mult in (1.0, 4.0, 32.0, 64.0):     # (the reference measures E up to 0.002, 0.02, 0.87 and, in one column, 2.6)
        h = mult * sd
        y1, _, e, _ = LI.attempt(lay, y0, fn, np.full(n, h))
        E = LI.error_norm(e, y0, y1, 1e-6, 1e-3)
        v, st, status, cols = trbdf2(lay, 0.0, h, h)
        assert status == 0 and st["failed"] == 0, (mult, st)
        ok, no = E <= 0.9, E >= 1.1
        seen |= {"accepted"} if ok.any() else set()
        seen |= {"rejected"} if no.any() else set()
        err = np.max(np.abs(v - y1), axis=1)
        print("x%g: E %.3g .. %.3g, accepted %d, rejected %d" % (mult, E.min(), E.max(), st["accepted"], st["rejected"]))
        assert np.all(err[ok] <= 1e-5), (mult, err, E)
        want = h * np.clip(0.9 * E ** (-1.0 / 3.0), 0.2, 5.0)
        np.testing.assert_allclose(cols[ok], want[ok], rtol=0.05, err_msg=f"x{mult} E={E}")
        assert st["rejected"] >= no.sum() and st["accepted"] >= n, (mult, E, st)
        if ok.all():
            assert st["accepted"] == n and st["rejected"] == 0, (mult, E, st)
    assert seen == {"accepted", "rejected"}, seen


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_uniform_map_against_the_per_column_kernel(dtype):
    """Column c of class c mod 16 at every level: lh_step_layered_implicit_euler against lh_step_implicit_euler on the
    same parameters as per-column arrays.  Not bitwise: rhs_kernel folds Ksat into the gradient factor."""
    lay = R.make_layered(dtype, 128, 64, R.uniform_map(128, 64), bc="dirichlet", ice=True)
    dt = 30 * R.stable_dt(lay)
    r = euler(lay, dt, 3)
    v_pc, mi, un, st = implicit_on_device(R.with_percol(lay), dt, 3)
    assert r["unconverged"] == 0 and un == 0
    err = np.max(np.abs(r["vl"].astype(np.float64) - v_pc.astype(np.float64)))
    print("layered against per-column: %.3g (iterations %d / %d)" % (err, r["max_iters"], mi))
    assert err <= PARITY[np.dtype(dtype)], float(err)
    assert np.max(np.abs(r["vl"] - lay.case.vl)) > 1e-4


# ------------------------------------------------------------ accuracy

def test_fixed_step_order_on_the_device():
    lay, sd, ref = order_case()
    T = 200 * sd
    errs = []
    for k in (25, 50, 100):
        v, st, status, _ = trbdf2(lay, 0.0, T, T / k, fixed=True)
        assert status == 0 and st["accepted"] == k * 24, (k, status, st)
        errs.append(np.max(np.abs(v - ref)))
    r = [a / b for a, b in zip(errs, errs[1:])]
    print("errors %s, ratios %s" % (errs, r))
    assert all(3.5 <= x <= 4.5 for x in r), (errs, r)


def test_adaptive_accuracy_and_per_column_steps():
    """200 stable steps from the stable step: no failed column, within 10 reltol nu of SSPRK33 at a quarter of the
    stable step; and every column keeps its own step: run alone (reltol 1e-5) the columns take different numbers
    of steps, which add up to the ensemble's."""
    lay, sd, ref = order_case()
    T = 200 * sd
    for rtol in (1e-3, 1e-5):
        v, st, status, cols = trbdf2(lay, 0.0, T, sd, reltol=rtol, abstol=1e-6)
        assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (rtol, status, st)
        err = float(np.max(np.abs(v - ref)))
        print("reltol %g: error %.3g, accepted %d, rejected %d" % (rtol, err, st["accepted"], st["rejected"]))
        assert err <= 10 * rtol * nu_max(lay), (rtol, err)
    accepted = [trbdf2(LI.columns(lay, [c]), 0.0, T, sd, reltol=1e-5, abstol=1e-6)[1]["accepted"] for c in range(24)]
    print("accepted steps per column: %s" % accepted)
    assert len(set(accepted)) > 1 and sum(accepted) == st["accepted"], (accepted, st)


def test_hydrostatic_three_horizon_column_stays_at_rest():
    lay = R.hydrostatic(np.float64)
    for dt in (3600.0, 86400.0):
        r = euler(lay, dt, 1)
        moved = float(np.max(np.abs(r["vl"] - lay.case.vl)))
        print("dt %g: moved %.3g in %d iterations" % (dt, moved, r["max_iters"]))
        assert r["unconverged"] == 0 and r["status"] == 0
        assert moved <= 10 * TOL[np.dtype(np.float64)] * nu_max(lay), moved


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_flux_faces_conserve_water(dtype):
    """sum (v1 - v0) dz = dt (F_bot - F_top) within nlev dz x the residual bound: every unclipped Newton update
    conserves water exactly for flux faces (the columns of the Jacobian sum to 1), so the budget error is at most
    the sum of the residuals.  The figure printed is the error in units of nlev dz 64 eps max(|v|, dt |f|)."""
    lay = horizon_case(dtype, 48, "flux")
    om = lay.case.om
    dz = (om.zmax - om.zmin) / om.nlev
    sd = R.stable_dt(lay)
    for mult in (10.0, 100.0):
        dt = mult * sd
        r = euler(lay, dt, 1, want_rhs=True)
        assert r["unconverged"] == 0
        change = np.sum(r["vl"].astype(np.float64) - lay.case.vl.astype(np.float64), axis=1) * dz
        want = dt * (r["f_bot"] - r["f_top"])
        bound, big = residual_bound(lay, r, dt, mult)
        err = np.abs(change - want)
        unit = om.nlev * dz * 64 * np.finfo(dtype).eps * big
        print("x%g: budget error %.3g of %.3g, %.3g round-off units" % (mult, err.max(), np.abs(want).max(), float(np.max(err / unit))))
        assert np.all(err <= om.nlev * dz * bound), (mult, float(err.max()))
        assert np.abs(want).min() > 0


# ------------------------------------------------------------ shapes, independence, call splitting: bitwise

def _one_column_runner(lay1, dt):
    """Both integrators on single columns through ONE one-column context (tests/test_gpu_layered.py's way): state and
    class map replaced per column; returns (state after four backward-Euler steps, state and step proposal after
    adaptive TR-BDF2 over the same interval)."""
    import torch
    g = layered_gpu(lay1)
    F = g.F
    Y, Ya = g.prognostic_and_aux()
    cols = torch.zeros(1, dtype=torch.float64 if lay1.case.dtype == np.float64 else torch.float32, device="cuda")

    def run(vl, cmap):
        g.set_soil_class_map(cmap)
        g.upload(Y, F.LH_VAR_VARTHETA_L, vl)
        F.check(g.L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, dt, 4, None, 0.0, 0), g.ctx)
        v_e = g.download(Y, F.LH_VAR_VARTHETA_L)
        g.upload(Y, F.LH_VAR_VARTHETA_L, vl)
        cols.zero_()
        torch.cuda.synchronize()
        F.check(g.L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 4 * dt, dt, 0.0, 0.0, 0, C.c_void_p(cols.data_ptr()), None), g.ctx)
        v_t = g.download(Y, F.LH_VAR_VARTHETA_L)
        return v_e, v_t, float(cols.cpu()[0])
    return g, run


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ncols", [1, 67, 130])
def test_shapes_and_independence_bitwise(dtype, ncols):
    """nlev 1, 2, 3 and 64 with 3 and 16 classes: EVERY column of the ensemble equals that column run alone, after four
    backward-Euler steps and after adaptive TR-BDF2 over the same interval (state and step proposal); permuted, the
    ensemble is the permuted result; four steps in one call equal 2 + 2; a theta_i plane known to be zero equals an
    uploaded zero plane."""
    for nlev in (1, 2, 3, 64):
        for ncls in (3, 16):
            lay = R.make_layered(dtype, ncols, nlev, R.horizon_map(ncols, nlev, ncls), classes=R.texture_classes()[:ncls])
            dt = 20 * R.stable_dt(lay)
            a = euler(lay, dt, 4)
            v_t, st, _, h_t = trbdf2(lay, 0.0, 4 * dt, dt)
            assert np.all(np.isfinite(a["vl"])) and np.any(a["vl"] != lay.case.vl), (nlev, ncls)
            assert np.all(np.isfinite(v_t)) and st["failed"] == 0, (nlev, ncls, st)
            g1, run1 = _one_column_runner(LI.columns(lay, [0], dtype), dt)
            try:
                for c in range(ncols):
                    e1, t1, h1 = run1(lay.case.vl[c:c + 1], lay.class_map[c:c + 1])
                    np.testing.assert_array_equal(e1[0], a["vl"][c], err_msg=str((nlev, ncls, c)))
                    np.testing.assert_array_equal(t1[0], v_t[c], err_msg=str((nlev, ncls, c)))
                    assert h1 == h_t[c], (nlev, ncls, c, h1, h_t[c])
            finally:
                g1.close()
            if ncols > 1:
                order = np.random.default_rng(5).permutation(ncols)
                perm = R.Layered(pc._w.reorder_columns(lay.case, order), lay.classes, np.ascontiguousarray(lay.class_map[order]))
                np.testing.assert_array_equal(euler(perm, dt, 4)["vl"], a["vl"][order])
            np.testing.assert_array_equal(euler(lay, dt, 2, calls=2)["vl"], a["vl"])
            np.testing.assert_array_equal(euler(lay, dt, 4, upload_zero_ti=True)["vl"], a["vl"])


def test_boundary_values_per_step_bitwise():
    """bcv: one call of n steps with the Dirichlet values of t_{k+1} equals n one-step calls with the value set by
    lh_set_bc."""
    lay = horizon_case(np.float64, 48, "dirichlet")
    dt, n = 20 * R.stable_dt(lay), 5
    top = [0.30 - 0.01 * k for k in range(n)]
    bcv = np.zeros((n, 2, 2))
    bcv[:, M.FACE_BOTTOM, M.COMP_HYDROLOGY] = 0.26
    bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = top
    a = euler(lay, dt, n, bcv=bcv)
    assert a["unconverged"] == 0
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        for k in range(n):
            g.F.check(g.L.lh_set_bc(g.ctx, M.FACE_TOP, M.COMP_HYDROLOGY, M.BC_DIRICHLET, top[k], None), g.ctx)
            g.F.check(g.L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, dt, 1, None, 0.0, 0), g.ctx)
        one_by_one = g.download(Y, g.F.LH_VAR_VARTHETA_L)
    np.testing.assert_array_equal(a["vl"], one_by_one)
    assert np.max(np.abs(a["vl"] - euler(lay, dt, n)["vl"])) > 1e-6


# ------------------------------------------------------------ statistics and flags

def test_statistics_and_flags():
    lay = horizon_case(np.float64, 67, "dirichlet", True)
    sd = R.stable_dt(lay)
    # the three getters report the call, and a refused call zeroes them
    with layered_gpu(lay) as g:
        F, L = g.F, g.L
        Y, Ya = g.prognostic_and_aux()
        F.check(L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 10 * sd, 2, None, 0.0, 0), g.ctx)
        mi, un, total = C.c_int32(), C.c_int64(), C.c_int64()
        F.check(L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        F.check(L.lh_implicit_iterations(g.ctx, C.byref(total)), g.ctx)
        assert mi.value >= 2 and un.value == 0 and 2 * 67 <= total.value <= 2 * 67 * mi.value, (mi.value, un.value, total.value)
        # a tolerance no iterate meets within two iterations: every column-step is counted and flagged
        F.check(L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 100 * sd, 1, None, 1e-30, 2), g.ctx)
        F.check(L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        assert mi.value == 2 and un.value == 67 and g.status() & STATUS_UNCONVERGED
        F.check(L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 20 * sd, sd, 0.0, 0.0, 0, None, None), g.ctx)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(L.lh_trbdf2_stats(g.ctx, st), g.ctx)
        s = dict(zip(KEYS, list(st)))
        assert s["accepted"] >= 67 and s["failed"] == 0 and s["newton_iterations"] >= 2 * s["accepted"], s
        assert s["wave_steps"] >= s["accepted"] + s["rejected"] and s["max_steps"] >= 1, s
        assert L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, -1.0, 1, None, 0.0, 0) == F.LH_EINVAL
        assert L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 1.0, 0.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
        F.check(L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        F.check(L.lh_trbdf2_stats(g.ctx, st), g.ctx)
        assert (mi.value, un.value) == (0, 0) and not any(st)
    # each tolerance defaults on its own, bit for bit
    T = 20 * sd
    ref, *_ = trbdf2(lay, 0.0, T, sd, abstol=1e-6, reltol=1e-3)
    for a, r in ((0.0, 1e-3), (1e-6, 0.0), (0.0, 0.0)):
        v, *_ = trbdf2(lay, 0.0, T, sd, abstol=a, reltol=r)
        np.testing.assert_array_equal(v, ref)
    v8, _, status8, _ = trbdf2(lay, 0.0, T, sd, abstol=1e-8, reltol=1e-3)
    v80, *_ = trbdf2(lay, 0.0, T, sd, abstol=1e-8, reltol=0.0)
    np.testing.assert_array_equal(v80, v8)
    assert status8 == 0 and np.any(v8 != ref)
    # fixed mode steps by exactly dt whatever dt_cols holds, and leaves dt in it
    dt = 10 * sd
    v0, st0, _, c0 = trbdf2(lay, 0.0, 3 * dt, dt, fixed=True)
    v1, st1, _, c1 = trbdf2(lay, 0.0, 3 * dt, dt, fixed=True, h0=0.1 * sd * (1.0 + np.arange(67)))
    np.testing.assert_array_equal(v1, v0)
    assert st1["accepted"] == st0["accepted"] == 3 * 67
    np.testing.assert_array_equal(c1, np.full(67, dt))
    # a tolerance Float32 cannot meet: h shrinks to the floor, the column fails (bit 4), keeps its last accepted
    # state and reports dt_cols = 0
    l32 = horizon_case(np.float32, 67, "flux")
    sd32 = R.stable_dt(l32)
    v, st, status, cols = trbdf2(l32, 0.0, 10 * sd32, sd32, abstol=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 67 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0
    np.testing.assert_array_equal(v, l32.case.vl)


# ------------------------------------------------------------ refusals

def _refused(g, rc, code, *words):
    assert rc == code, (rc, g.L.lh_last_error(g.ctx))
    msg = g.L.lh_last_error(g.ctx).decode()
    for w in words:
        assert w in msg, msg


def test_refusals_in_order():
    lay = R.make_layered(np.float64, 67, 8, R.horizon_map(67, 8, 3), classes=R.texture_classes()[:3])
    fac = R.make_layered(np.float64, 67, 8, R.horizon_map(67, 8, 3), classes=R.texture_classes()[:3], factors=True)
    F = pc._pkg()._ffi
    L = F.lib()
    E, I = "lh_step_layered_implicit_euler", "lh_integrate_layered_trbdf2"

    def both(g, Y, Ya, code, *words):
        _refused(g, L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), code, E, *words)
        _refused(g, L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), code, I, *words)

    # NULL context
    assert L.lh_step_layered_implicit_euler(None, None, None, 0.0, 10.0, 1, None, 0.0, 0) == F.LH_EINVAL
    assert L.lh_integrate_layered_trbdf2(None, None, None, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
    # no class map comes first: before conductivity factors, and with classes but no map
    with pc.GpuModel(fac.case) as g:
        Y, Ya = g.prognostic_and_aux()
        both(g, Y, Ya, F.LH_EMODEL, "class map")
        _refused(g, L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 10.0, 1, None, 0.0, 0), F.LH_EMODEL, "lh_step_implicit_euler")
        _refused(g, L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 10.0, 1.0, 0.0, 0.0, 0, None, None), F.LH_EMODEL, "lh_integrate_trbdf2")
        g.set_soil_classes(fac.classes)
        both(g, Y, Ya, F.LH_EMODEL, "class map")
        # with the map: per-column arrays before LH_MATH_LIBM before conductivity factors
        g.set_soil_class_map(fac.class_map)
        arr = np.full(67, 0.45)
        F.check(L.lh_set_percol_param(g.ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), g.ctx)
        F.check(L.lh_set_math_mode(g.ctx, F.LH_MATH_LIBM), g.ctx)
        both(g, Y, Ya, F.LH_EMODEL, "soil classes", "per-column")
        F.check(L.lh_set_percol_param(g.ctx, F.LH_PC["nu"], None), g.ctx)
        both(g, Y, Ya, F.LH_EMODEL, "soil classes", "LH_MATH_LIBM")
        F.check(L.lh_set_math_mode(g.ctx, F.LH_MATH_FAST), g.ctx)
        both(g, Y, Ya, F.LH_EMODEL, "conductivity factors")
        # bad arguments are LH_EINVAL whatever the configuration
        _refused(g, L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 0.0, 1, None, 0.0, 0), F.LH_EINVAL, E)
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        for rc in (L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, -1.0, 1, None, 0.0, 0),
                   L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 1.0, -1, None, 0.0, 0)):
            _refused(g, rc, F.LH_EINVAL, E)
        nan, inf = float("nan"), float("inf")
        bad = np.full(8, nan)
        for rc in (L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 1.0, 0.0, 1.0, 0.0, 0.0, 0, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 0.0, 0.0, 0.0, 0, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 1.0, -1e-6, 0.0, 0, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, nan, 0, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 1.0, inf, 0.0, 0, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 2, None, None),
                   L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, _dptr(bad))):
            _refused(g, rc, F.LH_EINVAL, I)
        # nothing to do is not an error
        F.check(L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 1.0, 0, None, 0.0, 0), g.ctx)
        F.check(L.lh_integrate_layered_trbdf2(g.ctx, Y, Ya, 3.0, 3.0, 1.0, 0.0, 0.0, 0, None, None), g.ctx)
        assert np.array_equal(g.download(Y, F.LH_VAR_VARTHETA_L), lay.case.vl)
        # the layered step moves the state; without the map the scalar call is what it is on a fresh scalar context
        dt = 2 * R.stable_dt(lay)
        F.check(L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, dt, 2, None, 0.0, 0), g.ctx)
        layered_v = g.download(Y, F.LH_VAR_VARTHETA_L)
        g.set_soil_class_map(None)
        both(g, Y, Ya, F.LH_EMODEL, "class map")
        Y2, _ = g.prognostic_and_aux()
        F.check(L.lh_step_implicit_euler(g.ctx, Y2, Ya, 0.0, dt, 2, None, 0.0, 0), g.ctx)
        scalar_v = g.download(Y2, F.LH_VAR_VARTHETA_L)
    fresh, *_ = implicit_on_device(lay.case, dt, 2)
    assert np.array_equal(scalar_v, fresh) and np.any(layered_v != fresh)


# ------------------------------------------------------------ the host mirror

def test_host_mirror_three_horizons_through_simulation():
    """The three-horizon SoilModel of tests/test_gpu_layered.py through Simulation(model, LayeredImplicitEuler()) and
    Simulation(model, LayeredTRBDF2()): each ends bitwise on the state of the same run through the C ABI."""
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
    ic = lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z}
    dt, nsteps = 25 * R.stable_dt(lay), 6

    def through_simulation(method):
        Y, Ya = lh.initialize_states(model, ic, 0.0)
        Y.soil.ϑ_l = lay.case.vl
        sim = lh.Simulation(model, method, Y_init=Y, dt=dt, tspan=(0.0, nsteps * dt), Ya_init=Ya)
        lh.run(sim)
        return np.array(sim.integrator.u.soil.ϑ_l), sim

    got, _ = through_simulation(lh.LayeredImplicitEuler())
    want = euler(lay, dt, nsteps)
    assert want["unconverged"] == 0
    assert np.array_equal(got, want["vl"]) and np.any(got != lay.case.vl)
    got, sim = through_simulation(lh.LayeredTRBDF2())
    want, st, status, _ = trbdf2(lay, 0.0, nsteps * dt, dt)
    assert status == 0 and st["failed"] == 0
    assert np.array_equal(got, want) and np.any(got != lay.case.vl)
    assert sim.integrator.trbdf2_stats["accepted"] == st["accepted"]
    got, _ = through_simulation(lh.LayeredTRBDF2(adaptive=False))
    want, *_ = trbdf2(lay, 0.0, nsteps * dt, dt, fixed=True)
    assert np.array_equal(got, want)
    # scope: a Richards model WITH soil classes, NoEffect factors; the error names the marker
    Y, Ya = lh.initialize_states(model, ic, 0.0)
    kw = dict(Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    plain = build(None)
    factors = build(sc, hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT),
                                                               impedance_factor=lh.IceImpedance(FT)))
    for name in ("LayeredImplicitEuler", "LayeredTRBDF2"):
        for m in (plain, factors):
            with pytest.raises(NotImplementedError, match=name):
                lh.Simulation(m, getattr(lh, name)(), **kw)
    with pytest.raises(NotImplementedError, match="LayeredImplicitEuler"):
        lh.step_implicit_layered(plain, Y, Ya, 0.0, dt, 1)
    with pytest.raises(NotImplementedError, match="LayeredTRBDF2"):
        lh.integrate_layered_trbdf2(plain, Y, Ya, 0.0, dt, dt)
    # the scalar markers keep refusing soil classes, and now say where to go
    for method in (lh.ImplicitEuler(), lh.TRBDF2()):
        with pytest.raises(NotImplementedError, match="LayeredImplicitEuler"):
            lh.Simulation(model, method, **kw)


# ------------------------------------------------------------ scale

def test_scale_1e6_columns():
    """1e6 x 64 Float64: the C2 ensemble with four horizons of 16 levels (conductive / tight alternating, classes whose
    theta_r and nu enclose C2's state), one backward-Euler step at 10x the layered stable step."""
    N = 1_000_000
    classes = R.texture_classes()[[2, 7, 4, 9]]
    horizons = (np.arange(64) * 4 // 64).astype(np.uint8)

    def layered(ncols):
        case = pc.make_case("c2_richards_f64", ncols=ncols)
        assert classes[:, 2].max() < case.vl.min() and classes[:, 4].min() > case.vl.max()
        return R.Layered(case, classes, np.repeat(horizons[None, :], ncols, axis=0))

    sd = R.stable_dt(layered(2000))
    lay = layered(N)
    with layered_gpu(lay, class_map=horizons) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        F.check(g.L.lh_step_layered_implicit_euler(g.ctx, Y, Ya, 0.0, 10 * sd, 1, None, 0.0, 0), g.ctx)
        mi, un = C.c_int32(), C.c_int64()
        F.check(g.L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        v1 = g.download(Y, F.LH_VAR_VARTHETA_L)
        assert un.value == 0 and g.status() == 0 and mi.value >= 1, (mi.value, un.value)
    assert np.all(np.isfinite(v1)) and np.any(v1 != lay.case.vl)


# ------------------------------------------------------------------ the same in the v_ldexp closure form
# (Float64 only: Float32 has one form.  ldexp_form: every context of the test is created under `vgfast=0` and
# asserts lh_closure_form == LH_CLOSURE_LDEXP when it is left; assertions and bounds are those of the tests above.)
from closure_form import ldexp_form  # noqa: E402,F401


@pytest.mark.parametrize("ice", [False, True], ids=["plain", "ice"])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
def test_residual_through_the_tendency_ldexp_form(bc, ice, ldexp_form):
    test_residual_through_the_tendency(np.float64, bc, ice)


@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet"])
def test_parity_with_the_numpy_reference_ldexp_form(bc, ldexp_form):
    test_parity_with_the_numpy_reference(np.float64, bc)


@pytest.mark.parametrize("ice", [False, True], ids=["plain", "ice"])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet"])
def test_fixed_step_trbdf2_parity_with_the_numpy_reference_ldexp_form(bc, ice, ldexp_form):
    test_fixed_step_trbdf2_parity_with_the_numpy_reference(np.float64, bc, ice)


def test_one_adaptive_step_against_the_numpy_reference_ldexp_form(ldexp_form):
    test_one_adaptive_step_against_the_numpy_reference()
