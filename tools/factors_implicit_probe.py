#!/usr/bin/env python3
"""What conductivity factors cost the implicit Richards integrators (lh_step_factors_implicit_euler,
lh_integrate_factors_trbdf2), in one process, medians of 5 timed calls after a warm-up:

  step:    ms per backward-Euler step and per Newton iteration of lh_step_factors_implicit_euler (both factors on,
           ice in every other column, T hashed per cell in [270, 295] K) against lh_step_implicit_euler on the same
           state with the factors off, both at 10x the stable step of the context without factors, ncols x 64 cells,
           Float64 and Float32: what the T load, the folded 2^(.) and the extra slope cost.
  explicit: a partly frozen 24 h infiltration (a top held at vartheta_l = 0.40 over free drainage, 0.08 of ice below
           0.6 m) under the adaptive call against lh_step_ssprk33 at its stable step: accepted steps per column and
           wall time.  SSPRK33 is timed over 50 steps in a context of its own and scaled to the 24 h / stable_dt steps
           it needs (the row says so).

usage: tools/factors_implicit_probe.py [ncols_step] [ncols_explicit ...]      (defaults: 1000000, then 65536 1000000)"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model
NLEV, DAY = 64, 86400.0


def case_of(dtype, ncols, factors, frozen_below=None):
    """Loam, 64 levels of 2 cm, the C2 wetting front; ice in every other column (hashed, at most 0.04) or, with
    frozen_below, 0.08 below that depth in every column; T hashed per cell in [270, 295] K."""
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.40) if frozen_below is not None else (M.BC_FLUX, -2e-9),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    om = M.CaseModel(M.MODEL_RICHARDS, NLEV, -0.02 * NLEV, 0.0, bc=bc, cf=M.default_cf(viscosity=factors, impedance=factors))
    c, lev = np.arange(ncols)[:, None], np.arange(NLEV)[None, :]
    vl = W.wetting_front(ncols, NLEV, om.zmin, 0.0, 0.35)
    if frozen_below is None:
        ti = np.where(c % 2 == 0, 0.04 * W.uhash(c, lev + 5, 1000), 0.0)
    else:
        zc, _ = W.grid_np(om.zmin, 0.0, NLEV)
        ti = np.where(zc[None, :] < frozen_below, 0.08, 0.0) * np.ones((ncols, 1))
    T = 270.0 + 25.0 * W.uhash(c, lev + 11, 1000)
    return W.Case("factors_probe", om, dtype, ncols, vl=vl.astype(dtype), ti=ti.astype(dtype), T_aux=T.astype(dtype))


def median_ms(gm, fn, reps=5):
    L, ctx = gm.L, gm.ctx
    fn()  # warm-up (and first-use allocations)
    out = []
    for _ in range(reps):
        F.check(L.lh_synchronize(ctx), ctx)
        F.check(L.lh_timer_start(ctx), ctx)
        fn()
        ms = C.c_float()
        F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
        out.append(ms.value)
    return statistics.median(out)


def newton_stats(gm):
    mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
    F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
    F.check(gm.L.lh_implicit_iterations(gm.ctx, C.byref(tot)), gm.ctx)
    return mi.value, un.value, tot.value


def step_cost(dtype, ncols, steps=4):
    rows, sd = [], None
    for factors, entry in ((False, "lh_step_implicit_euler"), (True, "lh_step_factors_implicit_euler")):
        case = case_of(dtype, ncols, factors)
        with W.GpuModel(case) as gm:
            L, ctx = gm.L, gm.ctx
            Y, Ya = gm.prognostic_and_aux()
            if sd is None:   # the stable step of the context WITHOUT factors: both calls take the same dt
                v = C.c_double()
                F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(v)), ctx)
                sd = v.value

            def call():
                gm.upload(Y, F.LH_VAR_VARTHETA_L, case.vl)   # every timed call starts from the same state
                F.check(L.lh_synchronize(ctx), ctx)
                F.check(L.lh_timer_start(ctx), ctx)
                F.check(getattr(L, entry)(ctx, Y, Ya, 0.0, 10 * sd, steps, None, 0.0, 0), ctx)
                ms = C.c_float()
                F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
                return ms.value
            call()
            ms = statistics.median(call() for _ in range(5)) / steps
            mi, un, tot = newton_stats(gm)
            mean_it = tot / (ncols * steps)
            rows.append(dict(probe="step", dtype=np.dtype(dtype).name, ncols=ncols, nlev=NLEV, entry=entry, dt_over_stable=10,
                             ms_per_step=round(ms, 4), mean_newton_iters=round(mean_it, 2), max_newton_iters=mi, unconverged=un,
                             ms_per_mean_iteration=round(ms / mean_it, 4)))
    rows.append(dict(probe="step", dtype=np.dtype(dtype).name, ncols=ncols,
                     factors_over_plain_per_step=round(rows[1]["ms_per_step"] / rows[0]["ms_per_step"], 3),
                     factors_over_plain_per_iteration=round(rows[1]["ms_per_mean_iteration"] / rows[0]["ms_per_mean_iteration"], 3)))
    return rows


def against_explicit(ncols, dtype=np.float64):
    case = case_of(dtype, ncols, True, frozen_below=-0.6)
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        v = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(v)), ctx)
        sd = v.value
        ms50 = median_ms(gm, lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd, 50, None), ctx))
        status_explicit = gm.status()
    need = DAY / sd
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        F.check(L.lh_synchronize(ctx), ctx)
        F.check(L.lh_timer_start(ctx), ctx)
        F.check(L.lh_integrate_factors_trbdf2(ctx, Y, Ya, 0.0, DAY, sd, 0.0, 0.0, 0, None, None), ctx)
        ms = C.c_float()
        F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(L.lh_trbdf2_stats(ctx, st), ctx)
        return dict(probe="explicit", dtype=np.dtype(dtype).name, ncols=ncols, nlev=NLEV, stable_dt_s=round(sd, 3),
                    ssprk33_steps_for_24h=int(need), ssprk33_ms_per_step=round(ms50 / 50, 4),
                    ssprk33_wall_s_for_24h_scaled_from_50_steps=round(ms50 / 50 * need / 1e3, 3), ssprk33_status=status_explicit,
                    trbdf2_wall_s=round(ms.value / 1e3, 3), trbdf2_accepted_per_column=round(st[0] / ncols, 1),
                    trbdf2_rejected_per_column=round(st[1] / ncols, 2), trbdf2_max_steps=int(st[3]), trbdf2_failed=int(st[4]),
                    status=gm.status())


def main():
    n_step = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_exp = [int(a) for a in sys.argv[2:]] or [65_536, 1_000_000]
    for dtype in (np.float64, np.float32):
        for r in step_cost(dtype, n_step):
            print(json.dumps(r), flush=True)
    for n in n_exp:
        print(json.dumps(against_explicit(n)), flush=True)


if __name__ == "__main__":
    main()
