#!/usr/bin/env python3
"""Cost of a backward-Euler step (lh_step_implicit_euler) against the fixed-dt SSPRK33 stepper, in one
process: ms per step, the mean and the largest Newton iteration count per column-step, for C2
(Richards, Float64, 1e6 x 64 columns) and the reference's Bonan infiltration case (150 levels,
replicated over an ensemble) at several dt / stable_dt.

Bytes per Newton iteration and cell (Float64): read v^k and v_n, write c' and d' (upward sweep), read
c', d' and v^k, write v^{k+1} (downward): 8 x 8 = 64 B; the first iteration writes v_n instead of
reading it.  GB/s multiplies the MEAN iteration count per column-step by those bytes: a wave runs
until its slowest lane has converged, so it understates what the waves stream when the counts of
neighbouring columns differ.
break-even = ms(implicit step) / ms(SSPRK33 step): the implicit step pays once its dt exceeds that many
explicit steps.
usage: tools/implicit_probe.py [ncols_c2] [ncols_bonan]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model


def bonan(ncols):
    sp = M.default_soil(nu=0.287, S_s=1e-3)
    vg = M.default_vg(n=3.96, alpha=2.7, Ksat=34 / 3600 / 100, theta_r=0.075)
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.267),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    om = M.CaseModel(M.MODEL_RICHARDS, 150, -1.5, 0.0, soil=sp, vg=vg, bc=bc)
    return W.Case("bonan", om, np.float64, ncols, vl=np.full((ncols, 150), 0.1), ti=np.zeros((ncols, 150)))


def timed(gm, fn, reps):
    L, ctx = gm.L, gm.ctx
    fn()  # warm-up (and first-use allocations)
    F.check(L.lh_synchronize(ctx), ctx)
    F.check(L.lh_timer_start(ctx), ctx)
    for _ in range(reps):
        fn()
    ms = C.c_float()
    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
    return ms.value / reps


def probe(case, mults, steps_per_call=4, reps=3):
    out = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(sd)), ctx)
        sd = sd.value
        cells = case.ncols * case.om.nlev
        ms_ex = timed(gm, lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd, steps_per_call, None), ctx),
                      reps) / steps_per_call
        out.append(dict(case=case.name, method="ssprk33", dt_over_stable=1.0, ms_per_step=round(ms_ex, 4)))
        for m in mults:
            Yi, _ = gm.prognostic_and_aux()
            call = lambda: F.check(L.lh_step_implicit_euler(ctx, Yi, Ya, 0.0, m * sd, steps_per_call, None, 0.0, 0), ctx)
            ms = timed(gm, call, reps) / steps_per_call
            mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
            F.check(L.lh_implicit_stats(ctx, C.byref(mi), C.byref(un)), ctx)
            F.check(L.lh_implicit_iterations(ctx, C.byref(tot)), ctx)
            mean_it = tot.value / (case.ncols * steps_per_call)   # of the last timed call
            out.append(dict(case=case.name, method="implicit_euler", dt_over_stable=m, ms_per_step=round(ms, 4),
                            mean_newton_iters=round(mean_it, 2), max_newton_iters=mi.value, unconverged=un.value,
                            GBps_at_mean_iters=round(64.0 * cells * mean_it / (ms * 1e-3) / 1e9, 1),
                            break_even_dt_ratio=round(ms / ms_ex, 2)))
    return out


def main():
    n_c2 = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_bo = int(sys.argv[2]) if len(sys.argv) > 2 else 65_536
    rows = probe(W.make_case("c2_richards_f64", ncols=n_c2), (1.0, 10.0, 100.0, 1000.0))
    rows += probe(bonan(n_bo), (1.0, 10.0, 100.0))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
