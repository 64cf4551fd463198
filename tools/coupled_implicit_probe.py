#!/usr/bin/env python3
"""Cost of an implicit step of the coupled model (lh_step_coupled_implicit, backward Euler and fixed-step
TR-BDF2) against the fixed-dt SSPRK33 stepper on the same ensemble in one process: ms per step, the mean and
the largest Newton iteration count per water stage, unconverged column-stages and the break-even dt ratio,
at 1x, 10x, 100x and 1000x the stable step.  One case per process (C3: c3_coupled_f32, 1e6 x 64 columns, or its
Float64 twin c3_coupled_f64); a row of JSON per measurement on stdout -- profiles/coupled_implicit_probe.jsonl
is the output of both cases, DESIGN.md section 4.16 its summary.

break-even = ms(implicit step) / ms(SSPRK33 step): the implicit step pays once its dt exceeds that many
explicit steps.  A TR-BDF2 step has two water stages: its iteration mean is per stage.
usage: tools/coupled_implicit_probe.py [case] [ncols] [steps_per_call]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W = pkg._ffi, pkg.workloads
MULTS = (1.0, 10.0, 100.0, 1000.0)


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


def probe(case, steps_per_call, reps=2):
    rows = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(sd)), ctx)
        sd = sd.value
        base = dict(case=case.name, ncols=case.ncols, nlev=case.om.nlev, stable_dt=sd)
        ms_ex = timed(gm, lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd, steps_per_call, None), ctx),
                      reps) / steps_per_call
        rows.append(dict(base, method="ssprk33", dt_over_stable=1.0, ms_per_step=round(ms_ex, 4)))
        for method, flags, stages in (("euler", 0, 1), ("trbdf2", F.LH_COUPLED_TRBDF2, 2)):
            for m in MULTS:
                # a fresh state per measurement (the timed calls continue from the warm-up's)
                F.check(L.lh_upload(ctx, Y, F.LH_VAR_VARTHETA_L, case.vl.ctypes.data, 1, case.om.nlev), ctx)
                F.check(L.lh_upload(ctx, Y, F.LH_VAR_RHOE_INT, case.rhoe.ctypes.data, 1, case.om.nlev), ctx)
                call = lambda: F.check(L.lh_step_coupled_implicit(ctx, Y, Ya, 0.0, m * sd, steps_per_call, flags, None,
                                                                  0.0, 0), ctx)
                ms = timed(gm, call, reps) / steps_per_call
                mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
                F.check(L.lh_implicit_stats(ctx, C.byref(mi), C.byref(un)), ctx)
                F.check(L.lh_implicit_iterations(ctx, C.byref(tot)), ctx)
                st = C.c_uint32()
                F.check(L.lh_get_status(ctx, C.byref(st)), ctx)
                rows.append(dict(base, method=method, dt_over_stable=m, ms_per_step=round(ms, 4),
                                 mean_newton_iters=round(tot.value / (case.ncols * steps_per_call * stages), 2),
                                 max_newton_iters=mi.value, unconverged=un.value, status=st.value,
                                 break_even_dt_ratio=round(ms / ms_ex, 2)))
    return rows


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c3_coupled_f32"
    ncols = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    for r in probe(W.make_case(name, ncols=ncols), steps):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
