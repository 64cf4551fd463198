#!/usr/bin/env python3
"""Cost of the adaptive TR-BDF2 of the coupled model (lh_integrate_coupled_trbdf2) over 64 stable steps from
h0 = the stable step, at reltol 1e-3, 1e-4 and 1e-5, against SSPRK33 at the stable step and against fixed-step
TR-BDF2 (lh_step_coupled_implicit, LH_COUPLED_TRBDF2) at the largest step that is at least as accurate.  Cases: C3
(c3_coupled_f32, 1e6 x 64), its Float64 twin, and `percol_f64`: the twin with per-column van Genuchten parameters
and porosity (a heterogeneous ensemble).  One row of JSON per measurement:
  ms_per_sim_second         call time / simulated seconds
  error                     max |rhoe_int - truth|, truth = SSPRK33 at an eighth of the stable step (the tests' yardstick)
  newton_per_stage          Newton iterations / (2 x attempted steps)
  steps_per_column          attempted steps / ncols
  divergence                wave_steps / (64 x waves x mean steps per column): what the slowest lane of a wave costs
Without arguments: every case in a process of its own, each under its own time limit, rows appended to
profiles/coupled_trbdf2_probe.jsonl (DESIGN.md section 4.17 is its summary).
usage: tools/coupled_trbdf2_probe.py [case [ncols]]"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("c3_coupled_f32", "c3_coupled_f64", "percol_f64")
SPAN = 64
FIXED_STEPS = (4, 8, 16, 32, 64, 128)
CASE_TIME_LIMIT = 240   # seconds per case


def make_case(W, name, ncols):
    import numpy as np
    if name != "percol_f64":
        return W.make_case(name, ncols=ncols)
    case = W.make_case("c3_coupled_f64", ncols=ncols)
    c, n = np.arange(ncols), case.om.nlev
    case.om.percol = dict(vg_n=1.4 + 1.2 * W.uhash(c, 2, n), vg_alpha=1.5 + 4.0 * W.uhash(c, 3, n),
                          vg_Ksat=10.0 ** (-7.0 + 2.0 * W.uhash(c, 4, n)), nu=case.om.soil.nu * (1.0 + 0.2 * W.uhash(c, 6, n)))
    case.name = name
    return case


def probe(name, ncols):
    import numpy as np
    import torch  # noqa: F401  (before any HIP library is loaded)
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    F, W = pkg._ffi, pkg.workloads
    case = make_case(W, name, ncols)
    nlev = case.om.nlev
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()

        def reset():
            F.check(L.lh_upload(ctx, Y, F.LH_VAR_VARTHETA_L, case.vl.ctypes.data, 1, nlev), ctx)
            F.check(L.lh_upload(ctx, Y, F.LH_VAR_RHOE_INT, case.rhoe.ctypes.data, 1, nlev), ctx)

        def timed(fn):
            F.check(L.lh_synchronize(ctx), ctx)
            F.check(L.lh_timer_start(ctx), ctx)
            fn()
            ms = C.c_float()
            F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
            return ms.value

        def status():
            st = C.c_uint32()
            F.check(L.lh_get_status(ctx, C.byref(st)), ctx)
            return st.value

        rhoe = lambda: gm.download(Y, F.LH_VAR_RHOE_INT).astype(np.float64)
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(sd)), ctx)
        sd = sd.value
        T = SPAN * sd
        base = dict(case=name, ncols=ncols, nlev=nlev, stable_dt=sd, span_stable_steps=SPAN)
        F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd / 8, 8 * SPAN, None), ctx)
        truth = rhoe()
        reset()
        ms = timed(lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd, SPAN, None), ctx))
        yield dict(base, method="ssprk33", ms_per_sim_second=ms / T, error=float(np.max(np.abs(rhoe() - truth))),
                   status=status())
        # (first-use allocations of both implicit paths, outside the timed calls)
        reset()
        F.check(L.lh_integrate_coupled_trbdf2(ctx, Y, Ya, 0.0, sd, sd, 0.0, 0.0, 0.0, 0, None, None), ctx)
        F.check(L.lh_step_coupled_implicit(ctx, Y, Ya, 0.0, sd, 1, F.LH_COUPLED_TRBDF2, None, 0.0, 0), ctx)
        fixed = []
        for n in FIXED_STEPS:
            reset()
            ms = timed(lambda: F.check(L.lh_step_coupled_implicit(ctx, Y, Ya, 0.0, T / n, n, F.LH_COUPLED_TRBDF2, None,
                                                                  0.0, 0), ctx))
            fixed.append(dict(base, method="fixed_trbdf2", steps=n, dt_over_stable=SPAN / n, ms_per_sim_second=ms / T,
                              error=float(np.max(np.abs(rhoe() - truth))), status=status()))
            yield fixed[-1]
        waves = (ncols + 63) // 64
        for reltol in (1e-3, 1e-4, 1e-5):
            reset()
            ms = timed(lambda: F.check(L.lh_integrate_coupled_trbdf2(ctx, Y, Ya, 0.0, T, sd, 0.0, 0.0, reltol, 0, None,
                                                                     None), ctx))
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            acc, rej, its, mx, failed, wave_steps, _ = list(st)
            err = float(np.max(np.abs(rhoe() - truth)))
            same = [r for r in fixed if r["error"] <= err]   # the largest fixed step at least as accurate
            yield dict(base, method="adaptive_trbdf2", reltol=reltol, ms_per_sim_second=ms / T, error=err,
                       accepted=acc, rejected=rej, failed=failed, max_steps=mx,
                       newton_per_stage=its / (2.0 * max(acc + rej, 1)), steps_per_column=(acc + rej) / ncols,
                       divergence=wave_steps / (64.0 * waves * max((acc + rej) / ncols, 1e-300)),
                       fixed_steps_for_same_error=same[0]["steps"] if same else None,
                       fixed_ms_per_sim_second_for_same_error=same[0]["ms_per_sim_second"] if same else None,
                       status=status())


def main():
    if len(sys.argv) > 1:
        ncols = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
        for r in probe(sys.argv[1], ncols):
            print(json.dumps(r), flush=True)
        return
    out = os.path.join(ROOT, "profiles", "coupled_trbdf2_probe.jsonl")
    with open(out, "w") as f:
        for name in CASES:   # one process per case: a case that fails or runs over its limit ends the run
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), name], stdout=subprocess.PIPE, text=True,
                                   timeout=CASE_TIME_LIMIT)
                rows, rc = p.stdout, p.returncode
            except subprocess.TimeoutExpired as e:   # (the rows the case had printed are kept)
                rows = e.stdout or ""
                rows, rc = rows if isinstance(rows, str) else rows.decode(), 124
            f.write(rows)
            f.flush()
            sys.stdout.write(rows)
            if rc != 0:
                sys.exit(rc)


if __name__ == "__main__":
    main()
