#!/usr/bin/env python3
"""Cost of the implicit integrators of layered soils (lh_step_layered_implicit_euler, lh_integrate_layered_trbdf2)
on the C2 shape (ice-free Richards, 1e6 x 64, Float64) in ONE process and ONE context (the same planes, the same
placement), with tools/layered_probe.py's classes and its four-horizon map.  Timed with lh_timer_* around `reps`
back-to-back calls after a warm-up; the backward-Euler figures are the median of `rounds` rounds that take every
variant once each, with the spread; a TR-BDF2 figure is one timed call after a warm-up call.

  backward Euler at 1x, 10x, 100x the layered stable step: ms per step, mean and largest Newton iteration count,
      max / mean (an upper bound on what the slowest lane of a wave costs the others), and the break-even ratio
      against the layered fused SSPRK33 step (ms implicit step / ms explicit step: the implicit step pays once its
      dt exceeds that many stable steps)
  adaptive TR-BDF2 over 100 stable steps at reltol 1e-3 and 1e-4: ms per call, steps, Newton iterations, and the
      lane-divergence factor wave_steps / (accepted + rejected) of lh_trbdf2_stats
  ms per Newton iteration (ms per step / mean iterations, at 10x) of three launches on the SAME problem -- the loam
      of C2 as the context's scalars (lh_step_implicit_euler), as six per-column arrays (lh_step_implicit_euler,
      PERCOL) and as four identical classes under the four-horizon map (lh_step_layered_implicit_euler) -- so that
      the three differ in where the constants come from and in nothing else.  Bytes per iteration and cell: 64
      (tools/implicit_probe.py) + 2 for the layered launch (the class byte, read in both sweeps).

usage: tools/layered_implicit_probe.py [ncols] [--inputs-only]      one JSON line per figure on stdout"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import layered_probe as LP

F, W = LP.F, LP.W
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
PC_KEYS = ("vg_n", "vg_alpha", "vg_theta_r", "vg_Ksat", "nu", "S_s")


def variants(ncols, nlev):
    four = np.repeat((np.arange(nlev) * 4 // nlev).astype(np.uint8)[None, :], ncols, axis=0)
    return dict(layered_4=(LP.classes16()[[0, 5, 9, 14]], four), layered_4_loam=(np.array([LP.LOAM] * 4), four))


def probe(ncols, steps=2, reps=3, rounds=3):
    case = W.make_case("c2_richards_f64", ncols=ncols)
    nlev = case.om.nlev
    lay = variants(ncols, nlev)
    rows = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y = gm.state(0)
        ones = np.ones(ncols)

        def configure(v):
            gm.set_soil_classes(None)
            for key, x in zip(PC_KEYS, LP.LOAM):
                a = np.ascontiguousarray(ones * x) if v == "percol" else None
                F.check(L.lh_set_percol_param(ctx, F.LH_PC[key], None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))), ctx)
            if v in lay:
                gm.set_soil_classes(*lay[v])

        def stable():
            sd = C.c_double()
            F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
            return sd.value

        def euler(v, dt):
            fn = L.lh_step_layered_implicit_euler if v in lay else L.lh_step_implicit_euler

            def call():
                F.check(L.lh_state_copy(ctx, Y, Y0), ctx)     # (every timed call solves the same steps)
                F.check(fn(ctx, Y, Ya, 0.0, dt, steps, None, 0.0, 0), ctx)
            ms = LP.timed(gm, call, reps)
            ms_copy = LP.timed(gm, lambda: F.check(L.lh_state_copy(ctx, Y, Y0), ctx), reps)
            mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
            F.check(L.lh_implicit_stats(ctx, C.byref(mi), C.byref(un)), ctx)
            F.check(L.lh_implicit_iterations(ctx, C.byref(tot)), ctx)
            mean_it = tot.value / (ncols * steps)
            per_step = (ms - ms_copy) / steps
            return dict(variant=v, ms_per_step=round(per_step, 4), mean_newton_iters=round(mean_it, 3),
                        max_newton_iters=mi.value, max_over_mean_iters=round(mi.value / mean_it, 2), unconverged=un.value,
                        ms_per_newton_iteration=round(per_step / mean_it, 4))

        def euler_rounds(cases):
            """every (variant, dt / stable dt) once per round, `rounds` rounds: the median ms with its spread"""
            runs = {c: [] for c in cases}
            for _ in range(rounds):
                for v, m in cases:
                    configure(v)
                    runs[(v, m)].append(euler(v, m * stable()))
            out = []
            for (v, m), rs in runs.items():
                ms = sorted(r["ms_per_step"] for r in rs)
                r = dict(rs[-1], dt_over_stable=m, ms_per_step=ms[len(ms) // 2], spread=[ms[0], ms[-1]])
                r["ms_per_newton_iteration"] = round(r["ms_per_step"] / r["mean_newton_iters"], 4)
                out.append(r)
            return out

        # the layered ensemble: backward Euler against the layered fused SSPRK33 step
        configure("layered_4")
        sd = stable()
        F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
        ex = sorted(LP.timed(gm, lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, 0.2 * sd, 4, None), ctx), reps) / 4
                    for _ in range(rounds))
        ms_ex = ex[len(ex) // 2]
        rows.append(dict(figure="ssprk33_step", variant="layered_4", stable_dt=sd, ms_per_step=round(ms_ex, 4),
                         spread=[round(ex[0], 4), round(ex[-1], 4)]))
        for r in euler_rounds([("layered_4", m) for m in (1.0, 10.0, 100.0)]):
            rows.append(dict(figure="backward_euler", break_even_dt_ratio=round(r["ms_per_step"] / ms_ex, 2), **r))
        configure("layered_4")
        T = 100 * sd
        for rtol in (1e-3, 1e-4):
            def call():
                F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                F.check(L.lh_integrate_layered_trbdf2(ctx, Y, Ya, 0.0, T, sd, 0.0, rtol, 0, None, None), ctx)
            ms = LP.timed(gm, call, 1)
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            s = dict(zip(KEYS, list(st)))
            att = s["accepted"] + s["rejected"]
            rows.append(dict(figure="adaptive_trbdf2", variant="layered_4", reltol=rtol, stable_steps=100, ms_per_call=round(ms, 3),
                             mean_steps=round(att / ncols, 2), max_steps=s["max_steps"], failed=s["failed"],
                             newton_iters_per_step=round(s["newton_iterations"] / max(att, 1), 2),
                             lane_divergence=round(s["wave_steps"] / max(att, 1), 3),
                             ms_per_explicit_interval=round(100 * ms_ex, 3)))
        # the same problem three ways: ms per Newton iteration
        for r in euler_rounds([(v, 10.0) for v in ("scalar", "percol", "layered_4_loam")]):
            rows.append(dict(figure="newton_iteration", **r))
        assert gm.status() == 0
        configure("scalar")
    for r in rows:
        r.update(dtype="float64", ncols=ncols, nlev=nlev)
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ncols = int(args[0]) if args else 1_000_000
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        case = W.make_case("c2_richards_f64", ncols=ncols)
        for v, (cls, m) in variants(ncols, case.om.nlev).items():
            assert m.shape == case.vl.shape and m.max() < len(cls)
            assert np.all(cls[:, 2] < case.vl.min()) and np.all(cls[:, 4] > case.vl.max()), v
        print("inputs ok")
        return
    for r in probe(ncols):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
