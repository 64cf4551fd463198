#!/usr/bin/env python3
"""Cost per step of adaptive SSPRK33 with the step held over chunks (lh_step_ssprk33_adaptive_hold) against
the two engines it sits between: lh_step_ssprk33_adaptive (three streamed launches per step) and the
fixed-dt persistent stepper (lh_step_ssprk33, at the mean dt the adaptive call took).

One process, one context per workload.  Every timed call starts from the SAME state: a device copy of the
initial condition is restored (lh_state_copy, outside the timed interval) before each call, so that every
variant steps the same physics and the fixed-dt stepper's step -- the mean dt an adaptive call takes from
that state over the same STEPS steps -- stays the step those states want.  The variants alternate within
a round, ROUNDS rounds after one warm-up round; HIP events on the context's stream (lh_timer_*).
Reported: median / min / max ms per step over the rounds, the spread (max - min) / median of each
variant, the status flags each variant left (bit 0: a non-finite tendency), and the verdict of the
comparison the feature is judged by: at hold = 16 the held call must beat the per-step adaptive call by
more than the run-to-run spread (the larger max - min of the two variants), on every workload.

usage (on a GPU): tools/adaptive_hold_cost.py [--out FILE] [workload ...]      (default: c2 c4, 1e6 columns)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np
import torch
import bench
import parity_cases as pc

STEPS, ROUNDS, COURANT, HOLDS = 64, 7, 0.2, (1, 4, 16, 64)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_hold_cost.txt"))
ap.add_argument("workloads", nargs="*", default=["c2", "c4"])
args = ap.parse_args()
ncols = int(os.environ.get("NCOLS", "1000000"))
lines = [f"ms per step, {ncols} columns, {STEPS} steps per timed call, {ROUNDS} alternating rounds, courant {COURANT}",
         f"{'workload':8s} {'variant':22s} {'median':>8s} {'min':>8s} {'max':>8s} {'spread':>7s}  engine"]

printed = 0
verdicts = []
for wl in args.workloads:
    case = bench.build_case(wl, ncols, 0)
    with pc.GpuModel(case) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y0, Ya = g.prognostic_and_aux()
        Y, _ = g.prognostic_and_aux()
        buf = torch.zeros(2, device="cuda", dtype=torch.float64 if case.dtype == np.float64 else torch.float32)
        torch.cuda.synchronize()
        dt_p, el_p = buf.data_ptr(), buf.data_ptr() + buf.element_size()
        # the mean dt of an adaptive call from the initial state, for the fixed-dt stepper
        F.check(L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, COURANT, 0.0, STEPS, dt_p, el_p), ctx)
        F.check(L.lh_synchronize(ctx), ctx)
        mean_dt = float(buf[1].item()) / STEPS
        A, X = "adaptive (per step)", "fixed dt (stepper)"
        variants = [(A, lambda: L.lh_step_ssprk33_adaptive(ctx, Y, Ya, 0.0, COURANT, 0.0, STEPS, dt_p, None)),
                    (X, lambda: L.lh_step_ssprk33(ctx, Y, Ya, 0.0, mean_dt, STEPS, None))]
        for h in HOLDS:
            variants.append((f"hold = {h}", lambda h=h: L.lh_step_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, COURANT, 0.0, STEPS // h, h, dt_p, None)))
        times = {name: [] for name, _ in variants}
        flags = {name: 0 for name, _ in variants}
        g.status()
        for rnd in range(ROUNDS + 1):   # round 0 warms every variant up
            for name, call in variants:
                F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                ms = C.c_float()
                F.check(L.lh_timer_start(ctx), ctx)
                F.check(call(), ctx)
                F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
                flags[name] |= g.status()
                if rnd:
                    times[name].append(ms.value / STEPS)
        engines = {A: "fused stages", X: ("stepper" if L.lh_step_engine(ctx, STEPS, 0) == 1 else "fused stages")}
        for h in HOLDS:
            engines[f"hold = {h}"] = "stepper" if L.lh_adaptive_hold_engine(ctx, h) == 1 else "fused stages"
        med, rng = {}, {}
        for name, _ in variants:
            t = np.array(times[name])
            med[name], rng[name] = float(np.median(t)), float(t.max() - t.min())
            lines.append(f"{wl:8s} {name:22s} {med[name]:8.4f} {t.min():8.4f} {t.max():8.4f} {rng[name] / med[name]:7.1%}  {engines[name]}"
                         f"  status {flags[name]}" + ("  NON-FINITE" if flags[name] & 1 else ""))
        lines.append(f"{wl:8s} mean dt {mean_dt:.6g} s (status bit 5 = 32: a held step overran the stable step of the state it reached)")
        for h in HOLDS:
            lines.append(f"{wl:8s} hold = {h}: {med[f'hold = {h}'] / med[A]:.3f} x adaptive, {med[f'hold = {h}'] / med[X]:.3f} x fixed dt")
        gain, spread = med[A] - med["hold = 16"], max(rng[A], rng["hold = 16"])
        ok = gain > spread and not any(f & 1 for f in flags.values())
        verdicts.append(ok)
        lines.append(f"{wl:8s} hold = 16 against adaptive: gain {gain:.4f} ms per step, spread {spread:.4f} ms: "
                     + ("FASTER by more than the spread" if ok else "NOT faster by more than the spread"))
    print("\n".join(lines[printed:]), flush=True)
    printed = len(lines)
lines.append("comparison (hold = 16 faster than the per-step adaptive call by more than the spread, every workload): "
             + ("MET" if verdicts and all(verdicts) else "NOT MET"))
print(lines[-1], flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
