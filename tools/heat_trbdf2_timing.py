#!/usr/bin/env python3
"""Time and accuracy of the adaptive TR-BDF2 of heat-only contexts (lh_integrate_heat_trbdf2,
lh_integrate_layered_heat_trbdf2) against fixed-step TR-BDF2 (lh_step_heat_implicit / lh_step_layered_heat_implicit with
LH_HEAT_TRBDF2) at the fewest equal steps that are at least as accurate, and against explicit stepping at the stable
step (lh_step_ssprk33), on the same context.

  tools/heat_trbdf2_timing.py [WORKLOAD [ncols [span]]]     WORKLOAD: scalar, layered, mixed (default: each in a child process)

Workloads, Float64, 64 levels, ncols columns (default 1e6) tiled from 256 distinct ones:
  layered   tools/layered_heat_implicit_timing.py's three horizons (the same in every column), Dirichlet faces
  scalar    the same state and faces on a context WITHOUT classes (the context's scalars in every cell, as that tool's
            scalar twin) -- a uniform ensemble
  mixed     the scalar case with static ice in the lower half of every other column and the water scaled per column
            between dry (x 0.3) and wet (x 1): columns that differ in rho_c_s and kappa within a wave
Every call starts from the same state (lh_state_copy from a kept copy, outside the timer) and is timed by device events
(lh_timer_*); one timed call per figure after an untimed call that takes the first-use allocations, so no spread is
measured.  Over `span` stable steps (default 2000) from h0 = the stable step:
  adaptive at reltol 1e-3 and 1e-4 (abstol_e at its default): ms, attempted steps per column (mean, max), lane
    divergence wave_steps / attempts, GB/s against 320 bytes per cell and attempt (the 40 plane words of
    lh_heat_trbdf2.hpp's header, Float64) and the max-norm distance to fixed TR-BDF2 at span / 4000 on the distinct columns;
  fixed TR-BDF2 at the fewest equal steps N whose distance is at most the adaptive call's (doubling, then bisection, on
    the distinct columns), timed at N on the large context;
  lh_step_ssprk33 at the stable step over the span.
The blocks are kept in profiles/heat_trbdf2_timing.txt."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "heat_trbdf2_timing.txt")
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
DISTINCT, BYTES_PER_ATTEMPT = 256, 320


def keep(header, text):
    """one block per workload in OUT, replaced when the workload is run again"""
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    kept = open(OUT).read() if os.path.exists(OUT) else ""
    blocks = [b for b in kept.split("\n\n") if b.strip() and b.splitlines()[0] != header]
    with open(OUT, "w") as f:
        f.write("\n\n".join(blocks + [text.rstrip("\n")]) + "\n")


def run(workload, ncols, span):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    import layered_heat_implicit_timing as T0   # ensemble, one_call; loads the package
    import heat_implicit_ref as H

    F, W = T0.F, T0.W
    layered = workload == "layered"
    NLEV = T0.NLEV

    def context(n):
        lay = T0.ensemble(n, distinct=DISTINCT)
        if layered:
            gm = W.GpuModel(lay.case)
            gm.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
            return gm
        case = lay.case
        if workload == "mixed":   # (by the column's index among the distinct ones, so that the tiling repeats it)
            c, lev = np.arange(n) % DISTINCT, np.arange(NLEV)
            wet = 0.3 + 0.7 * H.pc.uhash(c, 5, 1)
            ice = np.where((c % 2 == 0)[:, None] & (lev < NLEV // 2)[None, :], 0.05 * H.pc.uhash(c[:, None], lev[None, :] + 99, 1000), 0.0)
            case = dataclasses.replace(case, vl=np.ascontiguousarray(case.vl * wet[:, None]), ti=np.ascontiguousarray(ice))
        return W.GpuModel(case)

    big, small = context(ncols), context(min(DISTINCT, ncols))
    ctxs = {}
    for name, gm in (("big", big), ("small", small)):
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        ctxs[name] = (gm, Y0, Y, Ya)
    sd = C.c_double()
    F.check(big.L.lh_stable_dt(big.ctx, ctxs["big"][1], ctxs["big"][3], 0.5, C.byref(sd)), big.ctx)
    sd = sd.value
    T = span * sd
    adaptive_call = "lh_integrate_layered_heat_trbdf2" if layered else "lh_integrate_heat_trbdf2"
    fixed_call = "lh_step_layered_heat_implicit" if layered else "lh_step_heat_implicit"

    def restore(name):
        gm, Y0, Y, _ = ctxs[name]
        F.check(gm.L.lh_state_copy(gm.ctx, Y, Y0), gm.ctx)

    def state(name):
        gm, _, Y, _ = ctxs[name]
        return gm.download(Y, F.LH_VAR_RHOE_INT).astype(np.float64)

    def adaptive(name, t1, reltol, cols):
        gm, _, Y, Ya = ctxs[name]
        F.check(getattr(gm.L, adaptive_call)(gm.ctx, Y, Ya, 0.0, t1, sd, 0.0, reltol, 0, C.c_void_p(cols.data_ptr()), None), gm.ctx)

    def stats(gm):
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
        return dict(zip(KEYS, list(st)))

    def fixed(name, n, steps=None):
        gm, _, Y, Ya = ctxs[name]
        F.check(getattr(gm.L, fixed_call)(gm.ctx, Y, Ya, 0.0, T / n, n if steps is None else steps, F.LH_HEAT_TRBDF2, None), gm.ctx)

    def explicit(name, n):
        gm, _, Y, Ya = ctxs[name]
        F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, 0.0, sd, n, None), gm.ctx)

    def zeroed(n):
        cols = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return cols

    dist = lambda a, b: float(np.max(np.abs(a - b)))
    restore("small")
    fixed("small", 2 * span)
    want = state("small")
    scale = float(np.max(np.abs(want)))

    def fixed_error(n):
        restore("small")
        fixed("small", n)
        return dist(state("small"), want)

    header = "# tools/heat_trbdf2_timing.py %s %d %d" % (workload, ncols, span)
    lines = [header, "# %s: %d x %d Float64 columns over %d stable steps (%.4g s each) from h0 = the stable step; field scale %.3g; "
             "one timed call each" % (workload, ncols, NLEV, span, sd, scale)]
    restore("big")
    explicit("big", 1)                            # untimed
    restore("big")
    ms_x = T0.one_call(big, lambda: explicit("big", span))
    restore("small")
    explicit("small", span)
    err_x = dist(state("small"), want)
    lines.append("ssprk33 at sd        %10.2f ms/call  %d steps  distance %.3g" % (ms_x, span, err_x))
    for reltol in (1e-3, 1e-4):
        restore("small")
        adaptive("small", T, reltol, zeroed(small.case.ncols))
        err_a = dist(state("small"), want)
        hi = 1
        while fixed_error(hi) > err_a and hi < span:
            hi = min(2 * hi, span)
        lo = hi // 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fixed_error(mid) <= err_a:
                hi = mid
            else:
                lo = mid
        n_fixed, err_f = hi, fixed_error(hi)
        restore("big")
        adaptive("big", sd, reltol, zeroed(ncols))   # untimed: code objects, first-use allocations
        restore("big")
        cols = zeroed(ncols)
        ms_a = T0.one_call(big, lambda: adaptive("big", T, reltol, cols))
        st = stats(big)
        status = C.c_uint32()
        F.check(big.L.lh_get_status(big.ctx, C.byref(status)), big.ctx)
        restore("big")
        fixed("big", n_fixed, 1)                     # untimed: one step of the size that is timed
        restore("big")
        ms_f = T0.one_call(big, lambda: fixed("big", n_fixed))
        attempted = st["accepted"] + st["rejected"]
        gbs = BYTES_PER_ATTEMPT * float(NLEV) * st["wave_steps"] / (ms_a * 1e-3) / 1e9
        lines += ["adaptive reltol %-5g %10.2f ms/call  attempted steps per column mean %.2f max %d (accepted %.2f rejected %.2f)  "
                  "lane divergence %.3f  failed %d  status %d  distance %.3g  %.0f GB/s at 320 B per cell and attempt of the slowest lane"
                  % (reltol, ms_a, attempted / float(ncols), st["max_steps"], st["accepted"] / float(ncols), st["rejected"] / float(ncols),
                     st["wave_steps"] / float(attempted) if attempted else 0.0, st["failed"], status.value, err_a, gbs),
                  "fixed TR-BDF2        %10.2f ms/call  N = %d equal steps of %.1f stable steps (%s)  distance %.3g  adaptive / fixed %.2f  "
                  "adaptive / explicit %.4f"
                  % (ms_f, n_fixed, span / float(n_fixed), "the fewest at least as accurate" if err_f <= err_a else "NOT as accurate",
                     err_f, ms_a / ms_f, ms_a / ms_x)]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    keep(header, text)
    big.close()
    small.close()


def main():
    a = sys.argv[1:]
    ncols = int(a[1]) if len(a) > 1 else 1_000_000
    span = int(a[2]) if len(a) > 2 else 2000
    if a:
        run(a[0], ncols, span)
        return
    for w in ("scalar", "layered", "mixed"):      # one process per workload; a workload that fails ends the run
        subprocess.run([sys.executable, os.path.abspath(__file__), w, str(ncols), str(span)], check=True, timeout=280)


if __name__ == "__main__":
    main()
