#!/usr/bin/env python3
"""Time and accuracy of the adaptive TR-BDF2 of a layered coupled context (lh_integrate_layered_coupled_trbdf2) against
fixed-step TR-BDF2 (lh_step_layered_coupled_implicit with LH_COUPLED_TRBDF2) at the fewest steps that are at least as
accurate, and against explicit stepping at the stable step (lh_step_ssprk33), on the same context.

Ensemble: tools/layered_coupled_implicit_timing.py's -- three horizons (the same in every column), a flux top and a
free-draining bottom for the water, Dirichlet faces for the energy, 64 levels, Float64; 4096 distinct columns tiled to
ncols (default 1e6).  One case = (horizons, span in stable steps, reltol); ONE PROCESS PER CASE, so that no case sees
another's allocations or clocks:

  tools/layered_coupled_trbdf2_timing.py                       all eight cases (0,5,2 and 2,5,0; 64 and 512; 1e-3 and 1e-4),
                                                               each in a child process, in turn
  tools/layered_coupled_trbdf2_timing.py HORIZONS SPAN RELTOL [ncols]     one case in this process

A case: every call starts from the same state (lh_state_copy from a kept copy, outside the timer) and is timed by
device events around it (lh_timer_*).  The adaptive call runs once untimed over one stable step (code objects, the
first-use allocations of its scratch planes and statistics), then ONE timed call over the span from h0 = the stable
step at the default abstol / abstol_e.  Its accuracy is the max-norm distance, per variable, to lh_step_ssprk33 at an
eighth of the stable step on a second context that holds the 4096 distinct columns.  The fixed-step call is searched on
that small context for the fewest steps N <= span whose distance is at most the adaptive call's in both variables (doubling,
then bisection: the distance is taken to fall with N; where even N = span is not as accurate the line says so), then timed once at N on the large context after an untimed call of one
step of that size.  The explicit stepper is timed once over the span at the stable step after an untimed step.
Reported per case: ms per call; attempted steps per column (mean, max); Newton iterations per water stage; lane
divergence wave_steps / (accepted + rejected); failed columns; the two distances; N and the fixed-step call's ms, Newton
iterations per stage and unconverged stages; the explicit call's ms.  One timed call per figure: no spread is measured.
Every case's block is kept in profiles/layered_coupled_trbdf2_timing.txt."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "layered_coupled_trbdf2_timing.txt")
CASES = [(hz, span, reltol) for hz in ("0,5,2", "2,5,0") for span in (64, 512) for reltol in (1e-3, 1e-4)]
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")


def keep(header, text):
    """one block per case in OUT, replaced when the case is run again"""
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    kept = open(OUT).read() if os.path.exists(OUT) else ""
    blocks = [b for b in kept.split("\n\n") if b.strip() and b.splitlines()[0] != header]
    with open(OUT, "w") as f:
        f.write("\n\n".join(blocks + [text.rstrip("\n")]) + "\n")


def run_case(horizons, span, reltol, ncols):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    import layered_coupled_implicit_timing as T0   # ensemble, one_call; loads the package

    F, W = T0.F, T0.W
    hz = tuple(int(x) for x in horizons.split(","))
    big_lay = T0.ensemble(ncols, hz)
    small_lay = T0.ensemble(min(4096, ncols), hz)
    big, small = W.GpuModel(big_lay.case), W.GpuModel(small_lay.case)
    big.set_soil_classes(big_lay.classes, big_lay.class_map, thermal=big_lay.thermal)
    small.set_soil_classes(small_lay.classes, small_lay.class_map, thermal=small_lay.thermal)
    ctxs = {}
    for name, gm in (("big", big), ("small", small)):
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        ctxs[name] = (gm, Y0, Y, Ya)
    sd = C.c_double()
    F.check(big.L.lh_stable_dt(big.ctx, ctxs["big"][1], ctxs["big"][3], 0.5, C.byref(sd)), big.ctx)
    sd = sd.value
    T = span * sd

    def restore(name):
        gm, Y0, Y, _ = ctxs[name]
        F.check(gm.L.lh_state_copy(gm.ctx, Y, Y0), gm.ctx)

    def state(name):
        gm, _, Y, _ = ctxs[name]
        return (gm.download(Y, F.LH_VAR_VARTHETA_L).astype(np.float64), gm.download(Y, F.LH_VAR_RHOE_INT).astype(np.float64))

    def adaptive(name, t1, cols, zero=True):
        gm, _, Y, Ya = ctxs[name]
        if zero:              # (every column starts from h0 = dt)
            cols.zero_()
            torch.cuda.synchronize()
        F.check(gm.L.lh_integrate_layered_coupled_trbdf2(gm.ctx, Y, Ya, 0.0, t1, sd, 0.0, 0.0, reltol, 0, C.c_void_p(cols.data_ptr()),
                                                         None), gm.ctx)

    def trbdf2_stats(gm):
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
        return dict(zip(KEYS, list(st)))

    def fixed(name, n, steps=None):
        """n steps of T / n (steps: only the first so many)"""
        gm, _, Y, Ya = ctxs[name]
        F.check(gm.L.lh_step_layered_coupled_implicit(gm.ctx, Y, Ya, 0.0, T / n, n if steps is None else steps, F.LH_COUPLED_TRBDF2,
                                                      None, 0.0, 0), gm.ctx)

    def explicit(name, dt, n):
        gm, _, Y, Ya = ctxs[name]
        F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, 0.0, dt, n, None), gm.ctx)

    say = lambda text: print("  .. " + text, file=sys.stderr, flush=True)   # (progress; not part of the result)
    dist = lambda a, b: (float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1]))))

    # the yardstick and the accuracies, on the distinct columns
    say("contexts ready; ssprk33 at sd/8 on the distinct columns")
    restore("small")
    explicit("small", sd / 8, 8 * span)
    want = state("small")
    cols_small = torch.zeros(small_lay.case.ncols, dtype=torch.float64, device="cuda")
    restore("small")
    adaptive("small", T, cols_small)
    err_a = dist(state("small"), want)
    restore("small")
    explicit("small", sd, span)
    err_x = dist(state("small"), want)

    def fixed_error(n):
        restore("small")
        fixed("small", n)
        un = C.c_int64()
        mi = C.c_int32()
        F.check(small.L.lh_implicit_stats(small.ctx, C.byref(mi), C.byref(un)), small.ctx)
        return dist(state("small"), want), un.value

    good = lambda e: e[0] <= err_a[0] and e[1] <= err_a[1]
    say("adaptive distance %.3g %.3g; searching the fixed step" % err_a)
    hi = 1                # (at most `span` steps: a fixed step below the stable step is the explicit stepper's ground)
    while not good(fixed_error(hi)[0]) and hi < span:
        hi = min(2 * hi, span)
    lo = hi // 2          # (not good, or 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if good(fixed_error(mid)[0]):
            hi = mid
        else:
            lo = mid
    n_fixed = hi
    err_f, _ = fixed_error(n_fixed)
    found = good(err_f)
    say("fixed step: N = %d, distance %.3g %.3g; timing" % ((n_fixed,) + err_f))

    # the timed calls, on the large context
    cols = torch.zeros(ncols, dtype=torch.float64, device="cuda")
    restore("big")
    adaptive("big", sd, cols)                     # untimed: code objects, first-use allocations
    restore("big")
    cols.zero_()
    torch.cuda.synchronize()
    ms_a = T0.one_call(big, lambda: adaptive("big", T, cols, zero=False))
    st = trbdf2_stats(big)
    status = C.c_uint32()
    F.check(big.L.lh_get_status(big.ctx, C.byref(status)), big.ctx)
    restore("big")
    fixed("big", n_fixed, 1)                      # untimed: one step of the size that is timed
    restore("big")
    ms_f = T0.one_call(big, lambda: fixed("big", n_fixed))
    tot, mi, un = C.c_int64(), C.c_int32(), C.c_int64()
    F.check(big.L.lh_implicit_iterations(big.ctx, C.byref(tot)), big.ctx)
    F.check(big.L.lh_implicit_stats(big.ctx, C.byref(mi), C.byref(un)), big.ctx)
    restore("big")
    explicit("big", sd, 1)                        # untimed
    restore("big")
    ms_x = T0.one_call(big, lambda: explicit("big", sd, span))

    attempted = st["accepted"] + st["rejected"]
    header = "# tools/layered_coupled_trbdf2_timing.py %s %d %g %d" % (horizons, span, reltol, ncols)
    lines = [header,
             "# %d x %d Float64 columns, horizons %s bottom to top, over %d stable steps (%.4g s each) from h0 = the stable step, reltol %g; one timed call each"
             % (ncols, T0.NLEV, horizons, span, sd, reltol),
             "adaptive      %10.2f ms/call  attempted steps per column mean %.2f max %d  (accepted %.2f rejected %.2f)  Newton per stage %.2f  "
             "lane divergence %.3f  failed %d"
             % (ms_a, attempted / float(ncols), st["max_steps"], st["accepted"] / float(ncols), st["rejected"] / float(ncols),
                st["newton_iterations"] / (2.0 * attempted) if attempted else 0.0, st["wave_steps"] / float(attempted) if attempted else 0.0,
                st["failed"]),
             "adaptive      distance to ssprk33 at sd/8: vartheta_l %.3g  rhoe_int %.3g" % err_a,
             "fixed TR-BDF2 %10.2f ms/call  N = %d steps of %.2f stable steps (%s)  Newton per stage %.2f  unconverged stages %d  "
             "distance vartheta_l %.3g  rhoe_int %.3g"
             % (ms_f, n_fixed, span / float(n_fixed), "the fewest at least as accurate" if found else "NOT as accurate: N is the search's cap, one step per stable step",
                tot.value / float(2 * n_fixed * ncols), un.value, err_f[0], err_f[1]),
             "ssprk33 at sd %10.2f ms/call  %d steps  distance vartheta_l %.3g  rhoe_int %.3g" % ((ms_x, span) + err_x),
             "adaptive / fixed %.3f   adaptive / explicit %.3f   status word after the adaptive call %d"
             % (ms_a / ms_f, ms_a / ms_x, status.value)]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    keep(header, text)
    big.close()
    small.close()


def main():
    if len(sys.argv) >= 4:
        run_case(sys.argv[1], int(sys.argv[2]), float(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000)
        return
    ncols = sys.argv[1:2] or ["1000000"]
    for hz, span, reltol in CASES:       # one process per case; a case that fails ends the run
        subprocess.run([sys.executable, os.path.abspath(__file__), hz, str(span), repr(reltol)] + ncols, check=True, timeout=300)


if __name__ == "__main__":
    main()
