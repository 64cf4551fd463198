#!/usr/bin/env python3
"""Time of an implicit step of a layered coupled context (lh_step_layered_coupled_implicit, backward Euler and
fixed-step TR-BDF2) against the explicit layered step (lh_step_ssprk33: three fused-stage launches per stable step),
against lh_step_coupled_implicit on a scalar context of the same shape and state, and against lh_step_coupled_implicit
on the layered context's own planes with the map taken away for the call (the same placement in HBM), in one process.

Ensemble: layered_heat_ref.make_layered_heat's coupled case with three horizons (the same in every column), a flux top
and a free-draining bottom for the water, Dirichlet faces for the energy, 64 levels, Float64; 4096 distinct columns
tiled to ncols (default 1e6).  Calls of `steps_per_call` steps (default 3) at 30x the stable step.  Every timed call
starts from the same state (lh_state_copy from a kept copy, outside the timer), so every repetition does the same
Newton work.  Per configuration one warm-up call, then `reps` timed calls (lh_timer_*: device events around one call),
the configurations ALTERNATING inside a repetition; reported: the median ms per step, the spread (max - min) / median
over the repetitions, the mean Newton iterations per column-stage (lh_implicit_iterations) and the column-stages of a
call that did not converge (lh_implicit_stats).  `horizons`: the three classes of layered_ref.texture_classes bottom to
top, "0,5,2" (default) or e.g. "2,5,0"; the result of every run is kept, one block per horizons, in
profiles/layered_coupled_implicit_timing.txt.

usage: tools/layered_coupled_implicit_timing.py [ncols] [steps_per_call] [reps] [horizons]"""
import ctypes as C
import dataclasses
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model
import layered_heat_ref as LH  # noqa: E402  (tests/: the case builder the GPU tests use)
import layered_ref as R  # noqa: E402

NLEV = 64
MULT = 30.0


def ensemble(ncols, horizons=(0, 5, 2), dtype=np.float64, distinct=4096):
    """three horizons (layered_ref.hydrostatic's proportions and classes, an organic one in the middle), tiled"""
    n0 = min(distinct, ncols)
    row = np.zeros(NLEV, dtype=np.uint8)
    row[NLEV * 5 // 16:] = 1
    row[NLEV * 11 // 16:] = 2
    lay = LH.make_layered_heat(dtype, n0, NLEV, np.repeat(row[None, :], n0, axis=0), model=M.MODEL_COUPLED,
                               classes=R.texture_classes()[list(horizons)], thermal=LH.thermal_classes()[[0, 4, 2]], bc="dirichlet")
    om = lay.case.om
    om.bc[(M.FACE_TOP, M.COMP_HYDROLOGY)] = (M.BC_FLUX, -2e-9)
    om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (M.BC_FREE_DRAINAGE, 0.0)
    reps = -(-ncols // n0)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:ncols])
    case = dataclasses.replace(lay.case, ncols=ncols, vl=tile(lay.case.vl), ti=tile(lay.case.ti), rhoe=tile(lay.case.rhoe))
    return LH.LayeredHeat(case, lay.classes, lay.thermal, row)


def one_call(gm, fn):
    """ms of one call (device events around it)"""
    L, ctx = gm.L, gm.ctx
    F.check(L.lh_synchronize(ctx), ctx)
    F.check(L.lh_timer_start(ctx), ctx)
    fn()
    ms = C.c_float()
    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
    return ms.value


def main():
    ncols = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    spc = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    horizons = tuple(int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "0,5,2").split(","))
    lay = ensemble(ncols, horizons)
    layered = W.GpuModel(lay.case)
    layered.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    scalar = W.GpuModel(lay.case)          # the same state, the context's scalars in every cell
    runs = {}                              # (context, method) -> (GpuModel, call, restore, before, after, stages per step)
    nothing = lambda: None
    sd = C.c_double()
    stable = {}
    for name, gm in (("layered", layered), ("scalar", scalar)):
        Y0, Ya = gm.prognostic_and_aux()   # the kept copy of the start
        Y, _ = gm.prognostic_and_aux()
        F.check(gm.L.lh_stable_dt(gm.ctx, Y0, Ya, 0.5, C.byref(sd)), gm.ctx)
        stable[name] = sd.value
        dt = MULT * stable["layered"]      # (both contexts take the layered context's step)
        restore = lambda gm=gm, Y=Y, Y0=Y0: F.check(gm.L.lh_state_copy(gm.ctx, Y, Y0), gm.ctx)
        fn = gm.L.lh_step_layered_coupled_implicit if name == "layered" else gm.L.lh_step_coupled_implicit
        for method, flags in (("euler", 0), ("trbdf2", F.LH_COUPLED_TRBDF2)):
            stages = 2 if flags else 1
            runs[(name, method)] = (gm, lambda gm=gm, fn=fn, Y=Y, Ya=Ya, dt=dt, flags=flags:
                                    F.check(fn(gm.ctx, Y, Ya, 0.0, dt, spc, flags, None, 0.0, 0), gm.ctx), restore, nothing, nothing, stages)
            if name == "layered":
                runs[("same planes", method)] = (
                    gm, lambda gm=gm, Y=Y, Ya=Ya, dt=dt, flags=flags:
                    F.check(gm.L.lh_step_coupled_implicit(gm.ctx, Y, Ya, 0.0, dt, spc, flags, None, 0.0, 0), gm.ctx), restore,
                    lambda gm=gm: gm.set_soil_class_map(None), lambda gm=gm: gm.set_soil_class_map(lay.class_map), stages)
        if name == "layered":
            runs[(name, "ssprk33")] = (gm, lambda gm=gm, Y=Y, Ya=Ya, dt=sd.value:
                                       F.check(gm.L.lh_step_ssprk33(gm.ctx, Y, Ya, 0.0, dt, spc, None), gm.ctx), restore, nothing, nothing, 0)
    ms = {k: [] for k in runs}
    newton, unconverged = {}, {}

    def iterations(gm):
        tot = C.c_int64()
        F.check(gm.L.lh_implicit_iterations(gm.ctx, C.byref(tot)), gm.ctx)
        return tot.value

    for k, (gm, fn, restore, before, after, stages) in runs.items():       # warm-up: code objects, first-use allocations
        restore()
        before()
        fn()
        F.check(gm.L.lh_synchronize(gm.ctx), gm.ctx)
        if stages:
            newton[k] = iterations(gm) / float(ncols * spc * stages)
            mi, un = C.c_int32(), C.c_int64()
            F.check(gm.L.lh_implicit_stats(gm.ctx, C.byref(mi), C.byref(un)), gm.ctx)
            unconverged[k] = (un.value, mi.value)
        after()
    for _ in range(reps):
        for k, (gm, fn, restore, before, after, stages) in runs.items():
            restore()
            before()
            ms[k].append(one_call(gm, fn) / spc)
            after()
    status = []
    for gm in (layered, scalar):
        st = C.c_uint32()
        F.check(gm.L.lh_get_status(gm.ctx, C.byref(st)), gm.ctx)
        status.append(st.value)       # (bit 3: some column-stage did not converge within the default 50 iterations)
    med = {k: statistics.median(v) for k, v in ms.items()}
    hz = ",".join(str(h) for h in horizons)
    lines = ["# tools/layered_coupled_implicit_timing.py %d %d %d %s: %d x %d Float64 columns, three horizons (classes %s bottom to top), flux top / free drainage, Dirichlet energy faces;"
             % (ncols, spc, reps, hz, ncols, NLEV, hz),
             "# ms per step of calls of %d steps, every call from the same state: median of %d calls, spread = (max - min) / median;" % (spc, reps),
             "# implicit calls at %gx the layered stable step (%.3g s; the scalar context's own: %.3g s), ssprk33 at 1x; newton = mean iterations per column-stage;"
             % (MULT, stable["layered"], stable["scalar"]),
             "# unconverged = column-stages of one call (of %d per stage of a step) that reached the cap of 50 iterations, max = the largest count;" % (ncols * spc),
             "# contexts: layered (class map set), scalar (a second context, same state, no classes), same planes (lh_step_coupled_implicit on the",
             "# layered context's own planes, its map taken away for the call); status words at the end: layered %d, scalar %d" % tuple(status)]
    for k in runs:
        lines.append("%-11s %-8s %9.4f ms/step  spread %5.1f %%%s" % (k[0], k[1], med[k], 100.0 * (max(ms[k]) - min(ms[k])) / med[k],
                                                                    "  newton %.2f  unconverged %d  max %d" % ((newton[k],) + unconverged[k]) if k in newton else ""))
    e = med[("layered", "ssprk33")]
    for method in ("euler", "trbdf2"):
        l, s, p = med[("layered", method)], med[("scalar", method)], med[("same planes", method)]
        lines.append("layered / scalar %-7s %.3f   layered / same planes %.3f   per Newton iteration: layered %.4f, same planes %.4f ms"
                     % (method, l / s, l / p, l / newton[("layered", method)], p / newton[("same planes", method)]))
        lines.append("layered %-7s / layered ssprk33 step %.2f (break-even: the implicit step pays from this many stable steps)" % (method, l / e))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "layered_coupled_implicit_timing.txt")
    kept = open(path).read() if os.path.exists(path) else ""
    blocks = [b for b in kept.split("\n\n") if b.strip() and (" %s: " % hz) not in b.splitlines()[0]]   # (one block per horizons)
    with open(path, "w") as f:
        f.write("\n\n".join(blocks + [text.rstrip("\n")]) + "\n")
    layered.close()
    scalar.close()


if __name__ == "__main__":
    main()
