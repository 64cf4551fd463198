#!/usr/bin/env python3
"""Time of an implicit step of a layered heat-only context (lh_step_layered_heat_implicit, backward Euler and
fixed-step TR-BDF2) against lh_step_heat_implicit on a scalar context of the same shape and state, and against the
explicit layered step (lh_step_ssprk33: three fused-stage launches per stable step), in one process.

Ensemble: layered_heat_ref.make_layered_heat's heat-only case with three horizons (the same in every column) and
Dirichlet faces, 64 levels, Float64; 4096 distinct columns tiled to ncols (default 1e6).  Calls of `steps_per_call`
steps (default 30) at 30x the stable step; the prologue (every closure, the factorisation) is paid once per call and is
inside the timings; one-step calls are timed too, which gives the prologue.  The scalar call is also timed on the layered
context's own planes (its map taken away for that call): the same placement in HBM.  Per configuration one warm-up call,
then `reps` timed calls (lh_timer_*: device events around one call), the configurations ALTERNATING inside a repetition;
reported: the median ms per step and the spread (max - min) / median over the repetitions.  Writes profiles/layered_heat_implicit_timing.txt.

usage: tools/layered_heat_implicit_timing.py [ncols] [steps_per_call] [reps]"""
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


def ensemble(ncols, dtype=np.float64, distinct=4096):
    """three horizons (layered_ref.hydrostatic's proportions and classes, an organic one in the middle), tiled"""
    n0 = min(distinct, ncols)
    row = np.zeros(NLEV, dtype=np.uint8)
    row[NLEV * 5 // 16:] = 1
    row[NLEV * 11 // 16:] = 2
    lay = LH.make_layered_heat(dtype, n0, NLEV, np.repeat(row[None, :], n0, axis=0), model=M.MODEL_HEAT,
                               classes=R.texture_classes()[[0, 5, 2]], thermal=LH.thermal_classes()[[0, 4, 2]], bc="dirichlet")
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
    spc = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    lay = ensemble(ncols)
    layered = W.GpuModel(lay.case)
    layered.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    scalar = W.GpuModel(lay.case)          # the same state, the context's scalars in every cell
    runs = {}                              # (context, method, steps per call) -> (GpuModel, call, before, after)
    nothing = lambda: None
    sd = C.c_double()
    for name, gm in (("layered", layered), ("scalar", scalar)):
        Y, Ya = gm.prognostic_and_aux()
        F.check(gm.L.lh_stable_dt(gm.ctx, Y, Ya, 0.5, C.byref(sd)), gm.ctx)
        dt = 30.0 * sd.value
        fn = gm.L.lh_step_layered_heat_implicit if name == "layered" else gm.L.lh_step_heat_implicit
        for method, flags in (("euler", 0), ("trbdf2", F.LH_HEAT_TRBDF2)):
            Yi, _ = gm.prognostic_and_aux()
            for n in (spc, 1):
                runs[(name, method, n)] = (gm, lambda gm=gm, fn=fn, Yi=Yi, Ya=Ya, dt=dt, flags=flags, n=n:
                                           F.check(fn(gm.ctx, Yi, Ya, 0.0, dt, n, flags, None), gm.ctx), nothing, nothing)
            if name == "layered":
                # the scalar call on the SAME planes (this context with its map taken away for the call): what is left
                # of layered / scalar once the placement of the planes in HBM is the same
                runs[("same planes", method, spc)] = (
                    gm, lambda gm=gm, Yi=Yi, Ya=Ya, dt=dt, flags=flags:
                    F.check(gm.L.lh_step_heat_implicit(gm.ctx, Yi, Ya, 0.0, dt, spc, flags, None), gm.ctx),
                    lambda gm=gm: gm.set_soil_class_map(None), lambda gm=gm: gm.set_soil_class_map(lay.class_map))
        if name == "layered":
            Ye, _ = gm.prognostic_and_aux()
            runs[(name, "ssprk33", spc)] = (gm, lambda gm=gm, Ye=Ye, Ya=Ya, dt=sd.value:
                                            F.check(gm.L.lh_step_ssprk33(gm.ctx, Ye, Ya, 0.0, dt, spc, None), gm.ctx), nothing, nothing)
            stable_layered = sd.value
    ms = {k: [] for k in runs}
    for k, (gm, fn, before, after) in runs.items():       # warm-up: code objects, first-use allocations
        before()
        fn()
        F.check(gm.L.lh_synchronize(gm.ctx), gm.ctx)
        after()
    for _ in range(reps):
        for k, (gm, fn, before, after) in runs.items():
            before()
            ms[k].append(one_call(gm, fn) / k[2])
            after()
    for gm in (layered, scalar):
        st = C.c_uint32()
        F.check(gm.L.lh_get_status(gm.ctx, C.byref(st)), gm.ctx)
        assert st.value == 0, st.value
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = ["# tools/layered_heat_implicit_timing.py %d %d %d: %d x %d Float64 columns, three horizons, Dirichlet faces;" % (ncols, spc, reps, ncols, NLEV),
             "# ms per step of calls of N steps: median of %d calls, spread = (max - min) / median; implicit calls at 30x the stable step (%.1f s), ssprk33 at 1x;"
             % (reps, stable_layered),
             "# contexts: layered (class map set), scalar (a second context, same state, no classes), same planes (lh_step_heat_implicit on the layered",
             "# context's own planes, its map taken away for the call)"]
    for k in runs:
        lines.append("%-11s %-8s N=%-3d %9.4f ms/step  spread %5.1f %%" % (k[0], k[1], k[2], med[k], 100.0 * (max(ms[k]) - min(ms[k])) / med[k]))
    for method in ("euler", "trbdf2"):
        l, s, p = med[("layered", method, spc)], med[("scalar", method, spc)], med[("same planes", method, spc)]
        lines.append("layered / scalar %-7s %.3f   layered / same planes %.3f" % (method, l / s, l / p))
        lines.append("prologue (one-step call minus a step of the N=%d call) %-7s layered %.3f ms, scalar %.3f ms"
                     % (spc, method, med[("layered", method, 1)] - l, med[("scalar", method, 1)] - s))
        lines.append("layered %-7s / layered ssprk33 step %.3f (the implicit step pays from this many stable steps)"
                     % (method, l / med[("layered", "ssprk33", spc)]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "layered_heat_implicit_timing.txt"), "w") as f:
        f.write(text)
    layered.close()
    scalar.close()


if __name__ == "__main__":
    main()
