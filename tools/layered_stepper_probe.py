#!/usr/bin/env python3
"""The persistent column stepper of layered soils beside the fused stages it replaces
under `persist=2`: ms per SSPRK33 step of lh_step_ssprk33 calls of 1, 4 and 30 steps, in ONE process with one
context per variant, timed with lh_timer_* (device events) around `reps` back-to-back calls after a warm-up
call, every (variant, tuning, call length) once per round, 5 rounds, the median reported with the spread.

tunings   persist=0  three fused-stage launches per step: what a layered context runs by default (the baseline)
          persist=2  the column stepper, one launch per call
variants  scalar      the context's six scalars, no class map (column_stepper_wave_kernel under persist=2)
          layered_1   one class (the scalars), the map all zeros
          layered_4   four horizons of equal thickness, four classes
          layered_16  16 classes assigned per cell by uhash
shapes    c2 (1e6 x 64, all variants), n128 (500 000 x 128), col1 (1 x 64), cols4096 (4096 x 64): scalar and layered_16

usage: tools/layered_stepper_probe.py SHAPE f64|f32 [--inputs-only]      one JSON line per figure on stdout"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g
from layered_probe import maps

pkg = g.load_package()
F, W = pkg._ffi, pkg.workloads

SHAPES = {"c2": (1_000_000, 64, ("scalar", "layered_1", "layered_4", "layered_16")),
          "n128": (500_000, 128, ("scalar", "layered_16")),
          "col1": (1, 64, ("scalar", "layered_16")),
          "cols4096": (4096, 64, ("scalar", "layered_16"))}
CALLS = (1, 4, 30)                  # steps per lh_step_ssprk33 call
TUNINGS = (b"persist=0", b"persist=2")
ENGINE = {F.LH_ENGINE_FUSED_STAGES: "fused_stages", F.LH_ENGINE_COLUMN_STEPPER: "column_stepper"}


def make_case(shape, dtype):
    ncols, nlev, _ = SHAPES[shape]
    name = "c2_richards_f64" if dtype == np.float64 else "c2_richards_f32"
    return W.make_case(name if nlev == 64 else "%s_n%d" % (name, nlev), ncols=ncols)


class Variant:
    """one context with its own states; dt: 0.2 x the stable step of its parameters"""

    def __init__(self, case, name, layered):
        self.name, self.gm = name, W.GpuModel(case)
        gm = self.gm
        if name in layered:
            gm.set_soil_classes(*layered[name])
        self.Y0, self.Ya = gm.prognostic_and_aux()
        self.Y = gm.state(0)
        sd = C.c_double()
        F.check(gm.L.lh_stable_dt(gm.ctx, self.Y0, self.Ya, 0.5, C.byref(sd)), gm.ctx)
        self.dt = 0.2 * sd.value

    def ms_per_step(self, tuning, nsteps, reps):
        gm = self.gm
        L, ctx = gm.L, gm.ctx
        F.check(L.lh_set_tuning(ctx, tuning), ctx)
        F.check(L.lh_state_copy(ctx, self.Y, self.Y0), ctx)
        call = lambda: F.check(L.lh_step_ssprk33(ctx, self.Y, self.Ya, 0.0, self.dt, nsteps, None), ctx)
        call()                                        # warm-up
        F.check(L.lh_synchronize(ctx), ctx)
        F.check(L.lh_timer_start(ctx), ctx)
        for _ in range(reps):
            call()
        ms = C.c_float()
        F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
        return ms.value / (reps * nsteps), L.lh_step_engine(ctx, nsteps, 0)


def probe(shape, dtype, rounds=5):
    case = make_case(shape, dtype)
    ncols, nlev, names = SHAPES[shape]
    layered = maps(ncols, nlev)
    variants = [Variant(case, v, layered) for v in names]
    reps = {1: 5, 4: 3, 30: 1} if ncols >= 100_000 else {1: 50, 4: 20, 30: 5}
    t, engine = {}, {}
    try:
        for _ in range(rounds):
            for v in variants:
                for tuning in TUNINGS:
                    for nsteps in CALLS:
                        ms, e = v.ms_per_step(tuning, nsteps, reps[nsteps])
                        t.setdefault((v.name, tuning, nsteps), []).append(ms)
                        engine[(v.name, tuning, nsteps)] = e
        for v in variants:
            assert v.gm.status() == 0, v.name
    finally:
        for v in variants:
            v.gm.close()
    med = statistics.median
    rows = []
    for (name, tuning, nsteps), xs in t.items():
        r = dict(figure="ms_per_step", shape=shape, dtype=np.dtype(dtype).name, ncols=ncols, nlev=nlev, variant=name,
                 tuning=tuning.decode(), engine=ENGINE[engine[(name, tuning, nsteps)]], steps_per_call=nsteps,
                 ms=round(med(xs), 5), spread=[round(min(xs), 5), round(max(xs), 5)], reps=reps[nsteps], rounds=rounds)
        if tuning == b"persist=2":
            r["over_persist0"] = round(med(xs) / med(t[(name, b"persist=0", nsteps)]), 3)
            r["over_scalar_stepper"] = round(med(xs) / med(t[("scalar", b"persist=2", nsteps)]), 3)
        rows.append(r)
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2 or args[0] not in SHAPES or args[1] not in ("f64", "f32"):
        sys.exit(__doc__)
    shape, dtype = args[0], (np.float64 if args[1] == "f64" else np.float32)
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        case = make_case(shape, dtype)
        ncols, nlev, names = SHAPES[shape]
        assert case.vl.shape == (ncols, nlev)
        for v, (cls, m) in maps(ncols, nlev).items():
            assert m.shape == case.vl.shape and m.max() < len(cls)
            assert np.all(cls[:, 2] < case.vl.min()) and np.all(cls[:, 4] > case.vl.max()), v
        print("inputs ok")
        return
    for r in probe(shape, dtype):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
