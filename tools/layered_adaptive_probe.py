#!/usr/bin/env python3
"""Adaptive SSPRK33 for layered Richards soils: ms per SSPRK33 step of
lh_step_layered_ssprk33_adaptive_hold (calls of NCHUNKS chunks of `hold` steps) beside
  (a) fixed     lh_step_ssprk33 under `persist=2`, NCHUNKS calls of `hold` steps -- the fixed-step engine, the same kernel
                text without the step bound: the bound epilogue (and the one zero-step launch of a call) is the only extra;
  (b) by_hand   what a layered user did before: lh_stable_dt (a device-to-host read, a stream wait) followed by
                lh_step_ssprk33 of `hold` steps under the default tuning (the fused stages), NCHUNKS times.
One process per shape and type, 16 hashed classes, timed with lh_timer_* (device events; (b) includes its host
waits) around `reps` back-to-back calls after a warm-up call, every (path, hold) once per round, 5 rounds, the
median reported with the spread.

shapes    col1 (1 x 64), cols4096 (4096 x 64), c2 (1e6 x 64), n128 (500 000 x 128)

usage: tools/layered_adaptive_probe.py SHAPE f64|f32 [--chunks=N] [--inputs-only]     one JSON line per figure on stdout
       (append them to profiles/layered_adaptive_probe.jsonl)"""
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

SHAPES = {"col1": (1, 64), "cols4096": (4096, 64), "c2": (1_000_000, 64), "n128": (500_000, 128)}
HOLDS = (1, 4, 16, 30)
NCHUNKS = 4             # chunks per timed call (--chunks=N; 1 shows what a call's zero-step launch costs)
PATHS = ("adaptive_hold", "fixed", "by_hand")
COURANT = 0.1           # (the probe's states move little at this factor: every path steps the same kind of state)


def make_case(shape, dtype):
    ncols, nlev = SHAPES[shape]
    name = "c2_richards_f64" if dtype == np.float64 else "c2_richards_f32"
    return W.make_case(name if nlev == 64 else "%s_n%d" % (name, nlev), ncols=ncols)


class Probe:
    def __init__(self, case, classes, class_map):
        self.gm = gm = W.GpuModel(case)
        gm.set_soil_classes(classes, class_map)
        self.Y0, self.Ya = gm.prognostic_and_aux()
        self.Y = gm.state(0)
        self.words = torch.zeros(2, device="cuda", dtype=torch.float64 if case.dtype == np.float64 else torch.float32)
        torch.cuda.synchronize()
        self.dt_ptr = C.c_void_p(self.words.data_ptr())
        self.el_ptr = C.c_void_p(self.words.data_ptr() + self.words.element_size())
        self.dt = self.stable_dt(self.Y0)

    def stable_dt(self, Y):
        sd = C.c_double()
        F.check(self.gm.L.lh_stable_dt(self.gm.ctx, Y, self.Ya, COURANT, C.byref(sd)), self.gm.ctx)
        return sd.value

    def call(self, path, hold):
        L, ctx = self.gm.L, self.gm.ctx
        if path == "adaptive_hold":
            F.check(L.lh_step_layered_ssprk33_adaptive_hold(ctx, self.Y, self.Ya, 0.0, COURANT, 0.0, NCHUNKS, hold, self.dt_ptr,
                                                            self.el_ptr), ctx)
            return
        for _ in range(NCHUNKS):
            dt = self.dt if path == "fixed" else self.stable_dt(self.Y)
            F.check(L.lh_step_ssprk33(ctx, self.Y, self.Ya, 0.0, dt, hold, None), ctx)

    def ms_per_step(self, path, hold, reps):
        L, ctx = self.gm.L, self.gm.ctx
        F.check(L.lh_set_tuning(ctx, b"persist=2" if path == "fixed" else b""), ctx)
        F.check(L.lh_state_copy(ctx, self.Y, self.Y0), ctx)
        self.call(path, hold)                           # warm-up
        F.check(L.lh_synchronize(ctx), ctx)
        F.check(L.lh_timer_start(ctx), ctx)
        for _ in range(reps):
            self.call(path, hold)
        ms = C.c_float()
        F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
        return ms.value / (reps * NCHUNKS * hold)


def probe(shape, dtype, rounds=5):
    case = make_case(shape, dtype)
    ncols, nlev = SHAPES[shape]
    p = Probe(case, *maps(ncols, nlev)["layered_16"])
    reps = {1: 5, 4: 3, 16: 1, 30: 1} if ncols >= 100_000 else {1: 50, 4: 20, 16: 8, 30: 5}
    t = {}
    try:
        for _ in range(rounds):
            for path in PATHS:
                for hold in HOLDS:
                    t.setdefault((path, hold), []).append(p.ms_per_step(path, hold, reps[hold]))
        status = p.gm.status()
        assert not status & ~32, status      # (bit 5, a held step that overran, is a property of the state, not a failure)
    finally:
        p.gm.close()
    med = statistics.median
    rows = []
    for (path, hold), xs in t.items():
        r = dict(figure="ms_per_step", shape=shape, dtype=np.dtype(dtype).name, ncols=ncols, nlev=nlev, classes=16, path=path,
                 hold=hold, chunks_per_call=NCHUNKS, ms=round(med(xs), 5), spread=[round(min(xs), 5), round(max(xs), 5)], reps=reps[hold], rounds=rounds)
        if path == "adaptive_hold":
            r["over_fixed"] = round(med(xs) / med(t[("fixed", hold)]), 3)
            r["over_by_hand"] = round(med(xs) / med(t[("by_hand", hold)]), 3)
        rows.append(r)
    return rows


def main():
    global NCHUNKS
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    for a in sys.argv[1:]:
        if a.startswith("--chunks="):
            NCHUNKS = int(a.split("=", 1)[1])
    if len(args) != 2 or args[0] not in SHAPES or args[1] not in ("f64", "f32"):
        sys.exit(__doc__)
    shape, dtype = args[0], (np.float64 if args[1] == "f64" else np.float32)
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        case = make_case(shape, dtype)
        cls, m = maps(*SHAPES[shape])["layered_16"]
        assert case.vl.shape == SHAPES[shape] == m.shape and m.max() < len(cls)
        assert np.all(cls[:, 2] < case.vl.min()) and np.all(cls[:, 4] > case.vl.max())
        print("inputs ok")
        return
    for r in probe(shape, dtype):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
