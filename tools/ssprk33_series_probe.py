#!/usr/bin/env python3
"""lh_step_ssprk33_series beside the calls it stands next to: ms per SSPRK33 step of calls of
1, 4 and 30 steps on a Richards ensemble with a flux top, in ONE process per (shape, dtype) with one context, timed
with lh_timer_* (device events) around `reps` back-to-back calls after a warm-up call, every (row, call length) once
per round, 5 rounds, the median reported with the spread.

rows   plain          lh_step_ssprk33 without boundary values, persist=2 (the wave stepper; the parent's instructions)
       uniform_bcv    lh_step_ssprk33 with a uniform bc_stage_values, persist=2 (the same kernel reading the table)
       series_stepper lh_step_ssprk33_series, a per-column series of 25 knots on the top flux, persist=2
       series_fused   the same call under persist=0: one sampling launch and three fused-stage launches per step
shapes c2 (1e6 x 64), cols4096 (4096 x 64), col1 (1 x 64); c2v (f64 only): 1e6 x 50 columns with the viscosity factor,
       an aux T plane and a Dirichlet bottom (parity case richards_viscosity_f64) -- the FACTORS kernels, whose series
       instantiations are built for 5 waves per SIMD where the scalar ones have 6

usage: tools/ssprk33_series_probe.py SHAPE f64|f32 [--inputs-only]      one JSON line per figure on stdout"""
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model

SHAPES = {"c2": 1_000_000, "cols4096": 4096, "col1": 1, "c2v": 1_000_000}
NKNOTS = 25
CALLS = (1, 4, 30)
TOP_H = (M.FACE_TOP, M.COMP_HYDROLOGY)
FLUX = -2e-9
ROWS = (("plain", b"persist=2"), ("uniform_bcv", b"persist=2"), ("series_stepper", b"persist=2"), ("series_fused", b"persist=0"))
ENGINE = {F.LH_ENGINE_FUSED_STAGES: "fused_stages", F.LH_ENGINE_COLUMN_STEPPER: "column_stepper"}


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def make_case(shape, dtype):
    if shape == "c2v":
        case = W.make_case("richards_viscosity_f64", ncols=SHAPES[shape])
    else:
        case = W.make_case("c2_richards_f64" if dtype == np.float64 else "c2_richards_f32", ncols=SHAPES[shape])
    bc = dict(case.om.bc)
    bc[TOP_H] = (M.BC_FLUX, FLUX)
    return dataclasses.replace(case, om=dataclasses.replace(case.om, bc=bc))


def make_tables(ncols, dt):
    """25 irregular knots over the 31 dt the longest call needs; per column the flux scaled by a factor of its own"""
    gaps = 0.4 + W.uhash(np.arange(NKNOTS - 1), 41, 1)
    T = np.concatenate([[0.0], np.cumsum(gaps)]) * (31.5 * dt / gaps.sum())
    shape = FLUX * (0.5 + 2.0 * W.uhash(np.arange(NKNOTS), 42, 1))
    vals = np.ascontiguousarray(shape[:, None] * (0.5 + W.uhash(np.arange(ncols), 43, 1))[None, :])
    return np.ascontiguousarray(T), vals


def probe(shape, dtype, rounds=5):
    case = make_case(shape, dtype)
    ncols = case.ncols
    gm = W.GpuModel(case)
    L, ctx = gm.L, gm.ctx
    try:
        Y0, Ya = gm.prognostic_and_aux()
        Y = gm.state(0)
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        dt = 0.2 * sd.value
        T, vals = make_tables(ncols, dt)
        h = C.c_void_p()
        F.check(L.lh_bc_series_create(ctx, NKNOTS, _dptr(T), C.byref(h)), ctx)
        F.check(L.lh_bc_series_set(ctx, h, TOP_H[0], TOP_H[1], _dptr(vals), ncols, 1), ctx)
        bcv = np.zeros((max(CALLS), 3, 2, 2))
        bcv[:, :, TOP_H[0], TOP_H[1]] = FLUX * (0.5 + 2.0 * W.uhash(np.arange(3 * max(CALLS)), 44, 1)).reshape(-1, 3)

        def call(row, nsteps):
            if row == "plain":
                return L.lh_step_ssprk33(ctx, Y, Ya, 0.0, dt, nsteps, None)
            if row == "uniform_bcv":
                return L.lh_step_ssprk33(ctx, Y, Ya, 0.0, dt, nsteps, _dptr(bcv))
            return L.lh_step_ssprk33_series(ctx, Y, Ya, h, 0.0, dt, nsteps)

        reps = {1: 5, 4: 3, 30: 1} if ncols >= 100_000 else {1: 50, 4: 20, 30: 5}
        t, engine = {}, {}
        for _ in range(rounds):
            for row, tuning in ROWS:
                F.check(L.lh_set_tuning(ctx, tuning), ctx)
                for nsteps in CALLS:
                    F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                    F.check(call(row, nsteps), ctx)                # warm-up
                    F.check(L.lh_synchronize(ctx), ctx)
                    F.check(L.lh_timer_start(ctx), ctx)
                    for _ in range(reps[nsteps]):
                        F.check(call(row, nsteps), ctx)
                    ms = C.c_float()
                    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
                    t.setdefault((row, nsteps), []).append(ms.value / (reps[nsteps] * nsteps))
                    engine[(row, nsteps)] = (L.lh_step_series_engine(ctx, nsteps) if row.startswith("series")
                                             else L.lh_step_engine(ctx, nsteps, int(row == "uniform_bcv")))
        assert gm.status() == 0
    finally:
        gm.close()
    med = statistics.median
    rows = []
    for (row, nsteps), xs in t.items():
        r = dict(figure="ms_per_step", shape=shape, dtype=np.dtype(dtype).name, ncols=ncols, nlev=case.om.nlev, nknots=NKNOTS, row=row,
                 tuning=dict(ROWS)[row].decode(), engine=ENGINE[engine[(row, nsteps)]], steps_per_call=nsteps,
                 ms=round(med(xs), 5), spread=[round(min(xs), 5), round(max(xs), 5)], reps=reps[nsteps], rounds=rounds)
        if row.startswith("series"):
            r["over_uniform_bcv"] = round(med(xs) / med(t[("uniform_bcv", nsteps)]), 3)
        if row == "series_stepper":
            r["over_series_fused"] = round(med(xs) / med(t[("series_fused", nsteps)]), 3)
        rows.append(r)
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2 or args[0] not in SHAPES or args[1] not in ("f64", "f32") or (args[0] == "c2v" and args[1] != "f64"):
        sys.exit(__doc__)
    shape, dtype = args[0], (np.float64 if args[1] == "f64" else np.float32)
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        case = make_case(shape, dtype)
        T, vals = make_tables(case.ncols, 1.0)
        assert case.vl.shape == (SHAPES[shape], case.om.nlev) and vals.shape == (NKNOTS, case.ncols)
        assert np.all(np.diff(T) > 0) and T[0] == 0.0 and T[-1] >= 31.0
        print("inputs ok")
        return
    for r in probe(shape, dtype):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
