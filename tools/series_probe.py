#!/usr/bin/env python3
"""What one lh_integrate_series call saves over the chain of calls it stands for, on the C2 ensemble
(Richards, Float64, 1e6 x 64 columns) with a flux top under a 24-interval storm series (25 knots, one per
hour by default; a triangular hyetograph that peaks at 0.6 Ksat).  In one process, after a warm-up of each:

  (a) chain      24 lh_integrate_trbdf2 calls, bcv = the series' values at the two ends of each interval, and
                 lh_trbdf2_stats (which synchronises) after each: what soil.py's _advance_trbdf2 does for a
                 time-dependent boundary value
  (b) uniform    one lh_integrate_series call, the same series for every column
  (c) percolumn  one lh_integrate_series call, every column its own multiple (0.5 .. 1.5) of the series: another
                 problem than (a) and (b) -- the columns' step sequences differ, which the chain cannot express
  (d) percolumn_same  the per-column table of (c) with the SAME values in every column: the problem of (b), so
                 (d) - (b) is what the per-column table itself costs (its loads, the lane-varying boundary values)

Every repetition starts from the same state and a zeroed dt_cols buffer; the four are timed in turn within
each repetition (device events through lh_timer_*, and the host's clock around the same work including the
final synchronise).  (b) is checked bitwise against (a) once.  States no threshold: the numbers are the result.
One configuration per (ensemble size, interval length): by default 1e6 and 65536 columns (one rank's share of a
partitioned ensemble: the launches and synchronisations weigh more), hourly knots (about one stable step per
interval: the knots set the steps) and six-hourly ones (several adaptive steps per interval).
usage: tools/series_probe.py [ncols,...] [interval_s,...] [repetitions] [out.json (default profiles/series_probe.json)]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
NINT = 24
TOP_H = (M.FACE_TOP, M.COMP_HYDROLOGY)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def probe(ncols, interval, reps):
    case = W.make_case("c2_richards_f64", ncols=ncols)
    T = interval * np.arange(NINT + 1, dtype=np.float64)
    peak = -0.6 * case.om.vg.Ksat                                  # (negative: into the soil)
    storm = peak * (1.0 - np.abs(np.arange(NINT + 1) - 10.0) / 14.0).clip(0.0)   # rises for 10 h, falls for 14 h
    scale = 0.5 + W.uhash(np.arange(ncols), 9, 1)                  # per column: 0.5 .. 1.5 of it
    dt0 = interval / 4.0
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        cols = torch.zeros(ncols, dtype=torch.float64, device="cuda")
        colp = C.c_void_p(cols.data_ptr())
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()

        def series_of(values, ks, cs):
            h = C.c_void_p()
            F.check(L.lh_bc_series_create(ctx, NINT + 1, dptr(T), C.byref(h)), ctx)
            F.check(L.lh_bc_series_set(ctx, h, TOP_H[0], TOP_H[1], dptr(values), ks, cs), ctx)
            return h

        uniform = series_of(np.ascontiguousarray(storm), 1, 0)
        table = np.ascontiguousarray(storm[:, None] * scale[None, :])
        percol = series_of(table, ncols, 1)
        table[:] = storm[:, None]
        same = series_of(table, ncols, 1)
        del table

        def stats():
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            return dict(zip(KEYS, list(st)))

        def chain():
            total = dict.fromkeys(KEYS, 0)
            bcv = np.zeros((2, 2, 2))
            for k in range(NINT):
                bcv[0][TOP_H], bcv[1][TOP_H] = storm[k], storm[k + 1]
                F.check(L.lh_integrate_trbdf2(ctx, Y, Ya, T[k], T[k + 1], dt0, 0.0, 0.0, 0, colp, dptr(bcv)), ctx)
                for key, v in stats().items():
                    total[key] += v
            return total

        def one(h):
            F.check(L.lh_integrate_series(ctx, Y, Ya, h, T[0], T[-1], dt0, 0.0, 0.0, 0.0, 0, colp), ctx)
            return stats()

        runs = (("chain", chain), ("uniform", lambda: one(uniform)), ("percolumn", lambda: one(percol)),
                ("percolumn_same", lambda: one(same)))

        def reset():
            F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
            cols.zero_()
            torch.cuda.synchronize()
            F.check(L.lh_synchronize(ctx), ctx)

        def timed(fn):
            reset()
            t0 = time.perf_counter()
            F.check(L.lh_timer_start(ctx), ctx)
            s = fn()
            ms = C.c_float()
            F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)       # (synchronises)
            return ms.value, (time.perf_counter() - t0) * 1e3, s

        out = dict(case=case.name, ncols=ncols, nlev=case.om.nlev, intervals=NINT, interval_s=interval,
                   stable_dt_s=round(sd.value, 3), dt0_s=dt0, peak_flux_m_s=peak, repetitions=reps, runs={})
        end = {}
        for name, fn in runs:                                      # warm-up (first-use allocations), and the end states
            timed(fn)
            end[name] = gm.download(Y, F.LH_VAR_VARTHETA_L)
            end[name + "_cols"] = cols.cpu().numpy()
        out["uniform_bitwise_equal_to_chain"] = bool(np.array_equal(end["chain"], end["uniform"]) and
                                                     np.array_equal(end["chain_cols"], end["uniform_cols"]))
        out["status"] = gm.status()
        ms = {name: [] for name, _ in runs}
        wall = {name: [] for name, _ in runs}
        last = {}
        for _ in range(reps):
            for name, fn in runs:
                a, b, s = timed(fn)
                ms[name].append(round(a, 3))
                wall[name].append(round(b, 3))
                last[name] = s
        waves = -(-ncols // 64)
        for name, _ in runs:
            s = last[name]
            mean_steps = (s["accepted"] + s["rejected"]) / ncols
            out["runs"][name] = dict(device_ms=ms[name], wall_ms=wall[name], device_ms_median=float(np.median(ms[name])),
                                     wall_ms_median=float(np.median(wall[name])), stats=s,
                                     steps_per_col=round(mean_steps, 3),
                                     # the chain's wave_steps is a sum of per-interval maxima, the series' one maximum of totals
                                     divergence=round(s["wave_steps"] / (64 * waves * mean_steps), 3))
        a = out["runs"]["chain"]
        out["percolumn_same_bitwise_equal_to_chain"] = bool(np.array_equal(end["chain"], end["percolumn_same"]))
        for name in ("uniform", "percolumn", "percolumn_same"):
            r = out["runs"][name]
            r["speedup_over_chain_device"] = round(a["device_ms_median"] / r["device_ms_median"], 3)
            r["speedup_over_chain_wall"] = round(a["wall_ms_median"] / r["wall_ms_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1000000,65536").split(",")]
    intervals = [float(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "3600,21600").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "series_probe.json")
    rows = [probe(n, dt, reps) for n in sizes for dt in intervals]
    with open(path, "w") as f:
        json.dump(dict(probe="tools/series_probe.py", configurations=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
