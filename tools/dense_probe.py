#!/usr/bin/env python3
"""What hourly output costs the adaptive TR-BDF2 integration, with and without lh_integrate_dense, on the C2 ensemble
(Richards, Float64, 64 levels) with a flux top under a 24 h storm series (a triangular hyetograph that peaks at
0.6 Ksat; knots every `knot_s` seconds) and 24 snapshots, one per hour.  In one process, after a warm-up of each:

  (a) chain   24 lh_integrate_series calls, one per hour, each followed by lh_state_copy of Y into that hour's
              snapshot: existing code, the reference.  Every column cuts its step to land on every hour.
  (b) dense   one lh_integrate_dense call over the 24 h with the 24 hours as save times
  (c) nosave  the same call with nsave = 0 (bitwise lh_integrate_series over the 24 h): (b) - (c) is what the output
              itself costs

Every repetition starts from the same state and a zeroed dt_cols buffer; the three are timed in turn within each
repetition (device events through lh_timer_*, and the host's clock around the same work including the final
synchronise).  The counters of (a) are summed over its calls in an untimed pass (lh_trbdf2_stats synchronises).
States no threshold: the numbers are the result.  One configuration per (ensemble size, knot spacing): by default 1e6
and 65536 columns, hourly knots (the forcing's own breakpoints already fall on every hour) and six-hourly ones (the
output is what would set the steps).
usage: tools/dense_probe.py [ncols,...] [knot_s,...] [repetitions] [out.json (default profiles/dense_probe.json)]"""
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
HOURS = 24
HOUR = 3600.0
TOP_H = (M.FACE_TOP, M.COMP_HYDROLOGY)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def probe(ncols, knot_s, reps):
    case = W.make_case("c2_richards_f64", ncols=ncols)
    T = np.arange(0.0, HOURS * HOUR + 0.5 * knot_s, knot_s)
    assert T[-1] == HOURS * HOUR
    peak = -0.6 * case.om.vg.Ksat                                  # (negative: into the soil)
    storm = np.ascontiguousarray(peak * (1.0 - np.abs(T / HOUR - 10.0) / 14.0).clip(0.0))   # rises for 10 h, falls for 14 h
    saves = np.ascontiguousarray(HOUR * np.arange(1, HOURS + 1, dtype=np.float64))
    dt0 = HOUR / 4.0
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        snaps = [gm.state(0) for _ in range(HOURS)]
        handles = (C.c_void_p * HOURS)(*[s.value for s in snaps])
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        cols = torch.zeros(ncols, dtype=torch.float64, device="cuda")
        colp = C.c_void_p(cols.data_ptr())
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        h = C.c_void_p()
        F.check(L.lh_bc_series_create(ctx, len(T), dptr(T), C.byref(h)), ctx)
        F.check(L.lh_bc_series_set(ctx, h, TOP_H[0], TOP_H[1], dptr(storm), 1, 0), ctx)

        def stats():
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            return dict(zip(KEYS, list(st)))

        def chain(count=False):
            total = dict.fromkeys(KEYS, 0)
            a = 0.0
            for k in range(HOURS):
                F.check(L.lh_integrate_series(ctx, Y, Ya, h, a, saves[k], dt0, 0.0, 0.0, 0.0, 0, colp), ctx)
                F.check(L.lh_state_copy(ctx, snaps[k], Y), ctx)
                a = saves[k]
                if count:
                    for key, v in stats().items():
                        total[key] += v
            return total

        def dense(nsave):
            F.check(L.lh_integrate_dense(ctx, Y, Ya, h, 0.0, saves[-1], dt0, 0.0, 0.0, 0.0, 0, colp, nsave,
                                         dptr(saves) if nsave else None, handles if nsave else None), ctx)

        runs = (("chain", chain), ("dense", lambda: dense(HOURS)), ("nosave", lambda: dense(0)))

        def reset():
            F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
            cols.zero_()
            torch.cuda.synchronize()
            F.check(L.lh_synchronize(ctx), ctx)

        def timed(fn):
            reset()
            t0 = time.perf_counter()
            F.check(L.lh_timer_start(ctx), ctx)
            fn()
            ms = C.c_float()
            F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)       # (synchronises)
            return ms.value, (time.perf_counter() - t0) * 1e3

        out = dict(case=case.name, ncols=ncols, nlev=case.om.nlev, hours=HOURS, knot_s=knot_s, stable_dt_s=round(sd.value, 3),
                   dt0_s=dt0, peak_flux_m_s=peak, repetitions=reps, runs={})
        # warm-up (first-use allocations), the counters and the end states
        counters, end = {}, {}
        reset()
        counters["chain"] = chain(count=True)
        end["chain"] = gm.download(Y, F.LH_VAR_VARTHETA_L)
        mid_chain = gm.download(snaps[11], F.LH_VAR_VARTHETA_L)
        for name in ("dense", "nosave"):
            reset()
            dense(HOURS if name == "dense" else 0)
            counters[name] = stats()
            end[name] = gm.download(Y, F.LH_VAR_VARTHETA_L)
        reset()
        dense(HOURS)
        mid_dense = gm.download(snaps[11], F.LH_VAR_VARTHETA_L)
        last_dense = gm.download(snaps[-1], F.LH_VAR_VARTHETA_L)
        out["dense_Y_bitwise_equal_to_nosave"] = bool(np.array_equal(end["dense"], end["nosave"]))
        out["last_snapshot_bitwise_equal_to_Y"] = bool(np.array_equal(last_dense, end["dense"]))
        out["max_abs_difference_dense_vs_chain_at_12h"] = float(np.max(np.abs(mid_dense - mid_chain)))
        out["max_abs_difference_dense_vs_chain_at_24h"] = float(np.max(np.abs(end["dense"] - end["chain"])))
        out["status"] = gm.status()
        ms = {name: [] for name, _ in runs}
        wall = {name: [] for name, _ in runs}
        for _ in range(reps):
            for name, fn in runs:
                a, b = timed(fn)
                ms[name].append(round(a, 3))
                wall[name].append(round(b, 3))
        waves = -(-ncols // 64)
        for name, _ in runs:
            s = counters[name]
            mean_steps = (s["accepted"] + s["rejected"]) / ncols
            out["runs"][name] = dict(device_ms=ms[name], wall_ms=wall[name], device_ms_median=float(np.median(ms[name])),
                                     wall_ms_median=float(np.median(wall[name])), stats=s, steps_per_col=round(mean_steps, 3),
                                     # (the chain's wave_steps is a sum of per-call maxima, the others' one maximum of totals)
                                     wave_steps_per_wave=round(s["wave_steps"] / (64 * waves), 3))
        a = out["runs"]["chain"]
        for name in ("dense", "nosave"):
            r = out["runs"][name]
            r["speedup_over_chain_device"] = round(a["device_ms_median"] / r["device_ms_median"], 3)
            r["speedup_over_chain_wall"] = round(a["wall_ms_median"] / r["wall_ms_median"], 3)
        out["output_cost_device_ms"] = round(out["runs"]["dense"]["device_ms_median"] - out["runs"]["nosave"]["device_ms_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1000000,65536").split(",")]
    knots = [float(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "3600,21600").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "dense_probe.json")
    rows = [probe(n, k, reps) for n in sizes for k in knots]
    with open(path, "w") as f:
        json.dump(dict(probe="tools/dense_probe.py", configurations=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
