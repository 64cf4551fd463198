#!/usr/bin/env python3
"""What hourly output costs the adaptive TR-BDF2 integration of the heat-only model, with and without
lh_integrate_heat_dense (tools/dense_probe.py for the heat-only family): tools/heat_series_probe.py's
scalar ensemble (Float64, 64 levels, tiled from 4096 distinct columns, a Dirichlet bottom and a flux top) under a 24 h
diurnal surface heat flux (a half-sine of 150 W/m^2 into the soil by day, 40 W/m^2 out at night; knots every `knot_s`
seconds) and 24 snapshots, one per hour.  In one process, after a warm-up of each:

  (a) chain   24 lh_integrate_heat_series calls, one per hour, each followed by lh_state_copy of Y into that hour's
              snapshot: existing code, the reference.  Every column cuts its step to land on every hour, and runs its
              prologue (the closure sweep and a fresh f_n) there.
  (b) dense   one lh_integrate_heat_dense call over the 24 h with the 24 hours as save times
  (c) nosave  the same call with nsave = 0 (bitwise lh_integrate_heat_series over the 24 h): (b) - (c) is what the
              output itself costs

Every repetition starts from the same state and a zeroed dt_cols buffer; the three are timed in turn within each
repetition (device events through lh_timer_*, and the host's clock around the same work including the final
synchronise).  The counters of (a) are summed over its calls in an untimed pass (lh_trbdf2_stats synchronises).
States no threshold: the numbers are the result.
usage: tools/heat_dense_probe.py [ncols,...] [knot_s,...] [repetitions] [out.json (default profiles/heat_dense_probe.json)]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import layered_heat_implicit_timing as T0   # the ensemble; loads the package

F, W, M = T0.F, T0.W, T0.M
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
HOURS = 24
HOUR = 3600.0
TOP_E = (M.FACE_TOP, M.COMP_ENERGY)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def probe(ncols, knot_s, reps):
    lay = T0.ensemble(ncols)
    case = lay.case
    case.om.bc[TOP_E] = (M.BC_FLUX, 0.0)
    T = np.arange(0.0, HOURS * HOUR + 0.5 * knot_s, knot_s)
    assert T[-1] == HOURS * HOUR
    s = np.sin(2.0 * np.pi * (T / HOUR - 6.0) / 24.0)
    flux = np.ascontiguousarray(np.where(s > 0, -150.0 * s, 40.0))
    saves = np.ascontiguousarray(HOUR * np.arange(1, HOURS + 1, dtype=np.float64))
    dt0 = HOUR / 4.0
    RE = F.LH_VAR_RHOE_INT
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        snaps = [gm.state(1 << RE) for _ in range(HOURS)]
        handles = (C.c_void_p * HOURS)(*[x.value for x in snaps])
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        cols = torch.zeros(ncols, dtype=torch.float64, device="cuda")
        colp = C.c_void_p(cols.data_ptr())
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
        h = C.c_void_p()
        F.check(L.lh_bc_series_create(ctx, len(T), dptr(T), C.byref(h)), ctx)
        F.check(L.lh_bc_series_set(ctx, h, TOP_E[0], TOP_E[1], dptr(flux), 1, 0), ctx)

        def stats():
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            return dict(zip(KEYS, list(st)))

        def chain(count=False):
            total = dict.fromkeys(KEYS, 0)
            a = 0.0
            for k in range(HOURS):
                F.check(L.lh_integrate_heat_series(ctx, Y, Ya, h, a, saves[k], dt0, 0.0, 0.0, 0, colp), ctx)
                F.check(L.lh_state_copy(ctx, snaps[k], Y), ctx)
                a = saves[k]
                if count:
                    for key, v in stats().items():
                        total[key] += v
            return total

        def dense(nsave):
            F.check(L.lh_integrate_heat_dense(ctx, Y, Ya, h, 0.0, saves[-1], dt0, 0.0, 0.0, 0, colp, nsave,
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
                   dt0_s=dt0, repetitions=reps, runs={})
        # warm-up (first-use allocations), the counters and the end states
        counters, end = {}, {}
        reset()
        counters["chain"] = chain(count=True)
        end["chain"] = gm.download(Y, RE)
        mid_chain = gm.download(snaps[11], RE)
        for name in ("dense", "nosave"):
            reset()
            dense(HOURS if name == "dense" else 0)
            counters[name] = stats()
            end[name] = gm.download(Y, RE)
        reset()
        dense(HOURS)
        mid_dense = gm.download(snaps[11], RE)
        last_dense = gm.download(snaps[-1], RE)
        e = case.om.earth
        scale = lambda v: 1e-6 * e.cp_l * e.rho_liq + 1e-3 * np.abs(v)       # (the default abstol_e + reltol |v|)
        out["dense_Y_bitwise_equal_to_nosave"] = bool(np.array_equal(end["dense"], end["nosave"]))
        out["last_snapshot_bitwise_equal_to_Y"] = bool(np.array_equal(last_dense, end["dense"]))
        out["max_scaled_difference_dense_vs_chain_at_12h"] = float(np.max(np.abs(mid_dense - mid_chain) / scale(mid_chain)))
        out["max_scaled_difference_dense_vs_chain_at_24h"] = float(np.max(np.abs(end["dense"] - end["chain"]) / scale(end["chain"])))
        out["status"] = gm.status()
        del end, mid_chain, mid_dense, last_dense
        ms = {name: [] for name, _ in runs}
        wall = {name: [] for name, _ in runs}
        for _ in range(reps):
            for name, fn in runs:
                a, b = timed(fn)
                ms[name].append(round(a, 3))
                wall[name].append(round(b, 3))
        waves = -(-ncols // 64)
        for name, _ in runs:
            c = counters[name]
            mean_steps = (c["accepted"] + c["rejected"]) / ncols
            out["runs"][name] = dict(device_ms=ms[name], wall_ms=wall[name], device_ms_median=float(np.median(ms[name])),
                                     wall_ms_median=float(np.median(wall[name])), stats=c, steps_per_col=round(mean_steps, 3),
                                     # (the chain's wave_steps is a sum of per-call maxima, the others' one maximum of totals)
                                     wave_steps_per_wave=round(c["wave_steps"] / (64 * waves), 3))
        a = out["runs"]["chain"]
        for name in ("dense", "nosave"):
            r = out["runs"][name]
            r["speedup_over_chain_device"] = round(a["device_ms_median"] / r["device_ms_median"], 3)
            r["speedup_over_chain_wall"] = round(a["wall_ms_median"] / r["wall_ms_median"], 3)
        out["output_cost_device_ms"] = round(out["runs"]["dense"]["device_ms_median"] - out["runs"]["nosave"]["device_ms_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1000000").split(",")]
    knots = [float(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "3600,21600").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "heat_dense_probe.json")
    rows = []
    for n in sizes:
        for k in knots:
            rows.append(probe(n, k, reps))
            with open(path, "w") as f:   # (kept after every configuration)
                json.dump(dict(probe="tools/heat_dense_probe.py", configurations=rows), f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
