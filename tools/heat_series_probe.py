#!/usr/bin/env python3
"""What one lh_integrate_heat_series / lh_integrate_layered_coupled_series call saves over the chain of calls it stands
for (tools/series_probe.py for the heat-only and the layered coupled families).

Workloads, Float64, 64 levels, tiled from 4096 distinct columns:
  heat_scalar      tools/heat_trbdf2_timing.py's scalar ensemble (no class map), a Dirichlet bottom and a FLUX top
  heat_layered     its three-horizon ensemble (a class map with thermal supplements), the same faces
  layered_coupled  tools/layered_coupled_trbdf2_timing.py's three-horizon coupled ensemble: a flux top and a free-draining
                   bottom for the water, Dirichlet temperatures
under a series of 48 hourly knots: for heat a diurnal surface heat flux (a half-sine of 150 W/m^2 into the soil by day,
40 W/m^2 out at night); for the coupled family a storm on the top water flux (tools/series_probe.py's triangle) and a
diurnal top temperature (+- 5 K).  In one process, after a warm-up of each:

  (a) chain           47 calls of the wrapped entry point, bcv = the series' values at the two ends of each interval, and
                      lh_trbdf2_stats (which synchronises) after each
  (b) uniform         one series call, the same series for every column: bitwise (a), checked once
  (d) percolumn_same  the same values through a per-column table: the problem of (b); (d) - (b) is what the table costs
  (c) percolumn       every column its own amplitude (x 0.5 .. 1.5) and phase (+- 1 h) of the series: another problem,
                      which the chain cannot express

Every repetition starts from the same state and a zeroed dt_cols buffer; the four are timed in turn within each
repetition (device events through lh_timer_*, and the host's clock around the same work including the final
synchronise).  Reported per run: the median of the repetitions with [min, max], attempted steps per column, the lane
divergence wave_steps / attempts, and (a) / (b).

The prologue's share (heat only: every sub-interval re-runs heat_trbdf2_column's closure sweep and fresh f_n): the series
call over [T_0, T_46] with all its knots against the same call with the knots thinned to every second one, on a series
whose value is CONSTANT in time, so that both integrate the same problem; their attempt counts still differ (a step is
clipped at every breakpoint), so the thinned call's time is scaled to the full call's wave_steps before the difference
is taken.  An estimate, stated as such: share = (ms_full - ms_thin wave_steps_full / wave_steps_thin) / ms_full.

usage: tools/heat_series_probe.py [FAMILY[,FAMILY] [ncols[,ncols] [repetitions [out.json]]]]
       (default: all three families in child processes, heat at 1000000 and 65536 columns, the coupled family once at
        1000000; profiles/heat_series_probe.json)"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "heat_series_probe.json")
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")
NKNOTS, HOUR, DAY = 48, 3600.0, 86400.0
FAMILIES = ("heat_scalar", "heat_layered", "layered_coupled")


def probe(family, ncols, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    coupled = family == "layered_coupled"
    if coupled:
        import layered_coupled_implicit_timing as T0   # ensemble; loads the package
    else:
        import layered_heat_implicit_timing as T0
    F, W, M = T0.F, T0.W, T0.M
    TOP_E, TOP_H = (M.FACE_TOP, M.COMP_ENERGY), (M.FACE_TOP, M.COMP_HYDROLOGY)
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lay = T0.ensemble(ncols)
    om = lay.case.om
    T = HOUR * np.arange(NKNOTS, dtype=np.float64)
    hours = np.arange(NKNOTS, dtype=np.float64)
    scale = 0.5 + W.uhash(np.arange(ncols), 9, 1)                  # per column: an amplitude of 0.5 .. 1.5
    phase = 2.0 * (W.uhash(np.arange(ncols), 10, 1) - 0.5)         # ... and a phase of +- 1 h
    if coupled:
        peak = -0.6 * float(np.min(np.asarray(lay.classes)[:, 3]))   # of the tightest class's Ksat (negative: into the soil)
        top_T = om.bc[TOP_E][1]
        shapes = {TOP_H: lambda h: peak * (1.0 - np.abs(h % 24.0 - 10.0) / 14.0).clip(0.0),
                  TOP_E: lambda h: top_T + 5.0 * np.sin(2.0 * np.pi * h / 24.0)}
        percol = {TOP_H: lambda h: shapes[TOP_H](h) * scale[None, :],
                  TOP_E: lambda h: top_T + 5.0 * scale[None, :] * np.sin(2.0 * np.pi * h / 24.0)}
        wrapped, entry = "lh_integrate_layered_coupled_trbdf2", "lh_integrate_layered_coupled_series"
        moved = (F.LH_VAR_VARTHETA_L, F.LH_VAR_RHOE_INT)
    else:
        om.bc[TOP_E] = (M.BC_FLUX, 0.0)
        flux = lambda h: np.where(np.sin(2.0 * np.pi * (h - 6.0) / 24.0) > 0, -150.0 * np.sin(2.0 * np.pi * (h - 6.0) / 24.0), 40.0)
        shapes = {TOP_E: flux}
        percol = {TOP_E: lambda h: np.where(flux(h) < 0, flux(h) * scale[None, :], flux(h))}
        wrapped = "lh_integrate_layered_heat_trbdf2" if family == "heat_layered" else "lh_integrate_heat_trbdf2"
        entry = "lh_integrate_heat_series"
        moved = (F.LH_VAR_RHOE_INT,)
    uniform_v = {k: np.ascontiguousarray(f(hours)) for k, f in shapes.items()}
    dt0 = HOUR / 4.0
    gm = W.GpuModel(lay.case)
    if family != "heat_scalar":
        gm.set_soil_classes(lay.classes, lay.class_map, thermal=lay.thermal)
    with gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, _ = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        cols = torch.zeros(ncols, dtype=torch.float64, device="cuda")
        colp = C.c_void_p(cols.data_ptr())
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()

        def series_of(values, times=T):
            h = C.c_void_p()
            tt = np.ascontiguousarray(times)
            F.check(L.lh_bc_series_create(ctx, len(tt), dptr(tt), C.byref(h)), ctx)
            for (f, k), v in values.items():
                v = np.ascontiguousarray(v, dtype=np.float64)
                F.check(L.lh_bc_series_set(ctx, h, f, k, dptr(v), v.shape[1] if v.ndim == 2 else 1, 1 if v.ndim == 2 else 0), ctx)
            return h

        uniform = series_of(uniform_v)
        same = series_of({k: np.repeat(v[:, None], ncols, axis=1) for k, v in uniform_v.items()})
        varied = series_of({k: f((hours[:, None] + phase[None, :]) if not coupled or k == TOP_E else hours[:, None])
                            for k, f in percol.items()})

        def stats():
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            return dict(zip(KEYS, list(st)))

        def call_wrapped(a, b, bcv):
            if coupled:
                return getattr(L, wrapped)(ctx, Y, Ya, a, b, dt0, 0.0, 0.0, 0.0, 0, colp, dptr(bcv))
            return getattr(L, wrapped)(ctx, Y, Ya, a, b, dt0, 0.0, 0.0, 0, colp, dptr(bcv))

        def call_series(h, a, b):
            if coupled:
                return getattr(L, entry)(ctx, Y, Ya, h, a, b, dt0, 0.0, 0.0, 0.0, 0, colp)
            return getattr(L, entry)(ctx, Y, Ya, h, a, b, dt0, 0.0, 0.0, 0, colp)

        base = np.zeros((2, 2, 2))
        for (f, k), (_, v) in om.bc.items():
            base[:, f, k] = v

        def chain():
            total = dict.fromkeys(KEYS, 0)
            for j in range(NKNOTS - 1):
                bcv = base.copy()
                for key, v in uniform_v.items():
                    bcv[0][key], bcv[1][key] = v[j], v[j + 1]
                F.check(call_wrapped(T[j], T[j + 1], bcv), ctx)
                for key, v in stats().items():
                    total[key] += v
            return total

        def one(h, a=T[0], b=T[-1]):
            F.check(call_series(h, a, b), ctx)
            return stats()

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

        runs = [("chain", chain), ("uniform", lambda: one(uniform)), ("percolumn_same", lambda: one(same)),
                ("percolumn", lambda: one(varied))]
        out = dict(family=family, ncols=ncols, nlev=om.nlev, knots=NKNOTS, interval_s=HOUR, stable_dt_s=round(sd.value, 3),
                   dt0_s=dt0, repetitions=reps, runs={})
        end = {}
        for name, fn in runs:                                      # warm-up (first-use allocations), and the end states
            timed(fn)
            end[name] = [gm.download(Y, v) for v in moved] + [cols.cpu().numpy()]
        equal = lambda a, b: bool(all(np.array_equal(x, y) for x, y in zip(end[a], end[b])))
        out["uniform_bitwise_equal_to_chain"] = equal("chain", "uniform")
        out["percolumn_same_bitwise_equal_to_chain"] = equal("chain", "percolumn_same")
        out["status"] = gm.status()
        del end
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
            attempts = s["accepted"] + s["rejected"]
            out["runs"][name] = dict(device_ms=ms[name], wall_ms=wall[name], device_ms_median=float(np.median(ms[name])),
                                     device_ms_range=[min(ms[name]), max(ms[name])], wall_ms_median=float(np.median(wall[name])),
                                     wall_ms_range=[min(wall[name]), max(wall[name])], stats=s,
                                     steps_per_col=round(attempts / ncols, 3),
                                     # the chain's wave_steps is a sum of per-interval maxima, the series' one maximum of totals
                                     divergence=round(s["wave_steps"] / attempts, 3) if attempts else None,
                                     wave_steps_per_wave=round(s["wave_steps"] / (64.0 * waves), 3))
        a = out["runs"]["chain"]
        for name in ("uniform", "percolumn_same", "percolumn"):
            r = out["runs"][name]
            r["chain_over_this_device"] = round(a["device_ms_median"] / r["device_ms_median"], 3)
            r["chain_over_this_wall"] = round(a["wall_ms_median"] / r["wall_ms_median"], 3)
        if not coupled:   # the prologue's share: all knots against every second one, a value that is constant in time
            const = {TOP_E: np.full(NKNOTS, -60.0)}
            full, thin = series_of(const), series_of({TOP_E: const[TOP_E][::2]}, T[::2])
            b = T[NKNOTS - 2]                                    # the last knot both series hold
            pair = {}
            for name, h in (("full", full), ("thin", thin)):
                timed(lambda: one(h, T[0], b))
                got = [timed(lambda: one(h, T[0], b)) for _ in range(reps)]
                pair[name] = dict(device_ms=[round(g[0], 3) for g in got], device_ms_median=float(np.median([g[0] for g in got])),
                                  stats=got[-1][2], sub_intervals=NKNOTS - 2 if name == "full" else (NKNOTS - 2) // 2)
            f_, t_ = pair["full"], pair["thin"]
            scaled = t_["device_ms_median"] * f_["stats"]["wave_steps"] / t_["stats"]["wave_steps"]
            pair["thin_ms_scaled_to_full_wave_steps"] = round(scaled, 3)
            pair["prologue_share_estimate"] = round((f_["device_ms_median"] - scaled) / f_["device_ms_median"], 4)
            pair["ms_per_extra_sub_interval"] = round((f_["device_ms_median"] - scaled) / (f_["sub_intervals"] - t_["sub_intervals"]), 4)
            out["prologue"] = pair
    print(json.dumps(out), flush=True)
    return out


def main():
    a = sys.argv[1:]
    reps = int(a[2]) if len(a) > 2 else 5
    path = a[3] if len(a) > 3 else OUT
    if a and len(a[0].split(",")) == 1 and len(a) > 1 and len(a[1].split(",")) == 1 and os.environ.get("LH_SERIES_PROBE_CHILD"):
        probe(a[0], int(a[1]), reps)
        return
    families = a[0].split(",") if a else list(FAMILIES)
    rows = []
    for fam in families:
        sizes = [int(x) for x in a[1].split(",")] if len(a) > 1 else ([1_000_000] if fam == "layered_coupled" else [1_000_000, 65536])
        for n in sizes:   # one process per configuration; a configuration that fails ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), fam, str(n), str(1 if fam == "layered_coupled" and len(a) < 3 else reps)],
                               check=True, timeout=540, capture_output=True, text=True, env=dict(os.environ, LH_SERIES_PROBE_CHILD="1"))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
            with open(path, "w") as f:   # (kept after every configuration)
                json.dump(dict(probe="tools/heat_series_probe.py", configurations=rows), f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
