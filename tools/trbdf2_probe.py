#!/usr/bin/env python3
"""Cost and accuracy of the adaptive TR-BDF2 integrator (lh_integrate_trbdf2) against backward Euler
(lh_step_implicit_euler) and the fixed-dt SSPRK33 stepper, in one process, for C2 (Richards, Float64,
1e6 x 64 columns, over 20 stable steps) and the reference's Bonan infiltration case (150 levels, replicated
over an ensemble, over 1200 s).

Per method: ms per simulated second (one timed call after a warm-up call that makes the first-use
allocations), and the mean and the largest absolute error against SSPRK33 at a quarter of the stable step
(C2) or at 0.25 s (Bonan, the reference test's own step).  TR-BDF2 also reports its accepted and rejected
steps per column, Newton iterations per column, failed columns, and the lane-divergence factor
wave_steps / (64 x waves x mean steps per column): the work of waves that run until their slowest lane is
done, over the work the columns need (1 = no divergence).  Then the LH_TUNE variants of TR-BDF2 at
reltol 1e-4 (error-solve matrix, Newton test and cap) on C2 and Bonan, and on C5 (per-column parameters:
columns whose step sequences differ) for the divergence.
usage: tools/trbdf2_probe.py [ncols_c2] [ncols_bonan] [out.jsonl (default profiles/trbdf2_probe.jsonl)]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before any HIP library is loaded)
import __graft_entry__ as g

pkg = g.load_package()
F, W, M = pkg._ffi, pkg.workloads, pkg.case_model
KEYS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")


def bonan(ncols):
    sp = M.default_soil(nu=0.287, S_s=1e-3)
    vg = M.default_vg(n=3.96, alpha=2.7, Ksat=34 / 3600 / 100, theta_r=0.075)
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.267),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    om = M.CaseModel(M.MODEL_RICHARDS, 150, -1.5, 0.0, soil=sp, vg=vg, bc=bc)
    return W.Case("bonan", om, np.float64, ncols, vl=np.full((ncols, 150), 0.1), ti=np.zeros((ncols, 150)))


def timed_ms(gm, fn):
    L, ctx = gm.L, gm.ctx
    F.check(L.lh_synchronize(ctx), ctx)
    F.check(L.lh_timer_start(ctx), ctx)
    fn()
    ms = C.c_float()
    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
    return ms.value


def probe(case, T, dt_ie, dt_fine, rtols):
    out = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
        sd = sd.value
        nf = int(round(T / dt_fine))
        F.check(L.lh_step_ssprk33(ctx, Y0, Ya, 0.0, T / nf, nf, None), ctx)
        ref = gm.download(Y0, F.LH_VAR_VARTHETA_L)
        base = dict(case=case.name, ncols=case.ncols, nlev=case.om.nlev, T_s=T, stable_dt_s=round(sd, 6))

        def run(method, call, extra):
            Yw, _ = gm.prognostic_and_aux()
            call(Yw)                                  # warm-up (first-use allocations)
            Y, _ = gm.prognostic_and_aux()
            ms = timed_ms(gm, lambda: call(Y))
            v = gm.download(Y, F.LH_VAR_VARTHETA_L)
            err = np.abs(v - ref)
            r = dict(base, method=method, ms=round(ms, 3), ms_per_sim_s=round(ms / T, 5),
                     mean_abs_err=float(f"{err.mean():.3e}"), max_abs_err=float(f"{err.max():.3e}"), **extra)
            out.append(r)
            print(json.dumps(r), flush=True)
            return r

        ns = int(np.ceil(T / sd))
        run("ssprk33", lambda Y: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, T / ns, ns, None), ctx),
            dict(dt_s=round(T / ns, 6), steps=ns))
        ni = int(round(T / dt_ie))
        r = run("implicit_euler",
                lambda Y: F.check(L.lh_step_implicit_euler(ctx, Y, Ya, 0.0, T / ni, ni, None, 0.0, 0), ctx),
                dict(dt_s=round(T / ni, 6), steps=ni))
        mi, un = C.c_int32(), C.c_int64()
        F.check(L.lh_implicit_stats(ctx, C.byref(mi), C.byref(un)), ctx)
        r["unconverged"] = un.value
        waves = -(-case.ncols // 64)
        for rtol in rtols:
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()

            def call(Y, rtol=rtol):
                F.check(L.lh_integrate_trbdf2(ctx, Y, Ya, 0.0, T, sd, 1e-6, rtol, 0, None, None), ctx)

            r = run("trbdf2", call, dict(reltol=rtol, abstol=1e-6, dt0_s=round(sd, 6)))
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            s = dict(zip(KEYS, list(st)))
            mean_steps = (s["accepted"] + s["rejected"]) / case.ncols
            r.update(accepted_per_col=round(s["accepted"] / case.ncols, 2),
                     rejected_per_col=round(s["rejected"] / case.ncols, 2),
                     newton_per_col=round(s["newton_iterations"] / case.ncols, 1), max_steps=s["max_steps"],
                     failed=s["failed"], divergence=round(s["wave_steps"] / (64 * waves * mean_steps), 3))
            print(json.dumps(dict(case=case.name, reltol=rtol, stats=s)), flush=True)
    return out


def variants(case, T, dt_fine, tunes, rtol=1e-4):
    """TR-BDF2 at reltol rtol under each LH_TUNE string (trk= Newton test in 1e-4,
    trn= Newton cap; read when the context is created): ms per simulated second, steps, error."""
    out = []
    saved = os.environ.get("LH_TUNE")
    ref = None
    for tune in tunes:
        os.environ["LH_TUNE"] = tune
        with W.GpuModel(case) as gm:
            L, ctx = gm.L, gm.ctx
            Y0, Ya = gm.prognostic_and_aux()
            sd = C.c_double()
            F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
            sd = sd.value
            if ref is None:
                nf = int(round(T / dt_fine))
                F.check(L.lh_step_ssprk33(ctx, Y0, Ya, 0.0, T / nf, nf, None), ctx)
                ref = gm.download(Y0, F.LH_VAR_VARTHETA_L)
            call = lambda Y: F.check(L.lh_integrate_trbdf2(ctx, Y, Ya, 0.0, T, sd, 1e-6, rtol, 0, None, None), ctx)
            Yw, _ = gm.prognostic_and_aux()
            call(Yw)
            Y, _ = gm.prognostic_and_aux()
            ms = timed_ms(gm, lambda: call(Y))
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(L.lh_trbdf2_stats(ctx, st), ctx)
            s = dict(zip(KEYS, list(st)))
            err = np.abs(gm.download(Y, F.LH_VAR_VARTHETA_L) - ref)
            mean_steps = (s["accepted"] + s["rejected"]) / case.ncols
            r = dict(case=case.name, ncols=case.ncols, T_s=T, method="trbdf2", reltol=rtol, tune=tune, ms=round(ms, 3),
                     ms_per_sim_s=round(ms / T, 5), mean_abs_err=float(f"{err.mean():.3e}"),
                     max_abs_err=float(f"{err.max():.3e}"), accepted_per_col=round(s["accepted"] / case.ncols, 2),
                     rejected_per_col=round(s["rejected"] / case.ncols, 2),
                     newton_per_col=round(s["newton_iterations"] / case.ncols, 1), max_steps=s["max_steps"],
                     failed=s["failed"],
                     divergence=round(s["wave_steps"] / (64 * (-(-case.ncols // 64)) * mean_steps), 3))
            out.append(r)
            print(json.dumps(r), flush=True)
    if saved is None:
        os.environ.pop("LH_TUNE", None)
    else:
        os.environ["LH_TUNE"] = saved
    return out


def main():
    n_c2 = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_bo = int(sys.argv[2]) if len(sys.argv) > 2 else 65_536
    c2 = W.make_case("c2_richards_f64", ncols=n_c2)
    sub = W.make_case("c2_richards_f64", ncols=min(n_c2, 2000))
    with W.GpuModel(sub) as gm:
        Y, Ya = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(gm.L.lh_stable_dt(gm.ctx, Y, Ya, 0.5, C.byref(sd)), gm.ctx)
        sd = sd.value
    rows = probe(c2, 20 * sd, 10 * sd, sd / 4, (1e-3, 1e-4, 1e-5))
    rows += probe(bonan(n_bo), 1200.0, 0.5, 0.25, (1e-3, 1e-4, 1e-5))
    # the stage Newton's test and cap (defaults: trk=100, trn=10), and the lane divergence of an ensemble
    # whose columns differ (per-column van Genuchten parameters)
    tunes = ("", "trk=30", "trk=300", "trn=6", "trn=20")
    rows += variants(c2, 20 * sd, sd / 4, tunes)
    rows += variants(bonan(n_bo), 1200.0, 0.25, tunes)
    c5 = W.make_case("c5_percol_f64", ncols=n_c2)
    with W.GpuModel(W.make_case("c5_percol_f64", ncols=2000)) as gm:
        Y, Ya = gm.prognostic_and_aux()
        sd5 = C.c_double()
        F.check(gm.L.lh_stable_dt(gm.ctx, Y, Ya, 0.5, C.byref(sd5)), gm.ctx)
        sd5 = sd5.value
    rows += variants(c5, 20 * sd5, sd5 / 4, ("",))
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "trbdf2_probe.jsonl")
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
