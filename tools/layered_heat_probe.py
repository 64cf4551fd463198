#!/usr/bin/env python3
"""What per-cell soil classes with their thermal supplement cost the coupled model beside its scalar launch, in ONE
process and ONE context (the same planes, the same placement): lh_rhs and ms per fused lh_step_ssprk33 step on the
C3 shape (ice-free coupled water and heat, 1e6 x 64, Float64 and Float32), timed with lh_timer_* around `reps`
back-to-back calls after a warm-up, every variant once per round, `rounds` rounds, the median reported with the
spread.  The figure to read is `over_scalar`: each layered launch over the scalar coupled launch of the same run.

variants
  scalar          the context's scalars (rhs_kernel; the step as three fused-stage launches, persist=0)
  layered_1       one class (the scalars' numbers, hydraulic and thermal), the map all zeros
  layered_4       four horizons of 16 levels, four classes
  layered_16      16 classes assigned per cell by uhash (some with organic matter: the per-cell power is taken)

usage: tools/layered_heat_probe.py [ncols] [--inputs-only] [--run=N]      one JSON line per figure on stdout
--run=N puts "run": N in front of every line, so that the lines of several runs (one process each, possibly on
different cards) can be kept in one file: profiles/layered_heat_probe.jsonl is `--run=1` followed by `--run=2`."""
import ctypes as C
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

THERMAL = ("rho_c_ds", "kappa_solid", "rho_p", "kappa_sat_unfrozen", "kappa_sat_frozen", "nu_ss_gravel", "nu_ss_om", "nu_ss_quartz")


def classes16():
    """16 textures around C3's soil, every one valid for its state (theta_r < 0.15, nu > 0.44), and their thermal
    supplements; class 0 is C3's own soil.  Every third class is organic."""
    sp, vg = W.coupled_soil()
    k = np.arange(16)
    f = lambda a: (k * a) % 1.0
    cls = np.stack([1.5 + 1.3 * f(0.37), 1.5 + 3.0 * f(0.61), 0.06 * f(0.23), 10.0 ** (-7.5 + 2.0 * f(0.41)), 0.45 + 0.1 * f(0.29),
                    5e-4 + 1.5e-3 * f(0.17)], axis=1)
    om = np.where(k % 3 == 1, 0.1 + 0.3 * f(0.53), 0.0)
    th = np.stack([0.7e6 + 0.6e6 * f(0.618), 3.0 + 4.5 * f(0.37), 1500.0 + 1200.0 * f(0.29), 1.2 + 1.2 * f(0.43),
                   3.0 + 1.4 * f(0.71), 0.05 * f(0.47) * (1 - om), om, (0.2 + 0.7 * f(0.31)) * (1 - om)], axis=1)
    cls[0] = (vg.n, vg.alpha, vg.theta_r, vg.Ksat, sp.nu, sp.S_s)
    th[0] = [getattr(sp, n) for n in THERMAL]
    return cls, th


def maps(ncols, nlev):
    cls, th = classes16()
    lev = np.arange(nlev)
    four = np.repeat((lev * 4 // nlev).astype(np.uint8)[None, :], ncols, axis=0)
    hashed = np.empty((ncols, nlev), dtype=np.uint8)
    c = np.arange(ncols)
    for i in range(nlev):
        hashed[:, i] = (W.uhash(c, i, nlev, seed=W.SEED ^ 0x5EED) * 16).astype(np.uint8)
    pick = [0, 5, 9, 14]
    return dict(layered_1=(cls[:1], th[:1], np.zeros((ncols, nlev), dtype=np.uint8)), layered_4=(cls[pick], th[pick], four),
                layered_16=(cls, th, hashed))


def timed(gm, fn, reps):
    L, ctx = gm.L, gm.ctx
    fn()
    F.check(L.lh_synchronize(ctx), ctx)
    F.check(L.lh_timer_start(ctx), ctx)
    for _ in range(reps):
        fn()
    ms = C.c_float()
    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
    return ms.value / reps


def probe(dtype, ncols, rounds=5, reps=20, steps=4):
    case = W.make_case("c3_coupled_f64" if dtype == np.float64 else "c3_coupled_f32", ncols=ncols)
    nlev = case.om.nlev
    layered = maps(ncols, nlev)
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, dY = gm.state(0), gm.state(0)
        sd = C.c_double()
        dt = 0.0                # 0.2 x the stable step of the variant being timed (its classes set its bound)

        def configure(variant):
            gm.set_soil_class_map(None)
            gm.set_soil_classes(None)
            if variant in layered:
                cls, th, m = layered[variant]
                gm.set_soil_classes(cls, m, thermal=th)

        def rhs():
            F.check(L.lh_rhs(ctx, 0.0, Y0, Ya, dY), ctx)

        def step():
            F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, dt, steps, None), ctx)

        variants = ["scalar", "layered_1", "layered_4", "layered_16"]
        t = {(v, w): [] for v in variants for w in ("rhs", "step_fused")}
        F.check(L.lh_set_tuning(ctx, b"persist=0,graph=0"), ctx)     # the scalar step too as three fused-stage launches
        for _ in range(rounds):
            for v in variants:
                configure(v)
                F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
                dt = 0.2 * sd.value
                t[(v, "rhs")].append(timed(gm, rhs, reps))
                F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                t[(v, "step_fused")].append(timed(gm, step, 3) / steps)
        assert gm.status() == 0
        configure("scalar")
    med = statistics.median
    dn = np.dtype(dtype).name
    rows = []
    for (v, w), xs in t.items():
        rows.append(dict(figure=w, variant=v, dtype=dn, ncols=ncols, nlev=nlev, ms=round(med(xs), 4),
                         spread=[round(min(xs), 4), round(max(xs), 4)], over_scalar=round(med(xs) / med(t[("scalar", w)]), 3)))
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ncols = int(args[0]) if args else 1_000_000
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        for dtype in (np.float64, np.float32):
            case = W.make_case("c3_coupled_f64" if dtype == np.float64 else "c3_coupled_f32", ncols=ncols)
            for v, (cls, th, m) in maps(ncols, case.om.nlev).items():
                assert m.shape == case.vl.shape and m.max() < len(cls) == len(th)
                assert np.all(cls[:, 2] < case.vl.min()) and np.all(cls[:, 4] > case.vl.max()), v
        print("inputs ok")
        return
    run = [int(a[6:]) for a in sys.argv[1:] if a.startswith("--run=")]
    for dtype in (np.float64, np.float32):
        for r in probe(dtype, ncols):
            print(json.dumps(dict(run=run[0], **r) if run else r), flush=True)


if __name__ == "__main__":
    main()
