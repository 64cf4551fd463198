#!/usr/bin/env python3
"""What per-cell soil classes cost beside the scalar and the per-column launches, in ONE process and ONE
context (the same planes, the same placement): lh_rhs and ms per lh_step_ssprk33 step on the C2 shape (ice-free
Richards, 1e6 x 64, Float64 and Float32), timed with lh_timer_* around `reps` back-to-back calls after a
warm-up, every variant once per round, `rounds` rounds, the median reported with the spread.

variants
  scalar          the context's six scalars (rhs_kernel; the step also with the default engine, the column stepper)
  percol          six per-column arrays holding those scalars (rhs_kernel PERCOL)
  layered_1       one class (the scalars), the map all zeros
  layered_4       four horizons of 16 levels, four classes
  layered_16      16 classes assigned per cell by uhash
and lh_stream_probe on the same planes: the tendency's traffic without arithmetic (read vartheta_l, write
d vartheta_l), to which the layered launch adds one byte per cell.

Also the two accuracy figures of tests/test_gpu_layered.py::test_layered_matches_the_numpy_reference (the worst
cell of the 130 x 64 layered case against the NumPy reference and of its column-uniform twin against the
oracle), so that they are on record next to the timings.

usage: tools/layered_probe.py [ncols] [--inputs-only]      one JSON line per figure on stdout"""
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

LOAM = (1.56, 3.6, 0.0, 2.9e-7, 0.43, 1e-3)   # the defaults C2 runs with: (n, alpha, theta_r, Ksat, nu, S_s)


def classes16():
    """16 textures around the loam, every one valid for C2's state (theta_r < 0.15, nu > 0.37): class 0 is the loam"""
    k = np.arange(16)
    cls = np.stack([1.3 + 1.5 * ((k * 0.37) % 1.0), 1.5 + 4.0 * ((k * 0.61) % 1.0), 0.06 * ((k * 0.23) % 1.0),
                    10.0 ** (-7.5 + 3.0 * ((k * 0.41) % 1.0)), 0.40 + 0.1 * ((k * 0.29) % 1.0),
                    5e-4 + 1.5e-3 * ((k * 0.17) % 1.0)], axis=1)
    cls[0] = LOAM
    return cls


def maps(ncols, nlev):
    lev = np.arange(nlev)
    four = np.repeat((lev * 4 // nlev).astype(np.uint8)[None, :], ncols, axis=0)
    hashed = np.empty((ncols, nlev), dtype=np.uint8)
    c = np.arange(ncols)
    for i in range(nlev):
        hashed[:, i] = (W.uhash(c, i, nlev, seed=W.SEED ^ 0x5EED) * 16).astype(np.uint8)
    return dict(layered_1=(classes16()[:1], np.zeros((ncols, nlev), dtype=np.uint8)),
                layered_4=(classes16()[[0, 5, 9, 14]], four), layered_16=(classes16(), hashed))


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
    name = "c2_richards_f64" if dtype == np.float64 else "c2_richards_f32"
    case = W.make_case(name, ncols=ncols)
    nlev = case.om.nlev
    layered = maps(ncols, nlev)
    rows = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y0, Ya = gm.prognostic_and_aux()
        Y, dY = gm.state(0), gm.state(0)
        sd = C.c_double()
        dt = 0.0                # 0.2 x the stable step of the variant being timed (its classes set its bound)
        ones = np.ones(ncols)

        def configure(variant):
            gm.set_soil_classes(None)
            for key, v in zip(("vg_n", "vg_alpha", "vg_theta_r", "vg_Ksat", "nu", "S_s"), LOAM):
                a = np.ascontiguousarray(ones * v) if variant == "percol" else None
                F.check(L.lh_set_percol_param(ctx, F.LH_PC[key], None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))), ctx)
            if variant in layered:
                gm.set_soil_classes(*layered[variant])

        def rhs():
            F.check(L.lh_rhs(ctx, 0.0, Y0, Ya, dY), ctx)

        def step():
            F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, dt, steps, None), ctx)

        variants = ["scalar", "percol", "layered_1", "layered_4", "layered_16"]
        t = {(v, w): [] for v in variants for w in ("rhs", "step_fused", "step_default")}
        stream = []
        for _ in range(rounds):
            ms = C.c_float()
            F.check(L.lh_stream_probe(ctx, Y0, 0b01, dY, 0b01, reps, C.byref(ms)), ctx)
            stream.append(ms.value)
            for v in variants:
                configure(v)
                F.check(L.lh_stable_dt(ctx, Y0, Ya, 0.5, C.byref(sd)), ctx)
                dt = 0.2 * sd.value
                t[(v, "rhs")].append(timed(gm, rhs, reps))
                F.check(L.lh_set_tuning(ctx, b"persist=0"), ctx)     # three fused-stage launches per step
                F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                t[(v, "step_fused")].append(timed(gm, step, 3) / steps)
                F.check(L.lh_set_tuning(ctx, b""), ctx)
                if v in ("scalar", "percol"):                        # the default engine: the persistent column stepper
                    F.check(L.lh_state_copy(ctx, Y, Y0), ctx)
                    t[(v, "step_default")].append(timed(gm, step, 3) / steps)
        assert gm.status() == 0
        configure("scalar")
    med = lambda xs: statistics.median(xs)
    base = {w: med(t[("scalar", w)]) for w in ("rhs", "step_fused")}
    pcol = {w: med(t[("percol", w)]) for w in ("rhs", "step_fused")}
    dn = np.dtype(dtype).name
    rows.append(dict(figure="stream_probe", dtype=dn, ncols=ncols, nlev=nlev, ms=round(med(stream), 4),
                     spread=[round(min(stream), 4), round(max(stream), 4)]))
    for (v, w), xs in t.items():
        if not xs:
            continue
        r = dict(figure=w, variant=v, dtype=dn, ncols=ncols, nlev=nlev, ms=round(med(xs), 4),
                 spread=[round(min(xs), 4), round(max(xs), 4)])
        if w in base:
            r["over_scalar"] = round(med(xs) / base[w], 3)
            r["over_percol"] = round(med(xs) / pcol[w], 3)
        if w == "rhs":
            r["over_stream_probe"] = round(med(xs) / med(stream), 3)
        rows.append(r)
    return rows


def accuracy():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import test_gpu_layered as T
    rows = []
    for dtype in (np.float64, np.float32):
        worst, twin, share = T.layered_figures(dtype)
        rows.append(dict(figure="layered_worst_cell", dtype=np.dtype(dtype).name, shape=[130, 64], classes=16,
                         layered_vs_numpy_reference=worst, uniform_twin_vs_oracle=twin, share_within_plain_rel=share))
    return rows


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ncols = int(args[0]) if args else 1_000_000
    if "--inputs-only" in sys.argv:     # a rehearsal without a device: the inputs build, nothing is launched
        for dtype in (np.float64, np.float32):
            case = W.make_case("c2_richards_f64" if dtype == np.float64 else "c2_richards_f32", ncols=ncols)
            for v, (cls, m) in maps(ncols, case.om.nlev).items():
                assert m.shape == case.vl.shape and m.max() < len(cls)
                assert np.all(cls[:, 2] < case.vl.min()) and np.all(cls[:, 4] > case.vl.max()), v
        print("inputs ok")
        return
    for dtype in (np.float64, np.float32):
        for r in probe(dtype, ncols):
            print(json.dumps(r), flush=True)
    for r in accuracy():
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
