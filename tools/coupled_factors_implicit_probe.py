#!/usr/bin/env python3
"""What the impedance factor costs an implicit step of the coupled model (lh_step_coupled_factors_implicit; DESIGN
section 4.33): ms per step of the new call against lh_step_coupled_implicit on the same state with the factor off, in
one process, medians of 5 timed calls after a warm-up, with the mean Newton iterations per water stage beside them and
the ratio per Newton iteration.

One measurement per process: a dtype, a method ("euler" / "trbdf2") and a step in units of the stable step of the
context without the factor (both calls take the same dt), so that a driver can give every GPU step its own time limit.
The ensemble: the coupled soil, ncols x 64 levels of 2 cm, the C2 wetting front under a Dirichlet top over free drainage,
ice in every other column (hashed, at most 0.04), T = 284 + 5 z / 1.28 + 2 (u - 1/2), a Dirichlet T at the top and a
flux at the bottom -- the fields of tests/coupled_implicit_ref.py::coupled_case.

usage: tools/coupled_factors_implicit_probe.py f64|f32 euler|trbdf2 MULT [ncols]      (ncols defaults to 1000000)
A row of JSON per call and one with the ratios; profiles/coupled_factors_implicit_timing.txt is the output of the
eight runs."""
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
NLEV, DZ = 64, 0.02


def case_of(dtype, ncols, impedance):
    sp, vg = W.coupled_soil()
    zmin = -DZ * NLEV
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.34), (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0),
          (M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 276.0), (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_FLUX, 0.05)}
    om = M.CaseModel(M.MODEL_COUPLED, NLEV, zmin, 0.0, soil=sp, vg=vg, bc=bc, cf=M.default_cf(impedance=impedance))
    c, lev = np.arange(ncols), np.arange(NLEV)
    vl = W.wetting_front(ncols, NLEV, zmin, 0.0, 0.35).astype(dtype)
    ti = np.where((c % 2 == 0)[:, None], 0.04 * W.uhash(c[:, None], lev[None, :] + 5, 1000), 0.0).astype(dtype)
    zc, _ = W.grid_np(zmin, 0.0, NLEV)
    T = 284.0 + 5.0 * zc[None, :] / 1.28 + 2.0 * (W.uhash(c, 1, NLEV)[:, None] - 0.5)
    e = om.earth
    v64, t64 = vl.astype(np.float64), ti.astype(np.float64)
    rho_c_s = sp.rho_c_ds + np.minimum(v64, sp.nu - t64) * (e.cp_l * e.rho_liq) + t64 * (e.cp_i * e.rho_ice)
    rhoe = rho_c_s * (T - e.T_0) - t64 * e.rho_ice * e.LH_f0
    return W.Case("coupled_factors_probe", om, dtype, ncols, vl=vl, ti=ti, rhoe=rhoe.astype(dtype))


def measure(dtype, method, mult, ncols, steps=2):
    flags, stages = (F.LH_COUPLED_TRBDF2, 2) if method == "trbdf2" else (0, 1)
    rows, sd = [], None
    for impedance, entry in ((False, "lh_step_coupled_implicit"), (True, "lh_step_coupled_factors_implicit")):
        case = case_of(dtype, ncols, impedance)
        with W.GpuModel(case) as gm:
            L, ctx = gm.L, gm.ctx
            Y, Ya = gm.prognostic_and_aux()
            if sd is None:   # the stable step of the context WITHOUT the factor: both calls take the same dt
                v = C.c_double()
                F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(v)), ctx)
                sd = v.value

            def call():
                gm.upload(Y, F.LH_VAR_VARTHETA_L, case.vl)   # every timed call starts from the same state
                gm.upload(Y, F.LH_VAR_RHOE_INT, case.rhoe)
                F.check(L.lh_synchronize(ctx), ctx)
                F.check(L.lh_timer_start(ctx), ctx)
                F.check(getattr(L, entry)(ctx, Y, Ya, 0.0, mult * sd, steps, flags, None, 0.0, 0), ctx)
                ms = C.c_float()
                F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
                return ms.value
            call()
            ms = statistics.median(call() for _ in range(5)) / steps
            mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
            F.check(L.lh_implicit_stats(ctx, C.byref(mi), C.byref(un)), ctx)
            F.check(L.lh_implicit_iterations(ctx, C.byref(tot)), ctx)
            mean_it = tot.value / (ncols * steps * stages)
            rows.append(dict(dtype=np.dtype(dtype).name, method=method, ncols=ncols, nlev=NLEV, entry=entry, dt_over_stable=mult,
                             ms_per_step=round(ms, 4), mean_newton_iters_per_stage=round(mean_it, 2), max_newton_iters=mi.value,
                             unconverged=un.value, status=gm.status(), ms_per_step_and_mean_iteration=round(ms / mean_it, 4)))
    rows.append(dict(dtype=np.dtype(dtype).name, method=method, dt_over_stable=mult,
                     factors_over_plain_per_step=round(rows[1]["ms_per_step"] / rows[0]["ms_per_step"], 3),
                     factors_over_plain_per_iteration=round(rows[1]["ms_per_step_and_mean_iteration"]
                                                            / rows[0]["ms_per_step_and_mean_iteration"], 3)))
    return rows


def main():
    if len(sys.argv) < 4 or sys.argv[1] not in ("f64", "f32") or sys.argv[2] not in ("euler", "trbdf2"):
        sys.exit(__doc__)
    dtype = np.float64 if sys.argv[1] == "f64" else np.float32
    ncols = int(sys.argv[4]) if len(sys.argv) > 4 else 1_000_000
    for r in measure(dtype, sys.argv[2], float(sys.argv[3]), ncols):
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
