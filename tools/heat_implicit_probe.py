#!/usr/bin/env python3
"""Cost of an implicit step of the heat-only model (lh_step_heat_implicit, backward Euler and fixed-step
TR-BDF2) against the fixed-dt SSPRK33 stepper on the same ensemble, in one process: ms per step, the
effective bandwidth and the break-even dt ratio.  Writes profiles/heat_implicit_probe.jsonl.

Ensembles: the heat_dirichlet recipe of workloads.make_case on 64 levels, 1e6 columns, Float64 and Float32
(4096 distinct columns, tiled), and the 60-level analytic column of the reference's heat_test_interface.jl
replicated over 65 536 columns.

Plane passes per cell and step, each sizeof(FT) bytes: backward Euler 8 (forward sweep:
read rhoe, kc, the multiplier, write r'; back substitution: read r' and two factor planes, write rhoe), TR-BDF2 20.  The factorisation
(the prologue: 2 reads, 4 or 7 writes and every closure) is paid once per call and is inside the timings:
steps_per_call sets how far it is amortised.
break-even = ms(implicit step) / ms(SSPRK33 step): the implicit step pays once its dt exceeds that many
explicit steps.
usage: tools/heat_implicit_probe.py [ncols_ensemble] [ncols_analytic] [steps_per_call]"""
import ctypes as C
import dataclasses
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
PASSES = {"euler": 8, "trbdf2": 20}


def ensemble(ncols, dtype, nlev=64, distinct=4096):
    """make_case("heat_dirichlet_*") on nlev levels: `distinct` hashed columns, tiled to ncols."""
    base = W.make_case("heat_dirichlet_f64", ncols=min(distinct, ncols))
    sp, e = base.om.soil, base.om.earth
    om = dataclasses.replace(base.om, nlev=nlev, zmax=nlev / 60.0)
    N = base.ncols
    c = np.arange(N)
    lev = np.arange(nlev)
    vl = 0.1 + 0.35 * W.uhash(c[:, None], lev[None, :] + 7, 1000)
    ti = np.where(W.uhash(c, 8, nlev)[:, None] < 0.3, 0.05 * W.uhash(c[:, None], lev[None, :] + 99, 1000), 0.0)
    zc, _ = W.grid_np(0.0, om.zmax, nlev)
    T = 285.0 + 3.0 * np.sin(6.0 * zc)[None, :] + W.uhash(c, 9, nlev)[:, None]
    tl = np.minimum(vl, sp.nu - ti)
    rho_c_s = sp.rho_c_ds + tl * (e.cp_l * e.rho_liq) + ti * (e.cp_i * e.rho_ice)
    rhoe = rho_c_s * (T - e.T_0) - ti * e.rho_ice * e.LH_f0
    reps = -(-ncols // N)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:ncols].astype(dtype))
    return W.Case(f"heat_{nlev}lev_{np.dtype(dtype).name}", om, dtype, ncols, vl=tile(vl), ti=tile(ti), rhoe=tile(rhoe))


def analytic(ncols):
    """test/SoilModel/heat_test_interface.jl: 60 levels on (0, 1), unit diffusivity, T = 0."""
    sp = M.default_soil(nu=0.495, nu_ss_gravel=0.1, nu_ss_om=0.1, nu_ss_quartz=0.1, rho_c_ds=0.43314518988433487,
                        kappa_solid=8.0, kappa_sat_unfrozen=0.57, kappa_sat_frozen=2.29)
    n = 60
    bc = {(M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 0.0), (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_DIRICHLET, 5.0)}
    om = M.CaseModel(M.MODEL_HEAT, n, 0.0, 1.0, soil=sp, bc=bc)
    rhoe = np.full((ncols, n), sp.rho_c_ds * (0.0 - om.earth.T_0))
    return W.Case("heat_analytic_60lev_float64", om, np.float64, ncols, vl=np.zeros((ncols, n)), ti=np.zeros((ncols, n)),
                  rhoe=rhoe)


def timed(gm, fn, reps):
    L, ctx = gm.L, gm.ctx
    fn()  # warm-up (and first-use allocations)
    F.check(L.lh_synchronize(ctx), ctx)
    F.check(L.lh_timer_start(ctx), ctx)
    for _ in range(reps):
        fn()
    ms = C.c_float()
    F.check(L.lh_timer_stop(ctx, C.byref(ms)), ctx)
    return ms.value / reps


def probe(case, mult, steps_per_call, reps=3):
    out = []
    with W.GpuModel(case) as gm:
        L, ctx = gm.L, gm.ctx
        Y, Ya = gm.prognostic_and_aux()
        sd = C.c_double()
        F.check(L.lh_stable_dt(ctx, Y, Ya, 0.5, C.byref(sd)), ctx)
        sd = sd.value
        cells = case.ncols * case.om.nlev
        esize = np.dtype(case.dtype).itemsize
        ms_ex = timed(gm, lambda: F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, sd, steps_per_call, None), ctx),
                      reps) / steps_per_call
        out.append(dict(case=case.name, ncols=case.ncols, method="ssprk33", dt_over_stable=1.0, steps_per_call=steps_per_call,
                        ms_per_step=round(ms_ex, 4)))
        for method, flags in (("euler", 0), ("trbdf2", F.LH_HEAT_TRBDF2)):
            Yi, _ = gm.prognostic_and_aux()
            call = lambda: F.check(L.lh_step_heat_implicit(ctx, Yi, Ya, 0.0, mult * sd, steps_per_call, flags, None), ctx)
            ms = timed(gm, call, reps) / steps_per_call
            nbytes = PASSES[method] * esize
            out.append(dict(case=case.name, ncols=case.ncols, method="heat_" + method, dt_over_stable=mult,
                            steps_per_call=steps_per_call, ms_per_step=round(ms, 4), bytes_per_cell_step=nbytes,
                            GBps=round(nbytes * cells / (ms * 1e-3) / 1e9, 1), break_even_dt_ratio=round(ms / ms_ex, 2)))
        st = C.c_uint32()
        F.check(L.lh_get_status(ctx, C.byref(st)), ctx)
        assert st.value == 0, st.value
    return out


def main():
    n_en = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_an = int(sys.argv[2]) if len(sys.argv) > 2 else 65_536
    spc = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    rows = []
    for case in (ensemble(n_en, np.float64), ensemble(n_en, np.float32), analytic(n_an)):
        rows += probe(case, 30.0, spc)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "heat_implicit_probe.jsonl"), "w") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
