#!/usr/bin/env python3
"""Bitwise transcript of the NumPy references of the implicit integrators (tests/*_ref.py), for refactors of those
references: run it on the parent commit and on the branch in ONE environment and compare the two files.

  tools/reference_transcript.py OUT.json              call the public functions of the ten reference modules on a
                                                      fixed list of small ensembles and write the transcript
  tools/reference_transcript.py --compare A.json B.json   entry count and "equal", or the first entries that differ;
                                                      exit status 1 if any

One JSON entry per returned array: function, case, argument variant, field, dtype, shape, SHA-256 of the bytes, and
the values themselves where the array holds integers or booleans (the counters and flags of the `info` dicts).
The digests go through the platform's libm (E ** (-1/3), the closures' powers): a transcript is compared with
another one taken in the same environment, it is not a golden file.

A transcript proves nothing about a branch never taken, so the run asserts from the `info` dicts that the list
produced, at least once: a rejected step, a water stage that did not converge, a column that failed at hmin and one
stopped at max_steps, a clipped final step that could have grown (fac >= 1), and a round in which some columns had
finished while others were still stepping.  CPU side; needs the oracle library (`make -C oracle`)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = [(x, y) for x, y in zip(A, B) if x != y]
    if len(A) != len(B) or bad:
        print("%d entries against %d, %d differ" % (len(A), len(B), len(bad)))
        for x, y in bad[:10]:
            print("  ", x["function"], x["case"], x["variant"], x["field"], "|", y["function"], y["case"], y["variant"], y["field"])
        return 1
    print("%d entries, equal" % len(A))
    return 0


ENTRIES = []
SEEN = dict(rejected=0, unconverged=0, failed_hmin=0, stopped_max_steps=0, clipped_grow=0, staggered=0)


def _leaves(x, path=""):
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _leaves(x[k], path + "." + str(k))
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from _leaves(v, path + "[%d]" % i)
    else:
        yield path, x


def record(function, case, variant, result):
    if os.environ.get("TRANSCRIPT_PROGRESS"):
        print(function, case, variant, file=sys.stderr, flush=True)
    for field, v in _leaves(result):
        a = np.ascontiguousarray(v)
        if a.dtype == object:
            continue
        e = dict(function=function, case=case, variant=variant, field=field, dtype=a.dtype.name, shape=list(a.shape),
                 sha256=hashlib.sha256(a.tobytes()).hexdigest())
        if a.dtype.kind in "iub":
            e["values"] = a.astype(np.int64).ravel().tolist()
        ENTRIES.append(e)
    return result


def witness(info, t0, t1, h0=None, max_steps=None, adaptive=True):
    """what an integration's info dict shows of the loop's branches"""
    t, h, acc, rej, failed = (np.asarray(info[k]) for k in ("t", "h", "accepted", "rejected", "failed"))
    SEEN["rejected"] += int(rej.sum() > 0)
    SEEN["failed_hmin"] += int(np.any(failed & (h < 1e-10 * (t1 - t0))))
    if max_steps is not None:
        SEEN["stopped_max_steps"] += int(np.any((t < t1) & (acc + rej >= max_steps)))
    # a column that landed on t1 with a proposal larger than the span: its last step was clipped (hh <= span) and
    # the proposal is max(hh fac, h) with fac >= 1 (hh fac < hh otherwise)
    if adaptive:
        SEEN["clipped_grow"] += int(np.any((t == t1) & ~failed & (h > t1 - t0)))
    steps = acc + rej
    SEEN["staggered"] += int(not failed.any() and np.all(t == t1) and steps.min() < steps.max())


def bc_table(om, n, drift, M):
    """[n][2 faces][2 components]: the model's scalar boundary values, the Dirichlet ones drifting by `drift` over the table"""
    b = np.zeros((n, 2, 2))
    for (f, k), (kind, v) in om.bc.items():
        b[:, f, k] = v * (1.0 + (drift if kind == M.BC_DIRICHLET else 0.0) * np.arange(n) / max(n - 1, 1))
    return b


def main(out):
    import case_model as M
    import coupled_implicit_ref as CR
    import coupled_trbdf2_ref as CT
    import heat_implicit_ref as H
    import heat_trbdf2_ref as HT
    import implicit_ref as IR
    import layered_coupled_implicit_ref as LC
    import layered_coupled_trbdf2_ref as LT
    import layered_heat_implicit_ref as LHI
    import layered_heat_trbdf2_ref as LHT
    import layered_implicit_ref as LI
    import layered_ref as R
    import trbdf2_ref as TR

    O = IR.O
    rng = np.random.default_rng(7)
    DIR, FLUX, DRAIN = M.BC_DIRICHLET, M.BC_FLUX, M.BC_FREE_DRAINAGE

    # ------------------------------------------------------------------ thomas, step_factor, _sample
    lo, up = rng.uniform(-1, 1, (2, 5, 9))
    di, rhs = 2.5 + rng.uniform(0, 1, (5, 9)), rng.uniform(-1, 1, (5, 9))
    record("implicit_ref.thomas", "random", "", IR.thomas(lo, di, up, rhs))
    record("heat_implicit_ref.thomas", "random", "", H.thomas(lo, di, up, rhs))
    record("layered_heat_implicit_ref.thomas", "random", "", LHI.thomas(lo, di, up, rhs))
    E = np.array([0.0, 1e-300, 0.3, 0.729, 1.0, 7.0, 1e30, np.inf, np.nan])
    for name, mod in (("coupled_trbdf2_ref", CT), ("layered_coupled_trbdf2_ref", LT), ("heat_trbdf2_ref", HT), ("layered_heat_trbdf2_ref", LHT)):
        record(name + ".step_factor", "values", "", mod.step_factor(E))
    tab = rng.uniform(0, 1, (4, 2, 2))
    for name, mod in (("coupled_implicit_ref", CR), ("layered_coupled_implicit_ref", LC), ("heat_implicit_ref", H)):
        record(name + "._sample", "table", "k", mod._sample(tab, 2))
        record(name + "._sample", "table", "weighted", mod._sample(tab, 1, TR.GAMMA))
        assert mod._sample(None, 0) is None
    record("constants", "", "", [TR.GAMMA, TR.D, TR.B, TR.HMIN_FRAC, CR.GAMMA, CR.D, LC.GAMMA, LC.D, CT.GAMMA, CT.D, CT.B, CT.HMIN_FRAC,
                                 LT.GAMMA, LT.D, LT.B, LT.HMIN_FRAC, IR.DMAX_FRAC, IR.STALL, H.GAMMA, H.D])

    # ------------------------------------------------------------------ scalar Richards: implicit_ref, trbdf2_ref
    def richards(ncols, nlev, ice=False, percol=False, kinds=(DIR, DRAIN)):
        c = CR.coupled_case(*kinds, ncols=ncols, nlev=nlev, ice=ice, percol=percol, model=M.MODEL_RICHARDS)
        vl, ti = np.asarray(c.vl, np.float64), np.asarray(c.ti, np.float64)
        return c.om, vl, ti, O.stable_dt(c.om, vl, ti, None, 0.5)

    for cname, (om, vl, ti, sd) in (("plain", richards(4, 8)), ("percol", richards(5, 7, percol=True)), ("ice", richards(4, 9, ice=True)),
                                    ("flux", richards(3, 6, kinds=(FLUX, FLUX)))):
        ncols = vl.shape[0]
        f0 = IR.tendency(om, vl, ti)
        record("implicit_ref.tendency", cname, "", f0)
        record("implicit_ref._col_param", cname, "nu", IR._col_param(om, ncols, "nu", om.soil.nu))
        record("trbdf2_ref._col_param", cname, "theta_r", TR._col_param(om, ncols, "vg_theta_r", om.vg.theta_r))
        record("implicit_ref.fd_jacobian", cname, "scalar dt", IR.fd_jacobian(om, vl, ti, 20 * sd, f0))
        record("implicit_ref.fd_jacobian", cname, "per-column coef", IR.fd_jacobian(om, vl, ti, sd * (1.0 + np.arange(ncols)), f0))
        v1, its = record("implicit_ref.implicit_euler", cname, "3 steps of 20 sd", IR.implicit_euler(om, vl, ti, 20 * sd, 3))
        record("implicit_ref.residual", cname, "", IR.residual(om, v1, vl, ti, 20 * sd))
        record("implicit_ref.implicit_euler", cname, "max_iter 2", IR.implicit_euler(om, vl, ti, 100 * sd, 2, max_iter=2))
        coef = TR.D * sd * (1.0 + np.arange(ncols))
        record("trbdf2_ref.stage_solve", cname, "per-column coef", TR.stage_solve(om, vl, vl + coef[:, None] * f0, ti, coef))
        record("trbdf2_ref.stage_solve", cname, "max_iter 3", TR.stage_solve(om, vl, vl + 50 * coef[:, None] * f0, ti, 50 * coef, max_iter=3))
        hcol = sd * (2.0 + np.arange(ncols))
        y1, f1, e, _ = record("trbdf2_ref.attempt", cname, "no bcv", TR.attempt(om, vl, f0, ti, np.zeros(ncols), hcol))
        record("trbdf2_ref.error_norm", cname, "", TR.error_norm(e, vl, y1, 1e-6, 1e-3))
        T = 24 * sd
        v, info = record("trbdf2_ref.trbdf2", cname, "fixed", TR.trbdf2(om, vl, ti, 0.0, T, T / 5.5, adaptive=False))
        witness(info, 0.0, T, adaptive=False)
        v, info = record("trbdf2_ref.trbdf2", cname, "adaptive", TR.trbdf2(om, vl, ti, 0.0, T, sd))
        witness(info, 0.0, T)
        v, info = record("trbdf2_ref.trbdf2", cname, "adaptive, per-column h0", TR.trbdf2(om, vl, ti, 0.0, T, sd, h0=hcol, reltol=1e-4))
        witness(info, 0.0, T)
        v, info = record("trbdf2_ref.trbdf2", cname, "adaptive, h0 = 300 sd", TR.trbdf2(om, vl, ti, 0.0, 400 * sd, 300 * sd, abstol=1e-8, reltol=1e-5))
        witness(info, 0.0, 400 * sd)
        v, info = record("trbdf2_ref.trbdf2", cname, "adaptive, h0 > span", TR.trbdf2(om, vl, ti, 0.0, sd, 10 * sd))
        witness(info, 0.0, sd)
        if cname in ("plain", "percol"):
            bcv = bc_table(om, 2, -0.15, M)
            record("trbdf2_ref._with_bc", cname, "scalar t", sorted(TR._with_bc(om, bcv, 0.0, T, 0.3 * T).bc.items()))
            o = TR._with_bc(om, bcv, 0.0, T, 0.1 * T * np.arange(ncols))
            record("trbdf2_ref._with_bc", cname, "per-column t", [v for k, v in sorted(o.percol_bc.items())])
            record("trbdf2_ref.attempt", cname, "bcv, per-column t and h", TR.attempt(om, vl, f0, ti, 0.1 * hcol, hcol, bcv, 0.0, T))
            v, info = record("trbdf2_ref.trbdf2", cname, "fixed, bcv", TR.trbdf2(om, vl, ti, 0.0, T, T / 4, adaptive=False, bcv=bcv))
            witness(info, 0.0, T, adaptive=False)
            v, info = record("trbdf2_ref.trbdf2", cname, "adaptive, bcv, per-column h0", TR.trbdf2(om, vl, ti, 0.0, T, sd, bcv=bcv, h0=hcol))
            witness(info, 0.0, T)
        if cname == "plain":
            v, info = record("trbdf2_ref.trbdf2", cname, "tolerances 0: hmin", TR.trbdf2(om, vl, ti, 0.0, T, sd, abstol=0.0, reltol=0.0))
            witness(info, 0.0, T)
            v, info = record("trbdf2_ref.trbdf2", cname, "max_steps 4", TR.trbdf2(om, vl, ti, 0.0, T, sd, h0=hcol, max_steps=4))
            witness(info, 0.0, T, max_steps=4)

    # ------------------------------------------------------------------ layered Richards: layered_implicit_ref
    for cname, lay in (("cells", R.make_layered(np.float64, 5, 9, LC.cell_map(5, 9), bc="flux_drain")),
                       ("horizons", R.make_layered(np.float64, 6, 12, R.horizon_map(6, 12), bc="dirichlet", ice=True))):
        ncols = lay.case.ncols
        sd = R.stable_dt(lay)
        y = np.asarray(lay.case.vl, np.float64)
        f0 = LI.tendency(lay, y)
        nu = R.cell_params(lay)["nu"]
        record("layered_implicit_ref.tendency", cname, "", f0)
        record("layered_implicit_ref.fd_jacobian", cname, "scalar coef", LI.fd_jacobian(lay, y, 20 * sd, f0, nu))
        record("layered_implicit_ref.fd_jacobian", cname, "per-column coef", LI.fd_jacobian(lay, y, sd * (1.0 + np.arange(ncols)), f0, nu))
        coef = TR.D * sd * (1.0 + np.arange(ncols))
        record("layered_implicit_ref.stage_solve", cname, "per-column coef", LI.stage_solve(lay, y, y + coef[:, None] * f0, coef))
        record("layered_implicit_ref.stage_solve", cname, "scalar coef, max_iter 2", LI.stage_solve(lay, y, y, 100 * sd, max_iter=2))
        record("layered_implicit_ref.implicit_euler", cname, "3 steps of 20 sd", LI.implicit_euler(lay, 20 * sd, 3))
        record("layered_implicit_ref.implicit_euler", cname, "vl given", LI.implicit_euler(lay, 5 * sd, 2, vl=y * 0.98))
        hcol = sd * (2.0 + np.arange(ncols))
        record("layered_implicit_ref.attempt", cname, "", LI.attempt(lay, y, f0, hcol))
        T = 24 * sd
        v, info = record("layered_implicit_ref.trbdf2", cname, "fixed", LI.trbdf2(lay, 0.0, T, T / 5.5, adaptive=False))
        witness(info, 0.0, T, adaptive=False)
        v, info = record("layered_implicit_ref.trbdf2", cname, "adaptive", LI.trbdf2(lay, 0.0, T, sd))
        witness(info, 0.0, T)
        v, info = record("layered_implicit_ref.trbdf2", cname, "adaptive, per-column h0, vl given", LI.trbdf2(lay, 0.0, T, sd, h0=hcol, reltol=1e-4, vl=y * 0.98))
        witness(info, 0.0, T)
        v, info = record("layered_implicit_ref.trbdf2", cname, "adaptive, h0 = 300 sd", LI.trbdf2(lay, 0.0, 400 * sd, 300 * sd, abstol=1e-8, reltol=1e-5))
        witness(info, 0.0, 400 * sd)
        v, info = record("layered_implicit_ref.trbdf2", cname, "adaptive, h0 > span", LI.trbdf2(lay, 0.0, sd, 10 * sd))
        witness(info, 0.0, sd)
        if cname == "cells":
            v, info = record("layered_implicit_ref.trbdf2", cname, "tolerances 0: hmin", LI.trbdf2(lay, 0.0, T, sd, abstol=0.0, reltol=0.0))
            witness(info, 0.0, T)
            v, info = record("layered_implicit_ref.trbdf2", cname, "max_steps 4", LI.trbdf2(lay, 0.0, T, sd, h0=hcol, max_steps=4))
            witness(info, 0.0, T, max_steps=4)

    # ------------------------------------------------------------------ scalar coupled: coupled_implicit_ref, coupled_trbdf2_ref
    for cname, c in (("iced", CR.coupled_case(DIR, DRAIN, ncols=4, nlev=8, ice=True)), ("flux", CR.coupled_case(FLUX, FLUX, ncols=3, nlev=6)),
                     ("percol", CR.coupled_case(DIR, DIR, ncols=5, nlev=7, percol=True))):
        om = c.om
        v, ti, e = CR.f64(c)
        ncols = v.shape[0]
        sd = CR.stable_dt(c)
        fv, fe = record("coupled_implicit_ref.tendencies", cname, "", CR.tendencies(om, v, ti, e))
        fw = record("coupled_implicit_ref.water_tendency", cname, "", CR.water_tendency(om, v, ti))
        record("coupled_implicit_ref.energy_tendency", cname, "", CR.energy_tendency(om, v, ti, e))
        record("coupled_implicit_ref._fd_jacobian", cname, "scalar coef", CR._fd_jacobian(om, v, ti, 20 * sd, fw))
        record("coupled_implicit_ref._fd_jacobian", cname, "per-column coef", CR._fd_jacobian(om, v, ti, sd * (1.0 + np.arange(ncols)), fw))
        record("coupled_implicit_ref.newton_stage", cname, "round-off", CR.newton_stage(om, v, v, ti, 20 * sd))
        record("coupled_implicit_ref.newton_stage", cname, "tol 1e-8", CR.newton_stage(om, v, v, ti, 20 * sd, tol=1e-8))
        y, its, conv = record("coupled_implicit_ref.newton_stage", cname, "tol 1e-12, max_iter 1", CR.newton_stage(om, v, v, ti, 100 * sd, tol=1e-12, max_iter=1))
        record("coupled_implicit_ref.energy_bands", cname, "", CR.energy_bands(om, v, ti))
        record("coupled_implicit_ref.energy_stage", cname, "", CR.energy_stage(om, v, ti, e, 20 * sd))
        tab = bc_table(om, 4, -0.1, M)
        for method in ("euler", "trbdf2"):
            for vname, kw in (("", {}), ("bcv", dict(bcv=tab)), ("tol 1e-10", dict(tol=1e-10)), ("float32", dict(round_to=np.float32)),
                              ("bcv, tol 1e-9, float32", dict(bcv=tab, tol=1e-9, round_to=np.float32)), ("tol 1e-12, max_iter 2", dict(tol=1e-12, max_iter=2))):
                r = record("coupled_implicit_ref.coupled_implicit", cname, method + " " + vname, CR.coupled_implicit(om, v, ti, e, 30 * sd, 3, method, **kw))
                SEEN["unconverged"] += int(r[2]["unconverged"] > 0)
        v1, e1, _ = CR.coupled_implicit(om, v, ti, e, 30 * sd, 1)
        record("coupled_implicit_ref.residual", cname, "", CR.residual(om, v, e, ti, v1, e1, 30 * sd))
        record("coupled_implicit_ref.with_bc", cname, "", sorted(CR.with_bc(om, tab[2]).bc.items()))

        coef = CT.D * sd * (1.0 + np.arange(ncols))
        w = v + coef[:, None] * fw
        record("coupled_trbdf2_ref.water_stage", cname, "round-off", CT.water_stage(om, v, w, ti, coef))
        record("coupled_trbdf2_ref.water_stage", cname, "device rule", CT.water_stage(om, v, w, ti, coef, CT.device_newton()))
        record("coupled_trbdf2_ref.water_stage", cname, "cap 1", CT.water_stage(om, v, v + 80 * coef[:, None] * fw, ti, 80 * coef, (0.01, 1e-6, 1e-3, 1)))
        record("coupled_trbdf2_ref.energy_solve", cname, "", CT.energy_solve(om, v, ti, e, coef))
        record("coupled_trbdf2_ref.energy_solve", cname, "homogeneous, scalar coef", CT.energy_solve(om, v, ti, e, 3 * sd, homogeneous=True))
        bcv = bc_table(om, 2, -0.1, M)
        hcol = sd * (2.0 + np.arange(ncols))
        T = 24 * sd
        for vname, args, kw in (("scalar t and h", (0.0, 4 * sd), {}), ("per-column h", (0.0, hcol), {}), ("full", (0.0, 4 * sd), dict(block="full")),
                                ("bcv, scalar", (0.1 * T, 4 * sd, bcv, 0.0, T), {}), ("bcv, per-column t and h", (0.1 * hcol, hcol, bcv, 0.0, T), {}),
                                ("device rule, float32", (0.0, hcol), dict(newton=CT.device_newton(), round_to=np.float32)),
                                ("bcv, full, float32", (0.1 * T, hcol, bcv, 0.0, T), dict(block="full", round_to=np.float32)),
                                ("cap 1", (0.0, 60 * sd), dict(newton=(0.01, 1e-6, 1e-3, 1)))):
            if cname == "flux" and "per-column t" in vname:
                continue
            r = record("coupled_trbdf2_ref.attempt", cname, vname, CT.attempt(om, v, e, fv, fe, ti, *args, **kw))
            record("coupled_trbdf2_ref.error_norm", cname, vname, CT.error_norm(r["ev"], r["ee"], v, r["v1"], e, r["e1"], 1e-6, CT.abstol_e_default(om), 1e-3))
        runs = [("default", (0.0, T, sd), {}, None), ("device rule", (0.0, T, sd), dict(newton=CT.device_newton()), None),
                ("float32, per-column h0", (0.0, T, sd), dict(round_to=np.float32, h0=hcol, newton=CT.device_newton()), None),
                ("h0 = 300 sd, reltol 1e-5", (0.0, 400 * sd, 300 * sd), dict(reltol=1e-5, abstol=1e-8, newton=CT.device_newton(reltol=1e-5)), None),
                ("h0 > span", (0.0, sd, 10 * sd), {}, None), ("cap 1, max_steps 30", (0.0, T, 8 * sd), dict(newton=(0.01, 1e-6, 1e-3, 1), max_steps=30), 30)]
        if cname != "flux":
            runs.append(("bcv, per-column h0", (0.0, T, sd), dict(bcv=bcv, h0=hcol, newton=CT.device_newton()), None))
        if cname == "iced":
            runs.append(("tolerances 1e-14, float32: hmin", (0.0, T, sd), dict(abstol=1e-14, abstol_e=1e-14, reltol=1e-14, round_to=np.float32), None))
            runs.append(("max_steps 4", (0.0, T, sd), dict(h0=hcol, max_steps=4), 4))
        for vname, args, kw, cap in runs:
            r = record("coupled_trbdf2_ref.integrate", cname, vname, CT.integrate(om, v, ti, e, *args, **kw))
            witness(r[2], args[0], args[1], max_steps=cap)

    # ------------------------------------------------------------------ layered coupled
    for cname, lay in (("cells", LC.layered_case(np.float64, 4, 8, kind="cells", hyd=(FLUX, FLUX), energy="flux", ice=True)),
                       ("horizons", LC.layered_case(np.float64, 5, 10, kind="horizons", hyd=(DIR, DRAIN), energy="dirichlet")),
                       ("horizons32", LC.layered_case(np.float32, 3, 12, kind="horizons", hyd=(DIR, DRAIN), energy="mixed", ice=True, percol_bc=True))):
        v, e = LC.state64(lay)
        ncols = v.shape[0]
        sd = LC.stable_dt(lay)
        l64 = LC.with_bc(lay, None)
        om = l64.case.om
        fv, fe = record("layered_coupled_implicit_ref.tendencies", cname, "", LC.tendencies(l64, v, e))
        fw = record("layered_coupled_implicit_ref.water_tendency", cname, "", LC.water_tendency(l64, v))
        nu = R.cell_params(l64)["nu"].astype(np.float64)
        record("layered_coupled_implicit_ref._fd_jacobian", cname, "scalar coef", LC._fd_jacobian(l64, v, 20 * sd, fw, nu))
        record("layered_coupled_implicit_ref._fd_jacobian", cname, "per-column coef", LC._fd_jacobian(l64, v, sd * (1.0 + np.arange(ncols)), fw, nu))
        record("layered_coupled_implicit_ref.newton_stage", cname, "round-off", LC.newton_stage(l64, v, v, 20 * sd))
        record("layered_coupled_implicit_ref.newton_stage", cname, "tol 1e-8", LC.newton_stage(l64, v, v, 20 * sd, tol=1e-8))
        record("layered_coupled_implicit_ref.newton_stage", cname, "tol 1e-12, max_iter 1", LC.newton_stage(l64, v, v, 100 * sd, tol=1e-12, max_iter=1))
        record("layered_coupled_implicit_ref.energy_bands", cname, "", LC.energy_bands(l64, v))
        record("layered_coupled_implicit_ref.energy_stage", cname, "", LC.energy_stage(l64, v, e, 20 * sd))
        tab = bc_table(om, 4, -0.05, M)
        record("layered_coupled_implicit_ref.with_bc", cname, "", sorted(LC.with_bc(lay, tab[2]).case.om.bc.items()))
        for method in ("euler", "trbdf2"):
            for vname, kw in (("", {}), ("bcv", dict(bcv=tab)), ("tol 1e-10", dict(tol=1e-10)), ("float32", dict(round_to=np.float32)),
                              ("bcv, tol 1e-9, float32", dict(bcv=tab, tol=1e-9, round_to=np.float32)), ("tol 1e-12, max_iter 2", dict(tol=1e-12, max_iter=2))):
                r = record("layered_coupled_implicit_ref.coupled_implicit", cname, method + " " + vname, LC.coupled_implicit(lay, v, e, 30 * sd, 3, method, **kw))
                SEEN["unconverged"] += int(r[2]["unconverged"] > 0)
        v1, e1, _ = LC.coupled_implicit(lay, v, e, 30 * sd, 1)
        record("layered_coupled_implicit_ref.residual", cname, "", LC.residual(lay, v, e, v1, e1, 30 * sd))

        coef = LT.D * sd * (1.0 + np.arange(ncols))
        w = v + coef[:, None] * fw
        record("layered_coupled_trbdf2_ref.water_stage", cname, "round-off", LT.water_stage(l64, v, w, coef))
        record("layered_coupled_trbdf2_ref.water_stage", cname, "device rule", LT.water_stage(l64, v, w, coef, LT.device_newton()))
        record("layered_coupled_trbdf2_ref.water_stage", cname, "cap 1", LT.water_stage(l64, v, v + 80 * coef[:, None] * fw, 80 * coef, (0.01, 1e-6, 1e-3, 1)))
        record("layered_coupled_trbdf2_ref.energy_solve", cname, "", LT.energy_solve(l64, v, e, coef))
        record("layered_coupled_trbdf2_ref.energy_solve", cname, "homogeneous, scalar coef", LT.energy_solve(l64, v, e, 3 * sd, homogeneous=True))
        bcv = bc_table(om, 2, -0.05, M)
        hcol = sd * (2.0 + np.arange(ncols))
        T = 24 * sd
        o = LT.with_bc(lay, bcv, 0.0, T, 0.1 * T * np.arange(ncols))
        record("layered_coupled_trbdf2_ref.with_bc", cname, "per-column t", [x for k, x in sorted(o.case.om.percol_bc.items())] + sorted(o.case.om.bc.items()))
        record("layered_coupled_trbdf2_ref.with_bc", cname, "scalar t", sorted(LT.with_bc(lay, bcv, 0.0, T, 0.3 * T).case.om.bc.items()))
        for vname, args, kw in (("scalar t and h", (0.0, 4 * sd), {}), ("per-column h", (0.0, hcol), {}), ("full", (0.0, 4 * sd), dict(block="full")),
                                ("bcv, scalar", (0.1 * T, 4 * sd, bcv, 0.0, T), {}), ("bcv, per-column t and h", (0.1 * hcol, hcol, bcv, 0.0, T), {}),
                                ("device rule, float32", (0.0, hcol), dict(newton=LT.device_newton(), round_to=np.float32)),
                                ("bcv, full, float32", (0.1 * T, hcol, bcv, 0.0, T), dict(block="full", round_to=np.float32)),
                                ("cap 1", (0.0, 60 * sd), dict(newton=(0.01, 1e-6, 1e-3, 1)))):
            r = record("layered_coupled_trbdf2_ref.attempt", cname, vname, LT.attempt(lay, v, e, fv, fe, *args, **kw))
            record("layered_coupled_trbdf2_ref.error_norm", cname, vname, LT.error_norm(r["ev"], r["ee"], v, r["v1"], e, r["e1"], 1e-6, LT.abstol_e_default(lay), 1e-3))
        record("layered_coupled_trbdf2_ref.first_attempt", cname, "", LT.first_attempt(lay, 4 * sd, newton=LT.device_newton()))
        record("layered_coupled_trbdf2_ref.first_attempt", cname, "bcv, full, float32", LT.first_attempt(lay, 4 * sd, bcv=bcv, block="full", round_to=np.float32))
        runs = [("default", (0.0, T, sd), {}, None), ("device rule", (0.0, T, sd), dict(newton=LT.device_newton()), None),
                ("float32, per-column h0", (0.0, T, sd), dict(round_to=np.float32, h0=hcol, newton=LT.device_newton()), None),
                ("h0 = 300 sd, reltol 1e-5", (0.0, 400 * sd, 300 * sd), dict(reltol=1e-5, abstol=1e-8, newton=LT.device_newton(reltol=1e-5)), None),
                ("h0 > span", (0.0, sd, 10 * sd), {}, None), ("cap 1, max_steps 30", (0.0, T, 8 * sd), dict(newton=(0.01, 1e-6, 1e-3, 1), max_steps=30), 30),
                ("bcv, per-column h0", (0.0, T, sd), dict(bcv=bcv, h0=hcol, newton=LT.device_newton()), None)]
        if cname == "cells":
            runs.append(("tolerances 1e-14, float32: hmin", (0.0, T, sd), dict(abstol=1e-14, abstol_e=1e-14, reltol=1e-14, round_to=np.float32), None))
            runs.append(("max_steps 4", (0.0, T, sd), dict(h0=hcol, max_steps=4), 4))
        for vname, args, kw, cap in runs:
            r = record("layered_coupled_trbdf2_ref.integrate", cname, vname, LT.integrate(lay, v, e, *args, **kw))
            witness(r[2], args[0], args[1], max_steps=cap)

    # ------------------------------------------------------------------ heat only, scalar and layered
    def heat_runs(prefix, mod, cname, P, y0, sd, om):
        ncols = y0.shape[0]
        bcv = bc_table(om, 2, 0.02, M)
        hcol = sd * (20.0 + 10.0 * np.arange(ncols))
        T = 600 * sd
        fn = record(prefix + ".fresh_tendency", cname, "", mod.fresh_tendency(P, y0, None))
        record(prefix + ".fresh_tendency", cname, "bcv, float32", mod.fresh_tendency(P, y0, bcv, np.float32))
        record(prefix + ".abstol_e_default", cname, "", mod.abstol_e_default(om))
        for vname, args in (("", (np.zeros(ncols), hcol)), ("bcv, per-column t", (0.1 * hcol, hcol, bcv, 0.0, T)),
                            ("bcv, float32", (0.1 * hcol, hcol, bcv, 0.0, T, np.float32))):
            r = record(prefix + ".attempt", cname, vname, mod.attempt(P, y0, fn, *args))
            record(prefix + ".error_norm", cname, vname, mod.error_norm(r["e"], y0, r["y1"], mod.abstol_e_default(om), 1e-3))
        record(prefix + ".fixed_trbdf2", cname, "", mod.fixed_trbdf2(P, y0, 0.0, T, 7))
        record(prefix + ".fixed_trbdf2", cname, "bcv", mod.fixed_trbdf2(P, y0, 0.0, T, 5, bcv))
        record(prefix + ".true_local_error", cname, "", mod.true_local_error(P, y0, fn, np.zeros(ncols), hcol, sub=4))
        for vname, args, kw, cap in (("default", (0.0, T, sd), {}, None), ("float32", (0.0, T, sd), dict(ft=np.float32), None),
                                     ("bcv, per-column h0", (0.0, T, sd), dict(bcv=bcv, h0=hcol), None),
                                     ("bcv, float32, h0 with zeros", (0.0, T, sd), dict(bcv=bcv, ft=np.float32, h0=hcol * (np.arange(ncols) % 2)), None),
                                     ("h0 = span", (0.0, T, T), dict(reltol=1e-4), None), ("h0 > span", (0.0, sd, 10 * sd), {}, None),
                                     ("tolerances 1e-14, float32: hmin", (0.0, T, sd), dict(abstol_e=1e-14, reltol=1e-14, ft=np.float32), None),
                                     ("max_steps 3", (0.0, T, sd), dict(h0=hcol, max_steps=3), 3), ("empty span", (2.0, 2.0, sd), {}, None)):
            r = record(prefix + ".integrate", cname, vname, mod.integrate(P, y0, *args, **kw))
            if args[1] > args[0]:
                witness(r[1], args[0], args[1], max_steps=cap)

    for cname, c in (("dirichlet", H.heat_case(4, 8)), ("flux, ice", H.heat_case(3, 6, bottom=FLUX, top=FLUX, ice=True)),
                     ("percol_bc", H.heat_case(5, 7, top=FLUX, percol_bc=True))):
        vl, ti, y0 = H.f64(c)
        sd = H.stable_dt(c)
        bands, f00 = record("heat_implicit_ref.affine_parts", cname, "", H.affine_parts(c.om, vl, ti))
        record("heat_implicit_ref.stage_solve", cname, "", H.stage_solve(bands, 30 * sd, y0))
        tab = bc_table(c.om, 4, 0.02, M)
        for method in ("euler", "trbdf2"):
            record("heat_implicit_ref.heat_implicit", cname, method, H.heat_implicit(c.om, vl, ti, y0, 100 * sd, 3, method))
            record("heat_implicit_ref.heat_implicit", cname, method + " bcv", H.heat_implicit(c.om, vl, ti, y0, 100 * sd, 3, method, bcv=tab))
        heat_runs("heat_trbdf2_ref", HT, cname, HT.problem(c), y0, sd, c.om)
    for cname, lay in (("cells", LHT.sixteen_class_case(np.float64, 4, 8, ice=True)), ("horizons", LHI.layered_case(np.float64, 5, 10, kind="horizons"))):
        y0 = LHI.state64(lay)
        y0 = y0[-1] if isinstance(y0, tuple) else y0
        heat_runs("layered_heat_trbdf2_ref", LHT, cname, LHT.problem(lay), np.asarray(y0, np.float64), LHI.stable_dt(lay), lay.case.om)

    missing = [k for k, n in SEEN.items() if n == 0]
    assert not missing, "the case list never produced: %s (%s)" % (missing, SEEN)
    with open(out, "w") as f:
        json.dump(ENTRIES, f, indent=0)
    print("%d entries written to %s; branches seen (runs): %s" % (len(ENTRIES), out, SEEN))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
