"""NumPy reference for implicit steps of the coupled model (SoilEnergyModel + SoilHydrologyModel without
conductivity factors), built on the CPU oracle's tendency.

Two properties of the coupled tendency f = (f_w, f_e) make a stage Y - w - c f(Y) = 0 block triangular
(tests/test_coupled_implicit_reference.py asserts both):
  - f_w does not read rhoe_int;
  - f_e is affine in rhoe_int at fixed vartheta_l, theta_i.
So the stage is solved exactly by
  water:  implicit_ref's safeguarded Newton (finite-difference Jacobian, the DESIGN section 4.12 safeguard) on
          the oracle's coupled water tendency (evaluated with rhoe_int = 0: the bits do not depend on it);
  energy: the bands of the affine f_e at the new water state from three coloured evaluations (exact), then
          implicit_ref.thomas.

Methods of lh_step_coupled_implicit, fixed step h:
  backward Euler:  Y_1 - Y_n - h f(Y_1, t + h) = 0
  TR-BDF2, gamma = 2 - sqrt 2, d = gamma / 2:
    stage 1: Y_g - w1 - d h f(Y_g, t + gamma h) = 0,  w1 = Y_n + d h f_n
    stage 2: Y_1 - w2 - d h f(Y_1, t + h) = 0,        w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
    f_n+1 = (Y_1 - w2) / (d h); f_0 = f(Y_0, t) is the one tendency evaluation of a call.
Boundary values: None (the model's), or bcv [nsteps + 1][2 faces][2 components] at t + k h, both components;
backward Euler uses sample k + 1 for step k, TR-BDF2 (1 - gamma) v_k + gamma v_k+1 for stage 1, v_k+1 for
stage 2 and v_0 for f_0.  Per-column values of the model take precedence.

tol: None iterates Newton to round-off; a number stops it by the device's rule, max_i |delta_i| <=
tol max(|Y_i|, nu) on the Newton step, within max_iter iterations.

The Newton iteration with its stopping rules, the coloured bands and the sampling of bcv are integrator_core's
(newton_stage, fd_bands, sample); this module supplies the oracle's coupled tendencies, the exact energy bands and
the two methods' stage sequence.

Test infrastructure (tests/test_coupled_implicit_reference.py, tests/test_gpu_coupled_implicit.py)."""
from __future__ import annotations

import copy

import numpy as np

import case_model as M
import implicit_ref as R
import integrator_core as core
import parity_cases as pc

O = pc.O
GAMMA, D, _sample = core.GAMMA, core.D, core.sample
_c = lambda a: np.ascontiguousarray(a, dtype=np.float64)


def tendencies(om, vl, ti, rhoe):
    """(d vartheta_l / dt, d rhoe_int / dt) of the oracle's coupled model, Float64 [ncols, nlev]."""
    f = O.rhs(om, _c(vl), _c(ti), _c(rhoe))
    return f["vl"], f["rhoe"]


def water_tendency(om, vl, ti):
    return tendencies(om, vl, ti, np.zeros_like(_c(vl)))[0]


def energy_tendency(om, vl, ti, rhoe):
    return tendencies(om, vl, ti, rhoe)[1]


def with_bc(om, sample):
    """om with the scalar boundary values of one bcv sample [2 faces][2 components] (None: om)."""
    if sample is None:
        return om
    o = copy.copy(om)
    o.bc = dict(om.bc)
    for key, (kind, _) in om.bc.items():
        if kind in (M.BC_DIRICHLET, M.BC_FLUX):
            o.bc[key] = (kind, float(sample[key[0]][key[1]]))
    return o


def _fd_jacobian(om, vl, ti, coef, f0):
    """Bands (a, b, c) of J = I - coef d f_w / d vl by coloured forward differences (implicit_ref.fd_jacobian
    on the coupled water tendency)."""
    nu = R._col_param(om, vl.shape[0], "nu", om.soil.nu)[:, None]
    return core.fd_bands(lambda v: water_tendency(om, v, ti), vl, coef, f0, nu)


def safeguard(om, ncols):
    """(nu, theta_r) of the Newton stage's safeguard, one per column: [ncols, 1]"""
    return R._col_param(om, ncols, "nu", om.soil.nu)[:, None], R._col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None]


def newton_stage(om, y, w, ti, coef, tol=None, max_iter=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y.  Returns (Y, iterations [ncols],
    converged [ncols])."""
    ti = _c(ti)
    stop, cap = (core.round_off, 120) if tol is None else (core.fixed_step_rule(tol), 50)
    nu, tr = safeguard(om, np.shape(y)[0])
    return core.newton_stage(lambda v: water_tendency(om, v, ti), nu, tr, ti, coef, y, w, stop, cap if max_iter is None else max_iter)


def energy_bands(om, vl, ti):
    """Bands (lo, di, up) of A and f0 with f_e(rhoe) = A rhoe + f0 at the water state (vl, ti): three coloured
    evaluations (f_e,i reads cells i-1, i, i+1 only; exact for an affine f_e up to the rounding of f)."""
    vl = _c(vl)
    ncols, n = vl.shape
    f0 = energy_tendency(om, vl, ti, np.zeros((ncols, n)))
    lo, di, up = np.zeros((ncols, n)), np.zeros((ncols, n)), np.zeros((ncols, n))
    s = 2.0 ** 30   # (a power of two: exact scaling)
    for k in range(3):
        e = np.zeros((ncols, n))
        e[:, k::3] = s
        df = (energy_tendency(om, vl, ti, e) - f0) / s
        for j in range(k, n, 3):
            di[:, j] = df[:, j]
            if j > 0:
                up[:, j - 1] = df[:, j - 1]
            if j + 1 < n:
                lo[:, j + 1] = df[:, j + 1]
    return (lo, di, up), f0


def energy_stage(om, vl, ti, w, coef):
    """The energy stage Y - w - coef f_e(Y) = 0 at the water state vl: (I - coef A) Y = w + coef f0."""
    (lo, di, up), f0 = energy_bands(om, vl, ti)
    return R.thomas(-coef * lo, 1.0 - coef * di, -coef * up, w + coef * f0)


def coupled_implicit(om, vl, ti, rhoe, dt, nsteps, method="euler", bcv=None, tol=None, max_iter=None, round_to=None):
    """nsteps steps of the [ncols, nlev] state (vl, rhoe); ti is held.  round_to: a dtype every stage output is
    rounded to (what storing the state in that type costs).  Returns (vl, rhoe, info) with info = dict(iters =
    largest Newton count, unconverged = column-stages that did not converge)."""
    assert method in ("euler", "trbdf2")
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    v, e, ti = np.array(vl, dtype=np.float64), np.array(rhoe, dtype=np.float64), _c(ti)
    if bcv is not None:
        assert np.asarray(bcv).shape == (nsteps + 1, 2, 2)
    info = dict(iters=0, unconverged=0)

    def stage(o, guess, wv, we, coef):
        y, its, conv = newton_stage(o, guess, wv, ti, coef, tol, max_iter)
        info["iters"] = max(info["iters"], int(its.max()))
        info["unconverged"] += int((~conv).sum())
        y = rnd(y)
        return y, rnd(energy_stage(o, y, ti, we, coef))

    if method == "euler":
        for k in range(nsteps):
            v, e = stage(with_bc(om, _sample(bcv, k + 1)), v, v, e, dt)
        return v, e, info
    dh = D * dt
    fv, fe = tendencies(with_bc(om, _sample(bcv, 0)), v, ti, e)
    for k in range(nsteps):
        vg, eg = stage(with_bc(om, _sample(bcv, k, GAMMA)), v, v + dh * fv, e + dh * fe, dh)
        wv = (vg - (1.0 - GAMMA) ** 2 * v) / (GAMMA * (2.0 - GAMMA))
        we = (eg - (1.0 - GAMMA) ** 2 * e) / (GAMMA * (2.0 - GAMMA))
        v, e = stage(with_bc(om, _sample(bcv, k + 1)), vg, wv, we, dh)
        fv, fe = (v - wv) / dh, (e - we) / dh
    return v, e, info


def residual(om, vl0, e0, ti, vl1, e1, dt):
    """The full coupled backward-Euler residual (Y1 - Yn - dt f(Y1)) through the oracle: (water, energy)."""
    fv, fe = tendencies(om, vl1, ti, e1)
    return vl1 - vl0 - dt * fv, e1 - e0 - dt * fe


# ------------------------------------------------------------------ cases shared by the two test files

KINDS = [(M.BC_FLUX, M.BC_FLUX), (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET),
         (M.BC_DIRICHLET, M.BC_DIRICHLET), (M.BC_FLUX, M.BC_FREE_DRAINAGE)]   # tests/test_gpu_implicit.py::KINDS
HYD_VALUES = {M.BC_FLUX: -2e-9, M.BC_DIRICHLET: 0.34, M.BC_FREE_DRAINAGE: 0.0}
ENERGY_DEFAULT = ((M.BC_DIRICHLET, 276.0), (M.BC_FLUX, 0.05))   # (top, bottom)
DZ = 0.02


def coupled_case(top, bottom, dtype=np.float64, ncols=64, nlev=64, ice=False, percol=False, energy=ENERGY_DEFAULT,
                 model=M.MODEL_COUPLED):
    """tests/test_gpu_implicit.py::richards_case's fields (wetting_front, 0.04 uhash ice in every other column,
    the same hydrology BC values) on the coupled model with coupled_soil(), T = 284 + 5 z / 1.28 + 2 (u - 1/2),
    energy BCs (top, bottom).  model = MODEL_RICHARDS: the Richards model with the same hydrology."""
    n = nlev
    zmin = -DZ * n
    sp, vg = pc.coupled_soil()
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (top, HYD_VALUES[top]),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (bottom, 0.2 if bottom == M.BC_DIRICHLET else HYD_VALUES[bottom])}
    if model == M.MODEL_COUPLED:
        bc[(M.FACE_TOP, M.COMP_ENERGY)] = energy[0]
        bc[(M.FACE_BOTTOM, M.COMP_ENERGY)] = energy[1]
    om = M.CaseModel(model, n, zmin, 0.0, soil=sp, vg=vg, bc=bc)
    c = np.arange(ncols)
    if percol:
        om.percol = dict(vg_n=1.4 + 1.2 * pc.uhash(c, 2, n), vg_alpha=1.5 + 4.0 * pc.uhash(c, 3, n),
                         vg_Ksat=10.0 ** (-7.0 + 2.0 * pc.uhash(c, 4, n)), nu=0.35 + 0.15 * pc.uhash(c, 6, n))
        om.percol_bc = {k: v[1] * (1.0 + 0.05 * (pc.uhash(c, 77 + k[0], 1) - 0.5)) for k, v in bc.items()
                        if v[0] == M.BC_DIRICHLET and k[1] == M.COMP_HYDROLOGY}
    vl = pc.wetting_front(ncols, n, zmin, 0.0, 0.35).astype(dtype)
    ti = np.zeros((ncols, n))
    if ice:   # static ice in every other column, below the pore space left by the water
        ti = np.where((c % 2 == 0)[:, None], 0.04 * pc.uhash(c[:, None], np.arange(n)[None, :] + 5, 1000), 0.0)
    ti = ti.astype(dtype)
    if model != M.MODEL_COUPLED:
        return pc.Case("coupled_implicit_richards", om, dtype, ncols, vl=vl, ti=ti)
    zc, _ = pc.grid_np(zmin, 0.0, n)
    T = 284.0 + 5.0 * zc[None, :] / 1.28 + 2.0 * (pc.uhash(c, 1, n)[:, None] - 0.5)
    e = om.earth
    nu = om.percol.get("nu", np.full(ncols, sp.nu))[:, None]
    v64, t64 = vl.astype(np.float64), ti.astype(np.float64)
    tl = np.minimum(v64, nu - t64)
    rho_c_s = sp.rho_c_ds + tl * (e.cp_l * e.rho_liq) + t64 * (e.cp_i * e.rho_ice)
    rhoe = rho_c_s * (T - e.T_0) - t64 * e.rho_ice * e.LH_f0
    return pc.Case("coupled_implicit", om, dtype, ncols, vl=vl, ti=ti, rhoe=rhoe.astype(dtype))


def f64(case):
    """(vl, ti, rhoe) of a case as Float64 arrays (the values the device holds, exactly)."""
    return tuple(np.asarray(a, dtype=np.float64) for a in (case.vl, case.ti, case.rhoe))


def stable_dt(case):
    """The oracle's coupled stable step at courant 1/2."""
    vl, ti, rhoe = f64(case)
    return O.stable_dt(case.om, vl, ti, rhoe, 0.5)


# the order tests: T = 16 stable steps, the errors against oracle SSPRK33 at sd / 8
ORDER_SPAN = 16.0
ORDER_STEPS = {"euler": (4, 8, 16), "trbdf2": (4, 8, 16)}
ORDER_BANDS = {"euler": (1.8, 2.2), "trbdf2": (3.7, 4.5)}


def order_case(ncols=4):
    return coupled_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, ncols=ncols, ice=True)


def ssprk33_reference(case, span):
    """(vl, rhoe) of oracle SSPRK33 at sd / 8 over `span` stable steps."""
    vl, ti, re = (a.copy() for a in f64(case))
    sd = stable_dt(case)
    O.ssprk33(case.om, sd / 8, int(round(8 * span)), vl, ti, re)
    return vl, re


def order_ratios(method, solve, case=None):
    """Per variable the error ratios per halving of h of solve(case, dt, nsteps) -> (vl, rhoe) against
    ssprk33_reference (max norm): dict(vl=[...], rhoe=[...]) and the errors."""
    case = case or order_case()
    T = ORDER_SPAN * stable_dt(case)
    want = ssprk33_reference(case, ORDER_SPAN)
    errs = {"vl": [], "rhoe": []}
    for n in ORDER_STEPS[method]:
        got = solve(case, T / n, n)
        for name, g, w in zip(("vl", "rhoe"), got, want):
            errs[name].append(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w))))
    return {k: [v[i] / v[i + 1] for i in range(len(v) - 1)] for k, v in errs.items()}, errs
