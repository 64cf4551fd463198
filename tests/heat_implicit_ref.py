"""NumPy reference for implicit steps of the heat-only model (SoilEnergyModel + PrescribedHydrologyModel),
built on the CPU oracle's tendency.

With vartheta_l and theta_i prescribed the tendency is affine in rhoe_int: f(Y, t) = A Y + b(t), where
only b depends on the boundary values.  A is built by applying the oracle's tendency to unit vectors,
A[:, j] = f(e_j) - f(0) (three coloured evaluations: f_i reads cells i-1, i, i+1 only), no closure is
restated here.  A stage Y - w - c f(Y) = 0 is the tridiagonal system (I - c A) Y = w + c b, solved in
Float64 with Thomas (integrator_core.thomas; no pivoting: I - c A is a column-diagonally-dominant M-matrix).

Methods of lh_step_heat_implicit, fixed step h:
  backward Euler:  (I - h A) Y_1 = Y_n + h b(t + h)
  TR-BDF2, gamma = 2 - sqrt 2, d = gamma / 2:
    stage 1: (I - d h A) Y_g = Y_n + d h f(Y_n, t) + d h b(t + gamma h)
    stage 2: (I - d h A) Y_1 = w2 + d h b(t + h),  w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
Boundary values: None (the model's), or bcv [nsteps + 1][2 faces][2 components] at t + k h; backward Euler
uses sample k + 1 for step k, TR-BDF2 (1 - gamma) v_k + gamma v_k+1 for stage 1, v_k+1 for stage 2 and
v_k for f(Y_n, t).  Only the Dirichlet / flux ENERGY entries are read; per-column values of the model
take precedence.

Test infrastructure (tests/test_heat_implicit_reference.py, tests/test_gpu_heat_implicit.py)."""
from __future__ import annotations

import copy

import numpy as np

import case_model as M
import integrator_core as core
import parity_cases as pc

O = pc.O
GAMMA, D, thomas, _sample = core.GAMMA, core.D, core.thomas, core.sample


def tendency(om, vl, ti, rhoe):
    """The oracle's d rhoe_int / dt of the [ncols, nlev] Float64 state."""
    c = np.ascontiguousarray
    return O.rhs(om, c(vl, dtype=np.float64), c(ti, dtype=np.float64), c(rhoe, dtype=np.float64))["rhoe"]


def with_energy_bc(om, sample):
    """om with the scalar energy boundary values of one bcv sample [2 faces][2 components] (None: om)."""
    if sample is None:
        return om
    o = copy.copy(om)
    o.bc = dict(om.bc)
    for f in (M.FACE_BOTTOM, M.FACE_TOP):
        key = (f, M.COMP_ENERGY)
        if key in om.bc and om.bc[key][0] in (M.BC_DIRICHLET, M.BC_FLUX):
            o.bc[key] = (om.bc[key][0], float(sample[f][M.COMP_ENERGY]))
    return o


def affine_parts(om, vl, ti):
    """Bands (lo, di, up) of A, A[i, i-1] = lo[:, i], A[i, i] = di[:, i], A[i, i+1] = up[:, i], per column,
    and f(0)."""
    vl = np.asarray(vl, dtype=np.float64)
    ncols, n = vl.shape
    zero = np.zeros((ncols, n))
    f0 = tendency(om, vl, ti, zero)
    lo, di, up = np.zeros((ncols, n)), np.zeros((ncols, n)), np.zeros((ncols, n))
    s = 2.0 ** 30   # (a power of two: exact scaling; large, so that f(s e_j) - f(0) loses little to the constant)
    for k in range(3):
        e = np.zeros((ncols, n))
        e[:, k::3] = s
        df = (tendency(om, vl, ti, e) - f0) / s
        for j in range(k, n, 3):
            di[:, j] = df[:, j]
            if j > 0:
                up[:, j - 1] = df[:, j - 1]
            if j + 1 < n:
                lo[:, j + 1] = df[:, j + 1]
    return (lo, di, up), f0


def matrix(bands, coef):
    """Dense M = I - coef A per column: [ncols, n, n]."""
    lo, di, up = bands
    ncols, n = di.shape
    Mx = np.zeros((ncols, n, n))
    i = np.arange(n)
    Mx[:, i, i] = 1.0 - coef * di
    Mx[:, i[1:], i[:-1]] = -coef * lo[:, 1:]
    Mx[:, i[:-1], i[1:]] = -coef * up[:, :-1]
    return Mx


def cond_inf(bands, coef):
    """cond_inf(I - coef A) per column."""
    Mx = matrix(bands, coef)
    return np.array([np.linalg.cond(m, np.inf) for m in Mx])


def stage_solve(bands, coef, rhs):
    lo, di, up = bands
    return thomas(-coef * lo, 1.0 - coef * di, -coef * up, rhs)


def heat_implicit(om, vl, ti, rhoe, dt, nsteps, method="euler", bcv=None):
    """nsteps steps of the [ncols, nlev] rhoe_int state (Float64); vl, ti are held.  Returns the state."""
    assert method in ("euler", "trbdf2")
    y = np.array(rhoe, dtype=np.float64)
    vl = np.asarray(vl, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.float64)
    if bcv is not None:
        assert np.asarray(bcv).shape == (nsteps + 1, 2, 2)
    bands, _ = affine_parts(om, vl, ti)
    zero = np.zeros_like(y)
    b_at = lambda sample: tendency(with_energy_bc(om, sample), vl, ti, zero)   # b(t) = f(0, t)
    b_const = None if bcv is not None else b_at(None)
    for k in range(nsteps):
        if method == "euler":
            b1 = b_const if bcv is None else b_at(_sample(bcv, k + 1))
            y = stage_solve(bands, dt, y + dt * b1)
            continue
        dh = D * dt
        fn = tendency(with_energy_bc(om, _sample(bcv, k)), vl, ti, y)
        bg = b_const if bcv is None else b_at(_sample(bcv, k, GAMMA))
        yg = stage_solve(bands, dh, y + dh * fn + dh * bg)
        w2 = (yg - (1.0 - GAMMA) ** 2 * y) / (GAMMA * (2.0 - GAMMA))
        b1 = b_const if bcv is None else b_at(_sample(bcv, k + 1))
        y = stage_solve(bands, dh, w2 + dh * b1)
    return y


# ------------------------------------------------------------------ cases shared by the two test files

BC_VALUES = {M.BC_DIRICHLET: (290.0, 280.0), M.BC_FLUX: (3.0, -2.0), M.BC_NONE: (0.0, 0.0)}   # (bottom, top)


def heat_case(ncols, nlev, dtype=np.float64, bottom=M.BC_DIRICHLET, top=M.BC_DIRICHLET, ice=False,
              percol_bc=False, smooth=False):
    """parity_cases' heat_dirichlet case (its soil, its hashed vartheta_l, its T profile, dz = 1/60) cut to
    nlev levels, with the given energy boundary kinds.  ice: static ice in the lower half of every other
    column.  percol_bc: the Dirichlet values vary by column.  smooth: level-uniform water and a T profile
    that meets the Dirichlet values at the faces (for the order tests)."""
    base = pc.make_case("heat_dirichlet_f64", ncols=ncols)
    sp, e = base.om.soil, base.om.earth
    dz = 1.0 / 60
    zmax = nlev * dz
    bc = {}
    for face, kind, v in ((M.FACE_BOTTOM, bottom, 0), (M.FACE_TOP, top, 1)):
        if kind != M.BC_NONE:
            bc[(face, M.COMP_ENERGY)] = (kind, BC_VALUES[kind][v])
    om = M.CaseModel(M.MODEL_HEAT, nlev, 0.0, zmax, soil=sp, bc=bc)
    c = np.arange(ncols)
    if percol_bc:
        # (rounded to the working type here, so that the device and the reference hold the same numbers)
        om.percol_bc = {k: (v[1] + 2.0 * (pc.uhash(c, 77 + k[0], 1) - 0.5)).astype(dtype).astype(np.float64)
                        for k, v in bc.items() if v[0] == M.BC_DIRICHLET}
    lev = np.arange(nlev)
    vl = np.array(base.vl[:, :nlev], dtype=np.float64)
    ti = np.zeros((ncols, nlev))
    if ice:
        ti = np.where((c % 2 == 0)[:, None] & (lev < max(1, nlev // 2))[None, :],
                      0.05 * pc.uhash(c[:, None], lev[None, :] + 99, 1000), 0.0)
    zc, _ = pc.grid_np(0.0, zmax, nlev)
    if smooth:
        vl = np.full((ncols, nlev), 0.25)
        T = 290.0 - 10.0 * zc[None, :] / zmax + 3.0 * np.sin(np.pi * zc / zmax)[None, :] + 0.0 * c[:, None]
    else:
        T = 285.0 + 3.0 * np.sin(6.0 * zc)[None, :] + pc.uhash(c, 9, nlev)[:, None]
    tl = np.minimum(vl, sp.nu - ti)
    rho_c_s = sp.rho_c_ds + tl * (e.cp_l * e.rho_liq) + ti * (e.cp_i * e.rho_ice)
    rhoe = rho_c_s * (T - e.T_0) - ti * e.rho_ice * e.LH_f0
    return pc.Case("heat_implicit", om, dtype, ncols, vl=vl.astype(dtype), ti=ti.astype(dtype),
                   rhoe=rhoe.astype(dtype))


def f64(case):
    """(vl, ti, rhoe) of a case as Float64 arrays (the values the device holds, exactly)."""
    return tuple(np.asarray(a, dtype=np.float64) for a in (case.vl, case.ti, case.rhoe))


def stable_dt(case):
    """The explicit engines' cap, courant 1/2."""
    vl, ti, rhoe = f64(case)
    return O.stable_dt(case.om, vl, ti, rhoe, 0.5)


# test/SoilModel/heat_test_interface.jl: n = 60 on (0, 1), unit diffusivity, T = 0 top, 5 cos(2 pi t) bottom
ANALYTIC_A, ANALYTIC_OMEGA = 5.0, 2.0 * np.pi


def analytic_case():
    sp = M.default_soil(nu=0.495, nu_ss_gravel=0.1, nu_ss_om=0.1, nu_ss_quartz=0.1, rho_c_ds=0.43314518988433487,
                        kappa_solid=8.0, kappa_sat_unfrozen=0.57, kappa_sat_frozen=2.29)
    n = 60
    bc = {(M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 0.0),
          (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_DIRICHLET, ANALYTIC_A)}
    om = M.CaseModel(M.MODEL_HEAT, n, 0.0, 1.0, soil=sp, bc=bc)
    rhoe = np.full((1, n), sp.rho_c_ds * (0.0 - om.earth.T_0))   # T = 0, theta_l = theta_i = 0
    return pc.Case("heat_analytic", om, np.float64, 1, vl=np.zeros((1, n)), ti=np.zeros((1, n)), rhoe=rhoe)


def analytic_bcv(dt, nsteps, t0=0.0):
    bcv = np.zeros((nsteps + 1, 2, 2))
    bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY] = ANALYTIC_A * np.cos(ANALYTIC_OMEGA * (t0 + dt * np.arange(nsteps + 1)))
    return bcv


def analytic_mse(case, rhoe, tf):
    """mean((T - analytic)^2) at time tf, the reference's criterion (< 1e-6)."""
    om = case.om
    z, _ = O.grid(om.zmin, om.zmax, om.nlev)
    s = np.sqrt(ANALYTIC_OMEGA / 2) * (1 + 1j)
    want = np.real((np.exp(s * (1 - z)) - np.exp(-s * (1 - z))) * ANALYTIC_A * np.exp(1j * ANALYTIC_OMEGA * tf)
                   / (np.exp(s) - np.exp(-s)))
    T = om.earth.T_0 + np.asarray(rhoe, dtype=np.float64).reshape(-1) / om.soil.rho_c_ds
    return float(np.mean((want - T) ** 2))


# the order tests: a smooth case with constant Dirichlet values over ORDER_SPAN stable steps, in 4 .. 32 steps
# (dt = 500 .. 62.5 stable steps: the CPU reference sits inside the bands 1.8-2.2 / 3.6-4.4 with room)
ORDER_SPAN, ORDER_STEPS = 2000.0, (4, 8, 16, 32)


def order_errors(method, solve, steps=ORDER_STEPS):
    """Max-norm errors of solve(case, dt, nsteps) against the reference at dt / 16, per step count."""
    case = heat_case(2, 60, smooth=True)
    vl, ti, re = f64(case)
    span = ORDER_SPAN * stable_dt(case)
    errs = []
    for n in steps:
        ref = heat_implicit(case.om, vl, ti, re, span / n / 16, 16 * n, method)
        errs.append(float(np.max(np.abs(solve(case, span / n, n) - ref))))
    return errs
