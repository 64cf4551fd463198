"""NumPy backward-Euler reference for Richards columns, built on the CPU oracle's tendency.

Per step, Newton on R(v) = v - v_n - dt f(v) = 0 with f = oracle_py.rhs (the oracle-pinned
tendency), a finite-difference tridiagonal Jacobian (three coloured evaluations: cells i = k mod 3
are perturbed together, a Richards tendency of cell i depends on cells i-1, i, i+1 only) and the
safeguard of the device stepper, iterated to round-off: until the update stops
shrinking or is zero.  The iteration, the bands and the Thomas solve are integrator_core's (newton_stage,
fd_bands, thomas); this module supplies the oracle's tendency and the per-column nu, theta_r.

Test infrastructure (tests/test_implicit_reference.py, tests/test_gpu_implicit.py)."""
from __future__ import annotations

import numpy as np

import integrator_core as core
import parity_cases as pc

O = pc.O
DMAX_FRAC, STALL, thomas = core.DMAX_FRAC, core.STALL, core.thomas


def _col_param(om, ncols, key, scalar):
    a = om.percol.get(key)
    return np.full(ncols, scalar) if a is None else np.asarray(a, dtype=np.float64)


def tendency(om, vl, ti):
    return O.rhs(om, np.ascontiguousarray(vl), np.ascontiguousarray(ti))["vl"]


def residual(om, vl, vn, ti, dt):
    return vl - vn - dt * tendency(om, vl, ti)


def fd_jacobian(om, vl, ti, dt, f0):
    """Bands (a, b, c) of J = I - dt df/dv by coloured forward differences (dt: scalar or one per column)."""
    nu = _col_param(om, vl.shape[0], "nu", om.soil.nu)[:, None]
    return core.fd_bands(lambda v: tendency(om, v, ti), vl, dt, f0, nu)


def stage_solve(om, y0, w, ti, coef, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: scalar or one per column), to round-off, with the
    device's safeguard.  Returns (Y, iterations per column)."""
    ncols = np.shape(y0)[0]
    nu = _col_param(om, ncols, "nu", om.soil.nu)[:, None]
    tr = _col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None]
    return core.newton_stage(lambda v: tendency(om, v, ti), nu, tr, ti, coef, y0, w, core.round_off, max_iter)[:2]


def implicit_euler(om, vl, ti, dt, nsteps, max_iter=120):
    """nsteps backward-Euler steps of the [ncols, nlev] state (Float64).  Returns (state, iterations
    per step [nsteps, ncols])."""
    vl = np.array(vl, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.float64)
    iters = np.zeros((nsteps, vl.shape[0]), dtype=np.int64)
    for s in range(nsteps):
        vl, iters[s] = stage_solve(om, vl, vl, ti, dt, max_iter)
    return vl, iters
