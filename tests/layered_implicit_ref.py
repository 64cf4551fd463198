"""NumPy backward Euler and TR-BDF2 for layered soils (per-cell soil classes), built on the layered tendency
of tests/layered_ref.py: tests/implicit_ref.py and tests/trbdf2_ref.py with the column constants taken per cell.

Per stage, Newton on Y - w - coef f(Y) = 0 with f = layered_ref.rhs, a finite-difference tridiagonal Jacobian
(three coloured evaluations) and the device's safeguard with every cell's own class: the applied change of a
cell is at most DMAX_FRAC (nu - theta_r) of ITS class, a cell moves at most half way to ITS theta_r, and a cell
that crosses ITS nu - theta_i from below stops there; the stall rule is per column.  Iterates to round-off.
The iteration, the bands, TR-BDF2's stages, error estimate, controller and accept / reject loop are
integrator_core's; this module supplies the layered tendency and the per-cell nu, theta_r, theta_i.  Float64
only; boundary values are the model's constants.

Test infrastructure (tests/test_layered_implicit_reference.py, tests/test_gpu_layered_implicit.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

import integrator_core as core
import layered_ref as R
from integrator_core import B, D, DMAX_FRAC, GAMMA, HMIN_FRAC, STALL, error_norm, thomas


def columns(lay: R.Layered, idx=None, dtype=np.float64) -> R.Layered:
    """Columns idx of `lay` in the working type `dtype`: by default its Float64 twin (the state and theta_i as they
    are, widened), which is what the reference below integrates."""
    idx = np.arange(lay.case.ncols) if idx is None else np.asarray(idx)
    c = lay.case
    T = None if c.T_aux is None else np.asarray(c.T_aux)[idx].astype(dtype)
    case = dataclasses.replace(c, dtype=dtype, ncols=len(idx), vl=np.asarray(c.vl)[idx].astype(dtype),
                               ti=np.asarray(c.ti)[idx].astype(dtype), T_aux=T)
    return R.Layered(case, lay.classes, np.ascontiguousarray(np.asarray(lay.class_map)[idx]))


def tendency(lay, vl):
    return R.rhs(lay, np.ascontiguousarray(vl))


def fd_jacobian(lay, vl, coef, f0, nu):
    """Bands (a, b, c) of J = I - coef df/dv by coloured forward differences (coef: scalar or one per column)."""
    return core.fd_bands(lambda v: tendency(lay, v), vl, coef, f0, nu)


def stage_solve(lay, y0, w, coef, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: scalar or one per column), to round-off, with
    the device's per-cell safeguard.  Returns (Y, iterations per column)."""
    p = R.cell_params(lay)
    ti = np.asarray(lay.case.ti, dtype=np.float64)
    return core.newton_stage(lambda v: tendency(lay, v), p["nu"], p["theta_r"], ti, coef, y0, w, core.round_off, max_iter)[:2]


def implicit_euler(lay, dt, nsteps, vl=None):
    """nsteps backward-Euler steps of the [ncols, nlev] state (Float64).  Returns (state, iterations per step
    [nsteps, ncols])."""
    y = np.array(lay.case.vl if vl is None else vl, dtype=np.float64)
    iters = np.zeros((nsteps, y.shape[0]), dtype=np.int64)
    for s in range(nsteps):
        y, iters[s] = stage_solve(lay, y, y, dt)
    return y, iters


def attempt(lay, yn, fn, h):
    """One TR-BDF2 step of every column from (yn, fn) with steps h (per column).  Returns
    (Y_1, f_{n+1}, error estimate e, Newton iterations)."""
    solve = lambda y, w, c: stage_solve(lay, y, w, c)
    bands = lambda y, c: fd_jacobian(lay, y, c, tendency(lay, y), R.cell_params(lay)["nu"])
    return core.richards_attempt(solve, solve, bands, yn, fn, h)


def trbdf2(lay, t0, t1, dt, adaptive=True, abstol=1e-6, reltol=1e-3, h0=None, vl=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (Float64) from t0 to t1.  Fixed mode: steps of dt, the last one
    clipped onto t1.  Adaptive: per-column step control from h0 (default dt).  Returns (state, info) with
    info = dict(t, h, accepted, rejected, failed) per column."""
    y = np.array(lay.case.vl if vl is None else vl, dtype=np.float64)
    h = np.full(y.shape[0], float(dt)) if h0 is None else np.array(h0, dtype=np.float64)

    def one(state, f, t, hh):
        y1, f1, e, _ = attempt(lay, state[0], f[0], hh)
        return (y1,), (f1,), error_norm(e, state[0], y1, abstol, reltol) if adaptive else None, None

    (y,), info = core.adaptive_loop(one, (y,), (tendency(lay, y),), t0, t1, h, max_steps, adaptive)
    return y, info
