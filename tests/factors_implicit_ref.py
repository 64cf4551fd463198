"""NumPy backward Euler and TR-BDF2 for Richards columns WITH conductivity factors (TemperatureDependentViscosity,
IceImpedance), built on the CPU oracle's tendency at a prescribed temperature: tests/implicit_ref.py and
tests/trbdf2_ref.py with f = O.rhs(om, vl, ti, None, T).

T is prescribed and theta_i never changes, so f is a function of vartheta_l alone and reads cells i-1, i, i+1 only: the
Newton stage, its coloured finite-difference bands, the safeguard, TR-BDF2's stages, error estimate, controller and
accept / reject loop are integrator_core's, unchanged (newton_stage, richards_attempt, adaptive_loop, error_norm); this
module binds them to the tendency with factors and holds no algorithm text of its own.  Float64; boundary values are
the model's constants.

Test infrastructure (tests/test_factors_implicit_reference.py, tests/test_gpu_factors_implicit.py)."""
from __future__ import annotations

import numpy as np

import implicit_ref as IR
import integrator_core as core
import parity_cases as pc

O = pc.O
error_norm = core.error_norm


def tendency(om, vl, ti, T):
    return O.rhs(om, np.ascontiguousarray(vl), np.ascontiguousarray(ti), None, np.ascontiguousarray(T))["vl"]


def _safeguard(om, ncols):
    return (IR._col_param(om, ncols, "nu", om.soil.nu)[:, None], IR._col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None])


def fd_jacobian(om, vl, ti, T, coef, f0):
    """Bands (a, b, c) of J = I - coef df/dv by coloured forward differences (coef: scalar or one per column)."""
    return core.fd_bands(lambda v: tendency(om, v, ti, T), vl, coef, f0, _safeguard(om, vl.shape[0])[0])


def stage_solve(om, y0, w, ti, T, coef, stop=core.round_off, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: scalar or one per column) with the device's safeguard;
    stop: one of integrator_core's stopping rules (default: to round-off).  Returns (Y, iterations per column,
    converged per column)."""
    nu, tr = _safeguard(om, np.shape(y0)[0])
    return core.newton_stage(lambda v: tendency(om, v, ti, T), nu, tr, ti, coef, y0, w, stop, max_iter)


def implicit_euler(om, vl, ti, T, dt, nsteps, stop=core.round_off, max_iter=120):
    """nsteps backward-Euler steps of the [ncols, nlev] state (Float64).  Returns (state, iterations per step
    [nsteps, ncols], converged per step [nsteps, ncols])."""
    vl = np.array(vl, dtype=np.float64)
    ti, T = np.asarray(ti, dtype=np.float64), np.asarray(T, dtype=np.float64)
    iters = np.zeros((nsteps, vl.shape[0]), dtype=np.int64)
    conv = np.zeros((nsteps, vl.shape[0]), dtype=bool)
    for s in range(nsteps):
        vl, iters[s], conv[s] = stage_solve(om, vl, vl, ti, T, dt, stop, max_iter)
    return vl, iters, conv


def attempt(om, yn, fn, ti, T, h):
    """One TR-BDF2 step of every column from (yn, fn) with steps h (per column).  Returns
    (Y_1, f_{n+1}, error estimate e, Newton iterations)."""
    solve = lambda y, w, c: stage_solve(om, y, w, ti, T, c)[:2]
    bands = lambda y, c: fd_jacobian(om, y, ti, T, c, tendency(om, y, ti, T))
    return core.richards_attempt(solve, solve, bands, yn, fn, h)


def trbdf2(om, vl, ti, T, t0, t1, dt, adaptive=True, abstol=1e-6, reltol=1e-3, h0=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (Float64) from t0 to t1.  Fixed mode: steps of dt, the last one clipped onto
    t1.  Adaptive: per-column step control from h0 (default dt).  Returns (state, info) with
    info = dict(t, h, accepted, rejected, failed) per column."""
    y = np.array(vl, dtype=np.float64)
    ti, T = np.asarray(ti, dtype=np.float64), np.asarray(T, dtype=np.float64)
    h = np.full(y.shape[0], float(dt)) if h0 is None else np.array(h0, dtype=np.float64)

    def one(state, f, t, hh):
        y1, f1, e, _ = attempt(om, state[0], f[0], ti, T, hh)
        return (y1,), (f1,), error_norm(e, state[0], y1, abstol, reltol) if adaptive else None, None

    (y,), info = core.adaptive_loop(one, (y,), (tendency(om, y, ti, T),), t0, t1, h, max_steps, adaptive)
    return y, info
