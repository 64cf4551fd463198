"""NumPy TR-BDF2 reference for Richards columns, built on the CPU oracle's tendency.

The method of lh_integrate_trbdf2, with gamma = 2 - sqrt(2), d = gamma/2:
  stage 1: Y_g - w1 - d h f(Y_g, t + gamma h) = 0,  w1 = Y_n + d h f_n
  stage 2: Y_1 - w2 - d h f(Y_1, t + h) = 0,        w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
each stage solved by the Newton of tests/implicit_ref.py (its finite-difference tridiagonal Jacobian, its
Thomas solver and the device's safeguard) to round-off; the stage derivatives are recovered from the
converged stage equations, z = (Y - w) / d, and f_{n+1} = z_1 / h is the next f_n.  The error estimate is
e = (I - d h J(Y_1))^-1 (b1 h f_n + b2 z_g + b3 z_1), b = ((1 - sqrt 2)/3, 1/3, (sqrt 2 - 2)/3)
(Hosea & Shampine 1996), with the controller of the device.  Fixed and adaptive modes; in the adaptive
mode every column has its own t and h.  Boundary values: None (the model's), or bcv [2][2][2] =
[t0 | t1][face][component], linear in time between the call's two ends.

The stage formulas, the controller and the accept / reject loop are integrator_core's (richards_attempt,
step_factor, adaptive_loop), the Newton stage is implicit_ref.stage_solve; this module supplies the oracle's
tendency under the boundary values of a stage time (_with_bc).

Test infrastructure (tests/test_trbdf2_reference.py, tests/test_gpu_trbdf2.py)."""
from __future__ import annotations

import copy

import numpy as np

import case_model as M
import implicit_ref as IR
import integrator_core as core

GAMMA, D, B, HMIN_FRAC = core.GAMMA, core.D, core.B, core.HMIN_FRAC
_col_param = IR._col_param


def _with_bc(om, bcv, t0, t1, t):
    """om with its Dirichlet values at time(s) t (scalar, or one per column) interpolated from bcv."""
    if bcv is None:
        return om
    bcv = np.asarray(bcv, dtype=np.float64).reshape(2, 2, 2)
    s = (np.asarray(t, dtype=np.float64) - t0) / (t1 - t0) if t1 > t0 else np.ones_like(np.asarray(t, float))
    o = copy.copy(om)
    o.bc = dict(om.bc)
    o.percol_bc = dict(om.percol_bc)
    for (f, k), (kind, v) in om.bc.items():
        if kind != M.BC_DIRICHLET or (f, k) in om.percol_bc:
            continue
        val = bcv[0, f, k] + (bcv[1, f, k] - bcv[0, f, k]) * s
        if np.ndim(val) == 0:
            o.bc[(f, k)] = (kind, float(val))
        else:
            o.percol_bc[(f, k)] = np.ascontiguousarray(val)
    return o


stage_solve = IR.stage_solve   # Newton on Y - w - coef f(Y) = 0 to round-off: (Y, iterations per column)
error_norm = core.error_norm


def attempt(om, yn, fn, ti, t, h, bcv=None, t0=0.0, t1=1.0):
    """One TR-BDF2 step of every column from (yn, fn) at times t with steps h (per column).  Returns
    (Y_1, f_{n+1}, error estimate e, Newton iterations)."""
    h = np.asarray(h, dtype=np.float64)
    og, o1 = _with_bc(om, bcv, t0, t1, t + GAMMA * h), _with_bc(om, bcv, t0, t1, t + h)
    return core.richards_attempt(lambda y, w, c: stage_solve(og, y, w, ti, c), lambda y, w, c: stage_solve(o1, y, w, ti, c),
                                 lambda y, c: IR.fd_jacobian(o1, y, ti, c, IR.tendency(o1, y, ti)), yn, fn, h)


def trbdf2(om, vl, ti, t0, t1, dt, adaptive=True, abstol=1e-6, reltol=1e-3, bcv=None, h0=None,
           max_steps=100000):
    """Integrate the [ncols, nlev] state (Float64) from t0 to t1.  Fixed mode: steps of dt, the last one
    clipped onto t1.  Adaptive: per-column step control from h0 (default dt).  Returns (state, info) with
    info = dict(t, h, accepted, rejected, failed) per column."""
    y = np.array(vl, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.float64)
    fn = IR.tendency(_with_bc(om, bcv, t0, t1, t0), y, ti)
    h = np.full(y.shape[0], float(dt)) if h0 is None else np.array(h0, dtype=np.float64)

    def one(state, f, t, hh):
        y1, f1, e, _ = attempt(om, state[0], f[0], ti, t, hh, bcv, t0, t1)
        return (y1,), (f1,), error_norm(e, state[0], y1, abstol, reltol) if adaptive else None, None

    (y,), info = core.adaptive_loop(one, (y,), (fn,), t0, t1, h, max_steps, adaptive)
    return y, info
