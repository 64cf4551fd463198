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

Test infrastructure (tests/test_trbdf2_reference.py, tests/test_gpu_trbdf2.py)."""
from __future__ import annotations

import copy

import numpy as np

import case_model as M
import implicit_ref as IR

GAMMA = 2.0 - np.sqrt(2.0)
D = GAMMA / 2.0
B = ((1.0 - np.sqrt(2.0)) / 3.0, 1.0 / 3.0, (np.sqrt(2.0) - 2.0) / 3.0)
HMIN_FRAC = 1e-10


def _col_param(om, ncols, key, scalar):
    return IR._col_param(om, ncols, key, scalar)


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


def stage_solve(om, y0, w, ti, coef, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: one per column), to round-off, with the
    device's safeguard.  Returns (Y, iterations per column)."""
    vl = np.array(y0, dtype=np.float64)
    ncols = vl.shape[0]
    coef = np.broadcast_to(np.asarray(coef, dtype=np.float64), (ncols,)).copy()
    nu = _col_param(om, ncols, "nu", om.soil.nu)[:, None]
    tr = _col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None]
    dmax = IR.DMAX_FRAC * (nu - tr)
    iters = np.zeros(ncols, dtype=np.int64)
    active = np.ones(ncols, dtype=bool)
    prev = np.full(ncols, np.inf)
    lam = np.ones((ncols, 1))
    for it in range(max_iter):
        f0 = IR.tendency(om, vl, ti)
        R = vl - w - coef[:, None] * f0
        a, b, c = IR.fd_jacobian(om, vl, ti, coef, f0)
        d = IR.thomas(a, b, c, -R)
        new = vl + np.clip(lam * d, -dmax, dmax)
        floor = tr + 0.5 * (vl - tr)
        new = np.where(vl > tr, np.maximum(new, floor), np.maximum(new, vl))
        nue = nu - ti
        new = np.where((vl < nue) & (new > nue), nue, new)
        step = np.max(np.abs(d), axis=1)
        vl = np.where(active[:, None], new, vl)
        iters[active] = it + 1
        done = (step == 0) | ((step >= 0.5 * prev) & (step < 1e-12))
        stall = (step > IR.STALL * prev)[:, None]
        lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
        prev = np.where(active, step, prev)
        active &= ~done
        if not active.any():
            break
    return vl, iters


def attempt(om, yn, fn, ti, t, h, bcv=None, t0=0.0, t1=1.0):
    """One TR-BDF2 step of every column from (yn, fn) at times t with steps h (per column).  Returns
    (Y_1, f_{n+1}, error estimate e, Newton iterations)."""
    h = np.asarray(h, dtype=np.float64)
    dh = D * h
    w1 = yn + dh[:, None] * fn
    yg, i1 = stage_solve(_with_bc(om, bcv, t0, t1, t + GAMMA * h), yn, w1, ti, dh)
    w2 = (yg - (1.0 - GAMMA) ** 2 * yn) / (GAMMA * (2.0 - GAMMA))
    om2 = _with_bc(om, bcv, t0, t1, t + h)
    y1, i2 = stage_solve(om2, yg, w2, ti, dh)
    zg = (yg - w1) / D
    z1 = (y1 - w2) / D
    rhs = B[0] * (h[:, None] * fn) + B[1] * zg + B[2] * z1
    f1 = IR.tendency(om2, y1, ti)
    a, b, c = IR.fd_jacobian(om2, y1, ti, dh, f1)
    e = IR.thomas(a, b, c, rhs)
    return y1, z1 / h[:, None], e, i1 + i2


def error_norm(e, yn, y1, abstol, reltol):
    sc = abstol + reltol * np.maximum(np.abs(yn), np.abs(y1))
    return np.sqrt(np.mean((e / sc) ** 2, axis=1))


def trbdf2(om, vl, ti, t0, t1, dt, adaptive=True, abstol=1e-6, reltol=1e-3, bcv=None, h0=None,
           max_steps=100000):
    """Integrate the [ncols, nlev] state (Float64) from t0 to t1.  Fixed mode: steps of dt, the last one
    clipped onto t1.  Adaptive: per-column step control from h0 (default dt).  Returns (state, info) with
    info = dict(t, h, accepted, rejected, failed) per column."""
    y = np.array(vl, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.float64)
    ncols = y.shape[0]
    fn = IR.tendency(_with_bc(om, bcv, t0, t1, t0), y, ti)
    t = np.full(ncols, float(t0))
    h = np.full(ncols, float(dt)) if h0 is None else np.array(h0, dtype=np.float64)
    acc = np.zeros(ncols, dtype=np.int64)
    rej = np.zeros(ncols, dtype=np.int64)
    failed = np.zeros(ncols, dtype=bool)
    hmin = HMIN_FRAC * (t1 - t0)
    for _ in range(max_steps):
        act = (t < t1) & ~failed
        if not act.any():
            break
        clip = t + h * (1.0 + 1e-10) >= t1
        hh = np.where(clip, t1 - t, h)
        hh = np.where(act, hh, 1.0)   # (inactive columns: any positive step, not committed)
        y1, f1, e, _ = attempt(om, y, fn, ti, t, hh, bcv, t0, t1)
        if adaptive:
            E = error_norm(e, y, y1, abstol, reltol)
            with np.errstate(divide="ignore"):
                fac = 0.9 * E ** (-1.0 / 3.0)
            fac = np.where(np.isnan(fac), 0.2, np.clip(fac, 0.2, 5.0))
            ok = E <= 1.0
        else:
            fac = np.ones(ncols)
            ok = np.ones(ncols, dtype=bool)
        good = act & ok
        bad = act & ~ok
        y = np.where(good[:, None], y1, y)
        fn = np.where(good[:, None], f1, fn)
        t = np.where(good, np.where(clip, t1, t + hh), t)
        if adaptive:
            hn = np.where(clip & (fac >= 1.0), np.maximum(hh * fac, h), hh * fac)
            h = np.where(act, hn, h)
        acc += good
        rej += bad
        failed |= bad & ~(h >= hmin)
    return y, dict(t=t, h=h, accepted=acc, rejected=rej, failed=failed)
