"""NumPy backward Euler and TR-BDF2 for layered soils (per-cell soil classes), built on the layered tendency
of tests/layered_ref.py: tests/implicit_ref.py and tests/trbdf2_ref.py restated with the column constants
taken per cell.

Per stage, Newton on Y - w - coef f(Y) = 0 with f = layered_ref.rhs, a finite-difference tridiagonal Jacobian
(three coloured evaluations) and the device's safeguard with every cell's own class: the applied change of a
cell is at most DMAX_FRAC (nu - theta_r) of ITS class, a cell moves at most half way to ITS theta_r, and a cell
that crosses ITS nu - theta_i from below stops there; the stall rule is per column.  Iterates to round-off.
TR-BDF2's stages, error estimate and controller are trbdf2_ref's.  Float64 only; boundary values are the
model's constants.

Test infrastructure (tests/test_layered_implicit_reference.py, tests/test_gpu_layered_implicit.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

import layered_ref as R
from implicit_ref import DMAX_FRAC, STALL, thomas
from trbdf2_ref import B, D, GAMMA, HMIN_FRAC, error_norm


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
    n = vl.shape[1]
    a, b, c = np.zeros_like(vl), np.ones_like(vl), np.zeros_like(vl)
    for k in range(3):
        mask = (np.arange(n) % 3 == k)[None, :]
        h = np.sqrt(np.finfo(vl.dtype).eps) * np.maximum(np.abs(vl), nu)
        # perturb towards the dry side when the cell sits on the wet side of the kink at S = 1
        h = np.where(vl >= nu, -h, h) * mask
        df = tendency(lay, vl + h) - f0
        for i in range(k, n, 3):
            hi = h[:, i]
            b[:, i] -= coef * df[:, i] / hi
            if i > 0:
                c[:, i - 1] = -coef * df[:, i - 1] / hi
            if i + 1 < n:
                a[:, i + 1] = -coef * df[:, i + 1] / hi
    return a, b, c


def stage_solve(lay, y0, w, coef, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: scalar or one per column), to round-off, with
    the device's per-cell safeguard.  Returns (Y, iterations per column)."""
    vl = np.array(y0, dtype=np.float64)
    ncols = vl.shape[0]
    coef = np.broadcast_to(np.asarray(coef, dtype=np.float64), (ncols,)).copy()
    p = R.cell_params(lay)
    nu, tr = p["nu"], p["theta_r"]
    ti = np.asarray(lay.case.ti, dtype=np.float64)
    dmax = DMAX_FRAC * (nu - tr)
    iters = np.zeros(ncols, dtype=np.int64)
    active = np.ones(ncols, dtype=bool)
    prev = np.full(ncols, np.inf)
    lam = np.ones((ncols, 1))
    for it in range(max_iter):
        f0 = tendency(lay, vl)
        Rv = vl - w - coef[:, None] * f0
        a, b, c = fd_jacobian(lay, vl, coef, f0, nu)
        d = thomas(a, b, c, -Rv)
        new = vl + np.clip(lam * d, -dmax, dmax)
        floor = tr + 0.5 * (vl - tr)
        new = np.where(vl > tr, np.maximum(new, floor), np.maximum(new, vl))
        nue = nu - ti
        new = np.where((vl < nue) & (new > nue), nue, new)
        step = np.max(np.abs(d), axis=1)   # the Newton step itself, not what the safeguard let through
        vl = np.where(active[:, None], new, vl)
        iters[active] = it + 1
        # round-off: the update is zero or has stopped shrinking (after having become small)
        done = (step == 0) | ((step >= 0.5 * prev) & (step < 1e-12))
        stall = (step > STALL * prev)[:, None]
        lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
        prev = np.where(active, step, prev)
        active &= ~done
        if not active.any():
            break
    return vl, iters


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
    h = np.asarray(h, dtype=np.float64)
    dh = D * h
    w1 = yn + dh[:, None] * fn
    yg, i1 = stage_solve(lay, yn, w1, dh)
    w2 = (yg - (1.0 - GAMMA) ** 2 * yn) / (GAMMA * (2.0 - GAMMA))
    y1, i2 = stage_solve(lay, yg, w2, dh)
    zg = (yg - w1) / D
    z1 = (y1 - w2) / D
    rhs = B[0] * (h[:, None] * fn) + B[1] * zg + B[2] * z1
    a, b, c = fd_jacobian(lay, y1, dh, tendency(lay, y1), R.cell_params(lay)["nu"])
    e = thomas(a, b, c, rhs)
    return y1, z1 / h[:, None], e, i1 + i2


def trbdf2(lay, t0, t1, dt, adaptive=True, abstol=1e-6, reltol=1e-3, h0=None, vl=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (Float64) from t0 to t1.  Fixed mode: steps of dt, the last one
    clipped onto t1.  Adaptive: per-column step control from h0 (default dt).  Returns (state, info) with
    info = dict(t, h, accepted, rejected, failed) per column."""
    y = np.array(lay.case.vl if vl is None else vl, dtype=np.float64)
    ncols = y.shape[0]
    fn = tendency(lay, y)
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
        y1, f1, e, _ = attempt(lay, y, fn, hh)
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
