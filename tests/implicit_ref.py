"""NumPy backward-Euler reference for Richards columns, built on the CPU oracle's tendency.

Per step, Newton on R(v) = v - v_n - dt f(v) = 0 with f = oracle_py.rhs (the oracle-pinned
tendency), a finite-difference tridiagonal Jacobian (three coloured evaluations: cells i = k mod 3
are perturbed together, a Richards tendency of cell i depends on cells i-1, i, i+1 only) and the
safeguard of the device stepper: the applied change of a cell is at most
DMAX_FRAC (nu - theta_r), a cell moves at most half way to theta_r, and a cell that crosses
nu - theta_i from below stops there; a column whose Newton step stops shrinking takes half
steps until it shrinks again.  Iterates to round-off:
until the update stops shrinking or is zero.

Test infrastructure (tests/test_implicit_reference.py, tests/test_gpu_implicit.py)."""
from __future__ import annotations

import numpy as np

import parity_cases as pc

O = pc.O
DMAX_FRAC = 0.5   # the device's bound on one Newton update, in units of nu - theta_r
STALL = 0.9       # the device's rule: a Newton step larger than STALL x the previous one halves the next update


def _col_param(om, ncols, key, scalar):
    a = om.percol.get(key)
    return np.full(ncols, scalar) if a is None else np.asarray(a, dtype=np.float64)


def tendency(om, vl, ti):
    return O.rhs(om, np.ascontiguousarray(vl), np.ascontiguousarray(ti))["vl"]


def residual(om, vl, vn, ti, dt):
    return vl - vn - dt * tendency(om, vl, ti)


def thomas(a, b, c, d):
    """Solve the tridiagonal systems a_i x_{i-1} + b_i x_i + c_i x_{i+1} = d_i, one per row."""
    n = b.shape[1]
    cp = np.zeros_like(b)
    dp = np.zeros_like(b)
    cp[:, 0] = c[:, 0] / b[:, 0]
    dp[:, 0] = d[:, 0] / b[:, 0]
    for i in range(1, n):
        den = b[:, i] - a[:, i] * cp[:, i - 1]
        cp[:, i] = c[:, i] / den
        dp[:, i] = (d[:, i] - a[:, i] * dp[:, i - 1]) / den
    x = np.zeros_like(b)
    x[:, -1] = dp[:, -1]
    for i in range(n - 2, -1, -1):
        x[:, i] = dp[:, i] - cp[:, i] * x[:, i + 1]
    return x


def fd_jacobian(om, vl, ti, dt, f0):
    """Bands (a, b, c) of J = I - dt df/dv by coloured forward differences."""
    ncols, n = vl.shape
    nu = _col_param(om, ncols, "nu", om.soil.nu)[:, None]
    a, b, c = np.zeros_like(vl), np.ones_like(vl), np.zeros_like(vl)
    for k in range(3):
        mask = (np.arange(n) % 3 == k)[None, :]
        h = np.sqrt(np.finfo(vl.dtype).eps) * np.maximum(np.abs(vl), nu)
        # perturb towards the dry side when the cell sits on the wet side of the kink at S = 1
        h = np.where(vl >= nu, -h, h) * mask
        df = (tendency(om, vl + h, ti) - f0)
        for i in range(n):
            if not mask[0, i]:
                continue
            hi = h[:, i]
            b[:, i] -= dt * df[:, i] / hi
            if i > 0:
                c[:, i - 1] = -dt * df[:, i - 1] / hi
            if i + 1 < n:
                a[:, i + 1] = -dt * df[:, i + 1] / hi
    return a, b, c


def implicit_euler(om, vl, ti, dt, nsteps, max_iter=120):
    """nsteps backward-Euler steps of the [ncols, nlev] state (Float64).  Returns (state, iterations
    per step [nsteps, ncols])."""
    vl = np.array(vl, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.float64)
    ncols = vl.shape[0]
    nu = _col_param(om, ncols, "nu", om.soil.nu)[:, None]
    tr = _col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None]
    dmax = DMAX_FRAC * (nu - tr)
    iters = np.zeros((nsteps, ncols), dtype=np.int64)
    for s in range(nsteps):
        vn = vl.copy()
        active = np.ones(ncols, dtype=bool)
        prev = np.full(ncols, np.inf)
        lam = np.ones((ncols, 1))
        for it in range(max_iter):
            f0 = tendency(om, vl, ti)
            R = vl - vn - dt * f0
            a, b, c = fd_jacobian(om, vl, ti, dt, f0)
            d = thomas(a, b, c, -R)
            new = vl + np.clip(lam * d, -dmax, dmax)
            floor = tr + 0.5 * (vl - tr)
            new = np.where(vl > tr, np.maximum(new, floor), np.maximum(new, vl))
            # the saturation kink: a cell that crosses nu_eff from below stops there
            nue = nu - ti
            new = np.where((vl < nue) & (new > nue), nue, new)
            step = np.max(np.abs(d), axis=1)   # the Newton step itself, not what the safeguard let through
            upd = active[:, None]
            vl = np.where(upd, new, vl)
            iters[s, active] = it + 1
            # round-off: the update is zero or has stopped shrinking (after having become small)
            done = (step == 0) | ((step >= 0.5 * prev) & (step < 1e-12))
            stall = (step > STALL * prev)[:, None]
            lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
            prev = np.where(active, step, prev)
            active &= ~done
            if not active.any():
                break
    return vl, iters
