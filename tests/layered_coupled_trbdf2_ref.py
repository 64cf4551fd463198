"""NumPy reference for adaptive TR-BDF2 of a LAYERED coupled model (lh_integrate_layered_coupled_trbdf2, DESIGN
section 4.26): tests/coupled_trbdf2_ref.py's attempt / error_norm / step_factor / integrate over
tests/layered_coupled_implicit_ref.py's tendencies, finite-difference water Jacobian and exact energy bands.

Per column, with gamma = 2 - sqrt 2, d = gamma / 2, the column's step h and both components in Y:
  stage 1: Y_g - w1 - d h f(Y_g, t + gamma h) = 0,  w1 = Y_n + d h f_n
  stage 2: Y_1 - w2 - d h f(Y_1, t + h) = 0,        w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
each stage block triangular (f_w reads no rhoe_int, f_e is affine in it at fixed water, also with classes): the
water by the safeguarded Newton with every cell's own nu and theta_r, the energy by one tridiagonal solve at the new
water state.  z = (Y - w) / d, f_n+1 = z_1 / h.  Error estimate: r = b1 h f_n + b2 z_g + b3 z_1 in both components,
filtered by the diagonal blocks of I - d h J(Y_1) (block="diagonal", the device's) or by the whole block-triangular
matrix (block="full", J_ew e_w by a central difference); E, the controller and the landing on t1 are
coupled_trbdf2_ref's.  Boundary values: None (the case's) or bcv [2][2][2] = [t0 | t1][face][component], linear in
time; where the columns' stage times differ only Dirichlet values may change in time (per-column values).

newton: None iterates the water stages to round-off; (kappa, abstol, reltol, cap) stops them by the device's rule,
max_i |delta_i| / (abstol + reltol |Y_i|) <= kappa within cap iterations.  round_to: coupled_trbdf2_ref.attempt's.

Pure NumPy: imports neither the oracle nor the library's kernels.

Test infrastructure (tests/test_layered_coupled_trbdf2_reference.py, tests/test_gpu_layered_coupled_trbdf2.py)."""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import layered_ref as R
from implicit_ref import DMAX_FRAC, STALL, thomas

GAMMA = LC.GAMMA
D = LC.D
B = ((1.0 - np.sqrt(2.0)) / 3.0, 1.0 / 3.0, (np.sqrt(2.0) - 2.0) / 3.0)
HMIN_FRAC = 1e-10
ABSTOL, RELTOL = 1e-6, 1e-3
NEWTON_KAPPA, NEWTON_MAX = 0.01, 10   # the library's stage Newton test


def abstol_e_default(lay):
    """1e-6 rho_l c_l: the energy of 1e-6 K in water."""
    e = lay.case.om.earth
    return 1e-6 * (e.cp_l * e.rho_liq)


def device_newton(abstol=ABSTOL, reltol=RELTOL, kappa=NEWTON_KAPPA, cap=NEWTON_MAX):
    return (kappa, abstol, reltol, cap)


def with_bc(lay, bcv, t0, t1, t):
    """The Float64 twin of `lay` with its boundary values at time(s) t (a scalar, or one per column) interpolated
    from bcv: layered_coupled_implicit_ref.with_bc where t is one time; per-column Dirichlet values otherwise."""
    if bcv is None:
        return LC.with_bc(lay, None)
    b = np.asarray(bcv, dtype=np.float64).reshape(2, 2, 2)
    s = (np.asarray(t, dtype=np.float64) - t0) / (t1 - t0) if t1 > t0 else np.ones_like(np.asarray(t, dtype=np.float64))
    if np.ndim(s) == 0:
        return LC.with_bc(lay, b[0] + (b[1] - b[0]) * float(s))
    l64 = LH.as64(lay)
    om = copy.copy(l64.case.om)
    om.bc, om.percol_bc = dict(om.bc), dict(om.percol_bc)
    for (f, k), (kind, v) in l64.case.om.bc.items():
        if kind == M.BC_DIRICHLET and (f, k) not in l64.case.om.percol_bc:
            om.percol_bc[(f, k)] = np.ascontiguousarray(b[0, f, k] + (b[1, f, k] - b[0, f, k]) * s)
        elif kind == M.BC_FLUX:
            assert b[0, f, k] == b[1, f, k], "a flux that changes in time needs columns that agree in their stage times"
            om.bc[(f, k)] = (kind, float(b[0, f, k]))
    return LH.LayeredHeat(dataclasses.replace(l64.case, om=om), l64.classes, l64.thermal, l64.class_map)


def water_stage(l64, y0, w, coef, newton=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y0, coef one per column:
    layered_coupled_implicit_ref.newton_stage's iteration (the safeguard with every cell's own nu, theta_r) with
    coupled_trbdf2_ref.water_stage's two stopping rules.  Returns (Y, iterations [ncols], converged [ncols])."""
    vl = np.array(y0, dtype=np.float64)
    ncols = vl.shape[0]
    coef = np.broadcast_to(np.asarray(coef, dtype=np.float64), (ncols,)).copy()
    max_iter = 120 if newton is None else newton[3]
    p = R.cell_params(l64)
    nu, tr = p["nu"].astype(np.float64), p["theta_r"].astype(np.float64)
    ti = np.asarray(l64.case.ti, dtype=np.float64)
    dmax = DMAX_FRAC * (nu - tr)
    iters = np.zeros(ncols, dtype=np.int64)
    conv = np.zeros(ncols, dtype=bool)
    active = np.ones(ncols, dtype=bool)
    prev = np.full(ncols, np.inf)
    lam = np.ones((ncols, 1))
    for it in range(max_iter):
        f0 = LC.water_tendency(l64, vl)
        Rv = vl - w - coef[:, None] * f0
        a, b, c = LC._fd_jacobian(l64, vl, coef, f0, nu)
        d = thomas(a, b, c, -Rv)
        new = vl + np.clip(lam * d, -dmax, dmax)
        floor = tr + 0.5 * (vl - tr)
        new = np.where(vl > tr, np.maximum(new, floor), np.maximum(new, vl))
        nue = nu - ti
        new = np.where((vl < nue) & (new > nue), nue, new)
        step = np.max(np.abs(d), axis=1)
        vl = np.where(active[:, None], new, vl)
        iters[active] = it + 1
        if newton is None:
            done = (step == 0) | ((step >= 0.5 * prev) & (step < 1e-12))
        else:
            kappa, atol, rtol, _ = newton
            done = np.all(np.abs(d) <= kappa * (atol + rtol * np.abs(new)), axis=1)
        conv |= active & done
        stall = (step > STALL * prev)[:, None]
        lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
        prev = np.where(active, step, prev)
        active &= ~done
        if not active.any():
            break
    return vl, iters, conv


def energy_solve(l64, vl, rhs, coef, homogeneous=False):
    """(I - coef A) x = rhs + coef f0 at the water state vl, f_e(rhoe) = A rhoe + f0 (coef one per column);
    homogeneous: (I - coef A) x = rhs."""
    (lo, di, up), f0 = LC.energy_bands(l64, vl)
    c = np.broadcast_to(np.asarray(coef, dtype=np.float64), (vl.shape[0],))[:, None]
    return thomas(-c * lo, 1.0 - c * di, -c * up, rhs if homogeneous else rhs + c * f0)


def attempt(lay, vn, en, fvn, fen, t, h, bcv=None, t0=0.0, t1=1.0, newton=None, block="diagonal", round_to=None):
    """One TR-BDF2 step of every column from (vn, en) with tendencies (fvn, fen) at times t with steps h (scalars
    or one per column): coupled_trbdf2_ref.attempt's formulas, arguments (theta_i is the case's) and result."""
    ncols = vn.shape[0]
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (ncols,)).copy()
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (ncols,)).copy()
    if np.all(t == t[0]) and np.all(h == h[0]):
        tg, te = float(t[0] + GAMMA * h[0]), float(t[0] + h[0])   # (scalar boundary values where the columns agree)
    else:
        tg, te = t + GAMMA * h, t + h
    dh = rnd(D * h)
    c = dh[:, None]
    og = with_bc(lay, bcv, t0, t1, tg)
    w1v = rnd(vn + rnd(c * fvn))
    vg, i1, c1 = water_stage(og, vn, w1v, dh, newton)
    vg = rnd(vg)
    w1e = rnd(en + rnd(c * fen))
    eg = rnd(energy_solve(og, vg, w1e, dh))
    k2 = 1.0 / (GAMMA * (2.0 - GAMMA))
    wv = rnd(rnd(vg - rnd((1.0 - GAMMA) ** 2 * vn)) * k2)
    we = rnd(rnd(eg - rnd((1.0 - GAMMA) ** 2 * en)) * k2)
    o1 = og if bcv is None else with_bc(lay, bcv, t0, t1, te)
    v1, i2, c2 = water_stage(o1, vg, wv, dh, newton)
    v1 = rnd(v1)
    e1 = rnd(energy_solve(o1, v1, we, dh))
    hc = h[:, None]
    rv = B[0] * (hc * fvn) + B[1] * (vg - w1v) / D + B[2] * (v1 - wv) / D
    re = B[0] * (hc * fen) + B[1] * (eg - w1e) / D + B[2] * (e1 - we) / D
    f1 = LC.water_tendency(o1, v1)
    nu = R.cell_params(o1)["nu"].astype(np.float64)
    a, b, cc = LC._fd_jacobian(o1, v1, dh, f1, nu)
    ev = thomas(a, b, cc, rv)
    rhs_e = re
    if block == "full":   # + d h J_ew e_w: f_e along e_w at (v1, e1), central difference
        s = 1e-3 * np.max(np.abs(v1)) / max(float(np.max(np.abs(ev))), 1e-300)
        s = min(s, 1.0)
        jew = (LC.tendencies(o1, v1 + s * ev, e1)[1] - LC.tendencies(o1, v1 - s * ev, e1)[1]) / (2.0 * s)
        rhs_e = re + c * jew
    else:
        assert block == "diagonal"
    ee = energy_solve(o1, v1, rhs_e, dh, homogeneous=True)
    return dict(v1=v1, e1=e1, fv1=rnd(rnd(v1 - wv) / c), fe1=rnd(rnd(e1 - we) / c), ev=ev, ee=ee, rv=rv, re=re, iters=i1 + i2,
                conv=c1 & c2)


def error_norm(ev, ee, vn, v1, en, e1, abstol, abstol_e, reltol):
    qw = ev / (abstol + reltol * np.maximum(np.abs(vn), np.abs(v1)))
    qe = ee / (abstol_e + reltol * np.maximum(np.abs(en), np.abs(e1)))
    return np.sqrt((np.sum(qw ** 2, axis=1) + np.sum(qe ** 2, axis=1)) / (2 * ev.shape[1]))


def step_factor(E):
    """The controller's h_new / h: clamp(0.9 E^(-1/3), 0.2, 5), 0.2 for a NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = 0.9 * np.asarray(E, dtype=np.float64) ** (-1.0 / 3.0)
    return np.where(np.isnan(fac), 0.2, np.clip(fac, 0.2, 5.0))


def first_attempt(lay, h, bcv=None, newton=None, block="diagonal", round_to=None, abstol=ABSTOL, abstol_e=None, reltol=RELTOL):
    """One attempt of h (a call over [0, h]) from the case's own state: (the attempt's dict, E per column)."""
    v, e = LC.state64(lay)
    fv, fe = LC.tendencies(with_bc(lay, bcv, 0.0, h, 0.0), v, e)
    r = attempt(lay, v, e, fv, fe, 0.0, h, bcv, 0.0, h, newton, block, round_to)
    E = error_norm(r["ev"], r["ee"], v, r["v1"], e, r["e1"], abstol, abstol_e_default(lay) if abstol_e is None else abstol_e,
                   reltol)
    return r, E


def integrate(lay, vl, rhoe, t0, t1, dt, abstol=ABSTOL, abstol_e=None, reltol=RELTOL, bcv=None, h0=None, newton=None,
              round_to=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (vl, rhoe) of `lay` from t0 to t1, every column with its own t and h from h0
    (default dt).  Returns (vl, rhoe, info), info = dict(t, h, accepted, rejected, failed) per column."""
    v, e = np.array(vl, dtype=np.float64), np.array(rhoe, dtype=np.float64)
    ncols = v.shape[0]
    if abstol_e is None:
        abstol_e = abstol_e_default(lay)
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    fv, fe = (rnd(f) for f in LC.tendencies(with_bc(lay, bcv, t0, t1, float(t0)), v, e))
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
        hh = np.where(act, hh, hh[act][0])   # (inactive columns: an active column's step, not committed)
        ta = np.where(act, t, t[act][0])
        r = attempt(lay, v, e, fv, fe, ta, hh, bcv, t0, t1, newton, round_to=round_to)
        E = error_norm(r["ev"], r["ee"], v, r["v1"], e, r["e1"], abstol, abstol_e, reltol)
        fac = np.where(r["conv"], step_factor(E), 0.25)
        ok = r["conv"] & (E <= 1.0)
        good, bad = act & ok, act & ~ok
        g = good[:, None]
        v, e = np.where(g, r["v1"], v), np.where(g, r["e1"], e)
        fv, fe = np.where(g, r["fv1"], fv), np.where(g, r["fe1"], fe)
        t = np.where(good, np.where(clip, t1, t + hh), t)
        hn = np.where(clip & (fac >= 1.0) & ok, np.maximum(hh * fac, h), hh * fac)
        h = np.where(act, hn, h)
        acc += good
        rej += bad
        failed |= bad & ~(h >= hmin)
    return v, e, dict(t=t, h=h, accepted=acc, rejected=rej, failed=failed)


# ------------------------------------------------------------------ cases shared by the two test files

SPAN = 64.0   # the integrations' span in stable steps
CASES = {   # layered_coupled_implicit_ref.layered_case's arguments: (ncols, nlev, kind, hyd (top, bottom), energy, ice)
    "A": (8, 24, "horizons", (M.BC_FLUX, M.BC_FREE_DRAINAGE), "dirichlet", True),
    "B": (8, 12, "cells", (M.BC_FLUX, M.BC_FLUX), "flux", True),
    "C": (8, 12, "cells", (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), "dirichlet", False),
    "D": (8, 24, "horizons", (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), "mixed", True),
}


def make_case(name, dtype=np.float64, ncols=None, nlev=None):
    nc, nl, kind, hyd, energy, ice = CASES[name]
    return LC.layered_case(dtype, nc if ncols is None else ncols, nl if nlev is None else nlev, kind=kind, hyd=hyd, energy=energy,
                           ice=ice)


_SSPRK33 = {}


def ssprk33_reference(name, lay, span=SPAN, div=4):
    """(vl, rhoe) of layered_heat_ref.ssprk33 at sd / div over span stable steps on the Float64 twin; computed once
    per key and never modified."""
    key = (name, lay.case.ncols, lay.case.om.nlev, np.dtype(lay.case.dtype).name, span, div)
    if key not in _SSPRK33:
        sd = LC.stable_dt(lay)
        ref = LH.ssprk33(LH.as64(lay), sd / div, int(round(div * span)))
        _SSPRK33[key] = (ref["vl"].astype(np.float64), ref["rhoe"].astype(np.float64))
    return _SSPRK33[key]


_INTEGRATED = {}


def integrated(name, lay, reltol, round_to=None, span=SPAN):
    """integrate() over span stable steps from h0 = the stable step under the device's Newton rule; computed once per
    key and never modified."""
    key = (name, lay.case.ncols, lay.case.om.nlev, np.dtype(lay.case.dtype).name, reltol, None if round_to is None else np.dtype(round_to).name,
           span)
    if key not in _INTEGRATED:
        sd = LC.stable_dt(lay)
        v, e = LC.state64(lay)
        _INTEGRATED[key] = integrate(lay, v, e, 0.0, span * sd, sd, reltol=reltol, newton=device_newton(reltol=reltol),
                                     round_to=round_to)
    return _INTEGRATED[key]
