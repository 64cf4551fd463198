"""NumPy reference for adaptive TR-BDF2 of the coupled model (lh_integrate_coupled_trbdf2),
built on tests/coupled_implicit_ref.py: its oracle tendencies, its finite-difference water Jacobian and its exact
energy bands.

Per column, with gamma = 2 - sqrt 2, d = gamma / 2, the column's step h and both components in Y:
  stage 1: Y_g - w1 - d h f(Y_g, t + gamma h) = 0,  w1 = Y_n + d h f_n
  stage 2: Y_1 - w2 - d h f(Y_1, t + h) = 0,        w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
each stage block triangular: the water by the safeguarded Newton, the energy by one tridiagonal solve at the new
water state.  z = (Y - w) / d, f_n+1 = z_1 / h.  Error estimate: r = b1 h f_n + b2 z_g + b3 z_1 in both components,
filtered by the diagonal blocks of I - d h J(Y_1):
  (I - d h J_ww) e_w = r_w,   (I - d h J_ee) e_e = r_e     (block="diagonal", the device's)
or by the whole block-triangular matrix, (I - d h J_ee) e_e = r_e + d h J_ew e_w with J_ew e_w by a central
difference (block="full"), or not at all (the unfiltered r is returned as well).
  E = sqrt((sum q_w^2 + sum q_e^2) / (2 nlev)),  q_w = e_w / (abstol + reltol max(|v_n|, |v_1|)),
                                                 q_e = e_e / (abstol_e + reltol max(|rhoe_n|, |rhoe_1|))
and the controller of tests/trbdf2_ref.py (the device's).  Boundary values: None (the model's) or bcv [2][2][2] =
[t0 | t1][face][component], linear in time, both components.

newton: None iterates the water stages to round-off; (kappa, abstol, reltol, cap) stops them by the device's rule,
max_i |delta_i| / (abstol + reltol |Y_i|) <= kappa within cap iterations (a stage that does not get there rejects
the step with h / 4).

Test infrastructure (tests/test_coupled_trbdf2_reference.py, tests/test_gpu_coupled_trbdf2.py)."""
from __future__ import annotations

import numpy as np

import coupled_implicit_ref as CR
import implicit_ref as R
import trbdf2_ref as TR

GAMMA, D, B, HMIN_FRAC = TR.GAMMA, TR.D, TR.B, TR.HMIN_FRAC
ABSTOL, RELTOL = 1e-6, 1e-3
NEWTON_KAPPA, NEWTON_MAX = 0.01, 10   # the library's stage Newton test


def abstol_e_default(om):
    """1e-6 rho_l c_l: the energy of 1e-6 K in water."""
    return 1e-6 * (om.earth.cp_l * om.earth.rho_liq)


def device_newton(abstol=ABSTOL, reltol=RELTOL):
    return (NEWTON_KAPPA, abstol, reltol, NEWTON_MAX)


def water_stage(om, y0, w, ti, coef, newton=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y0, coef one per column (coupled_implicit_ref's
    Newton with the stopping rule above).  Returns (Y, iterations [ncols], converged [ncols])."""
    vl = np.array(y0, dtype=np.float64)
    ncols = vl.shape[0]
    coef = np.broadcast_to(np.asarray(coef, dtype=np.float64), (ncols,)).copy()
    max_iter = 120 if newton is None else newton[3]
    nu = R._col_param(om, ncols, "nu", om.soil.nu)[:, None]
    tr = R._col_param(om, ncols, "vg_theta_r", om.vg.theta_r)[:, None]
    dmax = R.DMAX_FRAC * (nu - tr)
    iters = np.zeros(ncols, dtype=np.int64)
    conv = np.zeros(ncols, dtype=bool)
    active = np.ones(ncols, dtype=bool)
    prev = np.full(ncols, np.inf)
    lam = np.ones((ncols, 1))
    for it in range(max_iter):
        f0 = CR.water_tendency(om, vl, ti)
        Rv = vl - w - coef[:, None] * f0
        a, b, c = CR._fd_jacobian(om, vl, ti, coef, f0)
        d = R.thomas(a, b, c, -Rv)
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
        stall = (step > R.STALL * prev)[:, None]
        lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
        prev = np.where(active, step, prev)
        active &= ~done
        if not active.any():
            break
    return vl, iters, conv


def energy_solve(om, vl, ti, rhs, coef, homogeneous=False):
    """(I - coef A) x = rhs + coef f0 at the water state vl, f_e(rhoe) = A rhoe + f0 (coef one per column);
    homogeneous: (I - coef A) x = rhs."""
    (lo, di, up), f0 = CR.energy_bands(om, vl, ti)
    c = np.broadcast_to(np.asarray(coef, dtype=np.float64), (vl.shape[0],))[:, None]
    return R.thomas(-c * lo, 1.0 - c * di, -c * up, rhs if homogeneous else rhs + c * f0)


def attempt(om, vn, en, fvn, fen, ti, t, h, bcv=None, t0=0.0, t1=1.0, newton=None, block="diagonal", round_to=None):
    """One TR-BDF2 step of every column from (vn, en) with tendencies (fvn, fen) at times t with steps h (scalars
    or one per column).  Returns a dict: v1, e1 (Y_1), fv1, fe1 (f_n+1), ev, ee (the filtered estimate), rv, re
    (the unfiltered one), iters, conv (both water stages).  round_to: a dtype to which everything the device keeps
    in a plane of its working type is rounded -- the stage outputs, w1, w2 and f_n+1, each after every operation
    that forms it -- and d h: what working in that type costs (None: nothing is rounded)."""
    ncols = vn.shape[0]
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (ncols,)).copy()
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (ncols,)).copy()
    if bcv is not None and np.all(t == t[0]) and np.all(h == h[0]):
        t, tg, te = t[0], t[0] + GAMMA * h[0], t[0] + h[0]   # (scalar boundary values where the columns agree)
    else:
        tg, te = t + GAMMA * h, t + h
    dh = rnd(D * h)
    c = dh[:, None]
    og = TR._with_bc(om, bcv, t0, t1, tg)
    w1v = rnd(vn + rnd(c * fvn))
    vg, i1, c1 = water_stage(og, vn, w1v, ti, dh, newton)
    vg = rnd(vg)
    w1e = rnd(en + rnd(c * fen))
    eg = rnd(energy_solve(og, vg, ti, w1e, dh))
    k2 = 1.0 / (GAMMA * (2.0 - GAMMA))
    wv = rnd(rnd(vg - rnd((1.0 - GAMMA) ** 2 * vn)) * k2)
    we = rnd(rnd(eg - rnd((1.0 - GAMMA) ** 2 * en)) * k2)
    o1 = TR._with_bc(om, bcv, t0, t1, te)
    v1, i2, c2 = water_stage(o1, vg, wv, ti, dh, newton)
    v1 = rnd(v1)
    e1 = rnd(energy_solve(o1, v1, ti, we, dh))
    hc = h[:, None]
    rv = B[0] * (hc * fvn) + B[1] * (vg - w1v) / D + B[2] * (v1 - wv) / D
    re = B[0] * (hc * fen) + B[1] * (eg - w1e) / D + B[2] * (e1 - we) / D
    f1 = CR.water_tendency(o1, v1, ti)
    a, b, cc = CR._fd_jacobian(o1, v1, ti, dh, f1)
    ev = R.thomas(a, b, cc, rv)
    rhs_e = re
    if block == "full":   # + d h J_ew e_w: f_e along e_w at (v1, e1), central difference
        s = 1e-3 * np.max(np.abs(v1)) / max(float(np.max(np.abs(ev))), 1e-300)
        s = min(s, 1.0)
        jew = (CR.energy_tendency(o1, v1 + s * ev, ti, e1) - CR.energy_tendency(o1, v1 - s * ev, ti, e1)) / (2.0 * s)
        rhs_e = re + c * jew
    else:
        assert block == "diagonal"
    ee = energy_solve(o1, v1, ti, rhs_e, dh, homogeneous=True)
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


def integrate(om, vl, ti, rhoe, t0, t1, dt, abstol=ABSTOL, abstol_e=None, reltol=RELTOL, bcv=None, h0=None,
              newton=None, round_to=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (vl, rhoe) from t0 to t1, every column with its own t and h from h0
    (default dt).  Returns (vl, rhoe, info), info = dict(t, h, accepted, rejected, failed) per column."""
    v, e, ti = np.array(vl, dtype=np.float64), np.array(rhoe, dtype=np.float64), np.asarray(ti, dtype=np.float64)
    ncols = v.shape[0]
    if abstol_e is None:
        abstol_e = abstol_e_default(om)
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    fv, fe = (rnd(f) for f in CR.tendencies(TR._with_bc(om, bcv, t0, t1, t0), v, ti, e))
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
        r = attempt(om, v, e, fv, fe, ti, ta, hh, bcv, t0, t1, newton, round_to=round_to)
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
