"""The algorithm text the NumPy references of the implicit integrators share, stated once: the Thomas solve, the
coloured forward-difference bands, the safeguarded Newton stage with its three stopping rules, the TR-BDF2 constants
and controller, the per-column accept / reject loop, and the coupled family's attempt, error norm and energy solve
over a provider.  The tests/*_ref.py modules supply what differs (tendencies, boundary values, the safeguard's nu,
theta_r, theta_i, rounding) and bind their public names to these functions.

Pure NumPy: imports nothing of the project, so the layered references stay free of the oracle and the library.

Test infrastructure."""
from __future__ import annotations

import numpy as np

DMAX_FRAC = 0.5   # the device's bound on one Newton update, in units of nu - theta_r
STALL = 0.9       # the device's rule: a Newton step larger than STALL x the previous one halves the next update
GAMMA = 2.0 - np.sqrt(2.0)
D = GAMMA / 2.0
B = ((1.0 - np.sqrt(2.0)) / 3.0, 1.0 / 3.0, (np.sqrt(2.0) - 2.0) / 3.0)
HMIN_FRAC = 1e-10


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


def sample(bcv, k, w=None):
    """Sample k of a table of boundary values [nsteps + 1][2 faces][2 components], or (1 - w) v_k + w v_k+1."""
    if bcv is None:
        return None
    b = np.asarray(bcv, dtype=np.float64)
    return b[k] if w is None else (1.0 - w) * b[k] + w * b[k + 1]


def rounder(dtype):
    """a -> a rounded through dtype (None: the identity)"""
    return (lambda a: a) if dtype is None else (lambda a: np.asarray(a).astype(dtype).astype(np.float64))


def fd_bands(f, vl, coef, f0, nu):
    """Bands (a, b, c) of J = I - coef df/dv by coloured forward differences: three evaluations of the tendency f,
    cells i = k mod 3 perturbed together (f_i reads cells i-1, i, i+1 only).  coef: scalar or one per column; nu
    broadcasts to [ncols, nlev] (one per column or one per cell)."""
    n = vl.shape[1]
    a, b, c = np.zeros_like(vl), np.ones_like(vl), np.zeros_like(vl)
    for k in range(3):
        mask = (np.arange(n) % 3 == k)[None, :]
        h = np.sqrt(np.finfo(vl.dtype).eps) * np.maximum(np.abs(vl), nu)
        # perturb towards the dry side when the cell sits on the wet side of the kink at S = 1
        h = np.where(vl >= nu, -h, h) * mask
        df = f(vl + h) - f0
        for i in range(k, n, 3):
            hi = h[:, i]
            b[:, i] -= coef * df[:, i] / hi
            if i > 0:
                c[:, i - 1] = -coef * df[:, i - 1] / hi
            if i + 1 < n:
                a[:, i + 1] = -coef * df[:, i + 1] / hi
    return a, b, c


# The three stopping rules of the Newton stage: rule(d, step, prev, new, nu) -> done [ncols], with d the Newton step,
# step = max_i |d_i|, prev the previous iteration's step, new the safeguarded iterate.

def round_off(d, step, prev, new, nu):
    """the update is zero or has stopped shrinking (after having become small)"""
    return (step == 0) | ((step >= 0.5 * prev) & (step < 1e-12))


def fixed_step_rule(tol):
    """the fixed-step entries' rule on the Newton step itself: max_i |d_i| <= tol max(|Y_i|, nu)"""
    return lambda d, step, prev, new, nu: np.all(np.abs(d) <= tol * np.maximum(np.abs(new), nu), axis=1)


def adaptive_rule(kappa, abstol, reltol):
    """the adaptive entries' rule: max_i |d_i| / (abstol + reltol |Y_i|) <= kappa"""
    return lambda d, step, prev, new, nu: np.all(np.abs(d) <= kappa * (abstol + reltol * np.abs(new)), axis=1)


def newton_stage(f, nu, tr, ti, coef, y0, w, stop=round_off, max_iter=120):
    """Newton on Y - w - coef f(Y) = 0 from the guess y0 (coef: scalar or one per column) with the device's safeguard
    (DESIGN section 4.12): the applied change of a cell is at most DMAX_FRAC (nu - theta_r), a cell moves at most
    half way to theta_r, a cell that crosses nu - theta_i from below stops there, and a column whose Newton step
    stops shrinking takes half steps until it shrinks again.  nu, tr broadcast to [ncols, nlev].  Returns
    (Y, iterations [ncols], converged [ncols])."""
    vl = np.array(y0, dtype=np.float64)
    ncols = vl.shape[0]
    coef = np.broadcast_to(np.asarray(coef, dtype=np.float64), (ncols,)).copy()
    dmax = DMAX_FRAC * (nu - tr)
    iters = np.zeros(ncols, dtype=np.int64)
    conv = np.zeros(ncols, dtype=bool)
    active = np.ones(ncols, dtype=bool)
    prev = np.full(ncols, np.inf)
    lam = np.ones((ncols, 1))
    for it in range(max_iter):
        f0 = f(vl)
        R = vl - w - coef[:, None] * f0
        a, b, c = fd_bands(f, vl, coef, f0, nu)
        d = thomas(a, b, c, -R)
        new = vl + np.clip(lam * d, -dmax, dmax)
        floor = tr + 0.5 * (vl - tr)
        new = np.where(vl > tr, np.maximum(new, floor), np.maximum(new, vl))
        # the saturation kink: a cell that crosses nu_eff from below stops there
        nue = nu - ti
        new = np.where((vl < nue) & (new > nue), nue, new)
        step = np.max(np.abs(d), axis=1)   # the Newton step itself, not what the safeguard let through
        vl = np.where(active[:, None], new, vl)
        iters[active] = it + 1
        done = stop(d, step, prev, new, nu)
        conv |= active & done
        stall = (step > STALL * prev)[:, None]
        lam = np.where(stall, np.maximum(0.5 * lam, 1.0 / 16), np.minimum(2.0 * lam, 1.0))
        prev = np.where(active, step, prev)
        active &= ~done
        if not active.any():
            break
    return vl, iters, conv


def richards_attempt(solve_g, solve_1, bands_1, yn, fn, h):
    """One TR-BDF2 step of every column of a one-component state from (yn, fn) with steps h (per column).
    solve_g / solve_1 (guess, w, coef) -> (Y, iterations): the stage solves at t + gamma h and t + h; bands_1(Y_1,
    coef): the bands of I - coef J(Y_1) at t + h.  Returns (Y_1, f_{n+1}, error estimate e, Newton iterations)."""
    h = np.asarray(h, dtype=np.float64)
    dh = D * h
    w1 = yn + dh[:, None] * fn
    yg, i1 = solve_g(yn, w1, dh)
    w2 = (yg - (1.0 - GAMMA) ** 2 * yn) / (GAMMA * (2.0 - GAMMA))
    y1, i2 = solve_1(yg, w2, dh)
    zg = (yg - w1) / D
    z1 = (y1 - w2) / D
    rhs = B[0] * (h[:, None] * fn) + B[1] * zg + B[2] * z1
    a, b, c = bands_1(y1, dh)
    e = thomas(a, b, c, rhs)
    return y1, z1 / h[:, None], e, i1 + i2


def error_norm(e, yn, y1, abstol, reltol):
    sc = abstol + reltol * np.maximum(np.abs(yn), np.abs(y1))
    return np.sqrt(np.mean((e / sc) ** 2, axis=1))


def step_factor(E):
    """The controller's h_new / h: clamp(0.9 E^(-1/3), 0.2, 5), 0.2 for a NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = 0.9 * np.asarray(E, dtype=np.float64) ** (-1.0 / 3.0)
    return np.where(np.isnan(fac), 0.2, np.clip(fac, 0.2, 5.0))


def adaptive_loop(attempt, state, fn, t0, t1, h, max_steps, adaptive=True, cap_fails=False):
    """The per-column accept / reject loop of TR-BDF2 from t0 to t1.  state, fn: tuples of [ncols, nlev] planes (Y_n
    and f_n, one per component); h [ncols]: the first proposals.  attempt(state, fn, t, hh) -> (candidate, f_n+1,
    E [ncols], converged [ncols] or None); a stage that did not converge rejects the step with h / 4.  Inactive
    columns (finished or failed) are attempted with an active column's t and step and not committed.
    adaptive=False: every step is accepted and h untouched (fixed steps, the last one clipped onto t1; E is not read).
    A column still short of t1 after max_steps attempts is left where it is, and marked failed where cap_fails.
    Returns (state, info), info = dict(t, h, accepted, rejected, failed) per column."""
    ncols = h.shape[0]
    t = np.full(ncols, float(t0))
    acc = np.zeros(ncols, dtype=np.int64)
    rej = np.zeros(ncols, dtype=np.int64)
    failed = np.zeros(ncols, dtype=bool)
    hmin = HMIN_FRAC * (t1 - t0)
    while True:
        capped = (t < t1) & (acc + rej >= max_steps)   # (every column still stepping has attempted every round)
        if cap_fails:
            failed |= capped
        act = (t < t1) & ~failed & ~capped
        if not act.any():
            break
        clip = t + h * (1.0 + 1e-10) >= t1
        hh = np.where(clip, t1 - t, h)
        hh = np.where(act, hh, hh[act][0])
        ta = np.where(act, t, t[act][0])
        cand, f1, E, conv = attempt(state, fn, ta, hh)
        if adaptive:
            fac, ok = step_factor(E), E <= 1.0
            if conv is not None:
                fac, ok = np.where(conv, fac, 0.25), conv & ok
        else:
            fac, ok = np.ones(ncols), np.ones(ncols, dtype=bool)
        good, bad = act & ok, act & ~ok
        g = good[:, None]
        state = tuple(np.where(g, c, s) for c, s in zip(cand, state))
        fn = tuple(np.where(g, c, s) for c, s in zip(f1, fn))
        t = np.where(good, np.where(clip, t1, t + hh), t)
        if adaptive:   # a clipped step that could have grown (fac >= 1, so accepted) does not shrink the proposal
            hn = np.where(clip & (fac >= 1.0), np.maximum(hh * fac, h), hh * fac)
            h = np.where(act, hn, h)
        acc += good
        rej += bad
        failed |= bad & ~(h >= hmin)
    return state, dict(t=t, h=h, accepted=acc, rejected=rej, failed=failed)


# ------------------------------------------------------------------ the coupled family (water + energy)

class CoupledProblem:
    """What differs between the coupled references, as callables on a model `o` at one stage time (the pattern of
    heat_trbdf2_ref.Problem):  at(bcv, t0, t1, t) -> o with the boundary values of time(s) t;  water_tendency(o, vl);
    tendencies(o, vl, rhoe) -> (f_w, f_e);  energy_bands(o, vl) -> ((lo, di, up), f0) of the affine f_e;
    safeguard(o) -> (nu, theta_r, theta_i) of the Newton stage."""

    def __init__(self, at, water_tendency, tendencies, energy_bands, safeguard):
        self.at, self.water_tendency, self.tendencies = at, water_tendency, tendencies
        self.energy_bands, self.safeguard = energy_bands, safeguard


def water_stage(P, o, y0, w, coef, newton=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y0.  newton: None (to round-off, at most 120
    iterations) or (kappa, abstol, reltol, cap).  Returns (Y, iterations [ncols], converged [ncols])."""
    nu, tr, ti = P.safeguard(o)
    stop, cap = (round_off, 120) if newton is None else (adaptive_rule(*newton[:3]), newton[3])
    return newton_stage(lambda v: P.water_tendency(o, v), nu, tr, ti, coef, y0, w, stop, cap)


def energy_solve(P, o, vl, rhs, coef, homogeneous=False):
    """(I - coef A) x = rhs + coef f0 at the water state vl, f_e(rhoe) = A rhoe + f0 (coef: scalar or one per
    column); homogeneous: (I - coef A) x = rhs."""
    (lo, di, up), f0 = P.energy_bands(o, vl)
    c = np.broadcast_to(np.asarray(coef, dtype=np.float64), (vl.shape[0],))[:, None]
    return thomas(-c * lo, 1.0 - c * di, -c * up, rhs if homogeneous else rhs + c * f0)


def coupled_attempt(P, vn, en, fvn, fen, t, h, bcv=None, t0=0.0, t1=1.0, newton=None, block="diagonal", round_to=None):
    """One TR-BDF2 step of every column from (vn, en) with tendencies (fvn, fen) at times t with steps h (scalars
    or one per column).  Returns a dict: v1, e1 (Y_1), fv1, fe1 (f_n+1), ev, ee (the filtered estimate), rv, re
    (the unfiltered one), iters, conv (both water stages).  round_to: a dtype to which everything the device keeps
    in a plane of its working type is rounded -- the stage outputs, w1, w2 and f_n+1, each after every operation
    that forms it -- and d h: what working in that type costs (None: nothing is rounded)."""
    ncols = vn.shape[0]
    rnd = rounder(round_to)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (ncols,)).copy()
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (ncols,)).copy()
    if np.all(t == t[0]) and np.all(h == h[0]):
        tg, te = t[0] + GAMMA * h[0], t[0] + h[0]   # (scalar boundary values where the columns agree)
    else:
        tg, te = t + GAMMA * h, t + h
    dh = rnd(D * h)
    c = dh[:, None]
    og = P.at(bcv, t0, t1, tg)
    w1v = rnd(vn + rnd(c * fvn))
    vg, i1, c1 = water_stage(P, og, vn, w1v, dh, newton)
    vg = rnd(vg)
    w1e = rnd(en + rnd(c * fen))
    eg = rnd(energy_solve(P, og, vg, w1e, dh))
    k2 = 1.0 / (GAMMA * (2.0 - GAMMA))
    wv = rnd(rnd(vg - rnd((1.0 - GAMMA) ** 2 * vn)) * k2)
    we = rnd(rnd(eg - rnd((1.0 - GAMMA) ** 2 * en)) * k2)
    o1 = P.at(bcv, t0, t1, te)
    v1, i2, c2 = water_stage(P, o1, vg, wv, dh, newton)
    v1 = rnd(v1)
    e1 = rnd(energy_solve(P, o1, v1, we, dh))
    hc = h[:, None]
    rv = B[0] * (hc * fvn) + B[1] * (vg - w1v) / D + B[2] * (v1 - wv) / D
    re = B[0] * (hc * fen) + B[1] * (eg - w1e) / D + B[2] * (e1 - we) / D
    f1 = P.water_tendency(o1, v1)
    a, b, cc = fd_bands(lambda v: P.water_tendency(o1, v), v1, dh, f1, P.safeguard(o1)[0])
    ev = thomas(a, b, cc, rv)
    rhs_e = re
    if block == "full":   # + d h J_ew e_w: f_e along e_w at (v1, e1), central difference
        s = 1e-3 * np.max(np.abs(v1)) / max(float(np.max(np.abs(ev))), 1e-300)
        s = min(s, 1.0)
        jew = (P.tendencies(o1, v1 + s * ev, e1)[1] - P.tendencies(o1, v1 - s * ev, e1)[1]) / (2.0 * s)
        rhs_e = re + c * jew
    else:
        assert block == "diagonal"
    ee = energy_solve(P, o1, v1, rhs_e, dh, homogeneous=True)
    return dict(v1=v1, e1=e1, fv1=rnd(rnd(v1 - wv) / c), fe1=rnd(rnd(e1 - we) / c), ev=ev, ee=ee, rv=rv, re=re, iters=i1 + i2,
                conv=c1 & c2)


def coupled_error_norm(ev, ee, vn, v1, en, e1, abstol, abstol_e, reltol):
    qw = ev / (abstol + reltol * np.maximum(np.abs(vn), np.abs(v1)))
    qe = ee / (abstol_e + reltol * np.maximum(np.abs(en), np.abs(e1)))
    return np.sqrt((np.sum(qw ** 2, axis=1) + np.sum(qe ** 2, axis=1)) / (2 * ev.shape[1]))


def coupled_integrate(P, vl, rhoe, t0, t1, dt, abstol, abstol_e, reltol, bcv=None, h0=None, newton=None, round_to=None,
                      max_steps=100000):
    """Integrate the [ncols, nlev] state (vl, rhoe) from t0 to t1, every column with its own t and h from h0
    (default dt).  Returns (vl, rhoe, info), info = dict(t, h, accepted, rejected, failed) per column."""
    v, e = np.array(vl, dtype=np.float64), np.array(rhoe, dtype=np.float64)
    rnd = rounder(round_to)
    fn = tuple(rnd(f) for f in P.tendencies(P.at(bcv, t0, t1, float(t0)), v, e))
    h = np.full(v.shape[0], float(dt)) if h0 is None else np.array(h0, dtype=np.float64)

    def attempt(state, fn, t, hh):
        r = coupled_attempt(P, *state, *fn, t, hh, bcv, t0, t1, newton, round_to=round_to)
        E = coupled_error_norm(r["ev"], r["ee"], state[0], r["v1"], state[1], r["e1"], abstol, abstol_e, reltol)
        return (r["v1"], r["e1"]), (r["fv1"], r["fe1"]), E, r["conv"]

    (v, e), info = adaptive_loop(attempt, (v, e), fn, t0, t1, h, max_steps)
    return v, e, info
