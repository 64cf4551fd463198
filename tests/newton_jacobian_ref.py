"""Closed-form Newton Jacobian of the implicit Richards solvers, J = I - dt df/dv, in plain NumPy (Float64).

f is the Richards water tendency every implicit integrator solves against (lh_implicit.hpp, lh_layered_implicit.hpp and
the water stage of the two coupled calls): with cells numbered from the bottom, dz the uniform spacing and
npsi = -psi,
  interior face, lower cell first:  F = -(K_lo + K_hi) ((npsi_lo - npsi_hi) + dz) / (2 dz^2)
  boundary faces:                   F = f_w / dz, f_w a flux, -K_c (free drainage) or the Dirichlet face's
                                    K_f (psi_f - psi_c +- dz/2) / (dz/2) with its sign conventions
  f_i = F_(i-1/2) - F_(i+1/2)
  K = Ksat sqrt(S) (1 - (1 - S^(1/m))^m)^2,  S = (v - theta_r) / (nu - theta_r)           (1 where S >= 1)
  psi = -(Se^(-1/m) - 1)^(1/n) / alpha,      Se = (v - theta_r) / (nu - theta_i - theta_r) (where Se < 1)
  psi = (v - (nu - theta_i)) / S_s                                                        (where Se >= 1)
and a cell at or below theta_r + eps(FT) is clamped: its K and psi are constants.  Every cell takes its own
parameters (a scalar, a per-column array or its class's), so the slopes of a face are those of its two cells.

Slopes, with t = S^(1/m), w = 1 - t, inner = 1 - w^m:
  dK/dv    = Ksat / (nu - theta_r) (K_r / (2 S) + 2 sqrt(S) inner w^(m-1) t / S)   (0 where S >= 1 or clamped)
  dnpsi/dv = -npsi / (n m w_e (v - theta_r)), w_e = 1 - Se^(1/m)                   (-1/S_s where Se >= 1, 0 clamped)
`dtype=np.float32` evaluates these two slopes (and nothing else) in Float32 arithmetic, as the device does on
purpose; dK_scale / dn_scale multiply them (the mutants the sensitivity tests feed the assertion).

Nothing here reads the oracle or the library: tests/test_newton_jacobian_reference.py compares the bands with central
differences of the oracle's tendency, tests/test_gpu_newton_jacobian.py the device's first Newton update with them.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import case_model as M

FIELDS = ("n", "alpha", "theta_r", "Ksat", "nu", "S_s")
DMAX_FRAC = 0.5   # the device's bound on one Newton update, in units of nu - theta_r (LH_IMPLICIT_DMAX_FRAC)


@dataclass
class Problem:
    """One ensemble of columns: the six parameters of every cell [ncols, nlev], the state, the grid spacing, the
    hydrology boundary kinds and per-column values (bottom, top), the bottom sign convention and eps of the
    working type (the clamp)."""
    p: dict
    vl: np.ndarray
    ti: np.ndarray
    dz: float
    kinds: tuple
    values: tuple
    consistent: bool
    eps: float


def _bc(om, face, ncols):
    kind, val = om.bc.get((face, M.COMP_HYDROLOGY), (M.BC_NONE, 0.0))
    pc = om.percol_bc.get((face, M.COMP_HYDROLOGY))
    return kind, (np.full(ncols, float(val)) if pc is None else np.asarray(pc, dtype=np.float64))


def _problem(case, p):
    om = case.om
    ncols = case.vl.shape[0]
    kb, vb = _bc(om, M.FACE_BOTTOM, ncols)
    kt, vt = _bc(om, M.FACE_TOP, ncols)
    return Problem(p, np.asarray(case.vl, dtype=np.float64), np.asarray(case.ti, dtype=np.float64),
                   (om.zmax - om.zmin) / om.nlev, (kb, kt), (vb, vt), bool(om.consistent_bottom_sign),
                   float(np.finfo(case.dtype).eps))


def problem_of_case(case):
    """A workloads.Case with scalar or per-column parameters (CaseModel.vg, .soil, .percol)."""
    om = case.om
    ncols, nlev = case.vl.shape
    scalar = dict(n=om.vg.n, alpha=om.vg.alpha, theta_r=om.vg.theta_r, Ksat=om.vg.Ksat, nu=om.soil.nu, S_s=om.soil.S_s)
    key = dict(n="vg_n", alpha="vg_alpha", theta_r="vg_theta_r", Ksat="vg_Ksat", nu="nu", S_s="S_s")
    p = {}
    for k in FIELDS:
        a = om.percol.get(key[k])
        col = np.full(ncols, float(scalar[k])) if a is None else np.asarray(a, dtype=np.float64)
        p[k] = np.repeat(col[:, None], nlev, axis=1)
    return _problem(case, p)


def problem_of_layered(lay):
    """A layered case (layered_ref.Layered or layered_heat_ref.LayeredHeat): classes [ncls, 6] in FIELDS order and
    a class map [ncols, nlev]."""
    cls = np.asarray(lay.classes, dtype=np.float64)
    m = np.asarray(lay.class_map)
    if m.ndim == 1:
        m = np.broadcast_to(m[None, :], lay.case.vl.shape)
    return _problem(lay.case, {k: np.ascontiguousarray(cls[m, j]) for j, k in enumerate(FIELDS)})


# ------------------------------------------------------------------ closures and their slopes

def closures(p, v, ti, eps, dtype=np.float64, dK_scale=1.0, dn_scale=1.0):
    """(K, npsi, dK/dv, dnpsi/dv) of cells with parameters p at (v, ti): values in Float64, the two slopes in
    `dtype` arithmetic (returned as Float64)."""
    n, alpha, thr, Ksat, nu, S_s = (np.asarray(p[k], dtype=np.float64) for k in FIELDS)
    v, ti = np.asarray(v, dtype=np.float64), np.asarray(ti, dtype=np.float64)
    m = 1.0 - 1.0 / n
    clamped = v <= thr + eps
    num = np.where(clamped, (thr + eps) - thr, v - thr)
    por, por_e = nu - thr, nu - ti - thr
    with np.errstate(all="ignore"):
        S = num / por
        unsat = S < 1.0
        Su = np.where(unsat, S, 0.5)
        t = Su ** (1.0 / m)
        inner = 1.0 - (1.0 - t) ** m
        K = Ksat * np.where(unsat, np.sqrt(Su) * inner * inner, 1.0)
        unsat_e = num < por_e
        Se = np.where(unsat_e, num / por_e, 0.5)
        npsi = np.where(unsat_e, (Se ** (-1.0 / m) - 1.0) ** (1.0 / n) / alpha, ((nu - ti) - v) / S_s)
        # the slopes, in `dtype`
        ft = np.dtype(dtype).type
        c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
        one, two, half = ft(1), ft(2), ft(0.5)
        m_, im_, n_ = c(m), c(1.0 / m), c(n)
        num_ = c(num)
        S_ = num_ * c(1.0 / por)
        S_ = np.where(unsat, S_, half)
        t_ = np.exp2(np.log2(S_) * im_)
        w_ = one - t_
        wm_ = np.exp2(np.log2(w_) * m_)
        inner_ = one - wm_
        sS_ = np.sqrt(S_)
        dkr = c(1.0 / por) * (half * sS_ * inner_ * inner_ / S_ + two * sS_ * inner_ * wm_ * t_ / (w_ * S_))
        pe_ = c(por_e)
        Se_ = np.where(unsat_e, num_ / pe_, half)
        we_ = one - np.exp2(np.log2(Se_) * im_)
        dnu = -c(npsi) / (n_ * m_ * we_ * num_)
        dK = Ksat * np.where(unsat, dkr.astype(np.float64), 0.0)
        dn = np.where(unsat_e, dnu.astype(np.float64), -1.0 / S_s)
    dK = np.where(clamped, 0.0, dK) * dK_scale
    dn = np.where(clamped, 0.0, dn) * dn_scale
    return K, npsi, dK, dn


def _boundary(pr, face, K_c, np_c, dK_c, dn_c):
    """(F, dF/dv_c) of one boundary face, F = f_w / dz, from the boundary cell's values and slopes."""
    i = 0 if face == M.FACE_BOTTOM else -1
    kind, val = pr.kinds[0 if face == M.FACE_BOTTOM else 1], pr.values[0 if face == M.FACE_BOTTOM else 1]
    dz, dzb = pr.dz, pr.dz / 2.0
    if kind == M.BC_FLUX:
        return val / dz, np.zeros_like(K_c)
    if kind == M.BC_FREE_DRAINAGE:
        return -K_c / dz, -dK_c / dz
    if kind == M.BC_DIRICHLET:
        at = {k: a[:, i] for k, a in pr.p.items()}
        K_f, np_f, _, _ = closures(at, val, pr.ti[:, i], pr.eps)
        psi_f, psi_c = -np_f, -np_c
        if face == M.FACE_BOTTOM:
            g = (psi_f - psi_c - dzb) if pr.consistent else (psi_f - psi_c + dzb)
            return K_f * g / dzb / dz, K_f * dn_c / dzb / dz
        return -K_f * (psi_f - psi_c + dzb) / dzb / dz, -K_f * dn_c / dzb / dz
    raise ValueError("the hydrology component needs a boundary condition at both faces")


def tendency_and_slopes(pr, vl=None, dtype=np.float64, dK_scale=1.0, dn_scale=1.0):
    """(f, df_i/dv_(i-1), df_i/dv_i, df_i/dv_(i+1)), each [ncols, nlev], at the state vl (default: the problem's)."""
    v = pr.vl if vl is None else np.asarray(vl, dtype=np.float64)
    ncols, n = v.shape
    K, npsi, dK, dn = closures(pr.p, v, pr.ti, pr.eps, dtype, dK_scale, dn_scale)
    F = np.zeros((ncols, n + 1))
    dF_lo = np.zeros((ncols, n + 1))   # d F_k / d v of the cell below face k
    dF_hi = np.zeros((ncols, n + 1))   # d F_k / d v of the cell above face k
    F[:, 0], dF_hi[:, 0] = _boundary(pr, M.FACE_BOTTOM, K[:, 0], npsi[:, 0], dK[:, 0], dn[:, 0])
    F[:, n], dF_lo[:, n] = _boundary(pr, M.FACE_TOP, K[:, -1], npsi[:, -1], dK[:, -1], dn[:, -1])
    if n > 1:
        cg = 1.0 / (2.0 * pr.dz * pr.dz)
        h = (npsi[:, :-1] - npsi[:, 1:]) + pr.dz
        Ks = K[:, :-1] + K[:, 1:]
        F[:, 1:n] = -Ks * h * cg
        dF_lo[:, 1:n] = -cg * (dK[:, :-1] * h + Ks * dn[:, :-1])
        dF_hi[:, 1:n] = -cg * (dK[:, 1:] * h - Ks * dn[:, 1:])
    f = F[:, :-1] - F[:, 1:]
    lo = np.zeros((ncols, n))
    up = np.zeros((ncols, n))
    lo[:, 1:] = dF_lo[:, 1:n]
    up[:, :-1] = -dF_hi[:, 1:n]
    di = dF_hi[:, :-1] - dF_lo[:, 1:]
    return f, lo, di, up


def bands(pr, dt, vl=None, dtype=np.float64, dK_scale=1.0, dn_scale=1.0):
    """The bands (a, b, c) of J = I - dt df/dv: row i is a_i x_(i-1) + b_i x_i + c_i x_(i+1)."""
    _, lo, di, up = tendency_and_slopes(pr, vl, dtype, dK_scale, dn_scale)
    return -dt * lo, 1.0 - dt * di, -dt * up


# ------------------------------------------------------------------ tridiagonal helpers

def tri_apply(a, b, c, x):
    y = b * x
    y[:, 1:] += a[:, 1:] * x[:, :-1]
    y[:, :-1] += c[:, :-1] * x[:, 1:]
    return y


def tri_abs_apply(a, b, c, x):
    return tri_apply(np.abs(a), np.abs(b), np.abs(c), np.abs(x))


def tri_solve(a, b, c, d):
    """Thomas' algorithm, one system per row of the arrays."""
    n = b.shape[1]
    cp, dp = np.zeros_like(b), np.zeros_like(b)
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


def newton_update(pr, dt, f, **kw):
    """d of the first Newton iteration from the problem's state: J d = dt f, with J from bands(**kw)."""
    a, b, c = bands(pr, dt, **kw)
    return tri_solve(a, b, c, dt * np.asarray(f, dtype=np.float64))


def residual_and_scale(J, d, dtf):
    """(r [ncols, nlev], s [ncols, nlev]): r = J d - dt f, s_i = sum_j |dt df_i/dv_j| |d_j| + |d_i|."""
    a, b, c = J
    r = tri_apply(a, b, c, d) - dtf
    s = tri_abs_apply(a, b - 1.0, c, d) + np.abs(d)
    return r, s


def q(J, d, dtf):
    """Per column: max_i |r_i| / max_i s_i."""
    r, s = residual_and_scale(J, d, dtf)
    return np.max(np.abs(r), axis=1) / np.max(s, axis=1)


def allowance(J, B, d, y1, dtf, eps):
    """The bound of the device assertion, per cell: B max_i s_i + 64 eps sum_j |J_ij| max(|Y1_j|, |dt f_j|)."""
    _, s = residual_and_scale(J, d, dtf)
    big = np.maximum(np.abs(y1), np.abs(dtf))
    return B * np.max(s, axis=1, keepdims=True) + 64.0 * eps * tri_abs_apply(*J, big)


def safeguard_inactive(pr, d):
    """Per cell: Newton's safeguard (the dmax clip, the half-way-to-theta_r rule, the stop on nu - theta_i) leaves
    the update d alone, with a factor 2 in hand; and no unsaturated cell is so near its kink (Se > 0.98) that a
    Float32 slope stops being a slope."""
    p, v = pr.p, pr.vl
    nue = p["nu"] - pr.ti
    por_e = nue - p["theta_r"]
    unsat = (v - p["theta_r"]) < por_e
    ad = np.abs(d)
    ok = 2.0 * ad <= DMAX_FRAC * (p["nu"] - p["theta_r"])
    ok &= d >= -0.25 * (v - p["theta_r"])
    ok &= ~unsat | (nue - v > 2.0 * ad)
    ok &= ~unsat | ((v - p["theta_r"]) <= 0.98 * por_e)
    return ok
