"""Closed-form Newton Jacobian of the implicit Richards solvers WITH conductivity factors (lh_factors_implicit.hpp),
J = I - dt df/dv, in plain NumPy (Float64): tests/newton_jacobian_ref.py with

  K = F K_NoEffect,  F = visc imp,  visc = exp(gamma (T - T_ref)),  imp = 10^(-Omega f_i),
  theta_l = min(v, nu - theta_i),  f_i = theta_i / (theta_l + theta_i)
  dK/dv = F dK_NoEffect/dv + K Omega ln10 theta_i / (theta_l + theta_i)^2     (second term only where v < nu - theta_i)

T is prescribed and theta_i constant, so visc is a constant of every cell; imp reads the cell's own RAW v (a cell
clamped at theta_r + eps has a constant K_NoEffect and psi and still the impedance term); on and above nu - theta_i the
impedance slope is 0, the side psi's slope takes there; theta_i = 0 gives imp = 1 and slope 0.  psi has no factor.  A
Dirichlet face state takes the boundary cell's theta_i and T with the face's own vartheta_l, and is a constant of the
step.  K_NoEffect, psi and their slopes are newton_jacobian_ref.closures, imported: nothing of it is edited.

`dtype=np.float32` evaluates the slopes -- F and the impedance term included -- in Float32 arithmetic, as the device
does on purpose.  Mutants for the sensitivity tests: dK_scale / dn_scale as there, and `mutant` =
"no_impedance_term" (the second term dropped), "no_viscosity_on_dK" (F without visc on dK_NoEffect),
"impedance_term_above" (the second term kept on and above nu - theta_i).

Nothing here reads the oracle or the library: tests/test_factors_implicit_reference.py compares the tendency and the
bands with the oracle, tests/test_gpu_factors_implicit.py the device's first Newton update with the bands."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import case_model as M
import newton_jacobian_ref as NJ
from newton_jacobian_ref import (DMAX_FRAC, allowance, q, residual_and_scale, safeguard_inactive, tri_abs_apply,  # noqa: F401
                                 tri_apply, tri_solve)

LN10, LOG2_10, LOG2_E = np.log(10.0), np.log2(10.0), np.log2(np.e)
MUTANTS = ("no_impedance_term", "no_viscosity_on_dK", "impedance_term_above")


@dataclass
class Problem(NJ.Problem):
    """newton_jacobian_ref.Problem with the prescribed temperature [ncols, nlev] and the factors (case_model.CondFactors)."""
    T: np.ndarray = None
    cf: M.CondFactors = None


def problem_of_case(case):
    """A workloads.Case with scalar or per-column parameters, conductivity factors (om.cf) and T_aux."""
    pr = NJ.problem_of_case(case)
    return Problem(**vars(pr), T=np.asarray(case.T_aux, dtype=np.float64), cf=case.om.cf)


def closures(pr, p, v, ti, T, dtype=np.float64, dK_scale=1.0, dn_scale=1.0, mutant=None):
    """(K, npsi, dK/dv, dnpsi/dv) with the factors of pr.cf, of cells with parameters p at (v, ti, T): values in
    Float64, the slopes in `dtype` arithmetic (returned as Float64)."""
    assert mutant is None or mutant in MUTANTS
    cf = pr.cf
    K0, npsi, dK0, dn = NJ.closures(p, v, ti, pr.eps, dtype, dK_scale, dn_scale)
    v, ti, T = (np.asarray(a, dtype=np.float64) for a in (v, ti, T))
    nue = np.asarray(p["nu"], dtype=np.float64) - ti
    below = v < nue
    tl = np.where(below, v, nue)
    with np.errstate(all="ignore"):
        visc = np.exp(cf.gamma * (T - cf.T_ref)) if cf.viscosity_kind else np.ones_like(v)
        imp = 10.0 ** (-cf.Omega * ti / (tl + ti)) if cf.impedance_kind else np.ones_like(v)
        K = K0 * visc * imp
        # the slopes' factors, in `dtype`
        ft = np.dtype(dtype).type
        c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
        visc_ = np.exp2(c(cf.gamma * (T - cf.T_ref)) * ft(LOG2_E)) if cf.viscosity_kind else np.ones_like(c(v))
        imp_, g_ = np.ones_like(c(v)), np.zeros_like(c(v))
        if cf.impedance_kind:
            ti_, itw_, Om_ = c(ti), ft(1) / (c(tl) + c(ti)), ft(cf.Omega)
            imp_ = np.exp2((-Om_ * (ti_ * itw_)) * ft(LOG2_10))
            g_ = (Om_ * ft(LN10)) * ti_ * itw_ * itw_
            if mutant != "impedance_term_above":
                g_ = np.where(below, g_, ft(0))
            if mutant == "no_impedance_term":
                g_ = np.zeros_like(g_)
        F_ = imp_ if mutant == "no_viscosity_on_dK" else visc_ * imp_
        dK = F_.astype(np.float64) * dK0 + K * g_.astype(np.float64)
    return K, npsi, dK, dn


def _boundary(pr, face, K_c, np_c, dK_c, dn_c):
    """(F, dF/dv_c) of one boundary face, F = f_w / dz: newton_jacobian_ref._boundary with the face state's K_f from
    the boundary cell's theta_i and T."""
    b = 0 if face == M.FACE_BOTTOM else 1
    i = 0 if face == M.FACE_BOTTOM else -1
    kind, val = pr.kinds[b], pr.values[b]
    dz, dzb = pr.dz, pr.dz / 2.0
    if kind == M.BC_FLUX:
        return val / dz, np.zeros_like(K_c)
    if kind == M.BC_FREE_DRAINAGE:
        return -K_c / dz, -dK_c / dz
    if kind == M.BC_DIRICHLET:
        at = {k: a[:, i] for k, a in pr.p.items()}
        K_f, np_f, _, _ = closures(pr, at, val, pr.ti[:, i], pr.T[:, i])
        psi_f, psi_c = -np_f, -np_c
        if face == M.FACE_BOTTOM:
            g = (psi_f - psi_c - dzb) if pr.consistent else (psi_f - psi_c + dzb)
            return K_f * g / dzb / dz, K_f * dn_c / dzb / dz
        return -K_f * (psi_f - psi_c + dzb) / dzb / dz, -K_f * dn_c / dzb / dz
    raise ValueError("the hydrology component needs a boundary condition at both faces")


def tendency_and_slopes(pr, vl=None, **kw):
    """(f, df_i/dv_(i-1), df_i/dv_i, df_i/dv_(i+1)), each [ncols, nlev], at the state vl (default: the problem's):
    newton_jacobian_ref.tendency_and_slopes over the closures with factors."""
    v = pr.vl if vl is None else np.asarray(vl, dtype=np.float64)
    ncols, n = v.shape
    K, npsi, dK, dn = closures(pr, pr.p, v, pr.ti, pr.T, **kw)
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


def bands(pr, dt, vl=None, **kw):
    """The bands (a, b, c) of J = I - dt df/dv: row i is a_i x_(i-1) + b_i x_i + c_i x_(i+1)."""
    _, lo, di, up = tendency_and_slopes(pr, vl, **kw)
    return -dt * lo, 1.0 - dt * di, -dt * up


def newton_update(pr, dt, f, **kw):
    """d of the first Newton iteration from the problem's state: J d = dt f, with J from bands(**kw)."""
    return tri_solve(*bands(pr, dt, **kw), dt * np.asarray(f, dtype=np.float64))
