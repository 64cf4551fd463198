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

The attempt, the error norm, the energy solve, the controller and the accept / reject loop are integrator_core's,
shared with coupled_trbdf2_ref, over the provider below: the layered tendencies, bands and boundary values and
every cell's own safeguard.  Pure NumPy: imports neither the oracle nor the library's kernels.

Test infrastructure (tests/test_layered_coupled_trbdf2_reference.py, tests/test_gpu_layered_coupled_trbdf2.py)."""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import integrator_core as core

GAMMA, D, B, HMIN_FRAC = core.GAMMA, core.D, core.B, core.HMIN_FRAC
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


def provider(lay):
    """integrator_core.CoupledProblem of the layered case `lay`: a stage's model is its Float64 twin under with_bc's
    boundary values."""
    return core.CoupledProblem(at=lambda bcv, t0, t1, t: with_bc(lay, bcv, t0, t1, t), water_tendency=LC.water_tendency,
                               tendencies=LC.tendencies, energy_bands=LC.energy_bands, safeguard=LC.safeguard)


error_norm, step_factor = core.coupled_error_norm, core.step_factor


def water_stage(l64, y0, w, coef, newton=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y0, coef one per column, with every cell's own nu,
    theta_r and coupled_trbdf2_ref.water_stage's two stopping rules.  Returns (Y, iterations [ncols], converged [ncols])."""
    return core.water_stage(provider(l64), l64, y0, w, coef, newton)


def energy_solve(l64, vl, rhs, coef, homogeneous=False):
    """(I - coef A) x = rhs + coef f0 at the water state vl, f_e(rhoe) = A rhoe + f0 (coef one per column);
    homogeneous: (I - coef A) x = rhs."""
    return core.energy_solve(provider(l64), l64, vl, rhs, coef, homogeneous)


def attempt(lay, vn, en, fvn, fen, t, h, bcv=None, t0=0.0, t1=1.0, newton=None, block="diagonal", round_to=None):
    """One TR-BDF2 step of every column from (vn, en) with tendencies (fvn, fen) at times t with steps h (scalars
    or one per column): coupled_trbdf2_ref.attempt's formulas, arguments (theta_i is the case's) and result."""
    return core.coupled_attempt(provider(lay), vn, en, fvn, fen, t, h, bcv, t0, t1, newton, block, round_to)


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
    return core.coupled_integrate(provider(lay), vl, rhoe, t0, t1, dt, abstol, abstol_e_default(lay) if abstol_e is None else abstol_e,
                                  reltol, bcv, h0, newton, round_to, max_steps)


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
