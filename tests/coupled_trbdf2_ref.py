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

The attempt, the error norm, the energy solve, the controller and the accept / reject loop are integrator_core's
(coupled_attempt, coupled_error_norm, energy_solve, step_factor, coupled_integrate) over the provider below, which
supplies the oracle's tendencies, bands and boundary values and the per-column safeguard.

Test infrastructure (tests/test_coupled_trbdf2_reference.py, tests/test_gpu_coupled_trbdf2.py)."""
from __future__ import annotations

import numpy as np

import coupled_implicit_ref as CR
import integrator_core as core
import trbdf2_ref as TR

GAMMA, D, B, HMIN_FRAC = core.GAMMA, core.D, core.B, core.HMIN_FRAC
ABSTOL, RELTOL = 1e-6, 1e-3
NEWTON_KAPPA, NEWTON_MAX = 0.01, 10   # the library's stage Newton test
error_norm, step_factor = core.coupled_error_norm, core.step_factor


def abstol_e_default(om):
    """1e-6 rho_l c_l: the energy of 1e-6 K in water."""
    return 1e-6 * (om.earth.cp_l * om.earth.rho_liq)


def device_newton(abstol=ABSTOL, reltol=RELTOL):
    return (NEWTON_KAPPA, abstol, reltol, NEWTON_MAX)


def provider(om, ti):
    """integrator_core.CoupledProblem of the oracle's coupled model `om` with theta_i held: a stage's model is om
    under trbdf2_ref._with_bc's boundary values."""
    return core.CoupledProblem(at=lambda bcv, t0, t1, t: TR._with_bc(om, bcv, t0, t1, t),
                               water_tendency=lambda o, v: CR.water_tendency(o, v, ti),
                               tendencies=lambda o, v, e: CR.tendencies(o, v, ti, e),
                               energy_bands=lambda o, v: CR.energy_bands(o, v, ti),
                               safeguard=lambda o: CR.safeguard(o, np.shape(ti)[0]) + (ti,))


def water_stage(om, y0, w, ti, coef, newton=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y0, coef one per column (coupled_implicit_ref's
    Newton with the stopping rule above).  Returns (Y, iterations [ncols], converged [ncols])."""
    return core.water_stage(provider(om, ti), om, y0, w, coef, newton)


def energy_solve(om, vl, ti, rhs, coef, homogeneous=False):
    """(I - coef A) x = rhs + coef f0 at the water state vl, f_e(rhoe) = A rhoe + f0 (coef one per column);
    homogeneous: (I - coef A) x = rhs."""
    return core.energy_solve(provider(om, ti), om, vl, rhs, coef, homogeneous)


def attempt(om, vn, en, fvn, fen, ti, t, h, bcv=None, t0=0.0, t1=1.0, newton=None, block="diagonal", round_to=None):
    """One TR-BDF2 step of every column from (vn, en) with tendencies (fvn, fen) at times t with steps h (scalars
    or one per column): integrator_core.coupled_attempt, its arguments and its dict."""
    return core.coupled_attempt(provider(om, ti), vn, en, fvn, fen, t, h, bcv, t0, t1, newton, block, round_to)


def integrate(om, vl, ti, rhoe, t0, t1, dt, abstol=ABSTOL, abstol_e=None, reltol=RELTOL, bcv=None, h0=None,
              newton=None, round_to=None, max_steps=100000):
    """Integrate the [ncols, nlev] state (vl, rhoe) from t0 to t1, every column with its own t and h from h0
    (default dt).  Returns (vl, rhoe, info), info = dict(t, h, accepted, rejected, failed) per column."""
    return core.coupled_integrate(provider(om, np.asarray(ti, dtype=np.float64)), vl, rhoe, t0, t1, dt, abstol,
                                  abstol_e_default(om) if abstol_e is None else abstol_e, reltol, bcv, h0, newton, round_to, max_steps)
