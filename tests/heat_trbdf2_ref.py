"""NumPy reference for the adaptive TR-BDF2 of the heat-only model (lh_integrate_heat_trbdf2),
on heat_implicit_ref's affine_parts / stage_solve.

With vartheta_l and theta_i prescribed, f(Y, t) = A Y + b(t).  Per column and attempt, with gamma = 2 - sqrt 2,
d = gamma / 2, the column's own step h and c = d h:
  stage 1: (I - c A) Y_g = Y_n + c f_n + c b(t + gamma h)
  stage 2: (I - c A) Y_1 = w2 + c b(t + h),   w2 = (Y_g - (1 - gamma)^2 Y_n) / (gamma (2 - gamma))
  z_g = (Y_g - (Y_n + c f_n)) / d,  z_1 = (Y_1 - w2) / d,  f_n+1 = z_1 / h
  e = (I - c A)^-1 (b1 h f_n + b2 z_g + b3 z_1)      (homogeneous: the stage matrix itself is the filter)
  E = sqrt(mean_i (e_i / (abstol_e + reltol max(|Y_n,i|, |Y_1,i|)))^2),  accepted when E <= 1,
  h <- h clamp(0.9 E^(-1/3), 0.2, 5); a clipped step that could have grown does not shrink the proposal.
The first f_n of a call is a fresh tendency at (Y, t0).  Everything is vectorised over columns, every column with its
own t and h, so per-column boundary arrays work.  b(t) is affine in the two energy boundary values: b = b(0, 0) +
v_bottom g_bottom + v_top g_top with the unit responses g taken once (exactly zero for a face whose value the model
does not read: no condition, or a per-column array, which takes precedence); the values of a stage time are bcv's
[t0 | t1][face][component] interpolated linearly in double and rounded once to FT, as on the device.

ft: None, or the type to which everything the device keeps in an FT plane is rounded (Y_n, f_n, Y_g, w2, Y_1), with
the boundary values, the tolerances and the step proposals handed out.  (r' of the device's forward sweeps is a plane
too; it is internal to the solve and has no counterpart in the Thomas solve here.)

The controller and the accept / reject loop are integrator_core's (step_factor, adaptive_loop, here with max_steps
failing the column); this module supplies the linear attempt, the boundary values and the FT rounding.

Test infrastructure (tests/test_heat_trbdf2_reference.py, tests/test_gpu_heat_trbdf2.py)."""
from __future__ import annotations

import numpy as np

import case_model as M
import heat_implicit_ref as H
import integrator_core as core
from integrator_core import B, D, GAMMA, HMIN_FRAC

MAX_STEPS = 100000   # LH_TRBDF2_MAX_STEPS
RELTOL = 1e-3
stage_solve = H.stage_solve


def abstol_e_default(om):
    """the library's default: 1e-6 K in water"""
    return 1e-6 * om.earth.cp_l * om.earth.rho_liq


class Problem:
    """f(Y, t) = A Y + b(t) of one ensemble.  tendency(y, sample): d rhoe_int / dt at the state y under the scalar
    energy boundary values of one sample [2 faces][2 components] (None: the model's own)."""

    def __init__(self, om, tendency, bands, shape):
        self.om, self.tendency, self.bands, self.shape = om, tendency, bands, shape
        zero = np.zeros(shape)
        s = 2.0 ** 10   # (a power of two: exact scaling)

        def b_of(vb, vt):
            smp = np.zeros((2, 2))
            smp[M.FACE_BOTTOM, M.COMP_ENERGY], smp[M.FACE_TOP, M.COMP_ENERGY] = vb, vt
            return tendency(zero, smp)
        self.b00 = b_of(0.0, 0.0)
        self.gb = (b_of(s, 0.0) - self.b00) / s
        self.gt = (b_of(0.0, s) - self.b00) / s

    def model_values(self):
        """the model's own scalar energy values (bottom, top); 0 where it has none"""
        get = lambda f: float(self.om.bc.get((f, M.COMP_ENERGY), (M.BC_NONE, 0.0))[1])
        return get(M.FACE_BOTTOM), get(M.FACE_TOP)

    def values(self, bcv, t0, t1, t, rnd):
        """(v_bottom, v_top) per column at the times t: bcv interpolated in double and rounded once, or the model's"""
        if bcv is None:
            vb, vt = self.model_values()
            return rnd(np.full(self.shape[0], vb)), rnd(np.full(self.shape[0], vt))
        b = np.asarray(bcv, dtype=np.float64).reshape(2, 2, 2)
        s = (np.asarray(t, dtype=np.float64) - t0) / (t1 - t0) if t1 > t0 else np.ones(self.shape[0])
        at = lambda f: rnd(b[0, f, M.COMP_ENERGY] + (b[1, f, M.COMP_ENERGY] - b[0, f, M.COMP_ENERGY]) * s)
        return at(M.FACE_BOTTOM), at(M.FACE_TOP)

    def b(self, vb, vt):
        return self.b00 + vb[:, None] * self.gb + vt[:, None] * self.gt


def problem(case):
    """The Problem of a heat_implicit_ref case (its Float64 values)."""
    vl, ti, _ = H.f64(case)
    bands, _ = H.affine_parts(case.om, vl, ti)
    return Problem(case.om, lambda y, smp: H.tendency(H.with_energy_bc(case.om, smp), vl, ti, y), bands, vl.shape)


_rounder = core.rounder


def fresh_tendency(P, y, bcv, ft=None):
    """f_n of a call's first step: the tendency at (Y, t0) under bcv's values of t0"""
    smp = None if bcv is None else _rounder(ft)(np.asarray(bcv, dtype=np.float64).reshape(2, 2, 2)[0])
    return P.tendency(y, smp)


def attempt(P, y, fn, t, hh, bcv=None, t0=0.0, t1=1.0, ft=None):
    """One TR-BDF2 attempt of every column from (y, f_n, t) with the steps hh [ncols].  Returns dict(y1, fn1, e, r)."""
    rnd = _rounder(ft)
    c = (D * np.asarray(hh, dtype=np.float64))[:, None]
    if ft is not None:
        c = rnd(c)   # (the device holds c = FT(d hh))
    w1 = y + c * fn
    bg = P.b(*P.values(bcv, t0, t1, t + GAMMA * hh, rnd))
    yg = rnd(stage_solve(P.bands, c, w1 + c * bg))
    w2 = rnd((yg - (1.0 - GAMMA) ** 2 * y) / (GAMMA * (2.0 - GAMMA)))
    b1 = P.b(*P.values(bcv, t0, t1, t + hh, rnd))
    y1 = rnd(stage_solve(P.bands, c, w2 + c * b1))
    hc = np.asarray(hh, dtype=np.float64)[:, None]
    r = B[0] * (hc * fn) + B[1] * (yg - w1) / D + B[2] * (y1 - w2) / D
    e = stage_solve(P.bands, c, r)
    return dict(y1=y1, fn1=rnd((y1 - w2) / (D * hc)), e=e, r=r, yg=yg, w2=w2)


def error_norm(e, yn, y1, abstol_e, reltol):
    return core.error_norm(e, yn, y1, abstol_e, reltol)


step_factor = core.step_factor


def integrate(P, rhoe, t0, t1, dt, abstol_e=None, reltol=RELTOL, bcv=None, h0=None, ft=None, max_steps=MAX_STEPS):
    """Integrate the [ncols, nlev] state from t0 to t1, every column with its own t and h from h0 (default, and where
    h0 <= 0: dt).  Returns (rhoe, info), info = dict(t, h, accepted, rejected, failed, dt_cols) per column; a failed
    column (h below the floor, or max_steps attempts) keeps its last accepted state and dt_cols 0."""
    rnd = _rounder(ft)
    y = rnd(np.array(rhoe, dtype=np.float64))
    ncols = y.shape[0]
    abstol_e = float(rnd(abstol_e_default(P.om) if not abstol_e else abstol_e))
    reltol = float(rnd(RELTOL if not reltol else reltol))
    h = np.full(ncols, float(dt))
    if h0 is not None:
        h = np.where(np.asarray(h0, dtype=np.float64) > 0, np.asarray(h0, dtype=np.float64), h)
    if not t1 > t0:
        none = np.zeros(ncols, dtype=np.int64)
        return y, dict(t=np.full(ncols, float(t0)), h=h, accepted=none, rejected=none.copy(), failed=np.zeros(ncols, dtype=bool), dt_cols=rnd(h))

    def one(state, f, t, hh):
        r = attempt(P, state[0], f[0], t, hh, bcv, t0, t1, ft)
        return (r["y1"],), (r["fn1"],), error_norm(r["e"], state[0], r["y1"], abstol_e, reltol), None

    (y,), info = core.adaptive_loop(one, (y,), (rnd(fresh_tendency(P, y, bcv, ft)),), t0, t1, h, max_steps, cap_fails=True)
    return y, dict(info, dt_cols=np.where(info["failed"], 0.0, rnd(info["h"])))


def fixed_trbdf2(P, rhoe, t0, t1, nsteps, bcv=None):
    """nsteps equal TR-BDF2 steps of the same formulas (f_n carried), the yardstick of the integration tests."""
    y = np.array(rhoe, dtype=np.float64)
    ncols = y.shape[0]
    fn = fresh_tendency(P, y, bcv)
    h = (t1 - t0) / nsteps
    for k in range(nsteps):
        r = attempt(P, y, fn, np.full(ncols, t0 + k * h), np.full(ncols, h), bcv, t0, t1)
        y, fn = r["y1"], r["fn1"]
    return y


def true_local_error(P, y, fn, t, hh, bcv=None, t0=0.0, t1=1.0, sub=32):
    """Y_1 of one attempt minus the state after `sub` equal sub-steps of the same span (DESIGN section 4.17's yardstick)"""
    one = attempt(P, y, fn, t, hh, bcv, t0, t1)["y1"]
    yy, ff = y, fn
    for k in range(sub):
        r = attempt(P, yy, ff, t + k * hh / sub, hh / sub, bcv, t0, t1)
        yy, ff = r["y1"], r["fn1"]
    return one - yy
