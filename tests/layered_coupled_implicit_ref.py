"""NumPy reference for implicit steps of a LAYERED coupled model (SoilEnergyModel + SoilHydrologyModel with per-cell
soil classes and their thermal supplement): tests/coupled_implicit_ref.py's construction with the tendency replaced
by the NumPy restatement of the layered tendency, layered_heat_ref.rhs in Float64.

The two properties that make a stage Y - w - c f(Y) = 0 block triangular survive classes
(tests/test_layered_coupled_implicit_reference.py asserts both): f_w does not read rhoe_int, and f_e is affine in
rhoe_int at fixed vartheta_l, theta_i.  So the stage is solved exactly by
  water:  the Newton of layered_implicit_ref.stage_solve (finite-difference Jacobian, the safeguard with every
          cell's own class) on the `vl` tendency, evaluated with rhoe_int = 0;
  energy: the bands of the affine f_e at the new water state from three coloured evaluations, then
          implicit_ref.thomas.
Backward Euler and TR-BDF2 (gamma = 2 - sqrt 2), the sampling of bcv (coupled_implicit_ref._sample, with_bc) and the
options tol= and round_to= are coupled_implicit_ref.coupled_implicit's.  The Newton iteration, the coloured bands
and the sampling of bcv are integrator_core's; this module supplies the layered tendencies, the exact energy bands,
every cell's own nu, theta_r, theta_i and the two methods' stage sequence.  Needs neither the oracle nor the library.

Test infrastructure (tests/test_layered_coupled_implicit_reference.py, tests/test_gpu_layered_coupled_implicit.py)."""
from __future__ import annotations

import copy
import dataclasses

import numpy as np

import case_model as M
import layered_heat_ref as LH
import layered_ref as R
import integrator_core as core
from integrator_core import DMAX_FRAC, STALL, thomas

GAMMA, D, _sample = core.GAMMA, core.D, core.sample


def with_bc(lay, sample):
    """The Float64 twin of `lay` with the scalar boundary values of one bcv sample [2 faces][2 components]
    (None: the case's own), as coupled_implicit_ref.with_bc."""
    l64 = LH.as64(lay)
    if sample is None:
        return l64
    om = copy.copy(l64.case.om)
    om.bc = dict(l64.case.om.bc)
    for key, (kind, _) in l64.case.om.bc.items():
        if kind in (M.BC_DIRICHLET, M.BC_FLUX):
            om.bc[key] = (kind, float(sample[key[0]][key[1]]))
    return LH.LayeredHeat(dataclasses.replace(l64.case, om=om), l64.classes, l64.thermal, l64.class_map)


def tendencies(l64, vl, rhoe):
    """(d vartheta_l / dt, d rhoe_int / dt) [ncols, nlev] of a Float64 layered case at the state (vl, rhoe)."""
    f = LH.rhs(l64, vl=np.asarray(vl, np.float64), rhoe=np.asarray(rhoe, np.float64))
    return f["vl"].astype(np.float64), f["rhoe"].astype(np.float64)


def water_tendency(l64, vl):
    return tendencies(l64, vl, np.zeros_like(vl))[0]


def _fd_jacobian(l64, vl, coef, f0, nu):
    """layered_implicit_ref.fd_jacobian on the coupled water tendency"""
    return core.fd_bands(lambda v: water_tendency(l64, v), vl, coef, f0, nu)


def safeguard(l64):
    """(nu, theta_r, theta_i) of the Newton stage's safeguard, every cell's own: [ncols, nlev]"""
    p = R.cell_params(l64)
    return p["nu"].astype(np.float64), p["theta_r"].astype(np.float64), np.asarray(l64.case.ti, dtype=np.float64)


def newton_stage(l64, y, w, coef, tol=None, max_iter=None):
    """The water stage Y - w - coef f_w(Y) = 0 from the guess y: the safeguard with every cell's own nu, theta_r and
    coupled_implicit_ref.newton_stage's two stopping rules.  Returns (Y, iterations [ncols], converged [ncols])."""
    stop, cap = (core.round_off, 120) if tol is None else (core.fixed_step_rule(tol), 50)
    return core.newton_stage(lambda v: water_tendency(l64, v), *safeguard(l64), coef, y, w, stop, cap if max_iter is None else max_iter)


def energy_bands(l64, vl):
    """Bands (lo, di, up) of A and f0 with f_e(rhoe) = A rhoe + f0 at the water state vl
    (coupled_implicit_ref.energy_bands)."""
    vl = np.asarray(vl, np.float64)
    ncols, n = vl.shape
    fe = lambda e: tendencies(l64, vl, e)[1]
    f0 = fe(np.zeros((ncols, n)))
    lo, di, up = np.zeros((ncols, n)), np.zeros((ncols, n)), np.zeros((ncols, n))
    s = 2.0 ** 30   # (a power of two: exact scaling)
    for k in range(3):
        e = np.zeros((ncols, n))
        e[:, k::3] = s
        df = (fe(e) - f0) / s
        for j in range(k, n, 3):
            di[:, j] = df[:, j]
            if j > 0:
                up[:, j - 1] = df[:, j - 1]
            if j + 1 < n:
                lo[:, j + 1] = df[:, j + 1]
    return (lo, di, up), f0


def energy_stage(l64, vl, w, coef):
    """The energy stage Y - w - coef f_e(Y) = 0 at the water state vl: (I - coef A) Y = w + coef f0."""
    (lo, di, up), f0 = energy_bands(l64, vl)
    return thomas(-coef * lo, 1.0 - coef * di, -coef * up, w + coef * f0)


def coupled_implicit(lay, vl, rhoe, dt, nsteps, method="euler", bcv=None, tol=None, max_iter=None, round_to=None):
    """nsteps steps of the [ncols, nlev] state (vl, rhoe) of `lay` (theta_i and the class map held), with
    coupled_implicit_ref.coupled_implicit's formulas, arguments and result: (vl, rhoe, info)."""
    assert method in ("euler", "trbdf2")
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    v, e = np.array(vl, dtype=np.float64), np.array(rhoe, dtype=np.float64)
    if bcv is not None:
        assert np.asarray(bcv).shape == (nsteps + 1, 2, 2)
    info = dict(iters=0, unconverged=0, total=0)
    const = with_bc(lay, None) if bcv is None else None
    at = lambda k, w=None: const if bcv is None else with_bc(lay, _sample(bcv, k, w))

    def stage(l64, guess, wv, we, coef):
        y, its, conv = newton_stage(l64, guess, wv, coef, tol, max_iter)
        info["iters"] = max(info["iters"], int(its.max()))
        info["unconverged"] += int((~conv).sum())
        info["total"] += int(its.sum())
        y = rnd(y)
        return y, rnd(energy_stage(l64, y, we, coef))

    if method == "euler":
        for k in range(nsteps):
            v, e = stage(at(k + 1), v, v, e, dt)
        return v, e, info
    dh = D * dt
    fv, fe = tendencies(at(0), v, e)
    for k in range(nsteps):
        vg, eg = stage(at(k, GAMMA), v, v + dh * fv, e + dh * fe, dh)
        wv = (vg - (1.0 - GAMMA) ** 2 * v) / (GAMMA * (2.0 - GAMMA))
        we = (eg - (1.0 - GAMMA) ** 2 * e) / (GAMMA * (2.0 - GAMMA))
        v, e = stage(at(k + 1), vg, wv, we, dh)
        fv, fe = (v - wv) / dh, (e - we) / dh
    return v, e, info


def residual(lay, vl0, e0, vl1, e1, dt):
    """The full backward-Euler residual (Y1 - Yn - dt f(Y1)) through layered_heat_ref.rhs: (water, energy)."""
    fv, fe = tendencies(with_bc(lay, None), vl1, e1)
    return vl1 - vl0 - dt * fv, e1 - e0 - dt * fe


def state64(lay):
    return np.asarray(lay.case.vl, dtype=np.float64), np.asarray(lay.case.rhoe, dtype=np.float64)


def stable_dt(lay):
    """The explicit engines' cap of the Float64 twin, courant 1/2."""
    return LH.stable_dt(LH.as64(lay), 0.5)


# ------------------------------------------------------------------ cases shared by the two test files

NCLS = 5     # classes 1 and 4 are organic (layered_heat_ref.thermal_classes: every third): any_om is on


def cell_map(ncols, nlev, ncls=NCLS):
    """a different class in every cell: neighbours in a column differ by 2 (mod ncls), neighbouring columns by 1"""
    c, i = np.arange(ncols)[:, None], np.arange(nlev)[None, :]
    return ((c + 2 * i) % ncls).astype(np.uint8)


def three_horizons(ncols, nlev):
    """the same three horizons in every column (layered_ref.hydrostatic's proportions)"""
    row = np.zeros(nlev, dtype=np.uint8)
    row[nlev * 5 // 16:] = 1
    row[nlev * 11 // 16:] = 2
    return np.repeat(row[None, :], ncols, axis=0)


def layered_case(dtype, ncols, nlev, kind="cells", hyd=(M.BC_FLUX, M.BC_FLUX), energy="flux", ice=False, classes=None,
                 percol_bc=False):
    """A coupled case of layered_heat_ref.make_layered_heat.  kind: "cells" (cell_map, 5 classes, two organic),
    "horizons" (three_horizons, an organic class in the middle) or "columns" (every column one of 3 classes).
    hyd: the hydrology kinds (top, bottom); a flux is coupled_implicit_ref's -2e-9, the Dirichlet values are
    layered_ref.make_layered's (0.30 at the top, 0.26 at the bottom: inside the pore space of every class).  energy: "flux" (both faces), "dirichlet" (both), "mixed" (Dirichlet bottom, flux top).
    percol_bc: the Dirichlet values vary by column, rounded to the working type."""
    if kind == "cells":
        cmap, cl, th = cell_map(ncols, nlev), R.texture_classes()[:NCLS], LH.thermal_classes()[:NCLS]
    elif kind == "horizons":
        cmap, cl, th = three_horizons(ncols, nlev), R.texture_classes()[[0, 5, 2]], LH.thermal_classes()[[0, 4, 2]]
    else:
        cmap, cl, th = R.uniform_map(ncols, nlev, 3), R.texture_classes()[[0, 5, 2]], LH.thermal_classes()[[0, 4, 2]]
    if classes is not None:
        cl = classes
    lay = LH.make_layered_heat(dtype, ncols, nlev, cmap, model=M.MODEL_COUPLED, classes=cl, thermal=th,
                               bc="flux" if energy == "flux" else "dirichlet", ice=ice, name="layered_coupled_implicit")
    om = lay.case.om
    values = {M.BC_FLUX: -2e-9, M.BC_FREE_DRAINAGE: 0.0}
    top, bottom = hyd
    om.bc[(M.FACE_TOP, M.COMP_HYDROLOGY)] = (top, 0.30 if top == M.BC_DIRICHLET else values[top])
    om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (bottom, 0.26 if bottom == M.BC_DIRICHLET else values[bottom])
    om.consistent_bottom_sign = False
    if energy == "mixed":
        om.bc[(M.FACE_TOP, M.COMP_ENERGY)] = (M.BC_FLUX, -0.8)
    om.percol_bc = {}
    if percol_bc:
        c = np.arange(ncols)
        uhash = LH._pkg.workloads.uhash
        spread = {M.COMP_ENERGY: 2.0, M.COMP_HYDROLOGY: 0.02}
        om.percol_bc = {k: (v[1] + spread[k[1]] * (uhash(c, 77 + k[0], 1) - 0.5)).astype(dtype).astype(np.float64)
                        for k, v in om.bc.items() if v[0] == M.BC_DIRICHLET}
    return lay


# the order tests: ORDER_SPAN stable steps of three-horizon columns, the errors against layered_heat_ref.ssprk33 at sd / 8
ORDER_SPAN = 16.0
ORDER_STEPS = {"euler": (4, 8, 16), "trbdf2": (4, 8, 16)}
ORDER_BANDS = {"euler": (1.8, 2.2), "trbdf2": (3.7, 4.5)}   # coupled_implicit_ref.ORDER_BANDS


def order_case(ncols=4, nlev=24):
    return layered_case(np.float64, ncols, nlev, kind="horizons", hyd=(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), energy="dirichlet",
                        ice=True)


def order_ratios(method, solve, lay=None):
    """Per variable the error ratios per halving of h of solve(lay, dt, nsteps) -> (vl, rhoe) against
    layered_heat_ref.ssprk33 at an eighth of the stable step (max norm), and the errors."""
    lay = order_case() if lay is None else lay
    sd = stable_dt(lay)
    ref = LH.ssprk33(LH.as64(lay), sd / 8, int(round(8 * ORDER_SPAN)))
    want = (ref["vl"].astype(np.float64), ref["rhoe"].astype(np.float64))
    errs = {"vl": [], "rhoe": []}
    for n in ORDER_STEPS[method]:
        got = solve(lay, ORDER_SPAN * sd / n, n)
        for name, g, w in zip(("vl", "rhoe"), got, want):
            errs[name].append(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w))))
    return {k: [v[i] / v[i + 1] for i in range(len(v) - 1)] for k, v in errs.items()}, errs
