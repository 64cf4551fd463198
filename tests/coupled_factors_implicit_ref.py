"""The NumPy reference and the cases for implicit steps of the coupled model with the IceImpedance factor
(lh_step_coupled_factors_implicit): tests/coupled_implicit_ref.py, imported and unchanged, on
cases whose model has the factor on.  The oracle's tendency reads om.cf, so CR.coupled_implicit, CR.residual,
CR.stable_dt and CR.order_ratios serve these cases as they are.

theta_i is constant and no closure of the water reads T (no viscosity factor), so the two properties CR's stage
solve rests on still hold (tests/test_coupled_factors_implicit_reference.py asserts both): f_w does not read
rhoe_int, and f_e is affine in rhoe_int.

Test infrastructure (tests/test_coupled_factors_implicit_reference.py, tests/test_gpu_coupled_factors_implicit.py)."""
from __future__ import annotations

import copy
import functools

import numpy as np

import case_model as M
import coupled_implicit_ref as CR
import parity_cases as pc

NCOLS = 67                      # one full wave and a ragged one
NLEVS = (1, 2, 3, 16)           # both faces on one cell, no interior cell, one interior cell, a column
ICE_GENERAL, ICE_LARGE = 0.04, 0.15   # the largest theta_i of a column with ice
TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}        # the library's defaults
VL_BOUND = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 2e-5}   # tests/test_gpu_coupled_implicit.py's
ENERGY_BOTTOM_DIRICHLET = ((M.BC_DIRICHLET, 276.0), (M.BC_DIRICHLET, 288.0))   # (top, bottom)


def factors_case(top, bottom, dtype=np.float64, ncols=NCOLS, nlev=16, most_ice=ICE_GENERAL, zero_ice=False, percol=False,
                 energy=CR.ENERGY_DEFAULT, model=M.MODEL_COUPLED, impedance=True):
    """CR.coupled_case(..., ice=True) with the impedance factor on.  most_ice: the largest theta_i of a column with
    ice (ice in every other column); the state keeps coupled_case's T, so rhoe_int is re-formed where theta_i is not
    coupled_case's own.  zero_ice: an all-zero theta_i plane (the factor is 1)."""
    case = CR.coupled_case(top, bottom, dtype=dtype, ncols=ncols, nlev=nlev, ice=not zero_ice, percol=percol, energy=energy,
                           model=model)
    case.om.cf = M.default_cf(impedance=impedance)
    if zero_ice or most_ice == ICE_GENERAL:
        return case
    om, c, n = case.om, np.arange(ncols), nlev
    case.ti = np.where((c % 2 == 0)[:, None], most_ice * pc.uhash(c[:, None], np.arange(n)[None, :] + 5, 1000), 0.0).astype(dtype)
    if model == M.MODEL_COUPLED:   # coupled_case's rhoe_int(T, vartheta_l, theta_i) at its T
        zc, _ = pc.grid_np(-CR.DZ * n, 0.0, n)
        T = 284.0 + 5.0 * zc[None, :] / 1.28 + 2.0 * (pc.uhash(c, 1, n)[:, None] - 0.5)
        e, sp = om.earth, om.soil
        nu = om.percol.get("nu", np.full(ncols, sp.nu))[:, None]
        v64, t64 = case.vl.astype(np.float64), case.ti.astype(np.float64)
        rho_c_s = sp.rho_c_ds + np.minimum(v64, nu - t64) * (e.cp_l * e.rho_liq) + t64 * (e.cp_i * e.rho_ice)
        case.rhoe = (rho_c_s * (T - e.T_0) - t64 * e.rho_ice * e.LH_f0).astype(dtype)
    return case


def without_factors(om):
    """om with both conductivity factors NoEffect."""
    o = copy.copy(om)
    o.cf = M.default_cf()
    return o


def noeffect_energy_mutant(om, *args, **kw):
    """CR.coupled_implicit with the MUTANT energy tendency: wherever the energy is formed (the stage's matrix and
    right-hand side, the tendency at the start of a TR-BDF2 call) K is the NoEffect one; the water keeps the factor as
    it should.  What an energy_sweep_up that forgot the factor would compute."""
    real = CR.tendencies
    CR.tendencies = lambda o, vl, ti, rhoe: (real(o, vl, ti, rhoe)[0], real(without_factors(o), vl, ti, rhoe)[1])
    try:
        return CR.coupled_implicit(om, *args, **kw)
    finally:
        CR.tendencies = real


# ------------------------------------------------------------------ the parity rule (tests/test_gpu_coupled_implicit.py::check_parity)

def references(case, dt, nsteps, method, cols=slice(None), bcv=None, solver=CR.coupled_implicit):
    """(the reference iterated to round-off, d, ||rhoe_int||): d is what the device's stopping rule alone costs
    (Float64) or what storing the state in Float32 alone costs -- tests/test_gpu_coupled_implicit.py::_references."""
    vl, ti, re = (a[cols] for a in CR.f64(case))
    run = lambda **kw: solver(case.om, vl, ti, re, dt, nsteps, method, bcv=bcv, **kw)
    exact = run()
    other = run(tol=TOL[np.dtype(np.float64)]) if case.dtype == np.float64 else run(round_to=np.float32)
    return exact, float(np.max(np.abs(other[1] - exact[1]))), float(np.max(np.abs(re)))


def parity_bound(case, d, scale):
    """The allowance of rhoe_int: 4 d + 64 eps ||rhoe_int||."""
    return 4 * d + 64 * float(np.finfo(case.dtype).eps) * scale


# The parity cases of the GPU test, by name: (kinds, ncols, nlev, energy, steps of one call ...) at 30x the stable step,
# both methods.  Built once, shared, never written.
PARITY = {}
for _name, _kinds in (("drain", CR.KINDS[1]), ("dirichlet", CR.KINDS[3])):
    PARITY["ensemble-" + _name] = dict(kinds=_kinds, ncols=NCOLS, nlev=16, energy=CR.ENERGY_DEFAULT, nsteps=(3,))
for _nc in (1, 67, 130):
    for _nl in NLEVS:
        PARITY["shape-%dx%d" % (_nc, _nl)] = dict(kinds=CR.KINDS[1], ncols=_nc, nlev=_nl, energy=CR.ENERGY_DEFAULT, nsteps=(1, 5))
for _name, _kinds in (("drain", CR.KINDS[1]), ("dirichlet-water", CR.KINDS[2])):
    PARITY["bottom-energy-" + _name] = dict(kinds=_kinds, ncols=NCOLS, nlev=16, energy=ENERGY_BOTTOM_DIRICHLET, nsteps=(3,))
METHODS = ("euler", "trbdf2")
DTYPES = (np.float64, np.float32)


@functools.lru_cache(maxsize=None)
def parity_case(name, dtype):
    """(case, dt) of one parity case."""
    p = PARITY[name]
    case = factors_case(*p["kinds"], dtype=dtype, ncols=p["ncols"], nlev=p["nlev"], energy=p["energy"])
    for a in (case.vl, case.ti, case.rhoe):
        a.setflags(write=False)
    return case, 30 * CR.stable_dt(case)


@functools.lru_cache(maxsize=None)
def parity_reference(name, dtype, nsteps, method):
    """references() of one parity case, computed once."""
    case, dt = parity_case(name, dtype)
    return references(case, dt, nsteps, method)


# ------------------------------------------------------------------ the residual cases of the GPU test

KIND_IDS = {M.BC_FLUX: "flux", M.BC_DIRICHLET: "dir", M.BC_FREE_DRAINAGE: "drain"}
# GPU test 1: the five boundary pairs with ice up to 0.04 and up to 0.15, and per-column parameters
RESIDUAL_CASES = ["%s-%s-ice%g" % (KIND_IDS[k[0]], KIND_IDS[k[1]], most) for k in CR.KINDS for most in (ICE_GENERAL, ICE_LARGE)]
RESIDUAL_CASES.append("percol")


def residual_case(which, dtype):
    """(label, kinds, case) of one name of RESIDUAL_CASES."""
    if which == "percol":
        return which, CR.KINDS[1], factors_case(*CR.KINDS[1], dtype=dtype, percol=True)
    k, most = divmod(RESIDUAL_CASES.index(which), 2)
    return which, CR.KINDS[k], factors_case(*CR.KINDS[k], dtype=dtype, most_ice=(ICE_GENERAL, ICE_LARGE)[most])


def residual_cases(dtype):
    return [residual_case(w, dtype) for w in RESIDUAL_CASES]


def order_case(nlev=16, ncols=4):
    """CR.order_case with the factor on."""
    return factors_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, ncols=ncols, nlev=nlev)
