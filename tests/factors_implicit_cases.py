"""The cases the tests of the implicit integrators with conductivity factors share (tests/test_factors_implicit_reference.py
on the CPU, tests/test_gpu_factors_implicit.py on the device): built once, shared and never written.

Every case is a Richards ensemble of 67 columns (one full wave and a ragged one) of 2 levels (both faces of a cell are
boundaries or the only interior face) or 16, on the grid zmin = -0.02 nlev, zmax = 0, loam, tests/test_gpu_implicit.py's
wetting front and five boundary pairs, static ice in every other column and T hashed per cell in [270, 295] K."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import case_model as M
import factors_jacobian_ref as FJ
import parity_cases as pc

NCOLS = 67
DZ = 0.02
KINDS = [(M.BC_FLUX, M.BC_FLUX), (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET),
         (M.BC_DIRICHLET, M.BC_DIRICHLET), (M.BC_FLUX, M.BC_FREE_DRAINAGE)]   # tests/test_gpu_implicit.py::KINDS (top, bottom)
KIND_IDS = {M.BC_FLUX: "flux", M.BC_DIRICHLET: "dir", M.BC_FREE_DRAINAGE: "drain"}
FACTORS = {"both": (True, True), "viscosity": (True, False), "impedance": (False, True), "none": (False, False)}
ICE_GENERAL, ICE_JACOBIAN = 0.04, 0.15   # the largest theta_i of a column with ice


@dataclasses.dataclass(frozen=True)
class Spec:
    dtype: str           # "f64" / "f32"
    nlev: int
    kinds: tuple         # (top, bottom)
    factors: str         # a key of FACTORS
    mult: float          # the step in units of the case's stable step
    ice: float = ICE_GENERAL
    variant: str = "plain"   # Jacobian cases: "plain", "equal" (columns equalised in stiffness), "above" (cells above nu - theta_i)

    @property
    def id(self):
        return "%s-n%d-%s-%s-%s-%s-x%g" % (self.dtype, self.nlev, KIND_IDS[self.kinds[0]], KIND_IDS[self.kinds[1]], self.factors,
                                           self.variant, self.mult)

    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32


IDS = lambda specs: [s.id for s in specs]


def hyd_bc(kinds):
    """tests/test_newton_jacobian_reference.py's boundary values: Dirichlet 0.30 (top) / 0.15 (bottom), a flux of -2e-9
    (top) / -2e-10 (bottom)."""
    top, bottom = kinds
    vt = {M.BC_FLUX: -2e-9, M.BC_DIRICHLET: 0.30, M.BC_FREE_DRAINAGE: 0.0}[top]
    vb = {M.BC_FLUX: -2e-10, M.BC_DIRICHLET: 0.15, M.BC_FREE_DRAINAGE: 0.0}[bottom]
    return {(M.FACE_TOP, M.COMP_HYDROLOGY): (top, vt), (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (bottom, vb)}


def temperature(nlev):
    c = np.arange(NCOLS)
    return 270.0 + 25.0 * pc.uhash(c[:, None], np.arange(nlev)[None, :] + 11, 1000)


def ice(nlev, most):
    c = np.arange(NCOLS)
    return np.where((c % 2 == 0)[:, None], most * pc.uhash(c[:, None], np.arange(nlev)[None, :] + 5, 1000), 0.0)


def make_case(dtype, nlev, kinds, factors="both", most_ice=ICE_GENERAL, se_max=None, gamma=None, zero_ice=False, wet=None,
              above=False):
    """se_max: no cell wetter than Se = se_max of its own pore space nu - theta_i (the Jacobian cases: next to the
    kink a Float32 slope stops being a slope, tests/newton_jacobian_ref.safeguard_inactive); wet [ncols]: the wetting
    front times this, per column; above: the bottom cell of every third column sits above nu - theta_i (the saturated
    branch of psi, a constant theta_l in the impedance factor)."""
    visc, imp = FACTORS[factors]
    cf = M.default_cf(viscosity=visc, impedance=imp) if gamma is None else M.default_cf(viscosity=visc, impedance=imp, gamma=gamma)
    om = M.CaseModel(M.MODEL_RICHARDS, nlev, -DZ * nlev, 0.0, bc=hyd_bc(kinds), cf=cf)
    vl = pc.wetting_front(NCOLS, nlev, -DZ * nlev, 0.0, 0.35)
    ti = np.zeros((NCOLS, nlev)) if zero_ice else ice(nlev, most_ice)
    if wet is not None:
        vl = vl * np.asarray(wet)[:, None]
    if se_max is not None:
        vl = np.minimum(vl, om.vg.theta_r + se_max * (om.soil.nu - ti - om.vg.theta_r))
    if above:
        # (S_s = 0.05, as the "regimes" case of tests/test_newton_jacobian_reference.py: the saturated cell's diffusivity
        # Ksat / S_s is then the unsaturated cells' and not 100 times it, and the column's other rows are not slack)
        om.soil = M.default_soil(S_s=0.05)
        sat = np.arange(NCOLS) % 3 == 0
        vl[sat, 0] = (om.soil.nu - ti[sat, 0]) + om.soil.S_s * 0.05
    return pc.Case("factors_implicit", om, dtype, NCOLS, vl=vl.astype(dtype), ti=ti.astype(dtype),
                   T_aux=temperature(nlev).astype(dtype))


def f64(case):
    """(vl, ti, T) of a case as Float64 arrays: what the device holds, widened."""
    return tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (case.vl, case.ti, case.T_aux))


def stable_dt(case):
    vl, ti, T = f64(case)
    return pc.O.stable_dt(case.om, vl, ti, None, 0.5, T)


@functools.lru_cache(maxsize=None)
def general(spec):
    """(case, dt) of one case of the residual, parity, adaptive and bitwise tests."""
    case = make_case(spec.np_dtype, spec.nlev, spec.kinds, spec.factors, spec.ice)
    for a in (case.vl, case.ti, case.T_aux):
        a.setflags(write=False)
    return case, spec.mult * stable_dt(case)


# ------------------------------------------------------------------ the Jacobian cases

@dataclasses.dataclass
class Prepared:
    spec: Spec
    obj: object          # the Case the GPU test runs
    pr: FJ.Problem
    dt: float
    tendency: object     # vl [ncols, nlev] Float64 -> the oracle's water tendency (Float64)
    J: tuple             # the reference bands
    dtf: np.ndarray      # dt f(Y0) of the oracle
    d: np.ndarray        # the reference's own first Newton update
    q32: float           # worst column of q with the slopes in Float32
    q_1pc: float         # the smaller of the 1 % mutants' q (dK or dnpsi off by 1 %), the minimum over the columns


SE_MAX = {"plain": 0.9, "above": 0.9, "equal": 0.7}


def stiffness(pr):
    """Per column: max_i |df_i/dv_i|, the size of the Jacobian's diagonal per unit of dt."""
    return np.max(np.abs(FJ.tendency_and_slopes(pr)[2]), axis=1)


def equalised(build, lo=0.3, hi=1.2, pick=lambda g: np.percentile(g, 30)):
    """tests/test_newton_jacobian_reference.py::equalised over the Jacobian with factors: build(w [ncols]) -> (case,
    Problem), wetter for larger w, with w in [lo, hi] such that every column is as stiff as the pick column of build(1),
    as far as [lo, hi] allows.  (The impedance factor of a column with theta_i = 0.15 is 10^-2.6: without this the
    columns without ice set the step and those with ice are slack, J = I to four digits, whatever the kernel does.)"""
    target = float(pick(stiffness(build(np.ones(NCOLS))[1])))
    a, b = np.full(NCOLS, lo), np.full(NCOLS, hi)
    for _ in range(50):
        w = np.sqrt(a * b)
        up = stiffness(build(w)[1]) < target
        a, b = np.where(up, w, a), np.where(up, b, w)
    return build(np.sqrt(a * b))


def _jacobian_specs():
    J = ICE_JACOBIAN
    out = [Spec("f64", 2, k, "both", 10.0, J) for k in KINDS]                         # every boundary slope, both cells at a face
    out += [Spec("f64", 16, k, "both", 2.0, J, "equal") for k in (KINDS[0], KINDS[4])]   # interior rows, room for the 1 % pin
    out += [Spec("f64", 16, KINDS[4], f, 2.0, J, "equal") for f in ("viscosity", "impedance")]
    out += [Spec("f64", n, KINDS[4], "both", 10.0, J, "above") for n in (2, 16)]
    out += [Spec("f32", 2, KINDS[3], "both", 10.0, J), Spec("f32", 16, KINDS[4], "both", 2.0, J, "equal")]
    return out


JACOBIAN = _jacobian_specs()
# the mutants (factors_jacobian_ref.MUTANTS) a case's Jacobian contains
def mutants_of(spec):
    m = []
    if FACTORS[spec.factors][1]:
        m.append("no_impedance_term")
    if FACTORS[spec.factors][0]:
        m.append("no_viscosity_on_dK")
    if FACTORS[spec.factors][1] and spec.variant == "above":
        m.append("impedance_term_above")
    return m


@functools.lru_cache(maxsize=None)
def prepared(spec):
    """Everything both test modules need of one Jacobian case (tests/test_newton_jacobian_reference.py::prepared)."""
    def build(w):
        c = make_case(spec.np_dtype, spec.nlev, spec.kinds, spec.factors, spec.ice, se_max=SE_MAX[spec.variant], wet=w,
                      above=spec.variant == "above")
        return c, FJ.problem_of_case(c)
    obj, pr = equalised(build) if spec.variant == "equal" else build(None)
    sd = stable_dt(obj)
    tendency = lambda v: pc.O.rhs(obj.om, np.ascontiguousarray(v), np.ascontiguousarray(pr.ti), None, np.ascontiguousarray(pr.T))["vl"]
    dt = spec.mult * sd
    J = FJ.bands(pr, dt)
    dtf = dt * tendency(pr.vl)
    d = FJ.tri_solve(*J, dtf)
    q32 = float(np.max(FJ.q(J, FJ.newton_update(pr, dt, dtf / dt, dtype=np.float32), dtf)))
    q_1pc = min(float(np.min(FJ.q(J, FJ.newton_update(pr, dt, dtf / dt, **{k: 1.01}), dtf))) for k in ("dK_scale", "dn_scale"))
    for a in (pr.vl, pr.ti, pr.T, dtf, d) + J:
        a.setflags(write=False)
    return Prepared(spec, obj, pr, dt, tendency, J, dtf, d, q32, q_1pc)
