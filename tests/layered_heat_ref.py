"""NumPy restatement of the layered COUPLED and HEAT-ONLY tendency: per-cell soil classes with a thermal
supplement, in the working type of the state.  The reference of tests/test_layered_heat_reference.py and
tests/test_gpu_layered_heat.py.

The water closures are tests/layered_ref.py's; the heat closures are the host functions of
landhydrology.jl_amd/parameterizations.py (`volumetric_heat_capacity`, `temperature_from_rhoe_int`,
`relative_saturation`, `kersten_number`, `saturated_thermal_conductivity`, `k_dry`, `thermal_conductivity`,
`volumetric_internal_energy_liq`) called once per class on that class's cells.  kappa and rho_e_int_l K go to
the faces through the same arithmetic mean as K (right_hand_side.jl:259, :361-365); the boundary fluxes are the
reference's (boundary_conditions.jl:295-444), a Dirichlet energy face taking kappa from the BOUNDARY CELL's own
class.  Test infrastructure: imports neither the oracle nor the HIP library.
"""
from __future__ import annotations

import copy
import dataclasses
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import layered_ref as R

P, M, grid_np, _pkg = R.P, R.M, R.grid_np, R._pkg

THERMAL_FIELDS = ("rho_c_ds", "kappa_solid", "rho_p", "kappa_sat_unfrozen", "kappa_sat_frozen", "nu_ss_gravel",
                  "nu_ss_om", "nu_ss_quartz")


@dataclass
class LayeredHeat:
    """A coupled or heat-only case (workloads.Case: om, dtype, vl, ti, rhoe) with soil classes [ncls, 6]
    (layered_ref.CLASS_FIELDS), their thermal supplement [ncls, 8] (THERMAL_FIELDS) and a class map
    [ncols, nlev].  Reads like a layered_ref.Layered wherever only the hydraulic side is used."""
    case: object
    classes: np.ndarray
    thermal: np.ndarray
    class_map: np.ndarray


def _ps(om):
    e = om.earth
    return SimpleNamespace(rho_cloud_liq=e.rho_liq, rho_cloud_ice=e.rho_ice, cp_l=e.cp_l, cp_i=e.cp_i, T_0=e.T_0,
                           LH_f0=e.LH_f0, K_therm=e.K_therm)


def _full_map(lay, class_map=None):
    m = np.asarray(lay.class_map if class_map is None else class_map)
    if m.ndim == 1:
        m = np.broadcast_to(m[None, :], (lay.case.ncols, m.shape[0]))
    return m


def class_soil(lay, k, FT):
    """the SoilParams-like object of class k: the context's scalars with the class's nu, S_s and thermal fields"""
    sp = copy.copy(lay.case.om.soil)
    sp.nu, sp.S_s = float(lay.classes[k, 4]), float(lay.classes[k, 5])
    for j, name in enumerate(THERMAL_FIELDS):
        setattr(sp, name, float(lay.thermal[k, j]))
    sp.FT = FT
    return sp


def heat_closures(lay, m, vl, ti, rhoe):
    """T, kappa and rho_c_s of cells whose classes are m (same shape as vl), class by class"""
    FT = vl.dtype.type
    ps = _ps(lay.case.om)
    T, kap, rcs = (np.zeros_like(vl) for _ in range(3))
    with np.errstate(all="ignore"):
        for k in np.unique(m):
            sel = m == k
            sp = class_soil(lay, int(k), FT)
            nu = FT(sp.nu)
            v, i, e = vl[sel], ti[sel], rhoe[sel]
            tl = P.volumetric_liquid_fraction(v, nu - i)
            c = P.volumetric_heat_capacity(tl, i, FT(sp.rho_c_ds), ps)
            T[sel] = P.temperature_from_rhoe_int(e, i, c, ps)
            Ke = P.kersten_number(i, P.relative_saturation(tl, i, nu), sp)
            ks = P.saturated_thermal_conductivity(tl, i, sp.kappa_sat_unfrozen, sp.kappa_sat_frozen)
            kap[sel] = P.thermal_conductivity(P.k_dry(ps, sp), Ke, ks)
            rcs[sel] = c
    return T, kap, rcs


def _bcv(om, face, comp, ncols, FT):
    kind, val = om.bc.get((face, comp), (M.BC_NONE, 0.0))
    pc = om.percol_bc.get((face, comp))
    v = np.full(ncols, val, dtype=np.float64) if pc is None else np.asarray(pc, dtype=np.float64)
    return kind, v.astype(FT)


def _fields(lay, vl=None, rhoe=None):
    case = lay.case
    FT = np.dtype(case.dtype).type
    return (np.asarray(case.vl if vl is None else vl, dtype=FT), np.asarray(case.ti, dtype=FT),
            np.asarray(case.rhoe if rhoe is None else rhoe, dtype=FT))


def _cells(lay, vl, ti, rhoe, class_map=None):
    """every cell's closures: dict(K, psi, T, kappa, rcs) and the per-cell hydraulic parameters"""
    om = lay.case.om
    m = _full_map(lay, class_map)
    p = R.cell_params(lay, class_map)
    T, kap, rcs = heat_closures(lay, m, vl, ti, rhoe)
    K = psi = None
    if om.model != M.MODEL_HEAT:
        with np.errstate(all="ignore"):
            K, psi = R.water_closures(om.cf, p, vl, ti, T)
    return dict(K=K, psi=psi, T=T, kappa=kap, rcs=rcs), p, m


def boundary_fluxes(lay, face, d, p, m, vl, ti, rhoe):
    """(f_energy, f_water) of one face of every column from the boundary cell's own class"""
    om = lay.case.om
    FT = vl.dtype.type
    n, N = om.nlev, vl.shape[0]
    i = 0 if face == M.FACE_BOTTOM else n - 1
    water = om.model != M.MODEL_HEAT
    dz = (FT(om.zmax) - FT(om.zmin)) / FT(n)
    dzb = dz / FT(2)
    sgn = FT(-1) if face == M.FACE_BOTTOM else FT(1)
    ke, ve = _bcv(om, face, M.COMP_ENERGY, N, FT)
    kh, vh = _bcv(om, face, M.COMP_HYDROLOGY, N, FT)
    at = {k: v[:, i] for k, v in p.items()}
    T_c = d["T"][:, i]
    T_f = ve if ke == M.BC_DIRICHLET else T_c
    vl_f = vh if (water and kh == M.BC_DIRICHLET) else vl[:, i]
    fe, fw = np.full(N, np.nan, FT), np.full(N, np.nan, FT)
    with np.errstate(all="ignore"):
        if ke == M.BC_FLUX:
            fe = ve.copy()
        elif ke == M.BC_DIRICHLET:
            _, kap_f, _ = heat_closures(lay, m[:, i], vl_f, ti[:, i], rhoe[:, i])
            fe = sgn * ((-kap_f * (ve - T_c)) / dzb)
        if water:
            if kh == M.BC_FLUX:
                fw = vh.copy()
            elif kh == M.BC_FREE_DRAINAGE:
                fw = -d["K"][:, i]
            elif kh == M.BC_DIRICHLET:
                K_f, psi_f = R.water_closures(om.cf, at, vh, ti[:, i], T_f)
                psi_c = d["psi"][:, i]
                if face == M.FACE_BOTTOM and om.consistent_bottom_sign:
                    fw = K_f * (psi_f - psi_c - dzb) / dzb
                else:
                    fw = sgn * (-K_f * (psi_f - psi_c + dzb) / dzb)
    return fe.astype(FT), fw.astype(FT)


def rhs(lay, vl=None, rhoe=None, class_map=None, faces=False):
    """dict(vl=..., rhoe=...) of tendencies [ncols, nlev] in the working type (heat-only: rhoe alone); with
    faces=True also dict(face -> (f_energy, f_water)) of the boundary fluxes it used."""
    om = lay.case.om
    FT = np.dtype(lay.case.dtype).type
    vl, ti, rhoe = _fields(lay, vl, rhoe)
    n = om.nlev
    water = om.model != M.MODEL_HEAT
    d, p, m = _cells(lay, vl, ti, rhoe, class_map)
    zc, _ = grid_np(om.zmin, om.zmax, n, FT)
    dz = (FT(om.zmax) - FT(om.zmin)) / FT(n)
    bot = boundary_fluxes(lay, M.FACE_BOTTOM, d, p, m, vl, ti, rhoe)
    top = boundary_fluxes(lay, M.FACE_TOP, d, p, m, vl, ti, rhoe)
    N = vl.shape[0]
    Fe, Fw = np.empty((N, n + 1), FT), np.zeros((N, n + 1), FT)
    Fe[:, 0], Fe[:, n] = bot[0], top[0]
    with np.errstate(all="ignore"):
        gh = None
        if water:
            Fw[:, 0], Fw[:, n] = bot[1], top[1]
            h = d["psi"] + zc[None, :]
            E = P.volumetric_internal_energy_liq(d["T"], _ps(om)) * d["K"]
        if n > 1:
            gT = (d["T"][:, 1:] - d["T"][:, :-1]) / dz
            Fe[:, 1:n] = -((d["kappa"][:, :-1] + d["kappa"][:, 1:]) / FT(2)) * gT
            if water:
                gh = (h[:, 1:] - h[:, :-1]) / dz
                Fw[:, 1:n] = -((d["K"][:, :-1] + d["K"][:, 1:]) / FT(2)) * gh
                Fe[:, 1:n] = Fe[:, 1:n] - ((E[:, :-1] + E[:, 1:]) / FT(2)) * gh
        out = dict(rhoe=np.ascontiguousarray(-((Fe[:, 1:] - Fe[:, :-1]) / dz), dtype=FT))
        if water:
            out["vl"] = np.ascontiguousarray(-((Fw[:, 1:] - Fw[:, :-1]) / dz), dtype=FT)
    return (out, {M.FACE_BOTTOM: bot, M.FACE_TOP: top}) if faces else out


def diagnostics(lay):
    vl, ti, rhoe = _fields(lay)
    d, _, _ = _cells(lay, vl, ti, rhoe)
    return d


def ssprk33(lay, dt, nsteps):
    """nsteps SSPRK33 steps (Shu-Osher form) of (vartheta_l, rhoe_int) in the working type: dict(vl, rhoe);
    the heat-only model keeps its prescribed vartheta_l"""
    FT = np.dtype(lay.case.dtype).type
    water = lay.case.om.model != M.MODEL_HEAT
    y = dict(vl=np.array(lay.case.vl, dtype=FT), rhoe=np.array(lay.case.rhoe, dtype=FT))
    keys = ("vl", "rhoe") if water else ("rhoe",)
    dt = FT(dt)
    f = lambda s: rhs(lay, s["vl"], s["rhoe"])
    for _ in range(nsteps):
        k = f(y)
        u = dict(y)
        for q in keys:
            u[q] = y[q] + dt * k[q]
        k = f(u)
        for q in keys:
            u[q] = (FT(3) * y[q] + u[q] + dt * k[q]) / FT(4)
        k = f(u)
        y = dict(y)
        for q in keys:
            y[q] = (y[q] + FT(2) * u[q] + FT(2) * dt * k[q]) / FT(3)
    return y


def stable_dt(lay, courant=0.5, class_map=None, parts=False):
    """min over cells of courant dz^2 / D, stable_dt_kernel's rule with every cell's own class: the water
    coefficient as layered_ref.stable_dt; the heat coefficient kappa / rho_c_s of a boundary cell, twice the
    larger of the face state's and the cell's kappa over the cell's rho_c_s on a Dirichlet face, and on an
    interior face the mean kappa over the smaller rho_c_s.  parts=True: (dt, dt of the water alone, of the heat alone)."""
    om = lay.case.om
    FT = np.dtype(lay.case.dtype).type
    vl, ti, rhoe = _fields(lay)
    n, N = om.nlev, vl.shape[0]
    water = om.model != M.MODEL_HEAT
    d, p, m = _cells(lay, vl, ti, rhoe, class_map)
    dz = (FT(om.zmax) - FT(om.zmin)) / FT(n)
    kap, rcs, T = d["kappa"], d["rcs"], d["T"]
    Dw, Dh = np.zeros_like(kap), np.zeros_like(kap)
    with np.errstate(all="ignore"):
        if water:
            K, psi = d["K"], d["psi"]
            mm = FT(1) - FT(1) / p["n"]
            nu_eff = p["nu"] - ti
            Se = P.effective_saturation(nu_eff, vl, p["theta_r"])
            u = Se ** (-FT(1) / mm) - FT(1)
            slope = np.abs(psi) * (u + FT(1)) / (p["n"] * mm * u * Se * (nu_eff - p["theta_r"]))
            dpsi = np.where((Se <= 1) & (u > 0), slope, FT(1) / p["S_s"]).astype(FT)
        for face, i in ((M.FACE_BOTTOM, 0), (M.FACE_TOP, n - 1)):
            ke, ve = _bcv(om, face, M.COMP_ENERGY, N, FT)
            kh, vh = _bcv(om, face, M.COMP_HYDROLOGY, N, FT)
            vl_f = vh if (water and kh == M.BC_DIRICHLET) else vl[:, i]
            T_f = ve if ke == M.BC_DIRICHLET else T[:, i]
            Dh[:, i] = np.maximum(Dh[:, i], kap[:, i] / rcs[:, i])
            if ke == M.BC_DIRICHLET:
                _, kf, _ = heat_closures(lay, m[:, i], vl_f, ti[:, i], rhoe[:, i])
                Dh[:, i] = np.maximum(Dh[:, i], FT(2) * np.maximum(kf, kap[:, i]) / rcs[:, i])
            if water:
                Dw[:, i] = np.maximum(Dw[:, i], K[:, i] * dpsi[:, i])
                if kh == M.BC_DIRICHLET:
                    at = {k: v[:, i] for k, v in p.items()}
                    K_f, _ = R.water_closures(om.cf, at, vh, ti[:, i], T_f)
                    Dw[:, i] = np.maximum(Dw[:, i], FT(2) * np.maximum(K_f, K[:, i]) * dpsi[:, i])
        if n > 1:
            Dh[:, 1:] = np.maximum(Dh[:, 1:], (kap[:, :-1] + kap[:, 1:]) * FT(0.5) / np.minimum(rcs[:, :-1], rcs[:, 1:]))
            if water:
                Dw[:, 1:] = np.maximum(Dw[:, 1:], (K[:, :-1] + K[:, 1:]) * FT(0.5) * np.maximum(dpsi[:, :-1], dpsi[:, 1:]))
        lim = lambda D: float((courant * float(dz) ** 2 / D[D > 0].astype(np.float64)).min()) if np.any(D > 0) else np.inf
        both = lim(np.maximum(Dw, Dh))
    return (both, lim(Dw), lim(Dh)) if parts else both


# ------------------------------------------------------------ the cases both test files use

def thermal_classes(ncls=16):
    """ncls thermal supplements whose neighbours differ clearly: rho_c_ds 1.0e6..2.4e6, kappa_sat_unfrozen
    0.6..2.6, kappa_sat_frozen 1.6..4.4, kappa_solid 2..7.5, rho_p 1300..2700; every third class is organic
    (nu_ss_om 0.15..0.45, the others 0), quartz and gravel fractions vary.  Deterministic: a function of k only."""
    k = np.arange(ncls, dtype=np.float64)
    f = lambda a: (k * a) % 1.0
    rho_c_ds = 1.0e6 + 1.4e6 * f(0.6180339887498949)
    kappa_solid = 2.0 + 5.5 * f(0.37)
    rho_p = 1300.0 + 1400.0 * f(0.29)
    ksu = 0.6 + 2.0 * f(0.43)
    ksf = ksu + 1.0 + 0.8 * f(0.71)
    om = np.where(k % 3 == 1, 0.15 + 0.3 * f(0.53), 0.0)
    quartz = (0.1 + 0.7 * f(0.31)) * (1.0 - om)
    gravel = 0.1 * f(0.47) * (1.0 - om)
    return np.stack([rho_c_ds, kappa_solid, rho_p, ksu, ksf, gravel, om, quartz], axis=1)


def _temperature_field(ncols, nlev, zc, ice):
    """a smooth T(z) per column, 276..290 K (ice: 268..282 K in the columns that carry ice)"""
    W = _pkg.workloads
    c = np.arange(ncols)
    ph = 6.28 * W.uhash(c, 61, nlev)[:, None]
    return 283.0 + 6.0 * np.cos(2.5 * zc[None, :] / max(abs(zc[0]), 1e-30) + ph) + 1.0 * W.uhash(c, 62, nlev)[:, None]


def rhoe_from_T(lay_classes, thermal, class_map, om, vl, ti, T, dtype):
    """rho e_int with temperature T in every cell, through the cell's own rho_c_ds and nu (Float64, rounded once)"""
    cls = np.asarray(lay_classes, np.float64)[class_map]
    th = np.asarray(thermal, np.float64)[class_map]
    e = om.earth
    tl = np.minimum(vl.astype(np.float64), cls[..., 4] - ti)
    rcs = th[..., 0] + tl * (e.cp_l * e.rho_liq) + ti * (e.cp_i * e.rho_ice)
    return (rcs * (T - e.T_0) - ti * e.rho_ice * e.LH_f0).astype(dtype)


ENERGY_BC = {"flux": ((M.BC_FLUX, 0.03), (M.BC_FLUX, -0.8)),
             "flux_drain": ((M.BC_FLUX, 0.03), (M.BC_FLUX, -0.8)),
             "dirichlet": ((M.BC_DIRICHLET, 281.0), (M.BC_DIRICHLET, 287.0)),
             "dirichlet_consistent": ((M.BC_DIRICHLET, 281.0), (M.BC_DIRICHLET, 287.0))}


# The boundary conditions of the per-cell (horizon map) cases that are compared in units of the field's largest
# tendency (parity_cases.PLAIN_REL).  Float32 resolves T = T_ref + rho e_int / rho_c_s to one ulp of 285 K, 3e-5 K,
# whatever the state; across dz = 0.02 m that is kappa 3e-5 / dz^2 = 0.08 W/m^3 of energy tendency in any
# implementation, the reference included.  The coupled model's field scale (1e5: the advected rho_e_l K at the
# Ksat jumps) is far above that; the heat-only model's smooth conduction (1e3) is not, so its case takes Dirichlet
# faces, whose 5 K across half a cell give the boundary cells 2e4.
PER_CELL_BC = {M.MODEL_COUPLED: "flux_drain", M.MODEL_HEAT: "dirichlet"}


def make_layered_heat(dtype, ncols, nlev, class_map, model=M.MODEL_COUPLED, classes=None, thermal=None, bc="flux_drain",
                      factors=False, ice=False, zmin=None, T=None, name="layered_heat"):
    """layered_ref.make_layered's water state (a wetting front in psi, continuous across horizons) with a smooth
    temperature field turned into rho e_int through every cell's own class; bc as there, the energy component a
    flux at both faces ("flux", "flux_drain") or Dirichlet at both (the Dirichlet cases).  model: coupled or
    heat-only (which keeps the water state as its prescribed vartheta_l, theta_i and only the energy component of bc)."""
    lay = R.make_layered(dtype, ncols, nlev, class_map, classes=classes, bc=bc, factors=factors, ice=ice, zmin=zmin, name=name)
    case, om = lay.case, lay.case.om
    thermal = thermal_classes(len(lay.classes)) if thermal is None else np.asarray(thermal, np.float64)
    assert thermal.shape == (len(lay.classes), len(THERMAL_FIELDS))
    om = dataclasses.replace(om, model=model, bc=dict(om.bc))
    (kb, vb), (kt, vt) = ENERGY_BC[bc]
    om.bc[(M.FACE_BOTTOM, M.COMP_ENERGY)] = (kb, vb)
    om.bc[(M.FACE_TOP, M.COMP_ENERGY)] = (kt, vt)
    if model == M.MODEL_HEAT:
        om.bc = {k: v for k, v in om.bc.items() if k[1] == M.COMP_ENERGY}
        om.cf = M.default_cf()
        om.consistent_bottom_sign = False
    zc, _ = grid_np(om.zmin, om.zmax, nlev)
    Tf = _temperature_field(ncols, nlev, zc, ice) if T is None else np.broadcast_to(np.asarray(T, np.float64), (ncols, nlev))
    if ice:   # the columns that carry ice are cold
        Tf = np.where(np.any(case.ti != 0, axis=1)[:, None], Tf - 12.0, Tf)
    rhoe = rhoe_from_T(lay.classes, thermal, lay.class_map, om, case.vl, case.ti.astype(np.float64), Tf, dtype)
    case = dataclasses.replace(case, om=om, rhoe=rhoe, T_aux=None)
    return LayeredHeat(case, lay.classes, thermal, lay.class_map)


def class_scalar_case(lay, k, cols):
    """The columns `cols` (all of class k at every level) as a case WITHOUT classes: the context's scalars are the
    class's numbers -- what the oracle and the scalar kernels take."""
    om = copy.deepcopy(lay.case.om)
    c = lay.classes[k]
    om.vg = M.VGParams(n=float(c[0]), alpha=float(c[1]), theta_r=float(c[2]), Ksat=float(c[3]))
    om.soil = class_soil(lay, k, np.float64)
    del om.soil.FT
    om.percol_bc = {key: np.asarray(v)[cols] for key, v in om.percol_bc.items()}
    take = lambda a: None if a is None else np.ascontiguousarray(a[cols])
    return dataclasses.replace(lay.case, om=om, ncols=len(cols), vl=take(lay.case.vl), ti=take(lay.case.ti),
                               rhoe=take(lay.case.rhoe), T_aux=None)


def per_class_cases(lay):
    """[(columns, scalar case)] of a column-uniform map, one entry per class present"""
    m = np.asarray(lay.class_map)
    assert np.all(m == m[:, :1]), "every column must have one class"
    return [(np.flatnonzero(m[:, 0] == k), class_scalar_case(lay, int(k), np.flatnonzero(m[:, 0] == k))) for k in np.unique(m[:, 0])]


def as64(lay):
    c = lay.case
    case = dataclasses.replace(c, dtype=np.float64, vl=c.vl.astype(np.float64), ti=c.ti.astype(np.float64),
                               rhoe=c.rhoe.astype(np.float64))
    return LayeredHeat(case, lay.classes, lay.thermal, lay.class_map)


T_REST = float(np.float32(273.16)) + 16.0


def isothermal_hydrostatic(dtype, model=M.MODEL_COUPLED, T0=T_REST, h0=-2.0, nlev=64, shift=0):
    """layered_ref.hydrostatic's column (three horizons, psi = h0 - z for the unshifted map, zero-flux faces) at
    the uniform temperature T0: rho e_int jumps at the horizons through the class's rho_c_ds and nu.  shift moves
    the map and leaves the state.  T0 is T_ref + 16 K with T_ref as Float32 holds it, a number both working
    types represent: T = T_ref + rho e_int / rho_c_s then rounds to T0 itself in every cell (the quotient's
    error, 2e-6 K in Float32, is far below half an ulp of T, 1.5e-5 K), so the column is isothermal in the
    working type and not only in exact arithmetic."""
    base = R.hydrostatic(dtype, h0=h0, nlev=nlev, shift=0)
    thermal = thermal_classes()[[0, 4, 2]]
    assert thermal[1, 6] > 0 and thermal[0, 6] == 0      # an organic horizon between two mineral ones
    om = dataclasses.replace(base.case.om, model=model, bc=dict(base.case.om.bc))
    for f in (M.FACE_BOTTOM, M.FACE_TOP):
        om.bc[(f, M.COMP_ENERGY)] = (M.BC_FLUX, 0.0)
    if model == M.MODEL_HEAT:
        om.bc = {k: v for k, v in om.bc.items() if k[1] == M.COMP_ENERGY}
    ti = np.zeros((1, nlev))
    rhoe = rhoe_from_T(base.classes, thermal, base.class_map, om, base.case.vl, ti, np.full((1, nlev), T0), dtype)
    case = dataclasses.replace(base.case, om=om, rhoe=rhoe)
    m = R.hydrostatic(dtype, h0=h0, nlev=nlev, shift=shift).class_map
    return LayeredHeat(case, base.classes, thermal, m)
