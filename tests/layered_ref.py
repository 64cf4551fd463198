"""NumPy restatement of the Richards tendency with PER-CELL soil parameters (layered soils), in the
working type of the state: the reference of tests/test_layered_reference.py and tests/test_gpu_layered.py.

The closures are the host functions of landhydrology.jl_amd/parameterizations.py (`effective_saturation`,
`matric_potential` through `pressure_head`, `hydraulic_conductivity`) called with arrays of parameters; the
face conductivity is the arithmetic mean of the two cell-centre conductivities, which is what the reference's
InterpolateC2F gives whatever the two cells' parameters are; the boundary fluxes are the reference's
(boundary_conditions.jl:295-401: VerticalFlux, Dirichlet with both bottom signs, FreeDrainage); SSPRK33 is the
Shu-Osher form.  Test infrastructure: imports neither the oracle nor the HIP library.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

import __graft_entry__ as _g

_pkg = _g.load_package()
P = _pkg.parameterizations
M = _pkg.case_model
grid_np = _pkg.workloads.grid_np

CLASS_FIELDS = ("n", "alpha", "theta_r", "Ksat", "nu", "S_s")


@dataclass
class Layered:
    """A Richards case (workloads.Case: om, dtype, vl, ti, T_aux) with soil classes [ncls, 6] (CLASS_FIELDS
    order, float64 like every parameter of the C ABI) and a class map [ncols, nlev] of indices into them."""
    case: object
    classes: np.ndarray
    class_map: np.ndarray


def cell_params(lay: Layered, class_map=None):
    """The six parameters of every cell, rounded to the working type: name -> [ncols, nlev]."""
    FT = np.dtype(lay.case.dtype).type
    m = np.asarray(lay.class_map if class_map is None else class_map)
    if m.ndim == 1:
        m = np.broadcast_to(m[None, :], (lay.case.ncols, m.shape[0]))
    cls = np.asarray(lay.classes, dtype=np.float64).astype(FT)
    return {k: np.ascontiguousarray(cls[m, j]) for j, k in enumerate(CLASS_FIELDS)}


def _hm(p):
    return SimpleNamespace(n=p["n"], alpha=p["alpha"], theta_r=p["theta_r"], Ksat=p["Ksat"])


def water_closures(cf, p, vl, ti, T):
    """K and psi of cells with parameters p (right_hand_side.jl:156-167): K from the saturation with the
    true porosity, psi from the one with nu_eff = nu - theta_i; the conductivity factors where switched on."""
    FT = vl.dtype.type
    nu_eff = p["nu"] - ti
    visc = imp = FT(1)
    if cf.viscosity_kind:
        visc = P.viscosity_factor(SimpleNamespace(gamma=cf.gamma, T_ref=cf.T_ref), T)
    if cf.impedance_kind:
        tl = P.volumetric_liquid_fraction(vl, nu_eff)
        with np.errstate(invalid="ignore", divide="ignore"):
            f_i = ti / (tl + ti)
        imp = P.impedance_factor(SimpleNamespace(Omega=cf.Omega), f_i)
    S = P.effective_saturation(p["nu"], vl, p["theta_r"])
    K = P.hydraulic_conductivity(_hm(p), S, visc, imp)
    psi = P.pressure_head(_hm(p), vl, nu_eff, p["S_s"])
    return np.asarray(K, FT), np.asarray(psi, FT)


def _bc(om, face, ncols, FT):
    kind, val = om.bc.get((face, M.COMP_HYDROLOGY), (M.BC_NONE, 0.0))
    pc = om.percol_bc.get((face, M.COMP_HYDROLOGY))
    v = np.full(ncols, val, dtype=np.float64) if pc is None else np.asarray(pc, dtype=np.float64)
    return kind, v.astype(FT)


def boundary_flux(om, face, p_cell, vl_c, ti_c, T_c, FT, dz):
    """The water flux of one boundary face of every column, from the boundary cell's own parameters."""
    ncols = vl_c.shape[0]
    kind, val = _bc(om, face, ncols, FT)
    dzb = dz / FT(2)
    if kind == M.BC_FLUX:
        return val.copy()
    if kind == M.BC_FREE_DRAINAGE:
        K_c, _ = water_closures(om.cf, p_cell, vl_c, ti_c, T_c)
        return -K_c
    if kind == M.BC_DIRICHLET:
        _, psi_c = water_closures(om.cf, p_cell, vl_c, ti_c, T_c)
        K_f, psi_f = water_closures(om.cf, p_cell, val, ti_c, T_c)
        if face == M.FACE_BOTTOM and om.consistent_bottom_sign:
            return K_f * (psi_f - psi_c - dzb) / dzb
        flux = -K_f * (psi_f - psi_c + dzb) / dzb
        return -flux if face == M.FACE_BOTTOM else flux
    raise ValueError("the hydrology component needs a boundary condition at both faces")


def rhs(lay: Layered, vl=None, class_map=None, faces=False):
    """d vartheta_l / dt [ncols, nlev] in the working type (and, with faces=True, the bottom and top
    boundary fluxes [ncols] it used)."""
    case, om = lay.case, lay.case.om
    FT = np.dtype(case.dtype).type
    vl = np.asarray(case.vl if vl is None else vl, dtype=FT)
    ti = np.asarray(case.ti, dtype=FT)
    n = om.nlev
    T = np.full_like(vl, FT(288)) if case.T_aux is None else np.asarray(case.T_aux, dtype=FT)
    p = cell_params(lay, class_map)
    zc, _ = grid_np(om.zmin, om.zmax, n, FT)
    dz = (FT(om.zmax) - FT(om.zmin)) / FT(n)
    with np.errstate(all="ignore"):
        K, psi = water_closures(om.cf, p, vl, ti, T)
        h = psi + zc[None, :]
        at = lambda i: {k: v[:, i] for k, v in p.items()}
        f_bot = boundary_flux(om, M.FACE_BOTTOM, at(0), vl[:, 0], ti[:, 0], T[:, 0], FT, dz)
        f_top = boundary_flux(om, M.FACE_TOP, at(n - 1), vl[:, n - 1], ti[:, n - 1], T[:, n - 1], FT, dz)
        F = np.empty((vl.shape[0], n + 1), dtype=FT)
        F[:, 0], F[:, n] = f_bot, f_top
        if n > 1:
            gh = (h[:, 1:] - h[:, :-1]) / dz
            F[:, 1:n] = -((K[:, :-1] + K[:, 1:]) / FT(2)) * gh
        d = -((F[:, 1:] - F[:, :-1]) / dz)
    d = np.ascontiguousarray(d, dtype=FT)
    return (d, f_bot.astype(FT), f_top.astype(FT)) if faces else d


def diagnostics(lay: Layered):
    case = lay.case
    FT = np.dtype(case.dtype).type
    vl, ti = np.asarray(case.vl, FT), np.asarray(case.ti, FT)
    T = np.full_like(vl, FT(288)) if case.T_aux is None else np.asarray(case.T_aux, dtype=FT)
    with np.errstate(all="ignore"):
        K, psi = water_closures(case.om.cf, cell_params(lay), vl, ti, T)
    return dict(K=K, psi=psi)


def ssprk33(lay: Layered, dt, nsteps, vl=None):
    """nsteps SSPRK33 steps (Shu-Osher form) of vartheta_l in the working type; theta_i stays."""
    FT = np.dtype(lay.case.dtype).type
    y = np.array(lay.case.vl if vl is None else vl, dtype=FT)
    dt = FT(dt)
    for _ in range(nsteps):
        u = y + dt * rhs(lay, y)
        u = (FT(3) * y + u + dt * rhs(lay, u)) / FT(4)
        y = (y + FT(2) * u + FT(2) * dt * rhs(lay, u)) / FT(3)
    return y


def stable_dt(lay: Layered, courant=0.5, class_map=None):
    """min over cells of courant dz^2 / D: D = K dpsi/dvl of a boundary cell, twice the larger of the face
    state's and the cell's K times the cell's slope on a Dirichlet face, and on an interior face the mean of
    the two conductivities times the larger slope -- with every cell's own parameters in its slope."""
    case, om = lay.case, lay.case.om
    FT = np.dtype(case.dtype).type
    vl, ti = np.asarray(case.vl, FT), np.asarray(case.ti, FT)
    n = om.nlev
    T = np.full_like(vl, FT(288)) if case.T_aux is None else np.asarray(case.T_aux, dtype=FT)
    p = cell_params(lay, class_map)
    dz = (FT(om.zmax) - FT(om.zmin)) / FT(n)
    with np.errstate(all="ignore"):
        K, psi = water_closures(om.cf, p, vl, ti, T)
        m = FT(1) - FT(1) / p["n"]
        nu_eff = p["nu"] - ti
        Se = P.effective_saturation(nu_eff, vl, p["theta_r"])
        u = Se ** (-FT(1) / m) - FT(1)
        slope = np.abs(psi) * (u + FT(1)) / (p["n"] * m * u * Se * (nu_eff - p["theta_r"]))
        dpsi = np.where((Se <= 1) & (u > 0), slope, FT(1) / p["S_s"]).astype(FT)
        D = np.zeros_like(K)
        for face, i in ((M.FACE_BOTTOM, 0), (M.FACE_TOP, n - 1)):
            D[:, i] = np.maximum(D[:, i], K[:, i] * dpsi[:, i])
            kind, val = _bc(om, face, vl.shape[0], FT)
            if kind == M.BC_DIRICHLET:
                at = {k: v[:, i] for k, v in p.items()}
                K_f, _ = water_closures(om.cf, at, val, ti[:, i], T[:, i])
                D[:, i] = np.maximum(D[:, i], FT(2) * np.maximum(K_f, K[:, i]) * dpsi[:, i])
        if n > 1:
            Dw = (K[:, :-1] + K[:, 1:]) * FT(0.5) * np.maximum(dpsi[:, :-1], dpsi[:, 1:])
            D[:, 1:] = np.maximum(D[:, 1:], Dw)
        dt = courant * float(dz) ** 2 / D[D > 0].astype(np.float64)
    return float(dt.min())


# ------------------------------------------------------------ the cases both test files use

def texture_classes(ncls=16):
    """ncls soil classes spanning sand to clay loam: n 1.25..3.2, alpha 0.8..7, theta_r 0..0.09, nu 0.36..0.52,
    Ksat over five decades (class k and k+1 differ by a factor >= 100 for every odd k: an interface between
    them is the sand-over-clay jump), S_s 5e-4..2e-3.  Deterministic: a function of k only."""
    k = np.arange(ncls, dtype=np.float64)
    s = (k * 0.6180339887498949) % 1.0
    n = 1.25 + 1.95 * ((k * 0.37) % 1.0)
    alpha = 0.8 + 6.2 * s
    theta_r = 0.09 * ((k * 0.23) % 1.0)
    nu = 0.36 + 0.16 * ((k * 0.41) % 1.0)
    Ksat = np.where(k % 2 == 0, 3e-5, 1e-7) * (1.0 + s)   # even: conductive, odd: tight; ratio >= 150
    S_s = 5e-4 + 1.5e-3 * ((k * 0.29) % 1.0)
    return np.stack([n, alpha, theta_r, Ksat, nu, S_s], axis=1)


def percol_from_uniform_map(lay: Layered):
    """The per-column parameter arrays (CaseModel.percol keys) of a map in which every column has one class."""
    m = np.asarray(lay.class_map)
    assert np.all(m == m[:, :1]), "every column must have one class"
    cls = np.asarray(lay.classes, dtype=np.float64)[m[:, 0]]
    keys = ("vg_n", "vg_alpha", "vg_theta_r", "vg_Ksat", "nu", "S_s")
    return {k: np.ascontiguousarray(cls[:, j]) for j, k in enumerate(keys)}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _state_from_potential(lay_classes, class_map, psi, ti, dtype):
    """vartheta_l with the matric potential psi (< 0) in every cell: theta_r + (nu - theta_i - theta_r) S(psi)
    with the cell's own retention curve (inverse_matric_potential), formed in Float64 and rounded once."""
    cls = np.asarray(lay_classes, dtype=np.float64)[class_map]
    n, alpha, thr, nu = cls[..., 0], cls[..., 1], cls[..., 2], cls[..., 4]
    S = P.inverse_matric_potential(SimpleNamespace(n=n, alpha=alpha, theta_r=thr, Ksat=cls[..., 3]), psi)
    return (thr + (nu - ti - thr) * S).astype(dtype)


def make_layered(dtype, ncols, nlev, class_map, classes=None, bc="flux_drain", factors=False, ice=False,
                 zmin=None, name="layered"):
    """A Richards case with a wetting front in the matric potential (continuous across horizons, as in the
    field: K jumps at an interface, psi does not) and the class map given ([ncols, nlev]).
    bc: "flux_drain" (VerticalFlux top, FreeDrainage bottom), "dirichlet" (both faces, the reference's bottom
    sign), "dirichlet_consistent" (the consistent bottom sign), "flux" (VerticalFlux at both faces)."""
    W = _pkg.workloads
    classes = texture_classes() if classes is None else np.asarray(classes, dtype=np.float64)
    class_map = np.ascontiguousarray(class_map, dtype=np.uint8)
    assert class_map.shape == (ncols, nlev)
    zmin = -0.02 * nlev if zmin is None else zmin
    H, top, bot = M.COMP_HYDROLOGY, M.FACE_TOP, M.FACE_BOTTOM
    bcs = {"flux_drain": {(top, H): (M.BC_FLUX, -2e-8), (bot, H): (M.BC_FREE_DRAINAGE, 0.0)},
           "dirichlet": {(top, H): (M.BC_DIRICHLET, 0.30), (bot, H): (M.BC_DIRICHLET, 0.26)},
           "dirichlet_consistent": {(top, H): (M.BC_DIRICHLET, 0.30), (bot, H): (M.BC_DIRICHLET, 0.26)},
           "flux": {(top, H): (M.BC_FLUX, -1e-8), (bot, H): (M.BC_FLUX, 3e-9)}}[bc]
    om = M.CaseModel(M.MODEL_RICHARDS, nlev, zmin, 0.0, bc=bcs, cf=M.default_cf(viscosity=factors, impedance=factors),
                     consistent_bottom_sign=(bc == "dirichlet_consistent"))
    zc, _ = grid_np(zmin, 0.0, nlev)
    c = np.arange(ncols)
    zf = zmin + (0.2 + 0.6 * W.uhash(c, 0, nlev)) * (0.0 - zmin)
    psi = -0.25 - 2.5 * (1.0 - _sigmoid((zc[None, :] - zf[:, None]) / 0.1))     # wet above the front, dry below
    ti = np.zeros((ncols, nlev))
    if ice:
        ti = np.where(W.uhash(c, 1, nlev)[:, None] < 0.5, 0.05 * W.uhash(c[:, None], np.arange(nlev)[None, :] + 17, 1000), 0.0)
    vl = _state_from_potential(classes, class_map, psi, ti, dtype)
    T = None
    if factors:
        T = (278.0 + 20.0 * W.uhash(c[:, None], np.arange(nlev)[None, :] + 50, 1000)).astype(dtype)
    case = W.Case(name, om, dtype, ncols, vl=vl, ti=ti.astype(dtype), T_aux=T)
    return Layered(case, classes, class_map)


def uniform_map(ncols, nlev, ncls=16):
    """every column one class: column c has class c mod ncls"""
    return np.repeat((np.arange(ncols) % ncls).astype(np.uint8)[:, None], nlev, axis=1)


def horizon_map(ncols, nlev, ncls=16):
    """Up to four horizons of unequal thickness that differ per column; the horizons of a column alternate
    between a conductive (even) and a tight (odd) class, so every interface is a Ksat jump >= 100
    (texture_classes; with all 16 classes).  Columns shorter than four levels get as many horizons as they have levels."""
    W = _pkg.workloads
    c = np.arange(ncols)
    m = np.zeros((ncols, nlev), dtype=np.uint8)
    nh = min(4, nlev)
    cuts = np.sort(np.stack([1 + (W.uhash(c, 31 + k, 1) * max(nlev - 1, 1)).astype(int) for k in range(nh - 1)], axis=1),
                   axis=1) if nh > 1 else np.zeros((ncols, 0), int)
    lev = np.arange(nlev)[None, :]
    hor = np.zeros((ncols, nlev), dtype=int)
    for k in range(nh - 1):
        hor += (lev >= cuts[:, k:k + 1]).astype(int)
    pairs = max(ncls // 2, 1)
    for h in range(nh):
        pick = (W.uhash(c, 41 + h, 1) * pairs).astype(int)
        if ncls >= 16:
            cls = (2 * pick + ((h + c) % 2)) % ncls
        else:   # fewer classes: any of them (no promise about the jump), still a different one per horizon where it can be
            cls = ((W.uhash(c, 41 + h, 1) * ncls).astype(int) + h) % ncls
        m = np.where(hor == h, cls[:, None], m)
    return np.ascontiguousarray(m, dtype=np.uint8)


def bottom_class_map(class_map):
    """the column-uniform twin of a map: every column's map set to its bottom class"""
    m = np.asarray(class_map)
    return np.ascontiguousarray(np.repeat(m[:, :1], m.shape[1], axis=1))


def with_percol(lay: Layered):
    """The same case with the (column-uniform) map expressed as per-column parameter arrays: what the CPU
    oracle and the per-column kernels take."""
    import copy
    case = copy.copy(lay.case)
    case.om = copy.deepcopy(lay.case.om)
    case.om.percol = percol_from_uniform_map(lay)
    return case


def hydrostatic(dtype, h0=-2.0, nlev=64, shift=0):
    """One 64-level column, three horizons (sand / clay loam / sand: Ksat ratios >= 150), in hydrostatic
    equilibrium psi = h0 - z for the UNSHIFTED map; shift moves the map by that many levels and leaves the
    state, which then sits in the wrong horizon next to each interface."""
    classes = texture_classes()[[0, 5, 2]]
    assert classes[0, 3] / classes[1, 3] >= 100 and classes[2, 3] / classes[1, 3] >= 100
    base = np.zeros(nlev, dtype=np.uint8)
    base[nlev * 5 // 16:] = 1
    base[nlev * 11 // 16:] = 2
    zmin = -0.02 * nlev
    zc, _ = grid_np(zmin, 0.0, nlev)
    vl = _state_from_potential(classes, base[None, :], (h0 - zc)[None, :], np.zeros((1, nlev)), dtype)
    H = M.COMP_HYDROLOGY
    om = M.CaseModel(M.MODEL_RICHARDS, nlev, zmin, 0.0, bc={(M.FACE_TOP, H): (M.BC_FLUX, 0.0), (M.FACE_BOTTOM, H): (M.BC_FLUX, 0.0)})
    case = _pkg.workloads.Case("layered_hydrostatic", om, dtype, 1, vl=vl, ti=np.zeros((1, nlev), dtype))
    m = np.roll(base, shift)
    if shift > 0:
        m[:shift] = base[0]
    return Layered(case, classes, m[None, :].copy())
