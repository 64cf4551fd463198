"""The closed forms of the soil closures and of one tendency evaluation in `mpmath`, cell by cell, and the
fixtures under tests/golden/exact/ made from them.

A THIRD statement of the formulas (after the reference and oracle/lh_oracle_impl.inc, whose citations of
SoilWaterParameterizations.jl, SoilHeatParameterizations.jl, right_hand_side.jl and boundary_conditions.jl
apply line by line): plain Python on `mpf` numbers at 200 bits, no vectorisation.  The oracle follows the
reference op for op in the working type, so where the reference's own arithmetic loses its digits (1 - (1 -
S^(1/m))^m for a dry cell, S^(-1/m) beyond the range of the type) a comparison with the oracle compares noise
with noise; this one has the digits, so nothing has to be masked.

Inputs are the numbers the device holds: states and parameters ROUNDED TO THE WORKING TYPE first and then taken
as exact.  The one computed constant of the contract, theta_r + eps(FT) (effective_saturation's clamp), is formed
in the working type as the reference forms it; m = 1 - 1/n, Delta z, rho c_p and every other derived constant is
exact.  `mpmath` is imported inside the functions only: the GPU tests import this module for the case builders,
the bounds' record and the fixture reader, and run where `mpmath` may not be installed.

Bounds (section "bounds" below): every constant is the project's (tests/parity_cases.py) or derived here.
"""
from __future__ import annotations

import copy
import functools
import os
import sys

import numpy as np

import parity_cases as pc

M = pc.M
ROOT = pc.ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))

PREC = 200
GOLDEN = os.path.join(ROOT, "tests", "golden", "exact")
THERMAL_FIELDS = ("rho_c_ds", "kappa_solid", "rho_p", "kappa_sat_unfrozen", "kappa_sat_frozen", "nu_ss_gravel",
                  "nu_ss_om", "nu_ss_quartz")


class Undefined(Exception):
    """the closed form has no value for this input (0/0 in the impedance factor, a negative base of a power)"""


def _mp():
    import mpmath
    return mpmath


def _ft(x, dtype):
    """x rounded to the working type, as a Python float"""
    return float(np.dtype(dtype).type(x))


def to_float(x):
    """an mpf rounded to Float64 (to nearest; +-Inf beyond the range)"""
    try:
        return float(x)
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


# ------------------------------------------------------------------ parameters of one cell

def _hydraulic(mp, dtype, n, alpha, theta_r, Ksat, nu, S_s):
    FT = np.dtype(dtype).type
    r = lambda v: mp.mpf(_ft(v, dtype))
    p = dict(n=r(n), alpha=r(alpha), thr=r(theta_r), Ksat=r(Ksat), nu=r(nu), S_s=r(S_s))
    p["m"] = 1 - 1 / p["n"]
    p["lim"] = mp.mpf(float(FT(theta_r) + FT(np.finfo(dtype).eps)))     # theta_r + eps(FT), IN the working type
    return p


def _thermal(mp, dtype, soil, over=None):
    r = lambda v: mp.mpf(_ft(v, dtype))
    t = {k: r(getattr(soil, k)) for k in THERMAL_FIELDS + ("a", "b", "kappa_dry_parameter")}
    if over is not None:
        for j, k in enumerate(THERMAL_FIELDS):
            t[k] = r(over[j])
    return t


def _earth(mp, dtype, e):
    r = lambda v: mp.mpf(_ft(v, dtype))
    d = dict(rho_l=r(e.rho_liq), rho_i=r(e.rho_ice), T0=r(e.T_0), LH_f0=r(e.LH_f0), k_air=r(e.K_therm))
    d["rhocp_l"] = mp.mpf(e.cp_l) * d["rho_l"]       # cp_l(param_set) is a Float64 constant of the reference
    d["rhocp_i"] = mp.mpf(e.cp_i) * d["rho_i"]
    return d


class Params:
    """per-cell parameters of a case: p.hyd(c, i), p.th(c, i) -> dicts of mpf (cached per column or class)"""

    def __init__(self, mp, case, classes=None, thermal=None, class_map=None):
        self.mp, self.case, self.om, self.dtype = mp, case, case.om, case.dtype
        self.classes, self.thermal = classes, thermal
        self.cmap = None
        if class_map is not None:
            m = np.asarray(class_map)
            self.cmap = np.broadcast_to(m[None, :], (case.ncols, m.shape[0])) if m.ndim == 1 else m
        self._h, self._t = {}, {}
        self.earth = _earth(mp, self.dtype, self.om.earth)
        cf = self.om.cf
        r = lambda v: mp.mpf(_ft(v, self.dtype))
        self.cf = dict(visc=bool(cf.viscosity_kind), imp=bool(cf.impedance_kind), gamma=r(cf.gamma), T_ref=r(cf.T_ref),
                       Omega=r(cf.Omega))

    def _key(self, c, i):
        return ("k", int(self.cmap[c, i])) if self.cmap is not None else ("c", c)

    def hyd(self, c, i):
        key = self._key(c, i)
        if key not in self._h:
            om = self.om
            if key[0] == "k":
                self._h[key] = _hydraulic(self.mp, self.dtype, *[float(x) for x in self.classes[key[1]]])
            else:
                g = lambda name, dflt: float(om.percol[name][c]) if name in om.percol else dflt
                self._h[key] = _hydraulic(self.mp, self.dtype, g("vg_n", om.vg.n), g("vg_alpha", om.vg.alpha),
                                          g("vg_theta_r", om.vg.theta_r), g("vg_Ksat", om.vg.Ksat), g("nu", om.soil.nu),
                                          g("S_s", om.soil.S_s))
        return self._h[key]

    def th(self, c, i):
        key = self._key(c, i) if self.thermal is not None else ("s",)
        if key not in self._t:
            self._t[key] = _thermal(self.mp, self.dtype, self.om.soil, None if key == ("s",) else self.thermal[key[1]])
        return self._t[key]


# ------------------------------------------------------------------ closures

def water_closures(mp, h, cf, vl, ti, T):
    """K and psi of one cell (right_hand_side.jl:156-167, :291-314) and the sub-expressions the bounds read.
    K takes S from the true porosity nu, psi takes Se from nu_eff = nu - theta_i; above Se = 1 psi is the
    saturated branch (vl - nu_eff)/S_s.  1 - (1 - t)^m and S^(-1/m) - 1 are formed through log1p / expm1: the
    plain forms lose |log2 t| of the 200 bits (a bone-dry clay cell has t = 1e-550)."""
    nu, thr, m, n = h["nu"], h["thr"], h["m"], h["n"]
    nu_eff = nu - ti
    tl = vl if vl < nu_eff else nu_eff
    vls = vl if vl > h["lim"] else h["lim"]
    S = (vls - thr) / (nu - thr)
    if S < 1:
        lnS = mp.log(S)
        t = mp.exp(lnS / m)
        w = 1 - t
        inner = -mp.expm1(m * mp.log1p(-t))
        Kr = mp.sqrt(S) * inner ** 2
    else:
        lnS, t, w, inner, Kr = mp.log(S), mp.mpf(1), mp.mpf(0), mp.mpf(1), mp.mpf(1)
    visc, imp, f_i = mp.mpf(1), mp.mpf(1), mp.mpf(0)
    if cf["visc"]:
        visc = mp.exp(cf["gamma"] * (T - cf["T_ref"]))
    if cf["imp"]:
        if tl + ti == 0:
            raise Undefined("f_i = 0/0")
        f_i = ti / (tl + ti)
        imp = mp.mpf(10) ** (-cf["Omega"] * f_i)
    Kfac = h["Ksat"] * visc * imp
    if not nu_eff - thr > 0:
        raise Undefined("no pore space left")
    Se = (vls - thr) / (nu_eff - thr)
    if Se <= 1:
        lnSe = mp.log(Se)
        u = mp.expm1(-lnSe / m)
        psi = -(u ** (1 / n)) / h["alpha"]          # -((Se^(-1/m) - 1) alpha^(-n))^(1/n)
    else:
        lnSe, u = mp.log(Se), mp.mpf(0)
        psi = (vl - nu_eff) / h["S_s"]
    return dict(K=Kr * Kfac, psi=psi, S=S, lnS=lnS, t=t, w=w, inner=inner, Kfac=Kfac, Se=Se, lnSe=lnSe, u=u, f_i=f_i,
                T=T, vl=vl, nu_eff=nu_eff)


def heat_capacity(mp, th, e, tl, ti):
    """volumetric_heat_capacity, SoilHeatParameterizations.jl:65-79"""
    return th["rho_c_ds"] + tl * e["rhocp_l"] + ti * e["rhocp_i"]


def temperature(mp, h, th, e, vl, ti, rhoe):
    """temperature_from_rhoe_int (:42-53) with the heat capacity of the cell's own water"""
    nu_eff = h["nu"] - ti
    tl = vl if vl < nu_eff else nu_eff
    return e["T0"] + (rhoe + ti * e["rho_i"] * e["LH_f0"]) / heat_capacity(mp, th, e, tl, ti)


def k_dry(mp, h, th, e):
    """:268-294"""
    rho_b = (1 - h["nu"]) * th["rho_p"]
    num = (th["kappa_dry_parameter"] * th["kappa_solid"] - e["k_air"]) * rho_b + e["k_air"] * th["rho_p"]
    return num / (th["rho_p"] - (1 - th["kappa_dry_parameter"]) * rho_b)


def kappa(mp, h, th, e, vl, ti, dtype):
    """thermal_conductivity of kersten_number, saturated_thermal_conductivity and k_dry (:114-188)"""
    eps = mp.mpf(float(np.finfo(dtype).eps))
    nu = h["nu"]
    nu_eff = nu - ti
    tl = vl if vl < nu_eff else nu_eff
    S_r = (tl + ti) / nu
    if S_r < 0:
        raise Undefined("S_r < 0")
    if ti < eps:
        x = (1 + th["nu_ss_om"] - th["a"] * th["nu_ss_quartz"] - th["nu_ss_gravel"]) / 2
        base = (1 + mp.exp(-th["b"] * S_r)) ** (-3) - ((1 - S_r) / 2) ** 3
        if base < 0:
            raise Undefined("kersten base < 0")
        Ke = (S_r ** x if S_r > 0 else mp.mpf(0)) * base ** (1 - th["nu_ss_om"])
    else:
        Ke = S_r ** (1 + th["nu_ss_om"])
    tw = tl + ti
    ks = mp.mpf(0) if tw < eps else th["kappa_sat_unfrozen"] ** (tl / tw) * th["kappa_sat_frozen"] ** (ti / tw)
    return Ke * ks + (1 - Ke) * k_dry(mp, h, th, e)


# ------------------------------------------------------------------ bounds

def bound_K(mp, a, ceps, cf, bT, tiny):
    """|dK| <= Kfac sqrt(S) ((inner + d)^2 - inner^2) + c eps K (1 + |ln S|),
    d = c eps (1 + (m t / w)(1 + |ln S| / m)),  t = S^(1/m), w = 1 - t, inner = 1 - w^m.

    The project's condK (parity_cases.closure_tolerances) written as an ABSOLUTE error of `inner`: a rounding of
    t = S^(1/m) by eps (1 + |ln S|/m) (the power itself and the rounded exponent product |ln t| = |ln S|/m, the
    bound stated in lh_fastmath.hpp) moves w = 1 - t by t eps (..) absolutely and inner = 1 - w^m by m w^(m-1)
    times that, <= (m t / w) eps (..) since w^m <= 1; inner's own subtraction adds eps.  K = Kfac sqrt(S) inner^2
    then moves by the first term; the second is sqrt(S) (half of a rounding of S and of ln S) and the products.
    No 1/inner appears, so a bone-dry cell (inner ~ m t far below eps) needs no cap on the conditioning and no
    mask: the bound there is Kfac sqrt(S) d^2, the size of the noise the working type makes of such a cell.
    Kfac = Ksat x viscosity factor x impedance factor; the factors add their condK terms |gamma (T - T_ref)| and
    Omega |f_i| ln 10 (the exponents of two more powers), and a COMPUTED temperature adds gamma K dT (K is
    proportional to exp(gamma T): derived, not in closure_tolerances, which compares two evaluations in the same
    type).  `tiny` (1 + Kfac) is the number format's own floor: below the smallest normal number of the working
    type neither K nor K/Kfac, which the kernels carry, has eps relative accuracy.
    Of the two terms that are not the issue's or closure_tolerances' -- gamma K dT and the `tiny` floor -- the oracle
    needs neither (it stays inside the bound on every fixture without them, measured); they are kept because they are
    derived from the contract (T is an output here, not an input) and from the number format, not fitted."""
    S, m = a["S"], a["m"]
    absln = abs(a["lnS"])
    if S < 1:
        d = ceps * (1 + (m * a["t"] / a["w"]) * (1 + absln / m))
        sq = mp.sqrt(S)
    else:
        d, sq = ceps, mp.mpf(1)
    b = a["Kfac"] * sq * ((a["inner"] + d) ** 2 - a["inner"] ** 2) + ceps * a["K"] * (1 + absln)
    if cf["visc"]:
        b += ceps * a["K"] * abs(cf["gamma"] * (a["T"] - cf["T_ref"])) + cf["gamma"] * a["K"] * bT
    if cf["imp"]:
        b += ceps * a["K"] * cf["Omega"] * abs(a["f_i"]) * mp.log(10)
    return b + tiny * (1 + a["Kfac"])


def bound_psi(mp, a, h, ceps):
    """closure_tolerances' psi terms from the exact values, without its 1e12 cap and 1e-300 floor:
    c eps |psi| (1 + (u+1)/(n u) + |ln Se|/(m n) + (u+1)/(n m u)) below saturation (a rounding of Se^(-1/m), of
    the exponent product, and of Se itself), 2 c eps |psi| above, and the O(eps^(1/n)) floor next to Se = 1.

    One term is not closure_tolerances' (the oracle alone left the bound without it, by a factor 3 at n = 1.03,
    S = 1e-9 of the `overflow` fixture): the reference forms m = 1 - 1/n IN THE WORKING TYPE, a difference of
    numbers of size 1, so its m carries eps/2 absolutely, eps/(2m) relatively -- 17 eps at n = 1.03 --, while the
    contract here takes m as exact.  psi depends on m through the exponent -1/m of Se: d ln|psi| / d ln m =
    ((u+1)/(n u)) |ln Se| / m, hence the term (1/(2m)) ((u+1)/(n u)) |ln Se| / m.  It is below the others unless
    m is small AND the cell dry (clay-like n, which the fixed cases and the fuzz test's n >= 1.15 barely reach)."""
    n, m = h["n"], h["m"]
    Se, u, psi = a["Se"], a["u"], abs(a["psi"])
    if Se < 1:
        cond = 1 + (u + 1) / (n * u) + abs(a["lnSe"]) / (m * n) + (u + 1) / (n * m * u)
        cond += (u + 1) / (n * u) * abs(a["lnSe"]) / m / (2 * m)
    else:
        cond = mp.mpf(2)
    b = ceps * psi * cond
    if abs(Se - 1) < 4 * ceps:
        b += (ceps * 4) ** (1 / n) / h["alpha"]
    if Se > 1:
        # derived: above saturation psi = (vl - nu_eff)/S_s is a difference of two numbers of size nu, of which
        # nu_eff = nu - theta_i is itself rounded: eps (|vl| + |nu_eff|) / S_s whatever the difference is.  (Not in
        # closure_tolerances; without it the oracle alone leaves the bound, by a factor 234 on `mixed_f32`: a cell
        # saturated next to ice, where 2 c eps |psi| of a psi near zero allows nothing.)
        b += ceps * (abs(a["vl"]) + abs(a["nu_eff"])) / h["S_s"]
    return b


def bound_T(mp, T, T0, ceps):
    return ceps * (abs(T) + abs(T - T0)) * 2


def bound_kappa(mp, k, ceps):
    return ceps * abs(k) * 8


# ------------------------------------------------------------------ one column

def _cell(mp, P, c, i, vl, ti, T_in, rhoe, ceps, tiny, water, heat):
    """closures and bounds of one (cell or Dirichlet face) state"""
    h, e = P.hyd(c, i), P.earth
    out = dict(K=mp.mpf(0), psi=mp.mpf(0), T=mp.mpf(0), kappa=mp.mpf(0), bK=mp.mpf(0), bpsi=mp.mpf(0), bT=mp.mpf(0),
               bkappa=mp.mpf(0))
    if heat:
        th = P.th(c, i)
        if T_in is None:
            out["T"] = temperature(mp, h, th, e, vl, ti, rhoe)
            out["bT"] = bound_T(mp, out["T"], e["T0"], ceps)
        else:
            out["T"] = T_in            # a Dirichlet face value: given
        out["kappa"] = kappa(mp, h, th, e, vl, ti, P.dtype)
        out["bkappa"] = bound_kappa(mp, out["kappa"], ceps)
    else:
        out["T"] = T_in
    if water:
        a = water_closures(mp, h, P.cf, vl, ti, out["T"])
        a["m"] = h["m"]
        out["K"], out["psi"] = a["K"], a["psi"]
        out["bK"] = bound_K(mp, a, ceps, P.cf, out["bT"], tiny)
        out["bpsi"] = bound_psi(mp, a, h, ceps)
    return out


def evaluate(case, c_w, classes=None, thermal=None, class_map=None, prec=PREC, columns=None):
    """Exact closures, tendencies, boundary fluxes and their bounds for `case` (a workloads.Case), every number
    rounded to Float64 at the very end.  c_w is the project's Cw.  -> dict of arrays; undefined cells hold NaN in
    every field (see `Undefined`), a psi beyond the working type's range is -Inf, and a tendency or flux that reads
    such a psi, or is itself beyond the Float64 range, is NaN: not part of the fixture."""
    mp = _mp()
    with mp.workprec(prec):
        return _evaluate(mp, case, c_w, classes, thermal, class_map, columns)


def _evaluate(mp, case, c_w, classes, thermal, class_map, columns):
    om, dtype = case.om, case.dtype
    N, n = case.ncols, om.nlev
    water, heat = om.model != M.MODEL_HEAT, om.model != M.MODEL_RICHARDS
    P = Params(mp, case, classes, thermal, class_map)
    fi = np.finfo(dtype)
    ceps, tiny = mp.mpf(float(fi.eps)) * c_w, mp.mpf(float(fi.tiny))
    psi_max = mp.mpf(float(fi.max))     # beyond the working type's range psi is -Inf (the log-domain closure saturates)
    zmin, zmax = mp.mpf(_ft(om.zmin, dtype)), mp.mpf(_ft(om.zmax, dtype))
    dz = (zmax - zmin) / n
    dzb = dz / 2
    zc = [zmin + (i + mp.mpf(1) / 2) * dz for i in range(n)]
    e = P.earth
    mpf = lambda a, c, i: None if a is None else mp.mpf(float(a[c, i]))
    names2 = ("K", "psi", "T", "kappa", "bK", "bpsi", "bT", "bkappa", "dvl", "drhoe", "b_dvl", "b_drhoe")
    out = {k: np.full((N, n), np.nan) for k in names2}
    for k in ("fw_bot", "fw_top", "fe_bot", "fe_top", "b_fw_bot", "b_fw_top", "b_fe_bot", "b_fe_top"):
        out[k] = np.full(N, np.nan)

    def bcv(face, comp, c):
        kind, v = om.bc.get((face, comp), (M.BC_NONE, 0.0))
        pcv = om.percol_bc.get((face, comp))
        return kind, mp.mpf(_ft(v if pcv is None else pcv[c], dtype))

    for c in (range(N) if columns is None else columns):
        try:
            cells = []
            for i in range(n):
                T_in = None
                if not heat:
                    T_in = mp.mpf(288) if case.T_aux is None else mpf(case.T_aux, c, i)
                cells.append(_cell(mp, P, c, i, mpf(case.vl, c, i), mpf(case.ti, c, i), T_in, mpf(case.rhoe, c, i), ceps,
                                   tiny, water, heat))
        except Undefined:
            continue
        K = [x["K"] for x in cells]
        psi = [x["psi"] for x in cells]
        T = [x["T"] for x in cells]
        kap = [x["kappa"] for x in cells]
        bK, bpsi, bT, bkap = ([x[k] for x in cells] for k in ("bK", "bpsi", "bT", "bkappa"))
        E = [e["rhocp_l"] * (T[i] - e["T0"]) * K[i] if (water and heat) else mp.mpf(0) for i in range(n)]
        bE = [e["rhocp_l"] * (bT[i] * abs(K[i]) + abs(T[i] - e["T0"]) * bK[i]) for i in range(n)]
        bh = [bpsi[i] + ceps * abs(zc[i]) for i in range(n)]
        psi_ok = [abs(p) <= psi_max for p in psi]
        Fw, Fe, dFw, dFe = ([mp.mpf(0)] * (n + 1) for _ in range(4))
        Fw, Fe, dFw, dFe = list(Fw), list(Fe), list(dFw), list(dFe)
        okw = [True] * (n + 1)
        for i in range(n - 1):          # interior face i+1 between cells i and i+1: arithmetic means
            g = (psi[i + 1] - psi[i] + dz) / dz
            okw[i + 1] = psi_ok[i] and psi_ok[i + 1]
            if water:
                Kb = (K[i] + K[i + 1]) / 2
                Fw[i + 1] = -Kb * g
                dFw[i + 1] = (bK[i] + bK[i + 1]) / 2 * abs(g) + Kb * (bh[i] + bh[i + 1]) / dz + ceps * abs(Kb * g)
            if heat:
                gT = (T[i + 1] - T[i]) / dz
                kb = (kap[i] + kap[i + 1]) / 2
                Fe[i + 1] = -kb * gT
                dFe[i + 1] = (bkap[i] + bkap[i + 1]) / 2 * abs(gT) + kb * (bT[i] + bT[i + 1]) / dz + ceps * abs(kb * gT)
                if water:
                    Eb = (E[i] + E[i + 1]) / 2
                    Fe[i + 1] -= Eb * g
                    dFe[i + 1] += (bE[i] + bE[i + 1]) / 2 * abs(g) + abs(Eb) * (bh[i] + bh[i + 1]) / dz + ceps * abs(Eb * g)
        # boundary faces (boundary_conditions.jl:174-444): the face state is the boundary cell with the Dirichlet
        # values put in, evaluated with the boundary cell's own parameters
        for face, ci, k in ((M.FACE_BOTTOM, 0, 0), (M.FACE_TOP, n - 1, n)):
            ke, ve = bcv(face, M.COMP_ENERGY, c)
            kh, vh = bcv(face, M.COMP_HYDROLOGY, c)
            vl_c, ti_c = mpf(case.vl, c, ci), mpf(case.ti, c, ci)
            vl_f = vh if (kh == M.BC_DIRICHLET and water) else vl_c
            T_f = ve if (ke == M.BC_DIRICHLET and heat) else T[ci]
            need_face = (heat and ke == M.BC_DIRICHLET) or (water and kh == M.BC_DIRICHLET)
            try:
                f = _cell(mp, P, c, ci, vl_f, ti_c, T_f, None, ceps, tiny, water, heat) if need_face else None
            except Undefined:
                okw[k] = False
                f = None
            if heat:
                if ke == M.BC_FLUX:
                    Fe[k], dFe[k] = ve, ceps * abs(ve)
                elif ke == M.BC_DIRICHLET and f is not None:
                    gTb = (T_f - T[ci]) / dzb
                    Fe[k] = -f["kappa"] * gTb * (-1 if face == M.FACE_BOTTOM else 1)
                    dFe[k] = f["bkappa"] * abs(gTb) + f["kappa"] * (bT[ci] + ceps * abs(ve)) / dzb + ceps * abs(f["kappa"] * gTb)
                elif ke != M.BC_DIRICHLET:
                    raise ValueError("the energy component needs a flux or a Dirichlet value at both faces")
            if water:
                if kh == M.BC_FLUX:
                    Fw[k], dFw[k] = vh, ceps * abs(vh)
                elif kh == M.BC_FREE_DRAINAGE:
                    Fw[k], dFw[k] = -K[ci], bK[ci]
                elif kh == M.BC_DIRICHLET and f is not None:
                    okw[k] = okw[k] and psi_ok[ci] and abs(f["psi"]) <= psi_max
                    if face == M.FACE_BOTTOM and om.consistent_bottom_sign:
                        Fw[k] = f["K"] * (f["psi"] - psi[ci] - dzb) / dzb
                    else:
                        Fw[k] = -f["K"] * (f["psi"] - psi[ci] + dzb) / dzb * (-1 if face == M.FACE_BOTTOM else 1)
                    gmax = max(abs(f["psi"] - psi[ci] + dzb), abs(f["psi"] - psi[ci] - dzb)) / dzb
                    dFw[k] = f["bK"] * gmax + f["K"] * (f["bpsi"] + bpsi[ci]) / dzb + ceps * f["K"] * gmax
                elif kh != M.BC_DIRICHLET:
                    raise ValueError("the hydrology component needs a boundary condition at both faces")
        # tendencies: (dF_lo + dF_hi)/dz as tendency_tolerance has it, plus c eps |d| for the final difference and
        # quotient, which is parity_cases.assert_tendencies_close's `allowed = tol + Cw eps |want|` (the oracle stays
        # inside without that last term, measured; it is kept because the project's own check has it)
        for i in range(n):
            for k in ("K", "psi", "T", "kappa", "bK", "bpsi", "bT", "bkappa"):
                out[k][c, i] = to_float(cells[i][k])
            if water and not psi_ok[i]:
                out["psi"][c, i], out["bpsi"][c, i] = -np.inf, 0.0
            if water and okw[i] and okw[i + 1]:
                d = -(Fw[i + 1] - Fw[i]) / dz
                out["dvl"][c, i] = to_float(d)
                out["b_dvl"][c, i] = to_float((dFw[i + 1] + dFw[i]) / dz + ceps * abs(d))
            # (the advective part of an energy flux reads psi as well)
            if heat and (not water or (okw[i] and okw[i + 1])):
                d = -(Fe[i + 1] - Fe[i]) / dz
                out["drhoe"][c, i] = to_float(d)
                out["b_drhoe"][c, i] = to_float((dFe[i + 1] + dFe[i]) / dz + ceps * abs(d))
        for nm, k in (("bot", 0), ("top", n)):
            if water and okw[k]:
                out["fw_" + nm][c], out["b_fw_" + nm][c] = to_float(Fw[k]), to_float(dFw[k])
            if heat:
                out["fe_" + nm][c], out["b_fe_" + nm][c] = to_float(Fe[k]), to_float(dFe[k])
    for k in ("dvl", "b_dvl", "drhoe", "b_drhoe"):     # a value beyond the Float64 range is not in the fixture
        out[k][~np.isfinite(out[k])] = np.nan
    bad = ~np.isfinite(out["dvl"]) | ~np.isfinite(out["b_dvl"])
    out["dvl"][bad], out["b_dvl"][bad] = np.nan, np.nan
    bad = ~np.isfinite(out["drhoe"]) | ~np.isfinite(out["b_drhoe"])
    out["drhoe"][bad], out["b_drhoe"][bad] = np.nan, np.nan
    return out


# ------------------------------------------------------------------ comparing with a fixture

CLOSURES = (("K", "bK"), ("psi", "bpsi"), ("T", "bT"), ("kappa", "bkappa"))
TENDENCIES = (("dvl", "b_dvl"), ("drhoe", "b_drhoe"))
FLUXES = (("fw_bot", "b_fw_bot"), ("fw_top", "b_fw_top"), ("fe_bot", "b_fe_bot"), ("fe_top", "b_fe_top"))


def fields_of(model):
    water, heat = model != M.MODEL_HEAT, model != M.MODEL_RICHARDS
    f = []
    if water:
        f += ["K", "psi", "dvl", "fw_bot", "fw_top"]
    if heat:
        f += ["T", "kappa", "drhoe", "fe_bot", "fe_top"]
    return f


def use_of_bound(got, exact, bound):
    """max over the fixture's cells of |got - exact| / bound.  A cell the fixture does not hold is NaN in `exact`;
    where `exact` is -Inf (psi beyond the range) `got` must be -Inf too.  No cell that the fixture holds is left
    out, whatever its conditioning."""
    got, exact, bound = (np.asarray(a, dtype=np.float64) for a in (got, exact, bound))
    held = ~np.isnan(exact)
    if not held.any():
        return 0.0
    g, x, b = got[held], exact[held], bound[held]
    inf = np.isinf(x)
    if np.any(g[inf] != x[inf]) or np.any(~np.isfinite(g[~inf])):
        return float("inf")
    err = np.abs(g[~inf] - x[~inf])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b[~inf])
    return float(r.max()) if r.size else 0.0


def ulp_errors(got, exact, dtype):
    """|got - exact| in ulp of the working type at the exact value, over the finite cells the fixture holds"""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    ok = np.isfinite(exact) & np.isfinite(got) & (exact != 0)
    ulp = np.abs(exact[ok]) * float(np.finfo(dtype).eps)
    return np.abs(got[ok] - exact[ok]) / np.maximum(ulp, float(np.finfo(np.float64).tiny))


# ------------------------------------------------------------------ the fixtures' cases

class Fixture:
    """name, the case (inputs included), Cw, and the layered supplement (classes, thermal, class_map) or None;
    `stored`: the input arrays the file holds (random ones; the others a formula reproduces bit for bit)"""

    def __init__(self, name, case, c_w, stored=(), classes=None, thermal=None, class_map=None, kind="fixed"):
        self.name, self.case, self.c_w, self.stored = name, case, c_w, tuple(stored)
        self.classes, self.thermal, self.class_map, self.kind = classes, thermal, class_map, kind

    @property
    def path(self):
        return os.path.join(GOLDEN, self.name + ".npz")


def _cw(dtype, fuzz=False):
    f64 = np.dtype(dtype) == np.float64
    return (4.0 if f64 else 16.0) if fuzz else (2.0 if f64 else 4.0)


def _tag(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _rhoe(om, sp_nu, vl, ti, T):
    e = om.earth
    tl = np.minimum(vl, sp_nu - ti)
    rcs = om.soil.rho_c_ds + tl * (e.cp_l * e.rho_liq) + ti * (e.cp_i * e.rho_ice)
    return rcs * (T - e.T_0) - ti * e.rho_ice * e.LH_f0


FUZZ_NLEV, FUZZ_NCOLS = 8, 64


def fuzz_fixture(dtype, model, factors, percol):
    """The first 64 columns x 8 levels of tools/fuzz_closures.fuzz_case(7, ...) whose closed forms have a value
    (the 0/0 impedance input, which tests/test_gpu_fuzz.py pins as NaN in, NaN out, is left out), as a column of
    8 levels with the same Dirichlet top and free-drainage bottom."""
    import fuzz_closures
    full = fuzz_closures.fuzz_case(7, dtype, factors, percol, model)
    n, N = FUZZ_NLEV, FUZZ_NCOLS
    om = copy.deepcopy(full.om)
    om.nlev, om.zmin = n, -0.05 * n
    # (an undefined closed form: f_i = 0/0 under the impedance factor, liquid below theta_r with ice to match)
    tl = np.minimum(full.vl.astype(np.float64), pc._percol(full, "nu", om.soil.nu)[:, None] - full.ti)
    good = ~np.any((tl[:, :n] + full.ti[:, :n] == 0) & bool(factors), axis=1)
    # half of the columns hold a cell that the fuzz test masks (its criterion: 1 - (1 - S^(1/m))^m < 64 eps)
    with np.errstate(all="ignore"):
        mm = 1.0 - 1.0 / pc._percol(full, "vg_n", om.vg.n)[:, None]
        th = pc._percol(full, "vg_theta_r", om.vg.theta_r)[:, None]
        S = (np.maximum(full.vl[:, :n].astype(np.float64), th + np.finfo(dtype).eps) - th) / (pc._percol(full, "nu", om.soil.nu)[:, None] - th)
        t = np.where(S < 1, S ** (1.0 / mm), 1.0)
        ill = np.any(np.where(S < 1, 1.0 - (1.0 - t) ** mm, 1.0) < 64 * np.finfo(dtype).eps, axis=1)
    good = np.sort(np.concatenate([np.flatnonzero(good & ill)[:N // 2], np.flatnonzero(good & ~ill)[:N // 2]]))
    assert good.size == N
    om.percol = {k: np.ascontiguousarray(np.asarray(v)[good]) for k, v in om.percol.items()}
    take = lambda a: None if a is None else np.ascontiguousarray(a[good, :n])
    name = f"fuzz_{'coupled' if model == M.MODEL_COUPLED else 'richards'}_fac{int(factors)}_pc{int(percol)}_{_tag(dtype)}"
    case = pc.Case(name, om, dtype, N, vl=take(full.vl), ti=take(full.ti), rhoe=take(full.rhoe), T_aux=take(full.T_aux))
    stored = ["vl", "ti"] + (["rhoe"] if case.rhoe is not None else []) + (["T_aux"] if case.T_aux is not None else [])
    stored += ["percol_" + k for k in om.percol]
    return Fixture(name, case, _cw(dtype, fuzz=True), stored, kind="fuzz")


def _richards_om(n, percol=None, bc=None, theta_r=0.0, nu=0.5, vg_n=2.0, consistent=False):
    H = M.COMP_HYDROLOGY
    bc = bc or {(M.FACE_TOP, H): (M.BC_FLUX, -1e-9), (M.FACE_BOTTOM, H): (M.BC_FREE_DRAINAGE, 0.0)}
    return M.CaseModel(M.MODEL_RICHARDS, n, -0.05 * n, 0.0, soil=M.default_soil(nu=nu), bc=bc,
                       vg=M.default_vg(n=vg_n, alpha=2.6, theta_r=theta_r, Ksat=1.2e-7), percol=percol or {},
                       consistent_bottom_sign=consistent)


def overflow_fixture(dtype):
    """Clay-like columns whose dry cells take S^(-1/m) out of the working type's range (the reference returns
    psi = -Inf there): every fourth column is an ordinary one (n = 2), and inside a clay-like column every third
    level is an ordinary moist cell, so a dry cell has neighbours above and below and beside it.  theta_r = 0,
    nu = 0.5: S = 2 vl.  Float64: n in {1.03, 1.05, 1.07}, S from 1e-6 down to 1e-16; Float32: n in {1.15, 1.2,
    1.3}, S from 1e-4 down to where |psi| stays inside the Float32 range."""
    f64 = np.dtype(dtype) == np.float64
    n, N = 16, 64
    ns = (1.03, 1.05, 1.07) if f64 else (1.15, 1.2, 1.3)
    lo = {1.03: 16.0, 1.05: 16.0, 1.07: 16.0, 1.15: 5.4, 1.2: 7.2, 1.3: 10.5}
    hi = 6.0 if f64 else 4.0
    vg_n = np.full(N, 2.0)
    S = np.empty((N, n))
    for c in range(N):
        for i in range(n):
            S[c, i] = 0.30 + 0.02 * i + 0.001 * c
        if c % 4 != 3:
            vg_n[c] = ns[c % 4]
            for i in range(n):
                if i % 3 != 1:
                    frac = ((c // 4) * n + i) / float((N // 4) * n - 1)
                    S[c, i] = 10.0 ** -(hi + (lo[vg_n[c]] - hi) * frac)
            if f64 and (c // 4) % 2 == 1:
                # the reference overflows once S^(-1/m) > 1.8e308, i.e. |psi| > 1.8e308^(1/n) / alpha (7.7e298 for
                # n = 1.03), and the Float64 range ends a few decades on: every third level of every second
                # clay-like column aims at |psi| between that threshold and 2.5e299 (for n = 1.07: S ~ 1e-20)
                p_lo = 308.2547 / vg_n[c] - np.log10(2.6) + 0.05
                for i in range(0, n, 3):
                    frac = ((c // 8) * 6 + i // 3) / 47.0
                    S[c, i] = 10.0 ** (-(p_lo + (299.4 - p_lo) * frac + np.log10(2.6)) * (vg_n[c] - 1.0))
    om = _richards_om(n, percol=dict(vg_n=vg_n))
    vl = (0.5 * S).astype(dtype)
    case = pc.Case(f"overflow_{_tag(dtype)}", om, dtype, N, vl=vl, ti=np.zeros((N, n), dtype))
    return Fixture(case.name, case, _cw(dtype), stored=["vl"])       # (10^x is not the same bits in every libm)


def _edge_values(dtype):
    """1 - k eps/2 for k = 1, 2, 3, 2^10, 2^20, 2^30 (Float32: 2^4, 2^8, 2^12), exactly 1, the first values above 1"""
    h = float(np.finfo(dtype).eps) / 2
    ks = (1, 2, 3, 2 ** 10, 2 ** 20, 2 ** 30) if np.dtype(dtype) == np.float64 else (1, 2, 3, 2 ** 4, 2 ** 8, 2 ** 12)
    return [1.0 - k * h for k in ks] + [1.0, 1.0 + 2 * h, 1.0 + 4 * h, 1.0 + 6 * h]


def _coupled_om(n, factors, theta_r=0.0):
    sp, vg = pc.coupled_soil()
    vg.theta_r = theta_r
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.3), (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0),
          (M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 277.0), (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_FLUX, 0.02)}
    return M.CaseModel(M.MODEL_COUPLED, n, -0.05 * n, 0.0, soil=sp, vg=vg, bc=bc,
                       cf=M.default_cf(viscosity=factors, impedance=factors))


def edge_fixture(dtype):
    """The saturation edge, coupled model: S (ice-free columns, vl = nu V) and Se (icy columns with theta_i =
    nu/2, vl = nu V / 2) take the values V of _edge_values exactly (theta_r = 0, nu = 0.5: no rounding in either
    saturation), for a clay-like (n = 1.2) and a sand-like (n = 3) column; a column starts its walk through V at a
    different value, so every V meets every neighbour and both boundary faces."""
    V = _edge_values(dtype)
    n, N = len(V), 64
    om = _coupled_om(n, factors=False)
    c, i = np.arange(N)[:, None], np.arange(n)[None, :]
    icy = ((c // 2) % 2 == 1)
    v = np.array(V)[(i + c // 4) % len(V)]
    vl = np.where(icy, 0.25 * v, 0.5 * v)
    ti = np.where(icy, 0.25, 0.0) + 0.0 * v
    om.percol = dict(vg_n=np.where(np.arange(N) % 2 == 0, 1.2, 3.0))
    T = 279.0 + 0.25 * i + 0.03125 * c
    rhoe = _rhoe(om, 0.5, vl, ti, T)
    case = pc.Case(f"edge_{_tag(dtype)}", om, dtype, N, vl=vl.astype(dtype), ti=ti.astype(dtype), rhoe=rhoe.astype(dtype))
    return Fixture(case.name, case, _cw(dtype), stored=["rhoe"])


def clamp_fixture(dtype, consistent=False):
    """The theta_r + eps clamp of effective_saturation, Richards: vl at theta_r - 1e-3, theta_r, theta_r + eps (as
    the working type forms it) and its two neighbours, among ordinary cells; theta_r in {0, 0.05, 0.1} and n in
    {2, 1.4} per column.  Both faces are Dirichlet faces: `clamp_*` has the reference's sign of the bottom flux
    (boundary_conditions.jl:395-398), `clampcs_*` the same columns under lh_set_bottom_sign_consistent(1)."""
    FT = np.dtype(dtype).type
    n, N = 8, 64
    thr = np.array([0.0, 0.05, 0.1])[np.arange(N) % 3]
    vg_n = np.where((np.arange(N) // 3) % 2 == 0, 2.0, 1.4)
    H = M.COMP_HYDROLOGY
    om = _richards_om(n, percol=dict(vg_theta_r=thr, vg_n=vg_n),
                      bc={(M.FACE_TOP, H): (M.BC_DIRICHLET, 0.3), (M.FACE_BOTTOM, H): (M.BC_DIRICHLET, 0.2)},
                      consistent=consistent)
    vl = np.empty((N, n), dtype)
    for c in range(N):
        t = FT(thr[c])
        lim = FT(t + FT(np.finfo(dtype).eps))
        special = [FT(t - FT(1e-3)), t, lim, np.nextafter(lim, FT(-1)), np.nextafter(lim, FT(1))]
        for i in range(n):
            # (every second pair of columns keeps its two bottom cells ordinary: there the bottom cell's tendency is
            # small enough to show the gravity term by which the two bottom signs differ)
            plain = (i + c) % 2 == 1 or (i < 2 and (c // 2) % 2 == 0)
            vl[c, i] = FT(0.2 + 0.03 * i + 0.001 * c) if plain else special[(i // 2 + c) % 5]
    case = pc.Case(f"clamp{'cs' if consistent else ''}_{_tag(dtype)}", om, dtype, N, vl=vl, ti=np.zeros((N, n), dtype))
    return Fixture(case.name, case, _cw(dtype))


def heat_fixture(dtype):
    """The heat-only model (vartheta_l and theta_i prescribed, rho e_int prognostic), Dirichlet temperatures at both
    faces: dry to saturated cells, a third of the columns with ice, one column in eight without any water at all
    (kappa = kappa_dry)."""
    n, N = 8, 64
    sp, _ = pc.coupled_soil()
    bc = {(M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 280.0), (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_DIRICHLET, 290.0)}
    om = M.CaseModel(M.MODEL_HEAT, n, 0.0, 0.05 * n, soil=sp, bc=bc)
    c, i = np.arange(N)[:, None], np.arange(n)[None, :]
    vl = 0.02 + 0.53 * pc.uhash(c, i + 7, 1000)                  # up to 0.55 > nu: theta_l = nu - theta_i there
    ti = np.where(c % 3 == 1, 0.15 * pc.uhash(c, i + 99, 1000), 0.0)
    vl = np.where(c % 8 == 5, 0.0, vl)
    ti = np.where(c % 8 == 5, 0.0, ti)
    T = 270.0 + 25.0 * pc.uhash(c, i + 55, 1000)
    rhoe = _rhoe(om, sp.nu, vl, ti, T)
    case = pc.Case(f"heat_{_tag(dtype)}", om, dtype, N, vl=vl.astype(dtype), ti=ti.astype(dtype), rhoe=rhoe.astype(dtype))
    return Fixture(case.name, case, _cw(dtype), stored=["vl", "ti", "rhoe"])


def mixed_fixture(dtype):
    """One wavefront of 64 columns, coupled, both conductivity factors: icy, saturated, clamped (vl = theta_r =
    0.05, at and below theta_r + eps) and ordinary lanes side by side, the pattern moving by level, so that every
    wave-level decision of the closures (the ballots for ice, saturation and the clamp) is taken in mixed company."""
    n, N = 8, 64
    om = _coupled_om(n, factors=True, theta_r=0.05)
    c, i = np.arange(N)[:, None], np.arange(n)[None, :]
    kind = (c * 3 + i * 5) % 7
    u = pc.uhash(c, i + 40, 1000)
    vl = 0.12 + 0.3 * u
    ti = np.where(kind % 2 == 1, 0.02 + 0.1 * pc.uhash(c, i + 90, 1000), 0.0)
    vl = np.where(kind == 2, 0.5 + 0.04 * u, vl)                 # saturated, ice-free
    vl = np.where(kind == 3, 0.5 - ti + 0.01 * u, vl)            # saturated next to ice
    vl = np.where(kind == 4, 0.05, vl)                           # at theta_r: clamped
    T = 268.0 + 20.0 * pc.uhash(c, i + 140, 1000)
    rhoe = _rhoe(om, 0.5, vl, ti, T)
    case = pc.Case(f"mixed_{_tag(dtype)}", om, dtype, N, vl=vl.astype(dtype), ti=ti.astype(dtype), rhoe=rhoe.astype(dtype))
    return Fixture(case.name, case, _cw(dtype), stored=["vl", "ti", "rhoe"])


SWEEP_NLEV, SWEEP_NCOLS = 12, 64


def sweep_log2_values():
    """S whose mantissa sits one ulp inside each end of each of the 2048 intervals of the log2 table (lh_fastmath.hpp,
    log2_core: the top 11 fraction bits of the mantissa in [0.5, 1) choose the interval; the one whose argument
    reduction reaches |r| = 2^-11 is the first), the binary exponent walking over 0, -1, -2."""
    j = np.arange(2048, dtype=np.float64)
    u = 2.0 ** -53
    lo = 0.5 + j / 4096.0 + u
    hi = 0.5 + (j + 1) / 4096.0 - u
    S = np.stack([lo, hi], axis=1).reshape(-1)
    return S * 2.0 ** -(np.arange(S.size) % 3)


@functools.lru_cache(maxsize=None)
def sweep_exp2_values():
    """S = 2^((k + 1/2) m / 2048) to the nearest Float64 and its two neighbours, k = -1 ... -2048, for m = 1/2
    (n = 2): log2(S)/m x 2048 = k + 1/2 +- 7e-13, both sides of every rounding tie of the exp2 shifter
    (lh_fastmath.hpp, exp2_scaled: k = rint(u)), and with them every one of the 2048 table entries k mod 2048."""
    mp = _mp()
    out = []
    with mp.workprec(PREC):
        for k in range(-1, -2049, -1):
            s0 = float(mp.mpf(2) ** ((mp.mpf(k) + mp.mpf(1) / 2) / 4096))
            out += [np.nextafter(s0, 0.0), s0, np.nextafter(s0, 2.0)]
    return np.array(out)


def sweep_fixture(which, part, values=None):
    """Part `part` of a table sweep: 64 columns x 12 levels of consecutive values (the last part wraps round),
    Richards, Float64, theta_r = 0, nu = 0.5 (S = 2 vl exactly), n = 2."""
    n, N = SWEEP_NLEV, SWEEP_NCOLS
    name = f"sweep_{which}_{part:02d}_f64"
    vl = None
    if values is not None:
        idx = (part * n * N + np.arange(n * N)) % values.size
        vl = (0.5 * values[idx]).reshape(N, n)
    om = _richards_om(n)
    case = pc.Case(name, om, np.float64, N, vl=vl, ti=np.zeros((N, n)))
    return Fixture(name, case, _cw(np.float64), stored=["vl"] if which == "exp2" else [], kind="sweep")


SWEEP_PARTS = {"log2": -(-4096 // (SWEEP_NLEV * SWEEP_NCOLS)), "exp2": -(-6144 // (SWEEP_NLEV * SWEEP_NCOLS))}


def layered_fixture(dtype, base):
    """The fuzz (Richards and coupled, factors on), saturation-edge and heat-only states spread over three soil classes by a
    map that changes class inside the column and between neighbouring columns; a Dirichlet face takes the
    boundary cell's own class (DESIGN.md sections 4.18 and 4.20)."""
    if base == "edge":
        fx = edge_fixture(dtype)
    elif base == "heat":
        fx = heat_fixture(dtype)
    else:
        fx = fuzz_fixture(dtype, M.MODEL_COUPLED if base == "fuzzc" else M.MODEL_RICHARDS, True, False)
    case = copy.copy(fx.case)
    case.om = copy.deepcopy(fx.case.om)
    case.om.percol = {}
    sp, vg = case.om.soil, case.om.vg
    # (nu and theta_r stay the case's own so that its states keep their meaning: the edge values stay on the edge)
    # (n >= 1.4: the Float32 fuzz states are bone dry, and the working-type references overflow below that)
    classes = np.array([[1.4, 2.6, vg.theta_r, 3e-5, sp.nu, 1e-3],
                        [3.0, 6.5, vg.theta_r, 1e-7, sp.nu, 2e-3],
                        [1.7, 0.9, vg.theta_r, 4e-6, sp.nu, 5e-4]])
    thermal = np.array([[1.0e6, 7.0, 2700.0, 2.0, 4.0, 0.0, 0.0, 0.92],
                        [1.3e6, 3.5, 2600.0, 1.4, 2.9, 0.1, 0.05, 0.4],
                        [0.9e6, 5.1, 2650.0, 1.7, 3.3, 0.0, 0.1, 0.6]])
    c, i = np.arange(case.ncols)[:, None], np.arange(case.om.nlev)[None, :]
    cmap = (((i * 3) // case.om.nlev + c) % 3).astype(np.uint8)
    case.name = f"layered_{base}_{_tag(dtype)}"
    stored = [s for s in fx.stored if not s.startswith("percol_")]
    return Fixture(case.name, case, fx.c_w, stored, classes=classes,
                   thermal=thermal if case.om.model != M.MODEL_RICHARDS else None, class_map=np.ascontiguousarray(cmap),
                   kind="layered")


def fixture_names():
    names = []
    for dt in ("f64", "f32"):
        for model in ("coupled", "richards"):
            for fac in (0, 1):
                for pcol in (0, 1):
                    names.append(f"fuzz_{model}_fac{fac}_pc{pcol}_{dt}")
        names += [f"overflow_{dt}", f"edge_{dt}", f"clamp_{dt}", f"clampcs_{dt}", f"mixed_{dt}", f"heat_{dt}"]
        names += [f"layered_{b}_{dt}" for b in ("fuzzr", "fuzzc", "edge", "heat")]
    for which, parts in SWEEP_PARTS.items():
        names += [f"sweep_{which}_{p:02d}_f64" for p in range(parts)]
    return names


def build_fixture(name, generate=False):
    """The Fixture called `name`.  generate=True makes the inputs from scratch (needs mpmath for the exp2 sweep);
    otherwise the inputs the file stores are read from it, so that nothing but NumPy is needed."""
    parts = name.split("_")
    dtype = np.float64 if parts[-1] == "f64" else np.float32
    if parts[0] == "fuzz":
        fx = fuzz_fixture(dtype, M.MODEL_COUPLED if parts[1] == "coupled" else M.MODEL_RICHARDS, parts[2] == "fac1",
                          parts[3] == "pc1")
    elif parts[0] == "layered":
        fx = layered_fixture(dtype, parts[1])
    elif parts[0] == "sweep":
        which, part = parts[1], int(parts[2])
        values = sweep_log2_values() if which == "log2" else (sweep_exp2_values() if generate else None)
        fx = sweep_fixture(which, part, values)
    else:
        fx = {"overflow": overflow_fixture, "edge": edge_fixture, "clamp": clamp_fixture, "mixed": mixed_fixture,
              "clampcs": lambda dt: clamp_fixture(dt, consistent=True), "heat": heat_fixture}[parts[0]](dtype)
    assert fx.name == name, (fx.name, name)
    if not generate:
        with np.load(fx.path) as z:
            for k in fx.stored:
                if k.startswith("percol_"):
                    fx.case.om.percol[k[len("percol_"):]] = z["in_" + k]
                else:
                    setattr(fx.case, k, z["in_" + k])
    return fx


def fixture_arrays(fx, prec=PREC, columns=None):
    """what the file of `fx` holds: the stored inputs (in_*), Cw, and the exact outputs of its model"""
    ex = evaluate(fx.case, fx.c_w, fx.classes, fx.thermal, fx.class_map, prec=prec, columns=columns)
    keep = fields_of(fx.case.om.model)
    out = {"c_w": np.float64(fx.c_w)}
    for pair in CLOSURES + TENDENCIES + FLUXES:
        if pair[0] in keep:
            out[pair[0]] = ex[pair[0]]
            if pair[0] not in ("T", "kappa"):      # (their bounds are one product of the exact value: load_exact)
                out[pair[1]] = ex[pair[1]]
    for k in fx.stored:
        out["in_" + k] = fx.case.om.percol[k[len("percol_"):]] if k.startswith("percol_") else getattr(fx.case, k)
    return out


def with_plain_bounds(fx, ex):
    """adds the bounds of T and kappa, which the files do not store: closure_tolerances' terms 2 c eps (|T| + |T -
    T_0|) and 8 c eps |kappa| of the exact values"""
    ex = dict(ex)
    ceps = float(np.finfo(fx.case.dtype).eps) * float(ex["c_w"])
    if "T" in ex:
        ex["bT"] = ceps * (np.abs(ex["T"]) + np.abs(ex["T"] - _ft(fx.case.om.earth.T_0, fx.case.dtype))) * 2.0
        ex["bkappa"] = ceps * np.abs(ex["kappa"]) * 8.0
    return ex


def load_exact(fx):
    with np.load(fx.path) as z:
        return with_plain_bounds(fx, {k: z[k] for k in z.files})


def lay_of(fx):
    """the fixture as tests/layered_ref.Layered or tests/layered_heat_ref.LayeredHeat"""
    if fx.thermal is None:
        import layered_ref as R
        return R.Layered(fx.case, fx.classes, fx.class_map)
    import layered_heat_ref as H
    return H.LayeredHeat(fx.case, fx.classes, fx.thermal, fx.class_map)


def working_type_values(fx):
    """The same quantities from the restatement IN THE WORKING TYPE that the rest of the suite compares with: the
    oracle (op for op the reference), or, for a layered fixture, tests/layered_ref.py / tests/layered_heat_ref.py.
    Keys as in the fixture files."""
    case, om = fx.case, fx.case.om
    out = {}
    with np.errstate(all="ignore"):
        if fx.classes is None:
            d = pc.O.diagnostics(om, case.vl, case.ti, case.rhoe, case.T_aux)
            r = pc.run_oracle_rhs(case)
            out.update(K=d["K"], psi=d["psi"], T=d["T"], kappa=d["kappa"], dvl=r.get("vl"), drhoe=r.get("rhoe"))
            for face, nm in ((M.FACE_BOTTOM, "bot"), (M.FACE_TOP, "top")):
                fe, fw = pc.O.boundary_fluxes(om, face, case.vl, case.ti, case.rhoe, case.T_aux)
                out["fe_" + nm], out["fw_" + nm] = fe, fw
        elif fx.thermal is None:
            import layered_ref as R
            lay = lay_of(fx)
            out.update(R.diagnostics(lay))
            out["dvl"], out["fw_bot"], out["fw_top"] = R.rhs(lay, faces=True)
        else:
            import layered_heat_ref as H
            lay = lay_of(fx)
            d = H.diagnostics(lay)
            out.update(K=d["K"], psi=d["psi"], T=d["T"], kappa=d["kappa"])
            r, faces = H.rhs(lay, faces=True)
            out["dvl"], out["drhoe"] = r.get("vl"), r["rhoe"]
            for face, nm in ((M.FACE_BOTTOM, "bot"), (M.FACE_TOP, "top")):
                out["fe_" + nm], out["fw_" + nm] = faces[face]
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items() if v is not None}


def uses(got, ex):
    """{field: use of its bound} for the fields the fixture `ex` holds"""
    return {k: use_of_bound(got[k], ex[k], ex[b]) for k, b in CLOSURES + TENDENCIES + FLUXES if k in ex}


def worst_cell(got, ex, k, b):
    """a description of the cell that uses most of its bound (for an assertion's message)"""
    g, x, bb = np.asarray(got[k], np.float64), ex[k], ex[b]
    with np.errstate(all="ignore"):
        r = np.where(np.isnan(x), 0.0, np.where(np.isinf(x) | ~np.isfinite(g), np.where(g == x, 0.0, np.inf),
                                               np.where(g == x, 0.0, np.abs(g - x) / bb)))
    i = np.unravel_index(np.argmax(r), r.shape)
    return f"{k} at {tuple(int(j) for j in i)}: got {g[i]!r} exact {x[i]!r} bound {bb[i]:.3g} (use {r[i]:.3g})"


def assert_inside(got, ex, label):
    u = uses(got, ex)
    bad = [worst_cell(got, ex, k, b) for k, b in CLOSURES + TENDENCIES + FLUXES if k in ex and not u[k] <= 1.0]
    assert not bad, f"{label}: outside the bound: " + "; ".join(bad)
    return u


def ulp_summary(got, ex, dtype, keys=("K", "psi", "dvl", "T", "kappa", "drhoe")):
    """'K 0.5/3.1 ...': median / largest error in ulp of the working type, for the record"""
    parts = []
    for k in keys:
        if k in ex and k in got:
            e = ulp_errors(got[k], ex[k], dtype)
            if e.size:
                parts.append(f"{k} {np.median(e):.3g}/{e.max():.3g}")
    return " ".join(parts)


# ------------------------------------------------------------------ the record

def record_line(who, fx_name, config, uses, extra=""):
    """one line of profiles/exact_reference_use.txt"""
    return (f"EXACT-USE {who:7s} {fx_name:32s} {config:14s} " + " ".join(f"{k}={v:.3g}" for k, v in uses.items())
            + (" | " + extra if extra else ""))
