"""Host-side mirror of the LandHydrology.jl SoilModel API for the hot path.

Julia is not available in the build image, so the host side above the C ABI is
written in Python with the reference's names, argument meaning and error
behaviour.  The Julia shim a maintainer would add is
`julia/LandHydrologyHIP.jl` (text only); both are thin: all
arithmetic happens in liblandhydro_hip.so on the GPU.

Reference files mirrored (under the reference tree):
  src/Domains/domain.jl                 Column, make_function_space
  src/SoilModel/parameters.jl           SoilParams
  src/SoilModel/SoilWaterParameterizations.jl  vanGenuchten, NoEffect, ...
  src/SoilModel/models.jl               SoilModel, SoilHydrologyModel, ...
  src/SoilModel/boundary_conditions.jl  NoBC, VerticalFlux, Dirichlet, FreeDrainage, ...
  src/SoilModel/initial_conditions.jl   initialize_states
  src/SoilModel/right_hand_side.jl      make_rhs, make_update_aux, coordinates
  src/Simulations/simulation.jl         Simulation, step!, run!

Build extension: `Column(..., ncolumns=N)` is an ensemble of N independent
columns (the reference has exactly one); every field is then [ncolumns, nelements].
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from . import _ffi as F
from .parameterizations import *  # noqa: F401,F403  (the exported SoilWater/SoilHeat helpers)

Float32, Float64 = np.float32, np.float64

# ------------------------------------------------------------------ Domains


class Column:
    """Column{FT}(zlim, nelements) -- src/Domains/domain.jl:12-33."""

    def __init__(self, FT=Float64, *, zlim, nelements, ncolumns: int = 1):
        self.FT = np.dtype(FT).type
        F.dtype_code(self.FT)
        zlim = (float(zlim[0]), float(zlim[1]))
        if not zlim[0] < zlim[1]:                       # @assert zlim[1] < zlim[2], domain.jl:30
            raise AssertionError("zlim[1] < zlim[2]")
        self.zlim = (self.FT(zlim[0]), self.FT(zlim[1]))
        self.nelements = int(nelements)
        self.ncolumns = int(ncolumns)
        if self.nelements < 1 or self.ncolumns < 1:
            raise ValueError("nelements and ncolumns must be >= 1")
        self.boundary_tags = ("bottom", "top")          # domain.jl:31

    def ndims(self):                                    # domain.jl:35
        return 1

    def length(self):                                   # domain.jl:37
        return self.zlim[1] - self.zlim[0]

    def size(self):                                     # domain.jl:39
        return self.length()

    def __repr__(self):                                 # Base.show, domain.jl:41-49
        return "[%0.1f, %0.1f]" % (self.zlim[0], self.zlim[1])


def make_function_space(domain: Column):
    """Centre and face z of the uniform column mesh (domain.jl:58-69).  The
    rounding of the centres is the library's (lh_coordinates)."""
    n = domain.nelements
    lo, hi = np.longdouble(domain.zlim[0]), np.longdouble(domain.zlim[1])
    zf = np.array([lo + (hi - lo) * k / n for k in range(n + 1)], dtype=np.longdouble)
    zf = zf.astype(domain.FT)
    zf[-1] = domain.zlim[1]
    zc = ((zf[:-1] + zf[1:]) / domain.FT(2)).astype(domain.FT)
    return zc, zf


# --------------------------------------------------------------- parameters


@dataclass
class EarthParameterSet:
    """The CLIMAParameters constants the soil model reads
    (SoilHeatParameterizations.jl:12-13), CLIMAParameters 0.1 values.  They are
    ABI inputs, never kernel literals."""
    rho_cloud_liq: float = 1e3
    rho_cloud_ice: float = 916.7
    cp_l: float = 4181.0
    cp_i: float = 2100.0
    T_0: float = 273.16
    LH_f0: float = 2.8344e6 - 2.5008e6   # LH_s0 - LH_v0
    K_therm: float = 2.4e-2
    # read by the prescribed-atmosphere BC only (boundary_conditions.jl:553-620 and the
    # SurfaceFluxes / Thermodynamics calls it makes): Planet.R_v, R_d, grav, cp_d, cp_v, LH_v0,
    # T_triple, press_triple; SubgridScale.von_karman_const
    R_v: float = 8.3144598 / 18.01528e-3
    R_d: float = 8.3144598 / 28.97e-3
    grav: float = 9.81
    cp_d: float = (8.3144598 / 28.97e-3) / (2.0 / 7.0)
    cp_v: float = 1859.0
    LH_v0: float = 2.5008e6
    T_triple: float = 273.16
    press_triple: float = 611.657
    von_karman_const: float = 0.4


_SOIL_DEFAULTS = dict(nu=0.43, S_s=1e-3, nu_ss_gravel=0.0, nu_ss_om=0.0, nu_ss_quartz=0.41,
                      rho_c_ds=2700.0, kappa_solid=3.97, rho_p=2700.0, kappa_sat_unfrozen=1.72,
                      kappa_sat_frozen=3.13, a=0.24, b=18.1, kappa_dry_parameter=0.053,
                      z_0m=0.001, z_0s=0.001)
# the reference's field names (parameters.jl:11-43) -> ASCII
_SOIL_ALIASES = {"ν": "nu", "ν_ss_gravel": "nu_ss_gravel", "ν_ss_om": "nu_ss_om",
                 "ν_ss_quartz": "nu_ss_quartz", "ρc_ds": "rho_c_ds", "κ_solid": "kappa_solid",
                 "ρp": "rho_p", "κ_sat_unfrozen": "kappa_sat_unfrozen",
                 "κ_sat_frozen": "kappa_sat_frozen", "κ_dry_parameter": "kappa_dry_parameter"}


class SoilParams:
    """SoilParams{FT}(; ν, S_s, ...) -- parameters.jl:11-43 (loam defaults).
    `nu` and `S_s` may be arrays of ncolumns values (per-column soils)."""

    def __init__(self, FT=Float64, **kw):
        self.FT = np.dtype(FT).type
        vals = dict(_SOIL_DEFAULTS)
        for k, v in kw.items():
            k = _SOIL_ALIASES.get(k, k)
            if k not in vals:
                raise TypeError(f"SoilParams has no field {k!r}")
            vals[k] = v
        self.__dict__.update(vals)

    # reference spellings
    ν = property(lambda s: s.nu)
    ρc_ds = property(lambda s: s.rho_c_ds)


class vanGenuchten:
    """vanGenuchten{FT}(; n, α, Ksat, θr) -- SoilWaterParameterizations.jl:150-169.
    Any field may be an array of ncolumns values (BASELINE config 5)."""

    def __init__(self, FT=Float64, *, n=1.56, alpha=None, Ksat=2.9e-7, theta_r=None, **kw):
        self.FT = np.dtype(FT).type
        alpha = kw.pop("α", alpha)
        theta_r = kw.pop("θr", theta_r)
        if kw:
            raise TypeError(f"vanGenuchten has no field(s) {sorted(kw)}")
        self.n = n
        self.alpha = 3.6 if alpha is None else alpha
        self.theta_r = 0.0 if theta_r is None else theta_r
        self.Ksat = Ksat

    @property
    def m(self):
        n = np.asarray(self.n, dtype=self.FT)
        return self.FT(1) - self.FT(1) / n

    α = property(lambda s: s.alpha)
    θr = property(lambda s: s.theta_r)


_THERMAL_FIELDS = ("rho_c_ds", "kappa_solid", "rho_p", "kappa_sat_unfrozen", "kappa_sat_frozen", "nu_ss_gravel",
                   "nu_ss_om", "nu_ss_quartz")   # lh_soil_class_thermal, in its order


class SoilThermal:
    """The thermal supplement of a soil class (build extension): the SoilParams fields a texture changes and
    the heat path reads, SoilThermal(FT; ρc_ds, κ_solid, ρp, κ_sat_unfrozen, κ_sat_frozen, ν_ss_gravel, ν_ss_om,
    ν_ss_quartz) with the defaults and spellings of SoilParams.  a, b and κ_dry_parameter stay scalars of the
    model's SoilParams.  Scalars only."""

    def __init__(self, FT=Float64, **kw):
        self.FT = np.dtype(FT).type
        vals = {k: _SOIL_DEFAULTS[k] for k in _THERMAL_FIELDS}
        for k, v in kw.items():
            k = _SOIL_ALIASES.get(k, k)
            if k not in vals:
                raise TypeError(f"SoilThermal has no field {k!r}")
            if np.ndim(v) != 0:
                raise ValueError(f"SoilThermal: {k} must be a scalar (a class is one texture)")
            vals[k] = v
        self.__dict__.update(vals)

    def numbers(self):
        """lh_soil_class_thermal"""
        return tuple(getattr(self, k) for k in _THERMAL_FIELDS)

    ρc_ds = property(lambda s: s.rho_c_ds)
    κ_solid = property(lambda s: s.kappa_solid)
    ρp = property(lambda s: s.rho_p)
    κ_sat_unfrozen = property(lambda s: s.kappa_sat_unfrozen)
    κ_sat_frozen = property(lambda s: s.kappa_sat_frozen)
    ν_ss_gravel = property(lambda s: s.nu_ss_gravel)
    ν_ss_om = property(lambda s: s.nu_ss_om)
    ν_ss_quartz = property(lambda s: s.nu_ss_quartz)


class SoilClass:
    """One soil class of a layered soil (build extension: the reference has one SoilParams and one
    vanGenuchten per model): a hydraulic model and the two SoilParams fields a texture changes,
    SoilClass(hydraulic_model=vanGenuchten(...), nu=, S_s=), and optionally its thermal supplement
    (thermal=SoilThermal(...)), which a model with a SoilEnergyModel needs of every class.  Scalars only."""

    def __init__(self, FT=Float64, *, hydraulic_model, nu=None, S_s=None, thermal=None, **kw):
        self.FT = np.dtype(FT).type
        nu = kw.pop("ν", nu)
        if kw:
            raise TypeError(f"SoilClass has no field(s) {sorted(kw)}")
        if thermal is not None and not isinstance(thermal, SoilThermal):
            raise TypeError("SoilClass: thermal must be a SoilThermal")
        self.thermal = thermal
        self.hydraulic_model = hydraulic_model
        self.nu = _SOIL_DEFAULTS["nu"] if nu is None else nu
        self.S_s = _SOIL_DEFAULTS["S_s"] if S_s is None else S_s
        for k, v in zip(("n", "alpha", "theta_r", "Ksat", "nu", "S_s"), self.numbers()):
            if np.ndim(v) != 0:
                raise ValueError(f"SoilClass: {k} must be a scalar (a class is one texture)")

    def numbers(self):
        """(n, alpha, theta_r, Ksat, nu, S_s): lh_soil_class"""
        hm = self.hydraulic_model
        return hm.n, hm.alpha, hm.theta_r, hm.Ksat, self.nu, self.S_s

    ν = property(lambda s: s.nu)


MAX_SOIL_CLASSES = 16   # LH_MAX_SOIL_CLASSES


class SoilClasses:
    """Layered soil (build extension): up to 16 SoilClass and the class of every cell, zero-based indices
    into `classes`.  `class_map` is [nelements] (bottom first; the same horizons in every column) or
    [ncolumns, nelements].  SoilModel(..., soil_classes=SoilClasses(...)): Richards models, and models with a
    SoilEnergyModel when every class carries its thermal supplement (SoilClass(..., thermal=SoilThermal(...)))."""

    def __init__(self, classes, class_map):
        self.classes = list(classes)
        if not 1 <= len(self.classes) <= MAX_SOIL_CLASSES:
            raise F.ModelError(F.LH_EINVAL, f"soil classes: 1 .. {MAX_SOIL_CLASSES} classes, got {len(self.classes)}")
        if not all(isinstance(k, SoilClass) for k in self.classes):
            raise TypeError("SoilClasses takes SoilClass objects")
        m = np.asarray(class_map)
        if m.ndim not in (1, 2) or not np.issubdtype(m.dtype, np.integer):
            raise ValueError("soil classes: class_map is an integer array [nelements] or [ncolumns, nelements]")
        if m.size and (m.min() < 0 or m.max() >= len(self.classes)):
            bad = np.argwhere((m < 0) | (m >= len(self.classes)))[0]
            raise F.ModelError(F.LH_EINVAL, f"soil classes: class {int(m[tuple(bad)])} at index {tuple(int(b) for b in bad)} "
                                            f"of the class map, {len(self.classes)} classes are set")
        self.class_map = np.ascontiguousarray(m, dtype=np.uint8)

    @property
    def has_thermal(self):
        """every class carries its thermal supplement"""
        return all(k.thermal is not None for k in self.classes)


def _check_soil_classes(model):
    """What the library refuses for a layered context (LH_EMODEL), raised when the model is built."""
    sc = model.soil_classes
    if not isinstance(sc, SoilClasses):
        raise TypeError("soil_classes must be a SoilClasses")
    richards = isinstance(model.energy_model, PrescribedTemperatureModel) and isinstance(model.hydrology_model, SoilHydrologyModel)
    if not richards and not (isinstance(model.energy_model, SoilEnergyModel) and sc.has_thermal):
        raise F.ModelError(F.LH_EMODEL, "soil classes are for Richards models only (SoilHydrologyModel + "
                                        "PrescribedTemperatureModel): the heat closures read the porosity -- unless every "
                                        "class carries its thermal supplement (SoilClass(..., thermal=SoilThermal(...)))")
    bcs = model.boundary_conditions
    if bcs is not None and isinstance(bcs.top, PrescribedAtmosForcing):
        raise F.ModelError(F.LH_EMODEL, "soil classes cannot be combined with a prescribed-atmosphere top")
    sp = model.soil_param_set
    vg = getattr(model.hydrology_model, "hydraulic_model", None)
    hm = vg if vg is not None else vanGenuchten(sp.FT)
    for name, v in (("n", hm.n), ("alpha", hm.alpha), ("theta_r", hm.theta_r), ("Ksat", hm.Ksat), ("nu", sp.nu), ("S_s", sp.S_s)):
        if np.ndim(v) != 0:
            raise F.ModelError(F.LH_EMODEL, f"soil classes cannot be combined with per-column parameter arrays ({name})")
    d = model.domain
    if sc.class_map.shape not in ((d.nelements,), (d.ncolumns, d.nelements)):
        raise ValueError(f"soil classes: class_map has shape {sc.class_map.shape}, expected ({d.nelements},) or "
                         f"({d.ncolumns}, {d.nelements})")


def _refuse_soil_classes(model, name):
    """The integrators and tools that have no layered kernels (LH_EMODEL in the library)."""
    if getattr(model, "soil_classes", None) is not None:
        if isinstance(model.energy_model, SoilEnergyModel):    # (the layered Newton integrators step Richards models)
            raise NotImplementedError(f"{name} is not available with soil classes (a layered coupled model steps with "
                                      "SSPRK33, LayeredCoupledImplicitEuler, LayeredCoupledTRBDF2 or "
                                      "LayeredCoupledAdaptiveTRBDF2, a layered heat-only "
                                      "model with SSPRK33, LayeredHeatImplicitEuler or LayeredHeatTRBDF2)")
        raise NotImplementedError(f"{name} is not available with soil classes (layered soils step with SSPRK33, "
                                  "LayeredImplicitEuler or LayeredTRBDF2)")


class NoEffect:
    """SoilWaterParameterizations.jl:38"""

    def __init__(self, FT=Float64):
        self.FT = FT


class TemperatureDependentViscosity:
    """SoilWaterParameterizations.jl:46-52"""

    def __init__(self, FT=Float64, *, gamma=2.64e-2, T_ref=288.0, **kw):
        self.FT = FT
        self.gamma = kw.pop("γ", gamma)
        self.T_ref = T_ref
        if kw:
            raise TypeError(f"unknown field(s) {sorted(kw)}")


class IceImpedance:
    """SoilWaterParameterizations.jl:62-65"""

    def __init__(self, FT=Float64, *, Omega=7.0, **kw):
        self.FT = FT
        self.Omega = kw.pop("Ω", Omega)
        if kw:
            raise TypeError(f"unknown field(s) {sorted(kw)}")


# ------------------------------------------------------------ component models


class SoilEnergyModel:
    """models.jl:17"""


class SoilHydrologyModel:
    """models.jl:28-33"""

    def __init__(self, FT=Float64, *, hydraulic_model=None, viscosity_factor=None,
                 impedance_factor=None):
        self.FT = np.dtype(FT).type
        self.hydraulic_model = hydraulic_model if hydraulic_model is not None else vanGenuchten(FT)
        self.viscosity_factor = viscosity_factor if viscosity_factor is not None else NoEffect(FT)
        self.impedance_factor = impedance_factor if impedance_factor is not None else NoEffect(FT)
        if not isinstance(self.viscosity_factor, (NoEffect, TemperatureDependentViscosity)):
            raise TypeError("viscosity_factor must be NoEffect or TemperatureDependentViscosity")
        if not isinstance(self.impedance_factor, (NoEffect, IceImpedance)):
            raise TypeError("impedance_factor must be NoEffect or IceImpedance")


class PrescribedTemperatureModel:
    """models.jl:51-54; default profile 288 K."""

    def __init__(self, T_profile: Optional[Callable] = None):
        self.is_default = T_profile is None
        self.T_profile = T_profile if T_profile is not None else (lambda z, t: 288.0 + 0.0 * z)


class PrescribedHydrologyModel:
    """models.jl:73-78; defaults: totally dry soil."""

    def __init__(self, vartheta_l_profile: Optional[Callable] = None,
                 theta_i_profile: Optional[Callable] = None, **kw):
        vartheta_l_profile = kw.pop("ϑ_l_profile", kw.pop("θ_l_profile", vartheta_l_profile))
        theta_i_profile = kw.pop("θ_i_profile", theta_i_profile)
        if kw:
            raise TypeError(f"unknown field(s) {sorted(kw)}")
        self.vartheta_l_profile = vartheta_l_profile or (lambda z, t: 0.0 * z)
        self.theta_i_profile = theta_i_profile or (lambda z, t: 0.0 * z)


# --------------------------------------------------------- boundary conditions


class NoBC:
    """boundary_conditions.jl:27"""


class VerticalFlux:
    """boundary_conditions.jl:43-46; positive = aligned with z-hat.  A scalar, or
    an array of ncolumns values."""

    def __init__(self, flux):
        self.flux = flux


class Dirichlet:
    """boundary_conditions.jl:61-64; state_value is t -> value (scalar or
    per-column array); a number is accepted as a constant."""

    def __init__(self, state_value):
        self.state_value = state_value if callable(state_value) else (lambda t, v=state_value: v)


class FreeDrainage:
    """boundary_conditions.jl:77"""


class SoilComponentBC:
    """boundary_conditions.jl:95-101"""

    def __init__(self, *, energy=None, hydrology=None):
        self.energy = energy if energy is not None else NoBC()
        self.hydrology = hydrology if hydrology is not None else NoBC()


class PrescribedAtmosForcing:
    """PrescribedAtmosForcing{FT}(; u_atm, θ_atm, z_atm, θ_scale, ρ_a_sfc, q_atm)
    (boundary_conditions.jl:119-132): the atmospheric state that drives the TOP face of a coupled
    water + heat soil model through Monin-Obukhov surface fluxes (:553-620), evaluated on the
    device from the top cell's state.  `u_atm`, `θ_atm`, `q_atm` may be arrays of ncolumns values
    (build extension).  Parity beyond the reference's equilibrium invariant is unpinned: the
    SurfaceFluxes / Thermodynamics formulas are restated from their published forms."""

    _FIELDS = ("u_atm", "theta_atm", "z_atm", "theta_scale", "rho_a_sfc", "q_atm")
    _ALIASES = {"θ_atm": "theta_atm", "θ_scale": "theta_scale", "ρ_a_sfc": "rho_a_sfc"}

    def __init__(self, FT=Float64, **kw):
        self.FT = np.dtype(FT).type
        vals = {}
        for k, v in kw.items():
            k = self._ALIASES.get(k, k)
            if k not in self._FIELDS:
                raise TypeError(f"PrescribedAtmosForcing has no field {k!r}")
            vals[k] = v
        missing = [k for k in self._FIELDS if k not in vals]
        if missing:                                  # Base.@kwdef without defaults: UndefKeywordError
            raise TypeError(f"PrescribedAtmosForcing: keyword argument(s) {missing} not assigned")
        self.__dict__.update(vals)

    θ_atm = property(lambda s: s.theta_atm)
    θ_scale = property(lambda s: s.theta_scale)
    ρ_a_sfc = property(lambda s: s.rho_a_sfc)


class SoilColumnBC:
    """boundary_conditions.jl:144-161"""

    def __init__(self, *, top=None, bottom=None):
        self.top = top if top is not None else SoilComponentBC()
        self.bottom = bottom if bottom is not None else SoilComponentBC()
        # SoilColumnBC{TBC <: Union{SoilComponentBC, PrescribedAtmosForcing}, BBC <: SoilComponentBC}
        if not isinstance(self.bottom, SoilComponentBC):
            raise TypeError("bottom must be a SoilComponentBC (a prescribed atmosphere is only valid at the top)")
        if not isinstance(self.top, (SoilComponentBC, PrescribedAtmosForcing)):
            raise TypeError("top must be a SoilComponentBC or a PrescribedAtmosForcing")


_BC_KIND = {NoBC: F.LH_BC_NONE, VerticalFlux: F.LH_BC_FLUX, Dirichlet: F.LH_BC_DIRICHLET,
            FreeDrainage: F.LH_BC_FREE_DRAINAGE}

# ------------------------------------------------------------------- states

_VAR = {"ϑ_l": 0, "θ_l": 0, "vartheta_l": 0, "θ_i": 1, "theta_i": 1, "ρe_int": 2, "rhoe_int": 2,
        "T": 3}
_NAMES = ["ϑ_l", "θ_i", "ρe_int", "T"]


class _Namespace:
    """`Y.soil` -- attribute access downloads the field as [ncolumns, nelements]."""

    def __init__(self, fv):
        object.__setattr__(self, "_fv", fv)

    def __getattr__(self, name):
        if name not in _VAR:
            raise AttributeError(name)
        return self._fv.get(name)

    def __setattr__(self, name, value):
        self._fv.set(name, value)


class FieldVector:
    """Device-resident analogue of Fields.FieldVector(; soil = (...)): one
    lh_state.  `fv.soil.ϑ_l` downloads, `fv.soil.ϑ_l = a` uploads (host arrays are
    level-fastest [ncolumns, nelements] like parent(field); a 1-D array of
    nelements is broadcast over columns)."""

    def __init__(self, model: "SoilModel", mask: int, zc=None):
        self.model = model
        self._be = model._backend()
        self.mask = mask
        h = C.c_void_p()
        F.check(F.lib().lh_state_create(self._be.ctx, mask, C.byref(h)), self._be.ctx)
        self.handle = h
        self.zc = zc
        self.soil = _Namespace(self)
        setattr(self, model.name, self.soil)

    def __del__(self):
        try:
            if self.handle and self._be.ctx:
                F.lib().lh_state_destroy(self._be.ctx, self.handle)
        except Exception:
            pass

    @property
    def names(self):
        return [n for i, n in enumerate(_NAMES) if self.mask & (1 << i)]

    def get(self, name) -> np.ndarray:
        d = self.model.domain
        out = np.empty((d.ncolumns, d.nelements), dtype=d.FT)
        F.check(F.lib().lh_download(self._be.ctx, self.handle, _VAR[name], out.ctypes.data, 1,
                                    d.nelements), self._be.ctx)
        return out

    def get_level(self, name, level) -> np.ndarray:
        """One level of one variable for every column ([ncolumns]; level -1 = the top
        cell): interior_values(X, :top, cs) of a host-evaluated boundary condition."""
        d = self.model.domain
        lev = int(level) % d.nelements if -d.nelements <= int(level) < d.nelements else int(level)
        out = np.empty(d.ncolumns, dtype=d.FT)
        F.check(F.lib().lh_download_level(self._be.ctx, self.handle, _VAR[name], lev, out.ctypes.data),
                self._be.ctx)
        return out

    def set(self, name, value):
        d = self.model.domain
        a = np.asarray(value, dtype=d.FT)
        if a.ndim == 0 or not a.any():
            # a constant (or all-zero) field is a fill; the library then knows a zero plane is
            # zero: a launch neither reads a zero θ_i plane nor re-stores dθ_i = 0
            F.check(F.lib().lh_state_fill(self._be.ctx, self.handle, _VAR[name],
                                          float(a) if a.ndim == 0 else 0.0), self._be.ctx)
            return
        if a.ndim == 1:
            # one value per level, the same in every column (what the reference's profile closures
            # and an initial condition f(z) give): nelements numbers cross PCIe, not a plane
            if a.shape != (d.nelements,):
                raise ValueError(f"expected shape {(d.nelements,)} for a per-level profile, got {a.shape}")
            a = np.ascontiguousarray(a)
            F.check(F.lib().lh_upload_profile(self._be.ctx, self.handle, _VAR[name], a.ctypes.data), self._be.ctx)
            return
        if a.shape != (d.ncolumns, d.nelements):
            raise ValueError(f"expected shape {(d.ncolumns, d.nelements)}, got {a.shape}")
        a = np.ascontiguousarray(a)
        F.check(F.lib().lh_upload(self._be.ctx, self.handle, _VAR[name], a.ctypes.data, 1,
                                  d.nelements), self._be.ctx)

    def similar(self) -> "FieldVector":
        return FieldVector(self.model, self.mask, self.zc)

    def copy(self) -> "FieldVector":
        o = self.similar()
        F.check(F.lib().lh_state_copy(self._be.ctx, o.handle, self.handle), self._be.ctx)
        return o

    def device_ptr(self, name):
        """Device pointer and element strides of one plane.  Until release_ptr the library assumes
        nothing about that plane (the holder may write through the pointer at any time)."""
        p, ls, cs = C.c_void_p(), C.c_int64(), C.c_int64()
        F.check(F.lib().lh_state_device_ptr(self._be.ctx, self.handle, _VAR[name], C.byref(p),
                                            C.byref(ls), C.byref(cs)), self._be.ctx)
        return p.value, ls.value, cs.value

    def release_ptr(self, name=None):
        """The holder of device_ptr pointers promises not to write through them any more
        (name None: every plane of this state)."""
        F.check(F.lib().lh_state_release_ptr(self._be.ctx, self.handle, -1 if name is None else _VAR[name]),
                self._be.ctx)


# -------------------------------------------------------------------- model


def _bc_values(model, t):
    """Evaluate the BC closures at time t -> {(face, comp): (kind, value)}."""
    out = {}
    for face, tag in ((F.LH_FACE_BOTTOM, "bottom"), (F.LH_FACE_TOP, "top")):
        fbc = getattr(model.boundary_conditions, tag)
        if isinstance(fbc, PrescribedAtmosForcing):      # set through lh_set_atmos_forcing
            continue
        for comp, cname in ((F.LH_COMP_ENERGY, "energy"), (F.LH_COMP_HYDROLOGY, "hydrology")):
            bc = getattr(fbc, cname)
            kind = _BC_KIND.get(type(bc))
            if kind is None:
                raise TypeError(f"unsupported boundary condition {type(bc).__name__}")
            val = 0.0
            if kind == F.LH_BC_FLUX:
                val = bc.flux
            elif kind == F.LH_BC_DIRICHLET:
                val = bc.state_value(t)
            out[(face, comp)] = (kind, val)
    return out


def _handle(Ya):
    """The library's state of Ya, or None for a Ya that stays on the host."""
    return Ya.handle if isinstance(Ya, FieldVector) else None


def _dptr(a):
    """double* of a contiguous float64 array, NULL for None."""
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _torch_ft_device(model):
    """(torch dtype of the model's FT, torch device of the model's context)."""
    import torch
    ft = torch.float64 if np.dtype(model.domain.FT) == np.float64 else torch.float32
    return ft, torch.device("cuda", model._backend().device_index())


class _Backend:
    """One lh_ctx: the device-side image of a SoilModel."""

    def device_index(self) -> int:
        return self._device

    def __init__(self, model: "SoilModel", stream=None, device=-1):
        d = model.domain
        L = F.lib()
        em, hm = model.energy_model, model.hydrology_model
        if isinstance(em, SoilEnergyModel) and isinstance(hm, SoilHydrologyModel):
            kind = F.LH_MODEL_COUPLED
        elif isinstance(em, SoilEnergyModel) and isinstance(hm, PrescribedHydrologyModel):
            kind = F.LH_MODEL_HEAT
        elif isinstance(em, PrescribedTemperatureModel) and isinstance(hm, SoilHydrologyModel):
            kind = F.LH_MODEL_RICHARDS
        else:
            kind = None   # prescribed/prescribed: empty RHS (right_hand_side.jl:103-112)
        self.kind = kind
        self.ctx = None
        self._keep = []
        self._device = int(device)
        if kind is None:
            return
        if self._device < 0:   # the current device, by number (buffers handed to the library live there)
            import torch
            self._device = int(torch.cuda.current_device()) if torch.cuda.is_available() else 0
            device = self._device
        cfg = F.lh_config(d.ncolumns, d.nelements, F.dtype_code(d.FT), float(d.zlim[0]),
                          float(d.zlim[1]), kind, device, stream)
        ctx = C.c_void_p()
        F.check(L.lh_create(C.byref(ctx), C.byref(cfg)), None)
        self.ctx = ctx
        ep = model.earth_param_set
        if ep is not None and kind != F.LH_MODEL_RICHARDS:
            e = F.lh_earth_params(ep.rho_cloud_liq, ep.rho_cloud_ice, ep.cp_l, ep.cp_i, ep.T_0,
                                  ep.LH_f0, ep.K_therm)
            F.check(L.lh_set_earth_params(ctx, C.byref(e)), ctx)
        sp = model.soil_param_set
        scal = {}
        for k in F.lh_soil_params._fields_:
            v = getattr(sp, k[0])
            scal[k[0]] = self._scalar_or_percol(k[0], v, d)
        s = F.lh_soil_params(**scal)
        F.check(L.lh_set_soil_params(ctx, C.byref(s)), ctx)
        if isinstance(hm, SoilHydrologyModel):
            vg = hm.hydraulic_model
            v = F.lh_vg_params(self._scalar_or_percol("vg_n", vg.n, d),
                               self._scalar_or_percol("vg_alpha", vg.alpha, d),
                               self._scalar_or_percol("vg_theta_r", vg.theta_r, d),
                               self._scalar_or_percol("vg_Ksat", vg.Ksat, d))
            F.check(L.lh_set_vg_params(ctx, C.byref(v)), ctx)
            vf, imf = hm.viscosity_factor, hm.impedance_factor
            vk = isinstance(vf, TemperatureDependentViscosity)
            ik = isinstance(imf, IceImpedance)
            F.check(L.lh_set_conductivity_factors(
                ctx, int(vk), vf.gamma if vk else 2.64e-2, vf.T_ref if vk else 288.0, int(ik),
                imf.Omega if ik else 7.0), ctx)
        sc = getattr(model, "soil_classes", None)
        if sc is not None:
            arr = (F.lh_soil_class * len(sc.classes))(*[F.lh_soil_class(*[float(x) for x in k.numbers()]) for k in sc.classes])
            F.check(L.lh_set_soil_classes(ctx, len(sc.classes), arr), ctx)
            if sc.has_thermal:   # (a Richards context ignores it; a model with an energy component needs it for the map)
                th = (F.lh_soil_class_thermal * len(sc.classes))(
                    *[F.lh_soil_class_thermal(*[float(x) for x in k.thermal.numbers()]) for k in sc.classes])
                F.check(L.lh_set_soil_class_thermal(ctx, len(sc.classes), th), ctx)
            m = sc.class_map    # [nelements]: a zero column stride broadcasts it over the columns
            F.check(L.lh_set_soil_class_map(ctx, m.ctypes.data_as(C.POINTER(C.c_uint8)), 1,
                                            0 if m.ndim == 1 else d.nelements), ctx)
        self.time_dependent_bc = False
        self.set_bcs(model, 0.0)

    def _scalar_or_percol(self, key, v, d):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            return float(a)
        if key not in F.LH_PC:
            raise ValueError(f"{key} cannot vary per column")
        if a.shape != (d.ncolumns,):
            raise ValueError(f"{key}: expected {d.ncolumns} per-column values, got shape {a.shape}")
        a = np.ascontiguousarray(a)
        F.check(F.lib().lh_set_percol_param(self.ctx, F.LH_PC[key],
                                            a.ctypes.data_as(C.POINTER(C.c_double))), self.ctx)
        return float(a[0])

    def set_atmos(self, model):
        """lh_set_atmos_forcing from SoilColumnBC.top (or its removal)."""
        L = F.lib()
        d = model.domain
        top = model.boundary_conditions.top
        if not isinstance(top, PrescribedAtmosForcing):
            if getattr(self, "_atmos_set", False):
                F.check(L.lh_set_atmos_forcing(self.ctx, None, None), self.ctx)
                self._atmos_set = False
            return
        ep, sp = model.earth_param_set, model.soil_param_set
        scal, percol = {}, np.zeros((3, d.ncolumns))
        any_pc = False
        for k, name in enumerate(("u_atm", "theta_atm", "q_atm")):
            a = np.asarray(getattr(top, name), dtype=np.float64)
            if a.ndim == 0:
                scal[name] = float(a)
                percol[k] = float(a)
            else:
                if a.shape != (d.ncolumns,):
                    raise ValueError(f"{name}: expected {d.ncolumns} per-column values")
                scal[name] = float(a[0])
                percol[k] = a
                any_pc = True
        f = F.lh_atmos_forcing(scal["u_atm"], scal["theta_atm"], float(top.z_atm), float(top.theta_scale),
                               float(top.rho_a_sfc), scal["q_atm"], float(sp.z_0m), float(sp.z_0s),
                               ep.R_v, ep.R_d, ep.grav, ep.cp_d, ep.cp_v, ep.LH_v0, ep.T_triple,
                               ep.press_triple, ep.von_karman_const)
        percol = np.ascontiguousarray(percol)
        F.check(L.lh_set_atmos_forcing(self.ctx, C.byref(f),
                                       percol.ctypes.data_as(C.POINTER(C.c_double)) if any_pc else None),
                self.ctx)
        self._atmos_set = True

    def set_bcs(self, model, t):
        if model.boundary_conditions is None:
            return
        L = F.lib()
        d = model.domain
        self.set_atmos(model)
        for (face, comp), (kind, val) in _bc_values(model, t).items():
            a = np.asarray(val, dtype=np.float64)
            if a.ndim == 0:
                F.check(L.lh_set_bc(self.ctx, face, comp, kind, float(a), None), self.ctx)
            else:
                if a.shape != (d.ncolumns,):
                    raise ValueError("per-column boundary values must have ncolumns entries")
                a = np.ascontiguousarray(a)
                F.check(L.lh_set_bc(self.ctx, face, comp, kind, float(a[0]),
                                    a.ctypes.data_as(C.POINTER(C.c_double))), self.ctx)

    def close(self):
        if self.ctx:
            F.lib().lh_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SoilModel:
    """SoilModel(FT; domain, energy_model, hydrology_model, boundary_conditions,
    soil_param_set, earth_param_set, name) -- models.jl:90-135."""

    def __init__(self, FT=Float64, *, domain, energy_model, hydrology_model, boundary_conditions,
                 soil_param_set=None, earth_param_set, name="soil", stream=None, device=-1, soil_classes=None):
        self.FT = np.dtype(FT).type
        if np.dtype(domain.FT) != np.dtype(self.FT):
            raise TypeError("domain FT differs from the model FT")   # AbstractVerticalDomain{FT}
        self.domain = domain
        self.energy_model = energy_model
        self.hydrology_model = hydrology_model
        self.boundary_conditions = boundary_conditions
        self.soil_param_set = soil_param_set if soil_param_set is not None else SoilParams(FT)
        self.earth_param_set = earth_param_set
        self.name = name
        self._stream, self._device = stream, device
        self._be = None
        # layered soils (build extension): SoilClasses, or None for the one soil of soil_param_set
        self.soil_classes = soil_classes
        if soil_classes is not None:
            _check_soil_classes(self)

    def _backend(self) -> _Backend:
        if self._be is None:
            self._be = _Backend(self, self._stream, self._device)
        return self._be

    def close(self):
        if self._be is not None:
            self._be.close()


def coordinates(model: SoilModel) -> np.ndarray:
    """coordinates(cs) (right_hand_side.jl:7-8): cell-centre z as the library
    holds them."""
    be = model._backend()
    n = model.domain.nelements
    if be.ctx is None:
        return make_function_space(model.domain)[0]
    z = np.empty(n, dtype=np.float64)
    F.check(F.lib().lh_coordinates(be.ctx, z.ctypes.data_as(C.POINTER(C.c_double))), be.ctx)
    return z.astype(model.domain.FT)


def _prognostic_mask(kind):
    return {F.LH_MODEL_RICHARDS: 0b0011, F.LH_MODEL_HEAT: 0b0100, F.LH_MODEL_COUPLED: 0b0111}[kind]


def _aux_mask(kind, model):
    """Planes of Ya the DEVICE reads: (ϑ_l, θ_i) for a prescribed hydrology; T for
    a prescribed temperature only when a viscosity factor consumes it
    (right_hand_side.jl:160).  Otherwise Ya stays a host object."""
    if kind == F.LH_MODEL_HEAT:
        return 0b0011
    if kind == F.LH_MODEL_RICHARDS and isinstance(model.hydrology_model.viscosity_factor,
                                                  TemperatureDependentViscosity):
        return 0b1000
    return 0


class _HostAux:
    """Ya for models whose aux fields never reach the device (or prescribed /
    prescribed models): plain host arrays with the same attribute access."""

    def __init__(self, zc, fields):
        self.zc = zc
        self.soil = type("soil", (), {})()
        for k, v in fields.items():
            setattr(self.soil, k, v)


def make_update_aux(component_model, model: Optional[SoilModel] = None):
    """make_update_aux (right_hand_side.jl:54-96): returns update_aux!(Ya, t),
    which overwrites the prescribed fields of Ya with the closures at time t."""
    if isinstance(component_model, PrescribedTemperatureModel):
        def update_aux(Ya, t):
            z = np.asarray(Ya.zc)
            Ya.soil.T = np.asarray(component_model.T_profile(z, t) + 0.0 * z)
            return Ya
        return update_aux
    if isinstance(component_model, PrescribedHydrologyModel):
        def update_aux(Ya, t):
            z = np.asarray(Ya.zc)
            Ya.soil.θ_l = np.asarray(component_model.vartheta_l_profile(z, t) + 0.0 * z)
            Ya.soil.θ_i = np.asarray(component_model.theta_i_profile(z, t) + 0.0 * z)
            return Ya
        return update_aux

    def update_aux(Ya, t):      # models that add no auxiliary variables (:91-96)
        return None
    return update_aux


def initialize_states(model: SoilModel, f: Callable, t0):
    """initialize_states(model, f, t0) -> (Y, Ya) (initial_conditions.jl:101-107).
    `f(z, model)` returns a dict (NamedTuple) of the prognostic variables at the
    centre coordinate z; it is called once with the vector of nelements centres
    (scalars, [nelements] or [ncolumns, nelements] values are accepted), or per
    level if it cannot take arrays."""
    be = model._backend()
    d = model.domain
    zc = coordinates(model)
    if be.kind is None:
        fields = {}
        if isinstance(model.energy_model, PrescribedTemperatureModel):
            fields["T"] = np.asarray(model.energy_model.T_profile(zc, t0) + 0.0 * zc)
        if isinstance(model.hydrology_model, PrescribedHydrologyModel):
            fields["θ_l"] = np.asarray(model.hydrology_model.vartheta_l_profile(zc, t0) + 0 * zc)
            fields["θ_i"] = np.asarray(model.hydrology_model.theta_i_profile(zc, t0) + 0 * zc)
        return {}, _HostAux(zc, fields)
    try:
        ic = f(zc, model)
        ic = {k: np.asarray(v) for k, v in ic.items()}
    except (TypeError, ValueError):
        per = [f(d.FT(z), model) for z in zc]
        ic = {k: np.array([p[k] for p in per]) for k in per[0]}
    Y = FieldVector(model, _prognostic_mask(be.kind), zc)
    want = set(Y.names)
    got = {_NAMES[_VAR[k]] for k in ic}
    if got != want:
        raise KeyError(f"initial condition must provide {sorted(want)}, got {sorted(ic)}")
    for k, v in ic.items():
        if v.ndim == 0:
            v = np.full(d.nelements, v)
        Y.set(k, v)
    am = _aux_mask(be.kind, model)
    Ya = FieldVector(model, am, zc) if am else _HostAux(zc, {})
    make_update_aux(model.energy_model)(Ya, t0)
    make_update_aux(model.hydrology_model)(Ya, t0)
    return Y, Ya


def default_initial_conditions(model: SoilModel):
    """models.jl:147-166: isothermal soil at T0 = 273.16, no ice, ϑ_l = ν/2; only
    for SoilEnergyModel + SoilHydrologyModel."""
    if not (isinstance(model.energy_model, SoilEnergyModel)
            and isinstance(model.hydrology_model, SoilHydrologyModel)):
        raise RuntimeError("No default IC exist for this type of soil model.")
    FT = model.FT
    ep, sp = model.earth_param_set, model.soil_param_set

    def ic(z, m):
        T = FT(273.16)
        theta_i = FT(0.0)
        theta_l = FT(0.5) * FT(sp.nu)
        # volumetric_heat_capacity / volumetric_internal_energy with FT rounding
        rho_i, rho_l = FT(ep.rho_cloud_ice), FT(ep.rho_cloud_liq)
        rhocp_i = FT(ep.cp_i * float(rho_i))
        rhocp_l = FT(ep.cp_l * float(rho_l))
        rho_c_s = FT(sp.rho_c_ds) + theta_l * rhocp_l + theta_i * rhocp_i
        rhoe = rho_c_s * (T - FT(ep.T_0)) - theta_i * rho_i * FT(ep.LH_f0)
        return {"ϑ_l": theta_l, "θ_i": theta_i, "ρe_int": rhoe}

    return initialize_states(model, ic, FT(0.0))


# Placement tuning (lh_tune_placement) is explicit: call `tune_placement(model, Y, Ya, dY)` once
# per (Y, dY) pair of a large ensemble.  LH_PLACEMENT_TUNE=1 opts in to the host mirror doing it
# by itself on the first rhs! / step of ensembles whose planes reach this size -- never moving
# the input state (device pointers a user holds for Y stay valid).
PLACEMENT_TUNE_MIN_PLANE_BYTES = 32 << 20


def _placement_tuning_wanted(model: SoilModel) -> bool:
    d = model.domain
    if os.environ.get("LH_PLACEMENT_TUNE", "0") != "1" or getattr(model, "soil_classes", None) is not None:
        return False
    return d.ncolumns * d.nelements * np.dtype(d.FT).itemsize >= PLACEMENT_TUNE_MIN_PLANE_BYTES


def tune_placement(model: SoilModel, Y: "FieldVector", Ya=None, dY: Optional["FieldVector"] = None,
                   max_candidates: int = 0, move_input: bool = False):
    """Build extension (no counterpart in the reference): let the library choose, by
    timing the real launch, where in HBM the state written by rhs! (dY given) or the
    SSPRK33 stage state (dY=None) lives -- lh_tune_placement.  Returns the launch
    time in ms before and after.  Results of later calls do not depend on it."""
    _refuse_soil_classes(model, "tune_placement")
    be = model._backend()
    ya = _handle(Ya)
    be.set_bcs(model, 0.0)
    b, a = C.c_float(), C.c_float()
    F.check(F.lib().lh_tune_placement(be.ctx, Y.handle, ya, dY.handle if dY is not None else None,
                                      int(max_candidates), F.LH_PLACE_MOVE_INPUT if move_input else 0,
                                      C.byref(b), C.byref(a)), be.ctx)
    return b.value, a.value


def make_rhs(model: SoilModel):
    """make_rhs(model) -> rhs!(dY, Y, Ya, t) (right_hand_side.jl:33-44).  In place
    on dY, returns dY.  Everything numerical happens in lh_rhs on the GPU."""
    be = model._backend()
    if be.kind is None:
        def rhs_empty(dY, Y, Ya, t):   # right_hand_side.jl:103-112
            make_update_aux(model.energy_model)(Ya, t)
            make_update_aux(model.hydrology_model)(Ya, t)
            return dY
        return rhs_empty
    update_en = make_update_aux(model.energy_model)
    update_hy = make_update_aux(model.hydrology_model)
    L = F.lib()
    needs_aux = bool(_aux_mask(be.kind, model))
    placed = set() if _placement_tuning_wanted(model) else None   # (Y, dY) pairs already placed

    def rhs(dY, Y, Ya, t):
        if needs_aux:
            update_en(Ya, t)
            update_hy(Ya, t)
        be.set_bcs(model, t)
        ya = _handle(Ya)
        if placed is not None and (id(Y), id(dY)) not in placed:
            placed.add((id(Y), id(dY)))
            F.check(L.lh_tune_placement(be.ctx, Y.handle, ya, dY.handle, 0, 0, None, None), be.ctx)
        F.check(L.lh_rhs(be.ctx, float(t), Y.handle, ya, dY.handle), be.ctx)
        return dY

    return rhs


def compute_turbulent_surface_fluxes(energy, hydrology, model: SoilModel, vartheta_l, theta_i, T):
    """compute_turbulent_surface_fluxes(energy, hydrology, model, ϑ_l, θ_i, T)
    (boundary_conditions.jl:553-620) -> (heat_flux, Ẽ): the surface heat flux and water volume
    flux the prescribed atmosphere of `model.boundary_conditions.top` drives for a top-cell state
    (scalars or arrays), evaluated on the device (lh_atmos_surface_fluxes).  Only
    SoilEnergyModel + SoilHydrologyModel has a method (test_prescribed_atmos_bc.jl:161-183)."""
    if not (isinstance(energy, SoilEnergyModel) and isinstance(hydrology, SoilHydrologyModel)):
        raise TypeError("no method compute_turbulent_surface_fluxes for "
                        f"({type(energy).__name__}, {type(hydrology).__name__})")
    be = model._backend()
    be.set_bcs(model, 0.0)
    vl, ti, T = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (vartheta_l, theta_i, T)))
    shape = vl.shape
    vl, ti, T = (np.ascontiguousarray(a.reshape(-1)) for a in (vl, ti, T))
    heat, water = np.empty_like(vl), np.empty_like(vl)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    F.check(F.lib().lh_atmos_surface_fluxes(be.ctx, vl.size, dp(vl), dp(ti), dp(T), dp(heat), dp(water)), be.ctx)
    FT = model.FT
    if shape == ():
        return FT(heat[0]), FT(water[0])
    return heat.reshape(shape).astype(FT), water.reshape(shape).astype(FT)


def boundary_fluxes(X, bc, face, model: SoilModel, cs=None, t=0.0):
    """boundary_fluxes(X, bc, face, model, cs, t) (boundary_conditions.jl:470-489, :516-533): the named
    pair (fρe_int, fϑ_l) of one face -- the two SetValue fluxes of the tendency -- for every column.

    * `bc` a PrescribedAtmosForcing and `X = (ϑ_l, θ_i, T)` host values of the top cell: the
      surface fluxes of those states (compute_turbulent_surface_fluxes), as the reference's tests
      call it.
    * `bc` a SoilComponentBC (the model's own `boundary_conditions.top` / `.bottom`) and `X` the
      device state -- `Y`, or `(Y, Ya)` when the model reads prescribed fields: evaluated on the
      device by the function the tendency kernel uses (lh_boundary_fluxes), [ncolumns] each; a
      component without a boundary condition gives NaN (`nothing` in the reference)."""
    tag = face.lstrip(":") if isinstance(face, str) else face
    if tag not in ("top", "bottom"):
        raise ValueError("Expected :top or :bottom")                 # boundary_conditions.jl:188
    if isinstance(bc, PrescribedAtmosForcing) and not isinstance(X, (FieldVector, tuple)) or (
            isinstance(bc, PrescribedAtmosForcing) and isinstance(X, tuple) and not isinstance(X[0], FieldVector)):
        if tag != "top":
            raise RuntimeError("Prescribed atmosphere-driven boundary conditions are only valid at the "
                               "top of the soil column.")            # :523-528
        vl, ti, T = X
        h, w = compute_turbulent_surface_fluxes(model.energy_model, model.hydrology_model, model, vl, ti, T)
        return {"fρe_int": h, "fϑ_l": w}
    if isinstance(bc, PrescribedAtmosForcing) and tag != "top":
        raise RuntimeError("Prescribed atmosphere-driven boundary conditions are only valid at the "
                           "top of the soil column.")
    if bc is not getattr(model.boundary_conditions, tag):
        raise ValueError("boundary_fluxes on the device evaluates the model's own boundary condition of that face: "
                         f"pass model.boundary_conditions.{tag}")
    Y, Ya = X if isinstance(X, tuple) else (X, None)
    be = model._backend()
    be.set_bcs(model, t)
    d = model.domain
    fe, fw = np.empty(d.ncolumns), np.empty(d.ncolumns)
    ya = _handle(Ya)
    F.check(F.lib().lh_boundary_fluxes(be.ctx, Y.handle, ya, float(t), F.LH_FACE_TOP if tag == "top" else F.LH_FACE_BOTTOM,
                                       fe.ctypes.data_as(C.POINTER(C.c_double)), fw.ctypes.data_as(C.POINTER(C.c_double))),
            be.ctx)
    return {"fρe_int": fe.astype(d.FT), "fϑ_l": fw.astype(d.FT)}


def stable_dt(model: SoilModel, Y: "FieldVector", Ya=None, courant: float = 0.5) -> float:
    """Build extension (the reference steps with a fixed user dt): the largest
    step the explicit diffusive bound allows on this rank's columns,
    courant * dz^2 / max face diffusivity (lh_stable_dt).  Across ranks take the
    minimum with `partition.global_min_dt`."""
    be = model._backend()
    out = C.c_double()
    ya = _handle(Ya)
    F.check(F.lib().lh_stable_dt(be.ctx, Y.handle, ya, float(courant), C.byref(out)), be.ctx)
    return out.value


def set_tuning(model: SoilModel, spec: str) -> None:
    """Build extension: the run-time launch overrides of the model's context (lh_set_tuning), in the words of the
    LH_TUNE environment variable, e.g. "persist=2".  Keys the string does not name go back to their defaults."""
    be = model._backend()
    F.check(F.lib().lh_set_tuning(be.ctx, str(spec).encode()), be.ctx)


def step_engine(model: SoilModel, nsteps: int, per_stage_boundary_values: bool = False) -> int:
    """Build extension: what an SSPRK33 call of `nsteps` steps on the model's context would run (lh_step_engine):
    _ffi.LH_ENGINE_COLUMN_STEPPER, all steps in one launch with the state in registers, or
    _ffi.LH_ENGINE_FUSED_STAGES, three launches per step."""
    be = model._backend()
    rc = F.lib().lh_step_engine(be.ctx, int(nsteps), 1 if per_stage_boundary_values else 0)
    if rc < 0:
        F.check(rc, be.ctx)
    return rc


def step_series_engine(model: SoilModel, nsteps: int) -> int:
    """Build extension: what a step_series call of `nsteps` steps on the model's context would run
    (lh_step_series_engine): _ffi.LH_ENGINE_COLUMN_STEPPER, one launch in which every column's wave samples its own
    series, or _ffi.LH_ENGINE_FUSED_STAGES, three launches per step behind one that samples the step's values."""
    be = model._backend()
    rc = F.lib().lh_step_series_engine(be.ctx, int(nsteps))
    if rc < 0:
        F.check(rc, be.ctx)
    return rc


def step_series(model: SoilModel, Y: "FieldVector", Ya, series: "BoundarySeries", t: float, dt: float, nsteps: int):
    """Build extension: `nsteps` SSPRK33 steps of `dt` from `t` under a BoundarySeries in one library call
    (lh_step_ssprk33_series): the result of lh_step_ssprk33, with the boundary value of every (face, component) of the
    series sampled per column at every stage time t_k, t_k + dt, t_k + dt / 2 (t_k = t + dt k).  A component without a
    series keeps the model's boundary value of `t` for the whole call (closures are not sampled at the stage times).
    Every stage time must lie within the knots (ValueError).  Asynchronous; returns the time reached."""
    if not isinstance(series, BoundarySeries):
        raise TypeError("step_series: series must be a BoundarySeries")
    nsteps, t, dt = int(nsteps), float(t), float(dt)
    if nsteps < 0 or not dt > 0:
        raise ValueError("step_series: need nsteps >= 0 and dt > 0")
    if not np.isfinite(t):
        raise ValueError("step_series: t is not finite")
    if nsteps:
        times = _stage_times(t, dt, nsteps)
        series._check_span(float(times.min()), float(times.max()))
    be = model._backend()
    be.set_bcs(model, t)
    F.check(F.lib().lh_step_ssprk33_series(be.ctx, Y.handle, _handle(Ya), series._device(model), t, dt, nsteps), be.ctx)
    return t + nsteps * dt


def step_adaptive(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, courant: float = 0.5,
                  nsteps: int = 1, dt_max: float = 0.0, profiles_constant: bool = False, hold: int = None):
    """Build extension: `nsteps` adaptive SSPRK33 steps of `Y` with nothing leaving the device
    (lh_step_ssprk33_adaptive: per step the tendency and the stable-step bound in one launch, the
    min over ranks when a communicator is attached, stages 2 and 3 -- three evaluations of the
    right-hand side per step).  Boundary values are those of time `t` (constant over the call: a
    time-dependent Dirichlet closure needs the stage times, i.e. `Simulation` with a fixed dt).
    The stage times of an adaptive step are not known in advance, so prescribed profiles the device
    reads (T with a viscosity factor, the water fields of a heat-only model) cannot be probed for
    time dependence: the caller states `profiles_constant=True` (they are then taken at time `t`).
    `hold` > 1 (lh_step_ssprk33_adaptive_hold): the step size is formed once per CHUNK of `hold` steps
    and held over it -- `nsteps` then counts chunks, the call takes `nsteps * hold` steps, with one
    stepper launch (and one collective) per chunk where the persistent column stepper serves it.  Bit
    5 of the status reports a held step that exceeded the stable step of the state it produced.
    A Richards model with soil_classes (up to 128 levels) has the held form only
    (lh_step_layered_ssprk33_adaptive_hold: one launch of the layered column stepper per chunk, which leaves the
    next bound): it is taken for every `hold` that is given, `hold=1` included.  Without `hold` the call is
    lh_step_ssprk33_adaptive, which has no layered form and refuses as before.
    Returns (simulated time advanced, last dt)."""
    layered = getattr(model, "soil_classes", None) is not None
    if layered and (hold is None or not isinstance(model.energy_model, PrescribedTemperatureModel)):
        _refuse_soil_classes(model, "step_adaptive" if hold is not None else "step_adaptive without hold=k")
    hold = 1 if hold is None else hold
    if int(hold) < 1:
        raise ValueError("step_adaptive: hold must be >= 1")
    if _time_dependent(model):
        raise ValueError("step_adaptive needs boundary values that do not depend on time")
    if _device_reads_aux(model, Ya):
        if not profiles_constant:
            raise ValueError("step_adaptive: the device reads prescribed profiles whose time dependence cannot be "
                             "probed at unknown stage times; pass profiles_constant=True if they do not depend on t")
        make_update_aux(model.energy_model)(Ya, t)
        make_update_aux(model.hydrology_model)(Ya, t)
    be = model._backend()
    L = F.lib()
    ya = _handle(Ya)
    be.set_bcs(model, t)
    import torch
    # [dt, elapsed] on the CONTEXT's device; the zero fill runs on torch's stream, the library on its
    # own (non-blocking) one: the fill must have completed before the first `*elapsed += dt`
    dtype, dev = _torch_ft_device(model)
    buf = torch.zeros(2, device=dev, dtype=dtype)
    torch.cuda.synchronize(dev)
    dt_ptr, elapsed_ptr = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + buf.element_size())
    if layered:
        F.check(L.lh_step_layered_ssprk33_adaptive_hold(be.ctx, Y.handle, ya, float(t), float(courant), float(dt_max),
                                                        int(nsteps), int(hold), dt_ptr, elapsed_ptr), be.ctx)
    elif int(hold) == 1:
        F.check(L.lh_step_ssprk33_adaptive(be.ctx, Y.handle, ya, float(t), float(courant), float(dt_max), int(nsteps),
                                           dt_ptr, elapsed_ptr), be.ctx)
    else:
        F.check(L.lh_step_ssprk33_adaptive_hold(be.ctx, Y.handle, ya, float(t), float(courant), float(dt_max),
                                                int(nsteps), int(hold), dt_ptr, elapsed_ptr), be.ctx)
    F.check(L.lh_synchronize(be.ctx), be.ctx)
    dt, elapsed = (float(x) for x in buf.cpu())
    return elapsed, dt


# --------------------------------------------------------------- Simulations


# Each method marker states what it refuses (check_scope: NotImplementedError, as the library's LH_EMODEL)
# and how a Simulation advances `nsteps` intervals of dt with it (advance: returns the time reached, None
# for it.t + nsteps dt; _advance keeps the step count and the time).  A family's first marker says both; its layered
# and series forms carry what differs: `_layered`, the library call that serves a model without soil classes, the forcing.


@dataclass(frozen=True)
class _Scope:
    """What one integrator family serves, and the words of its refusals ({name}: the marker or function that refuses).
    The library's own words and order (LH_EMODEL) are mirrored here, and GPU tests match them."""
    energy: type
    hydrology: type
    pair: str                      # another model pair
    no_classes: str                # a layered call on a model without soil classes ({scalar}: the call that serves it)
    factors: Optional[str] = None  # conductivity factors other than NoEffect (None: not refused)
    atmos: Optional[str] = None    # a prescribed-atmosphere top (None: not refused)
    no_factors: Optional[str] = None  # a factors call on a model whose factors are both NoEffect (None: not refused)
    viscosity: Optional[str] = None   # a viscosity factor other than NoEffect, refused on its own (None: not refused)
    no_impedance: Optional[str] = None  # an impedance call on a model whose impedance factor is NoEffect (None: not refused)


_RICHARDS = _Scope(      # lh_step_[layered_]implicit_euler, lh_integrate_[layered_]trbdf2
    PrescribedTemperatureModel, SoilHydrologyModel,
    "{name} is provided for Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)",
    "{name} is provided for models with soil_classes (without them: ImplicitEuler, TRBDF2)",
    "{name} supports the NoEffect conductivity factors only",
    "{name} does not support a prescribed-atmosphere top")
_RICHARDS_FACTORS = _Scope(   # lh_step_factors_implicit_euler, lh_integrate_factors_trbdf2
    PrescribedTemperatureModel, SoilHydrologyModel,
    _RICHARDS.pair, _RICHARDS.no_classes, None, _RICHARDS.atmos,
    "{name} is provided for models with a conductivity factor other than NoEffect (without one: ImplicitEuler, TRBDF2)")
_HEAT_FIXED = _Scope(    # lh_step_[layered_]heat_implicit
    SoilEnergyModel, PrescribedHydrologyModel,
    "{name} is provided for heat-only models only (SoilEnergyModel + PrescribedHydrologyModel)",
    "{name} is provided for models with soil_classes (without them: HeatImplicitEuler, HeatTRBDF2)")
_HEAT_ADAPTIVE = _Scope(  # lh_integrate_[layered_]heat_trbdf2, lh_integrate_heat_series
    SoilEnergyModel, PrescribedHydrologyModel,
    "{name}: heat-only models (SoilEnergyModel + PrescribedHydrologyModel)",
    "{name}: the context has no class map (lh_set_soil_class_map); lh_integrate_heat_trbdf2 steps a model without soil "
    "classes")
_COUPLED = _Scope(       # lh_step_[layered_]coupled_implicit, lh_integrate_[layered_]coupled_trbdf2, ..._coupled_series
    SoilEnergyModel, SoilHydrologyModel,
    "{name}: coupled models only (SoilEnergyModel + SoilHydrologyModel)",
    "{name}: the context has no class map (lh_set_soil_class_map); {scalar} steps a model without soil classes",
    "{name}: conductivity factors other than NoEffect are not supported",
    "{name}: a prescribed-atmosphere top is not supported")
_COUPLED_FACTORS = _Scope(   # lh_step_coupled_factors_implicit
    SoilEnergyModel, SoilHydrologyModel,
    _COUPLED.pair, _COUPLED.no_classes, None, _COUPLED.atmos, None,
    "{name}: a viscosity factor other than NoEffect is not supported: the water then reads the unknown T and the stage is "
    "no longer block triangular",
    "{name}: the context has no impedance factor (lh_set_conductivity_factors); lh_step_coupled_implicit steps a model "
    "without conductivity factors")


def _check_scope(model, name, scope, layered=False, scalar=None):
    """NotImplementedError for what the library calls of `scope` refuse with LH_EMODEL, in their order: the model
    pair, the class map (layered: its absence), conductivity factors (a factors call: their absence; an impedance
    call: a viscosity factor, then the impedance factor's absence), an atmosphere top."""
    if not (isinstance(model.energy_model, scope.energy) and isinstance(model.hydrology_model, scope.hydrology)):
        raise NotImplementedError(scope.pair.format(name=name))
    if not layered:
        _refuse_soil_classes(model, name)
    elif getattr(model, "soil_classes", None) is None:
        raise NotImplementedError(scope.no_classes.format(name=name, scalar=scalar))
    hm, bcs = model.hydrology_model, model.boundary_conditions
    if scope.viscosity and not isinstance(hm.viscosity_factor, NoEffect):
        raise NotImplementedError(scope.viscosity.format(name=name))
    if scope.no_impedance and isinstance(hm.impedance_factor, NoEffect):
        raise NotImplementedError(scope.no_impedance.format(name=name))
    if scope.no_factors and isinstance(hm.viscosity_factor, NoEffect) and isinstance(hm.impedance_factor, NoEffect):
        raise NotImplementedError(scope.no_factors.format(name=name))
    if scope.factors and not (isinstance(hm.viscosity_factor, NoEffect) and isinstance(hm.impedance_factor, NoEffect)):
        raise NotImplementedError(scope.factors.format(name=name))
    if scope.atmos and bcs is not None and isinstance(bcs.top, PrescribedAtmosForcing):
        raise NotImplementedError(scope.atmos.format(name=name))


def _marker_scope(self, model):
    """check_scope of every marker but SSPRK33: its family's refusals under the marker's own name"""
    _check_scope(model, type(self).__name__, self._scope, self._layered, self._scalar)


def _chunk_end(it, nsteps):
    """The end of a chunk of nsteps intervals of dt, as the fixed-step methods reach it; tf itself at the last."""
    last = it._nsteps_done + nsteps >= int(round((it.tf - it.t0) / it.dt))
    return it.tf if last else it.t0 + (it._nsteps_done + nsteps) * it.dt


def _refresh_prescribed(model, Ya, t):
    """The prescribed profiles of THIS time in a Ya the device reads; a call holds them at these values."""
    if isinstance(Ya, FieldVector):
        make_update_aux(model.energy_model)(Ya, t)
        make_update_aux(model.hydrology_model)(Ya, t)


class SSPRK33:
    """OrdinaryDiffEq.SSPRK33 marker (the only stepper the reference's tests use)."""

    def check_scope(self, model):
        pass

    def advance(self, sim, nsteps):
        return _advance_ssprk33(sim, nsteps)


class SeriesSSPRK33(SSPRK33):
    """SSPRK33 under a BoundarySeries (lh_step_ssprk33_series): every advance is set_bcs at the chunk's start and ONE
    step_series call for the chunk, every column with its own boundary values at every stage time.  forcing: the
    BoundarySeries (required); its values replace the model's on its (face, component)s, a time-dependent closure on
    the same component included (Dirichlet closures are not sampled, as under TRBDF2(forcing=...)).  Every model
    SSPRK33 steps, conductivity factors and a prescribed-atmosphere top included.  Prescribed profiles the device
    reads must not change over a chunk: that case is SSPRK33's stage-by-stage path, which takes no series.
    (A marker of its own rather than SSPRK33(forcing=...): SSPRK33's constructor is pinned without arguments.)"""

    def __init__(self, forcing):
        self.forcing = _series_forcing(type(self).__name__, forcing)

    def check_scope(self, model):
        _series_forcing(type(self).__name__, self.forcing)

    def advance(self, sim, nsteps):
        return _advance_ssprk33_series(sim, nsteps)


class ImplicitEuler:
    """OrdinaryDiffEq.ImplicitEuler marker: backward Euler with Newton and one tridiagonal solve per
    column and iteration (lh_step_implicit_euler).  Richards models without conductivity factors
    and without a prescribed atmosphere; a heat-only model steps implicitly under HeatImplicitEuler /
    HeatTRBDF2 (lh_step_heat_implicit).  tol / max_iter: None = the library's defaults."""
    _scope, _layered, _scalar = _RICHARDS, False, None
    check_scope = _marker_scope

    def __init__(self, tol=None, max_iter=None):
        self.tol = tol
        self.max_iter = max_iter

    def advance(self, sim, nsteps):
        it = sim.integrator
        call = step_implicit_layered if self._layered else step_implicit
        call(sim.model, it.u, it.p, it.t, it.dt, nsteps, self.tol, self.max_iter)


class TRBDF2:
    """OrdinaryDiffEq.TRBDF2 marker: L-stable, second-order TR-BDF2 with per-column error control
    (lh_integrate_trbdf2).  abstol / reltol: None = OrdinaryDiffEq's defaults (1e-6, 1e-3), each on its
    own: TRBDF2(reltol=1e-5) keeps abstol 1e-6.
    adaptive=False: steps of exactly the Simulation's dt, no error control.  The Simulation's dt is the
    initial step and the interval at which Dirichlet closures are sampled; a model without them runs a
    whole saveat chunk per library call.  Same scope as ImplicitEuler.
    forcing: None or a BoundarySeries; with it every advance is one integrate_series call (the series' values
    replace the model's on its (face, component)s, Dirichlet closures are not sampled)."""
    _scope, _layered, _scalar = _RICHARDS, False, None
    check_scope = _marker_scope

    def __init__(self, abstol=None, reltol=None, adaptive=True, forcing=None):
        self.abstol = abstol
        self.reltol = reltol
        self.adaptive = adaptive
        self.forcing = forcing

    def advance(self, sim, nsteps):
        return _advance_trbdf2(sim, _chunk_end(sim.integrator, nsteps))

    def integrate(self, model, Y, Ya, t0, t1, dt, dt_cols):
        call = integrate_layered_trbdf2 if self._layered else integrate_trbdf2
        return call(model, Y, Ya, t0, t1, dt, self.abstol, self.reltol, self.adaptive, dt_cols)

    def integrate_forcing(self, model, Y, Ya, t0, t1, dt, dt_cols):
        """One library call from t0 to t1 under self.forcing: what _advance_trbdf2 makes of an advance."""
        return integrate_series(model, Y, Ya, self.forcing, t0, t1, dt, self.abstol, None, self.reltol, self.adaptive, dt_cols)


class LayeredImplicitEuler(ImplicitEuler):
    """ImplicitEuler for a Richards model with soil_classes (lh_step_layered_implicit_euler): the same Newton,
    with the Jacobian, the safeguard and the convergence test taking every cell's own class."""
    _layered = True


class LayeredTRBDF2(TRBDF2):
    """TRBDF2 for a Richards model with soil_classes (lh_integrate_layered_trbdf2): the same stages, error
    estimate and per-column controller over LayeredImplicitEuler's Newton."""
    _layered = True


class FactorsImplicitEuler(ImplicitEuler):
    """ImplicitEuler for a Richards model whose hydrology has a conductivity factor other than NoEffect
    (TemperatureDependentViscosity and / or IceImpedance; lh_step_factors_implicit_euler): the same Newton, with the
    factors in the tendency and their slope in the Jacobian.  A model with soil_classes, one whose factors are both
    NoEffect (ImplicitEuler serves it) and a prescribed-atmosphere top are refused.  Simulation refreshes the
    prescribed profiles between library calls and a call holds them: with a time-dependent T_profile the viscosity
    factor is piecewise constant over a saveat chunk (over the run without saveat)."""
    _scope = _RICHARDS_FACTORS

    def advance(self, sim, nsteps):
        it = sim.integrator
        _refresh_prescribed(sim.model, it.p, it.t)   # (held through the chunk)
        step_implicit_factors(sim.model, it.u, it.p, it.t, it.dt, nsteps, self.tol, self.max_iter)


class FactorsTRBDF2(TRBDF2):
    """TRBDF2 for a Richards model whose hydrology has a conductivity factor other than NoEffect
    (lh_integrate_factors_trbdf2): the same stages, error estimate and per-column controller over
    FactorsImplicitEuler's Newton; scope as FactorsImplicitEuler.  No forcing: boundary-value series do not take
    these models.  Simulation refreshes the prescribed profiles at the start of every saveat chunk and the chunk
    holds them: with a time-dependent T_profile the viscosity factor is piecewise constant over a saveat chunk."""
    _scope = _RICHARDS_FACTORS

    def __init__(self, abstol=None, reltol=None, adaptive=True):
        super().__init__(abstol, reltol, adaptive)

    def advance(self, sim, nsteps):
        it = sim.integrator
        _refresh_prescribed(sim.model, it.p, it.t)   # (held through the chunk)
        return _advance_trbdf2(sim, _chunk_end(it, nsteps))

    def integrate(self, model, Y, Ya, t0, t1, dt, dt_cols):
        return integrate_factors_trbdf2(model, Y, Ya, t0, t1, dt, self.abstol, self.reltol, self.adaptive, dt_cols)


class HeatImplicitEuler:
    """Backward Euler of a heat-only model, SoilEnergyModel + PrescribedHydrologyModel
    (lh_step_heat_implicit): the tendency is affine in ρe_int, so a step is one exact tridiagonal solve
    with a matrix factored once per library call -- no Newton, no tolerance.  Simulation runs one call
    per saveat chunk (per run without saveat); the prescribed ϑ_l and θ_i are refreshed between calls and
    held within one."""
    method = "euler"
    _scope, _layered, _scalar = _HEAT_FIXED, False, None
    check_scope = _marker_scope

    def advance(self, sim, nsteps):
        it, model = sim.integrator, sim.model
        _refresh_prescribed(model, it.p, it.t)
        call = step_implicit_layered_heat if self._layered else step_implicit_heat
        call(model, it.u, it.p, it.t, it.dt, nsteps, self.method)


class HeatTRBDF2(HeatImplicitEuler):
    """Fixed-step TR-BDF2 of a heat-only model (lh_step_heat_implicit with LH_HEAT_TRBDF2): second order,
    L-stable, two exact tridiagonal solves per step of the Simulation's dt, no error control.  Calls and
    prescribed profiles as HeatImplicitEuler."""
    method = "trbdf2"


class LayeredHeatImplicitEuler(HeatImplicitEuler):
    """HeatImplicitEuler for a heat-only model with soil_classes (lh_step_layered_heat_implicit): every cell takes
    ρc_s and κ from its own class, the tendency stays affine in ρe_int and a step one exact tridiagonal solve.
    Calls and prescribed profiles as HeatImplicitEuler."""
    _layered = True


class LayeredHeatTRBDF2(LayeredHeatImplicitEuler):
    """HeatTRBDF2 for a heat-only model with soil_classes (lh_step_layered_heat_implicit with LH_HEAT_TRBDF2)."""
    method = "trbdf2"


class HeatAdaptiveTRBDF2:
    """TR-BDF2 of a heat-only model with per-column error control (lh_integrate_heat_trbdf2): HeatTRBDF2's exact
    stage solves under TRBDF2's controller, the error estimate filtered by the stage matrix itself.  abstol_e (on
    ρe_int) and reltol: 0.0 = the library's defaults (1e-6 ρ_l c_l, 1e-3), each on its own.  The Simulation's dt is the
    initial step and the interval at which Dirichlet closures are sampled, as for TRBDF2; the per-column proposals carry
    over from call to call.  The prescribed ϑ_l and θ_i are refreshed once per saveat chunk and held through it, as for
    HeatImplicitEuler.  No forcing: under a BoundarySeries use HeatSeriesTRBDF2."""
    _scope, _layered, _scalar = _HEAT_ADAPTIVE, False, None
    check_scope = _marker_scope

    def __init__(self, abstol_e=0.0, reltol=0.0):
        self.abstol_e = abstol_e
        self.reltol = reltol

    def advance(self, sim, nsteps):
        it = sim.integrator
        _refresh_prescribed(sim.model, it.p, it.t)   # (held through the chunk)
        return _advance_trbdf2(sim, _chunk_end(it, nsteps))

    def integrate(self, model, Y, Ya, t0, t1, dt, dt_cols):
        call = integrate_layered_heat_trbdf2 if self._layered else integrate_heat_trbdf2
        return call(model, Y, Ya, t0, t1, dt, self.abstol_e, self.reltol, dt_cols)


class LayeredHeatAdaptiveTRBDF2(HeatAdaptiveTRBDF2):
    """HeatAdaptiveTRBDF2 for a heat-only model with soil_classes (lh_integrate_layered_heat_trbdf2): every cell takes
    ρc_s and κ from its own class.  Tolerances, the Simulation's dt and the sampling of Dirichlet closures as
    HeatAdaptiveTRBDF2.  No forcing: under a BoundarySeries use LayeredHeatSeriesTRBDF2."""
    _layered = True


def _series_forcing(name, forcing):
    """The required BoundarySeries of a series marker"""
    if not isinstance(forcing, BoundarySeries):
        raise TypeError(f"{name}: forcing must be a BoundarySeries")
    return forcing


class HeatSeriesTRBDF2(HeatAdaptiveTRBDF2):
    """HeatAdaptiveTRBDF2 under a BoundarySeries (lh_integrate_heat_series): every advance is ONE library call, bitwise
    the chain of integrate_heat_trbdf2 calls over the sub-intervals between the series' knots, every column with its
    own boundary values.  forcing: the BoundarySeries (required); its values replace the model's on its
    (face, component)s, and Dirichlet closures are not sampled.  Tolerances, scope and the refresh of the prescribed
    profiles (once per saveat chunk) as HeatAdaptiveTRBDF2."""

    def __init__(self, forcing, abstol_e=0.0, reltol=0.0):
        super().__init__(abstol_e, reltol)
        self.forcing = _series_forcing(type(self).__name__, forcing)

    def integrate_forcing(self, model, Y, Ya, t0, t1, dt, dt_cols):
        return integrate_heat_series(model, Y, Ya, self.forcing, t0, t1, dt, self.abstol_e, self.reltol, dt_cols)


class LayeredHeatSeriesTRBDF2(LayeredHeatAdaptiveTRBDF2):
    """LayeredHeatAdaptiveTRBDF2 under a BoundarySeries (lh_integrate_heat_series on a model with soil_classes): as
    HeatSeriesTRBDF2, the chain being that of integrate_layered_heat_trbdf2 calls."""

    def __init__(self, forcing, abstol_e=0.0, reltol=0.0):
        super().__init__(abstol_e, reltol)
        self.forcing = _series_forcing(type(self).__name__, forcing)

    integrate_forcing = HeatSeriesTRBDF2.integrate_forcing   # (lh_integrate_heat_series picks the kernel by the map)


class CoupledImplicitEuler:
    """Backward Euler of the coupled model, SoilEnergyModel + SoilHydrologyModel without conductivity factors
    (lh_step_coupled_implicit): the water stage by ImplicitEuler's safeguarded Newton, the energy stage by one
    tridiagonal solve at the new water state -- the Jacobian is block lower-triangular, so this is exactly the
    monolithic implicit step.  Simulation runs one call per saveat chunk (per run without saveat), Dirichlet
    closures sampled at the step times.  tol / max_iter: None = the library's defaults (ImplicitEuler's)."""
    method = "euler"
    _scope, _layered, _scalar = _COUPLED, False, "lh_step_coupled_implicit"
    check_scope = _marker_scope

    def __init__(self, tol=None, max_iter=None):
        self.tol = tol
        self.max_iter = max_iter

    def step(self, model, Y, Ya, t, dt, nsteps):
        """The library call of one chunk."""
        call = step_implicit_layered_coupled if self._layered else step_implicit_coupled
        return call(model, Y, Ya, t, dt, nsteps, self.method, self.tol, self.max_iter)

    def advance(self, sim, nsteps):
        it = sim.integrator
        it.implicit_stats = self.step(sim.model, it.u, it.p, it.t, it.dt, nsteps)
        return _chunk_end(it, nsteps)


class CoupledTRBDF2(CoupledImplicitEuler):
    """Fixed-step TR-BDF2 of the coupled model (lh_step_coupled_implicit with LH_COUPLED_TRBDF2): second order,
    L-stable, two stages per step of the Simulation's dt, no error control.  Scope, calls and arguments as
    CoupledImplicitEuler."""
    method = "trbdf2"


class LayeredCoupledImplicitEuler(CoupledImplicitEuler):
    """CoupledImplicitEuler for a coupled model with soil_classes (lh_step_layered_coupled_implicit): the water stage
    by LayeredImplicitEuler's Newton, the energy stage by one tridiagonal solve with ρc_s, κ and the true conductivity
    of every cell from its own class -- still exactly the monolithic implicit step.  Calls and arguments as
    CoupledImplicitEuler."""
    _layered = True


class LayeredCoupledTRBDF2(LayeredCoupledImplicitEuler):
    """CoupledTRBDF2 for a coupled model with soil_classes (lh_step_layered_coupled_implicit with LH_COUPLED_TRBDF2)."""
    method = "trbdf2"


class CoupledFactorsImplicitEuler(CoupledImplicitEuler):
    """CoupledImplicitEuler for a coupled model whose hydrology has the IceImpedance factor and no viscosity factor
    (lh_step_coupled_factors_implicit): the water stage by FactorsImplicitEuler's Newton, the energy stage by one
    tridiagonal solve whose advected energy carries the same K -- θ_i is constant and no closure of the water reads T,
    so this is still exactly the monolithic implicit step.  A model with soil_classes, a viscosity factor, a model
    without the impedance factor (CoupledImplicitEuler serves it) and a prescribed-atmosphere top are refused.  Calls
    and arguments as CoupledImplicitEuler."""
    _scope = _COUPLED_FACTORS

    def step(self, model, Y, Ya, t, dt, nsteps):
        return step_implicit_coupled_factors(model, Y, Ya, t, dt, nsteps, self.method, self.tol, self.max_iter)


class CoupledFactorsTRBDF2(CoupledFactorsImplicitEuler):
    """CoupledTRBDF2 for a coupled model with the IceImpedance factor (lh_step_coupled_factors_implicit with
    LH_COUPLED_TRBDF2); scope as CoupledFactorsImplicitEuler."""
    method = "trbdf2"


class CoupledAdaptiveTRBDF2:
    """TR-BDF2 of the coupled model with per-column error control over both components
    (lh_integrate_coupled_trbdf2): CoupledTRBDF2's stages, TRBDF2's controller.  abstol (on ϑ_l), abstol_e (on
    ρe_int) and reltol: None = the library's defaults (1e-6, 1e-6 ρ_l c_l, 1e-3), each on its own.  The Simulation's
    dt is the initial step and the interval at which Dirichlet closures are sampled, as for TRBDF2.  Scope as
    CoupledImplicitEuler.  forcing: None or a BoundarySeries, as TRBDF2's."""
    _scope, _layered, _scalar = _COUPLED, False, "lh_integrate_coupled_trbdf2"
    check_scope = _marker_scope

    def __init__(self, abstol=None, abstol_e=None, reltol=None, forcing=None):
        self.abstol = abstol
        self.abstol_e = abstol_e
        self.reltol = reltol
        self.forcing = forcing

    def advance(self, sim, nsteps):
        return _advance_trbdf2(sim, _chunk_end(sim.integrator, nsteps))

    def integrate(self, model, Y, Ya, t0, t1, dt, dt_cols):
        call = integrate_layered_coupled_trbdf2 if self._layered else integrate_coupled_trbdf2
        return call(model, Y, Ya, t0, t1, dt, self.abstol, self.abstol_e, self.reltol, dt_cols)

    def integrate_forcing(self, model, Y, Ya, t0, t1, dt, dt_cols):
        return integrate_series(model, Y, Ya, self.forcing, t0, t1, dt, self.abstol, self.abstol_e, self.reltol, True, dt_cols)


class LayeredCoupledAdaptiveTRBDF2(CoupledAdaptiveTRBDF2):
    """CoupledAdaptiveTRBDF2 for a coupled model with soil_classes (lh_integrate_layered_coupled_trbdf2):
    LayeredCoupledTRBDF2's stages with every cell's own class under the same per-column controller and error norm over
    both components.  Tolerances, the Simulation's dt and the sampling of Dirichlet closures as CoupledAdaptiveTRBDF2.
    No forcing: under a BoundarySeries use LayeredCoupledSeriesTRBDF2."""
    _layered = True

    def __init__(self, abstol=None, abstol_e=None, reltol=None):
        super().__init__(abstol, abstol_e, reltol)


class LayeredCoupledSeriesTRBDF2(LayeredCoupledAdaptiveTRBDF2):
    """LayeredCoupledAdaptiveTRBDF2 under a BoundarySeries (lh_integrate_layered_coupled_series): every advance is ONE
    library call, bitwise the chain of integrate_layered_coupled_trbdf2 calls over the sub-intervals between the series'
    knots.  forcing: the BoundarySeries (required), as HeatSeriesTRBDF2's.  Tolerances and scope as
    LayeredCoupledAdaptiveTRBDF2.  check_scope is the parent's, so a model without soil_classes is pointed to
    lh_integrate_coupled_trbdf2 when the Simulation is built; under a forcing the call that serves such a model is
    integrate_series (CoupledAdaptiveTRBDF2(forcing=...)), which is what integrate_layered_coupled_series and the library
    name."""

    def __init__(self, forcing, abstol=None, abstol_e=None, reltol=None):
        super().__init__(abstol, abstol_e, reltol)
        self.forcing = _series_forcing(type(self).__name__, forcing)

    def integrate_forcing(self, model, Y, Ya, t0, t1, dt, dt_cols):
        return integrate_layered_coupled_series(model, Y, Ya, self.forcing, t0, t1, dt, self.abstol, self.abstol_e,
                                                self.reltol, dt_cols)


@dataclass(frozen=True)
class _FixedStep:
    """What differs between the fixed-step entry points; _step_fixed is their one body."""
    symbol: str            # the library call
    scope: tuple           # _check_scope's arguments after the model: the name in the refusals, the family, layered, scalar
    flag: Optional[int]    # the flag of method "trbdf2"; None: no `method`, backward Euler with boundary values at t_{n+1}
    newton: bool           # tol / max_iter are passed and lh_implicit_stats is returned


_STEP_IMPLICIT = _FixedStep("lh_step_implicit_euler", ("ImplicitEuler", _RICHARDS), None, True)
_STEP_IMPLICIT_LAYERED = _FixedStep("lh_step_layered_implicit_euler", ("LayeredImplicitEuler", _RICHARDS, True), None, True)
_STEP_IMPLICIT_FACTORS = _FixedStep("lh_step_factors_implicit_euler", ("FactorsImplicitEuler", _RICHARDS_FACTORS), None, True)
_STEP_HEAT = _FixedStep("lh_step_heat_implicit", ("step_implicit_heat", _HEAT_FIXED), F.LH_HEAT_TRBDF2, False)
_STEP_HEAT_LAYERED = _FixedStep("lh_step_layered_heat_implicit", ("step_implicit_layered_heat", _HEAT_FIXED, True),
                                F.LH_HEAT_TRBDF2, False)
_STEP_COUPLED = _FixedStep("lh_step_coupled_implicit", ("step_implicit_coupled", _COUPLED), F.LH_COUPLED_TRBDF2, True)
_STEP_COUPLED_LAYERED = _FixedStep("lh_step_layered_coupled_implicit",
                                   ("step_implicit_layered_coupled", _COUPLED, True, "lh_step_coupled_implicit"),
                                   F.LH_COUPLED_TRBDF2, True)
_STEP_COUPLED_FACTORS = _FixedStep("lh_step_coupled_factors_implicit", ("step_implicit_coupled_factors", _COUPLED_FACTORS),
                                   F.LH_COUPLED_TRBDF2, True)


def _step_fixed(fl, model, Y, Ya, t, dt, nsteps, method=None, tol=None, max_iter=None):
    """One fixed-step library call: the method's name, the scope, the boundary values at the step times, set_bcs, the
    call, and the Newton statistics where the family has a Newton."""
    if fl.flag is not None and method not in ("euler", "trbdf2"):
        raise ValueError(f'{fl.scope[0]}: method must be "euler" or "trbdf2"')
    _check_scope(model, *fl.scope)
    be = model._backend()
    L = F.lib()
    ya = _handle(Ya)
    if fl.flag is None:
        times = [t + (k + 1) * dt for k in range(int(nsteps))]   # t_{n+1} of every step
    else:
        times = [t + k * dt for k in range(int(nsteps) + 1)]     # the nsteps + 1 step times
    bcv = _sampled_bcv(model, times, t)
    be.set_bcs(model, t)
    flag = () if fl.flag is None else (fl.flag if method == "trbdf2" else 0,)
    newton = (float(tol or 0.0), int(max_iter or 0)) if fl.newton else ()
    F.check(getattr(L, fl.symbol)(be.ctx, Y.handle, ya, float(t), float(dt), int(nsteps), *flag, _dptr(bcv), *newton), be.ctx)
    if not fl.newton:
        return None
    mi, un = C.c_int32(), C.c_int64()
    F.check(L.lh_implicit_stats(be.ctx, C.byref(mi), C.byref(un)), be.ctx)
    return int(mi.value), int(un.value)


def step_implicit_coupled(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0,
                          nsteps: int = 1, method: str = "euler", tol=None, max_iter=None):
    """Build extension: `nsteps` implicit steps of the coupled model in one library call
    (lh_step_coupled_implicit), method "euler" (backward Euler) or "trbdf2" (fixed-step TR-BDF2).
    Time-dependent Dirichlet closures of both components are sampled at the nsteps + 1 step times t + k dt
    (per-column values at `t`).  Returns (largest Newton iteration count of any water stage, number of
    column-stages that did not converge)."""
    return _step_fixed(_STEP_COUPLED, model, Y, Ya, t, dt, nsteps, method, tol, max_iter)


def step_implicit_layered_coupled(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0,
                                  nsteps: int = 1, method: str = "euler", tol=None, max_iter=None):
    """Build extension: step_implicit_coupled for a coupled model with soil_classes
    (lh_step_layered_coupled_implicit); arguments, sampling of the boundary values and the result as
    step_implicit_coupled."""
    return _step_fixed(_STEP_COUPLED_LAYERED, model, Y, Ya, t, dt, nsteps, method, tol, max_iter)


def step_implicit_coupled_factors(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0,
                                  nsteps: int = 1, method: str = "euler", tol=None, max_iter=None):
    """Build extension: step_implicit_coupled for a coupled model whose hydrology has the IceImpedance factor and no
    viscosity factor (lh_step_coupled_factors_implicit); arguments, sampling of the boundary values and the result as
    step_implicit_coupled."""
    return _step_fixed(_STEP_COUPLED_FACTORS, model, Y, Ya, t, dt, nsteps, method, tol, max_iter)


def _sampled_bcv(model, times, base_t):
    """Boundary values of the scalar closures at `times` (any shape; the caller writes the times with its
    own expression, so that the bits the library receives are the caller's): an array of shape
    np.shape(times) + (2, 2), [..., face, component], or None when no boundary condition is a Dirichlet
    closure (nothing depends on time).  Every entry first takes its scalar value at `base_t`; a scalar
    Dirichlet value is then that of its own time.  A flux value is a constant of the model (`bc.flux`), so
    sampling every kind at every time gives the same numbers.  Per-column values stay 0 here: they reach
    the library through set_bcs."""
    if not _time_dependent(model):
        return None
    times = np.asarray(times)
    vals = np.zeros(times.shape + (2, 2))
    base = (Ellipsis,)   # the pass that fills every time with the values at base_t
    for k, t in [(base, base_t)] + [(k, times[k]) for k in np.ndindex(times.shape)]:
        for (f, c), (kind, v) in _bc_values(model, t).items():
            if np.ndim(v) == 0 and (k is base or kind == F.LH_BC_DIRICHLET):
                vals[k + (f, c)] = float(v)
    return vals


def step_implicit_heat(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0,
                       nsteps: int = 1, method: str = "euler"):
    """Build extension: `nsteps` implicit steps of the heat-only model in one library call
    (lh_step_heat_implicit), method "euler" (backward Euler) or "trbdf2" (fixed-step TR-BDF2).  Every
    stage is one exact tridiagonal solve; the matrix is factored once per call.  Time-dependent Dirichlet
    energy closures are sampled at the nsteps + 1 step times t + k dt (per-column values at `t`).  The
    prescribed ϑ_l and θ_i are those `Ya` holds: they are held at these values through the call."""
    return _step_fixed(_STEP_HEAT, model, Y, Ya, t, dt, nsteps, method)


def step_implicit_layered_heat(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0,
                               nsteps: int = 1, method: str = "euler"):
    """Build extension: step_implicit_heat for a heat-only model with soil_classes
    (lh_step_layered_heat_implicit); arguments and sampling of the boundary values as step_implicit_heat."""
    return _step_fixed(_STEP_HEAT_LAYERED, model, Y, Ya, t, dt, nsteps, method)


def step_implicit(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0, nsteps: int = 1,
                  tol=None, max_iter=None):
    """Build extension: `nsteps` backward-Euler steps of `Y` (lh_step_implicit_euler): per step Newton on
    Y - Yn - dt f(Y) = 0 with f exactly make_rhs's tendency.  Time-dependent Dirichlet closures are
    evaluated at t_{n+1} of every step (per-column values at `t`).  Returns
    (largest Newton iteration count of any column-step, number of column-steps that did not converge)."""
    return _step_fixed(_STEP_IMPLICIT, model, Y, Ya, t, dt, nsteps, None, tol, max_iter)


def step_implicit_layered(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0, nsteps: int = 1,
                          tol=None, max_iter=None):
    """Build extension: step_implicit for a Richards model with soil_classes (lh_step_layered_implicit_euler);
    arguments and return value as step_implicit."""
    return _step_fixed(_STEP_IMPLICIT_LAYERED, model, Y, Ya, t, dt, nsteps, None, tol, max_iter)


def step_implicit_factors(model: SoilModel, Y: "FieldVector", Ya=None, t: float = 0.0, dt: float = 1.0, nsteps: int = 1,
                          tol=None, max_iter=None):
    """Build extension: step_implicit for a Richards model with a conductivity factor other than NoEffect
    (lh_step_factors_implicit_euler); arguments and return value as step_implicit.  The prescribed T is the one `Ya`
    holds: it is held at these values through the call."""
    return _step_fixed(_STEP_IMPLICIT_FACTORS, model, Y, Ya, t, dt, nsteps, None, tol, max_iter)


TRBDF2_ABSTOL, TRBDF2_RELTOL = 1e-6, 1e-3   # OrdinaryDiffEq's defaults (the library's for a 0)


def _trbdf2_tolerances(abstol, reltol):
    """(abstol, reltol) with each None replaced by its own default; negative or non-finite values are
    passed on for the library to refuse (LH_EINVAL)."""
    return (TRBDF2_ABSTOL if abstol is None else float(abstol),
            TRBDF2_RELTOL if reltol is None else float(reltol))


def _tolerance_args(convention, abstol, abstol_e, reltol):
    """The tolerance arguments of an adaptive library call under its convention for a None: "richards" (abstol, reltol)
    and "coupled" (abstol, abstol_e, reltol) give abstol and reltol OrdinaryDiffEq's defaults (_trbdf2_tolerances) and
    abstol_e 0.0, for the library its 1e-6 rho_l c_l of the earth parameters; "heat" (abstol_e, reltol) gives both 0.0,
    the library's own defaults, each on its own."""
    if convention != "heat":
        abstol, reltol = _trbdf2_tolerances(abstol, reltol)
    if convention == "richards":
        return abstol, reltol
    abstol_e = 0.0 if abstol_e is None else float(abstol_e)
    if convention == "coupled":
        return abstol, abstol_e, reltol
    return abstol_e, 0.0 if reltol is None else float(reltol)


@dataclass(frozen=True)
class _Adaptive:
    """What differs between the adaptive TR-BDF2 entry points; _integrate is their one body."""
    symbol: str                    # the library call (without "lh_": the function, in its own messages)
    tolerances: str                # _tolerance_args' convention
    scope: Optional[tuple] = None  # _check_scope's arguments after the model; None: the library's own refusals only
    series: Optional[str] = None   # a BoundarySeries is "required" or "optional"; None: closures sampled at t0 and t1


_INTEGRATE = _Adaptive("lh_integrate_trbdf2", "richards", ("TRBDF2", _RICHARDS))
_INTEGRATE_LAYERED = _Adaptive("lh_integrate_layered_trbdf2", "richards", ("LayeredTRBDF2", _RICHARDS, True))
_INTEGRATE_FACTORS = _Adaptive("lh_integrate_factors_trbdf2", "richards", ("FactorsTRBDF2", _RICHARDS_FACTORS))
_INTEGRATE_COUPLED = _Adaptive("lh_integrate_coupled_trbdf2", "coupled", ("CoupledAdaptiveTRBDF2", _COUPLED))
_INTEGRATE_COUPLED_LAYERED = _Adaptive("lh_integrate_layered_coupled_trbdf2", "coupled",
                                       ("LayeredCoupledAdaptiveTRBDF2", _COUPLED, True, "lh_integrate_coupled_trbdf2"))
_INTEGRATE_HEAT = _Adaptive("lh_integrate_heat_trbdf2", "heat", ("HeatAdaptiveTRBDF2", _HEAT_ADAPTIVE))
_INTEGRATE_HEAT_LAYERED = _Adaptive("lh_integrate_layered_heat_trbdf2", "heat", ("LayeredHeatAdaptiveTRBDF2", _HEAT_ADAPTIVE, True))
_INTEGRATE_SERIES = _Adaptive("lh_integrate_series", "coupled", None, "required")
_INTEGRATE_DENSE = _Adaptive("lh_integrate_dense", "coupled", None, "optional")
# (lh_integrate_heat_series picks the kernel by the class map, and refuses in the words of the call it chains)
_INTEGRATE_HEAT_SERIES = _Adaptive("lh_integrate_heat_series", "heat", ("HeatSeriesTRBDF2", _HEAT_ADAPTIVE), "required")
_INTEGRATE_HEAT_SERIES_LAYERED = _Adaptive("lh_integrate_heat_series", "heat",
                                           ("LayeredHeatSeriesTRBDF2", _HEAT_ADAPTIVE, True), "required")
_INTEGRATE_COUPLED_SERIES_LAYERED = _Adaptive("lh_integrate_layered_coupled_series", "coupled",
                                              ("LayeredCoupledSeriesTRBDF2", _COUPLED, True, "lh_integrate_series"), "required")
# (the dense twins of the three above: their scope checks, the series optional)
_INTEGRATE_HEAT_DENSE = _Adaptive("lh_integrate_heat_dense", "heat", _INTEGRATE_HEAT_SERIES.scope, "optional")
_INTEGRATE_HEAT_DENSE_LAYERED = _Adaptive("lh_integrate_heat_dense", "heat", _INTEGRATE_HEAT_SERIES_LAYERED.scope, "optional")
_INTEGRATE_COUPLED_DENSE_LAYERED = _Adaptive("lh_integrate_layered_coupled_dense", "coupled",
                                             ("LayeredCoupledSeriesTRBDF2", _COUPLED, True, "lh_integrate_dense"), "optional")


def _integrate(fl, model, Y, Ya, t0, t1, dt, abstol=None, abstol_e=None, reltol=None, adaptive=True, dt_cols=None,
               series=None, saves=None):
    """One adaptive library call, in this order: the series and its span, the scope, the backend, set_bcs at t0 (after
    the closures are sampled at t0 and t1 where there is no series), the series' handle, the per-column step buffer,
    the tolerances, the flags, the call, lh_trbdf2_stats.  `saves`: integrate_dense's checked save times; the result
    is then (statistics, one state like Y per save time)."""
    if fl.series and not (isinstance(series, BoundarySeries) or (series is None and fl.series == "optional")):
        raise TypeError(f"{fl.symbol[3:]}: series must be a BoundarySeries" + (" or None" if fl.series == "optional" else ""))
    if series is not None:
        series._check_span(t0, t1)
    if fl.scope is not None:
        _check_scope(model, *fl.scope)
    be = model._backend()
    ya = _handle(Ya)
    bcv = () if fl.series else (_dptr(_sampled_bcv(model, (t0, t1), t0)),)
    be.set_bcs(model, t0)
    h = () if not fl.series else (None if series is None else series._device(model),)
    ptr = _dt_cols_pointer(model, dt_cols)
    tolerances = _tolerance_args(fl.tolerances, abstol, abstol_e, reltol)
    flags = 0 if adaptive else F.LH_TRBDF2_FIXED
    dense = ()
    if saves is not None:
        snaps = [Y.similar() for _ in range(saves.size)]
        handles = (C.c_void_p * max(saves.size, 1))(*[sn.handle.value for sn in snaps])
        dense = (int(saves.size), _dptr(saves) if saves.size else None, handles if saves.size else None)
    F.check(getattr(F.lib(), fl.symbol)(be.ctx, Y.handle, ya, *h, float(t0), float(t1), float(dt), *tolerances, flags, ptr,
                                        *bcv, *dense), be.ctx)
    st = _trbdf2_stats(be)
    return st if saves is None else (st, snaps)


def integrate_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                     dt: float = 1.0, abstol=None, reltol=None, adaptive=True, dt_cols=None):
    """Build extension: TR-BDF2 of `Y` from t0 to t1 in one library call (lh_integrate_trbdf2), every
    column with its own step.  `dt`: the initial step (adaptive) or the step (adaptive=False).
    Time-dependent Dirichlet closures are evaluated at t0 and t1 and interpolated linearly in between
    (per-column values at t0).  abstol / reltol: None = 1e-6 / 1e-3, each on its own.  `dt_cols`: None or a
    device tensor of ncols steps in the model's FT, read as the initial steps (<= 0: dt) and overwritten by
    the next proposals (0: failed column); with adaptive=False it is not read and receives dt.
    Returns lh_trbdf2_stats as a dict."""
    return _integrate(_INTEGRATE, model, Y, Ya, t0, t1, dt, abstol, None, reltol, adaptive, dt_cols)


def integrate_layered_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                             dt: float = 1.0, abstol=None, reltol=None, adaptive=True, dt_cols=None):
    """Build extension: integrate_trbdf2 for a Richards model with soil_classes (lh_integrate_layered_trbdf2);
    arguments and return value as integrate_trbdf2."""
    return _integrate(_INTEGRATE_LAYERED, model, Y, Ya, t0, t1, dt, abstol, None, reltol, adaptive, dt_cols)


def integrate_factors_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                             dt: float = 1.0, abstol=None, reltol=None, adaptive=True, dt_cols=None):
    """Build extension: integrate_trbdf2 for a Richards model with a conductivity factor other than NoEffect
    (lh_integrate_factors_trbdf2); arguments and return value as integrate_trbdf2.  The prescribed T is the one `Ya`
    holds: it is held at these values through the call."""
    return _integrate(_INTEGRATE_FACTORS, model, Y, Ya, t0, t1, dt, abstol, None, reltol, adaptive, dt_cols)


def _dt_cols_pointer(model, dt_cols):
    """The device pointer of a per-column step buffer (None: NULL), checked against the model."""
    if dt_cols is None:
        return None
    import torch
    if dt_cols.dtype != _torch_ft_device(model)[0] or not dt_cols.is_cuda or dt_cols.numel() != model.domain.ncolumns \
            or not dt_cols.is_contiguous():
        raise ValueError("dt_cols must be a contiguous device tensor of ncolumns values in the model's FT")
    torch.cuda.synchronize(dt_cols.device)   # (written on torch's stream, read on the library's)
    return C.c_void_p(dt_cols.data_ptr())


_TRBDF2_STATS = ("accepted", "rejected", "newton_iterations", "max_steps", "failed", "wave_steps", "unconverged")


def _trbdf2_stats(be):
    st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
    F.check(F.lib().lh_trbdf2_stats(be.ctx, st), be.ctx)
    return dict(zip(_TRBDF2_STATS, (int(x) for x in st)))


def integrate_coupled_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                             dt: float = 1.0, abstol=None, abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: TR-BDF2 of the coupled model's `Y` from t0 to t1 in one library call
    (lh_integrate_coupled_trbdf2), every column with its own error-controlled step over ϑ_l and ρe_int.  `dt`: the
    initial step.  Time-dependent Dirichlet closures of both components are evaluated at t0 and t1 and
    interpolated linearly in between (per-column values at t0).  abstol / abstol_e / reltol: None = 1e-6 /
    1e-6 ρ_l c_l / 1e-3, each on its own.  `dt_cols` as integrate_trbdf2.  Returns lh_trbdf2_stats as a dict
    (unconverged stays 0)."""
    return _integrate(_INTEGRATE_COUPLED, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, True, dt_cols)


def integrate_layered_coupled_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                                     dt: float = 1.0, abstol=None, abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: integrate_coupled_trbdf2 for a coupled model with soil_classes
    (lh_integrate_layered_coupled_trbdf2); arguments, sampling of the boundary values and the result as
    integrate_coupled_trbdf2."""
    return _integrate(_INTEGRATE_COUPLED_LAYERED, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, True, dt_cols)


def integrate_heat_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                          dt: float = 1.0, abstol_e=0.0, reltol=0.0, dt_cols=None):
    """Build extension: TR-BDF2 of the heat-only model's `Y` from t0 to t1 in one library call
    (lh_integrate_heat_trbdf2), every column with its own error-controlled step over ρe_int.  `dt`: the initial step.
    Time-dependent Dirichlet closures are evaluated at t0 and t1 and interpolated linearly in between (per-column
    values at t0).  abstol_e / reltol: 0.0 (or None) = 1e-6 ρ_l c_l / 1e-3, each on its own.  `dt_cols` as
    integrate_trbdf2.  The prescribed ϑ_l and θ_i are those `Ya` holds.  Returns lh_trbdf2_stats as a dict
    (newton_iterations and unconverged stay 0)."""
    return _integrate(_INTEGRATE_HEAT, model, Y, Ya, t0, t1, dt, None, abstol_e, reltol, True, dt_cols)


def integrate_layered_heat_trbdf2(model: SoilModel, Y: "FieldVector", Ya=None, t0: float = 0.0, t1: float = 1.0,
                                  dt: float = 1.0, abstol_e=0.0, reltol=0.0, dt_cols=None):
    """Build extension: integrate_heat_trbdf2 for a heat-only model with soil_classes
    (lh_integrate_layered_heat_trbdf2); arguments, sampling of the boundary values and the result as
    integrate_heat_trbdf2."""
    return _integrate(_INTEGRATE_HEAT_LAYERED, model, Y, Ya, t0, t1, dt, None, abstol_e, reltol, True, dt_cols)


_SERIES_FACE = {"bottom": F.LH_FACE_BOTTOM, "top": F.LH_FACE_TOP, F.LH_FACE_BOTTOM: F.LH_FACE_BOTTOM,
                F.LH_FACE_TOP: F.LH_FACE_TOP}
_SERIES_COMP = {"energy": F.LH_COMP_ENERGY, "hydrology": F.LH_COMP_HYDROLOGY, F.LH_COMP_ENERGY: F.LH_COMP_ENERGY,
                F.LH_COMP_HYDROLOGY: F.LH_COMP_HYDROLOGY}


class BoundarySeries:
    """Build extension: boundary values as piecewise-linear time series, per column or for all columns
    (lh_bc_series).  BoundarySeries(times, {(face, component): values}): `times` are nknots >= 2 finite, strictly
    increasing knot times; face is "bottom" / "top" (or LH_FACE_*), component "energy" / "hydrology" (or
    LH_COMP_*); `values` has shape [nknots] (every column the same) or [nknots, ncolumns].  Validated here with
    the library's own rules (ValueError).  At t in [T_k, T_k+1] a series is v_k + (v_k+1 - v_k) ((t - T_k) /
    (T_k+1 - T_k)) in Float64, and exactly v_k on a knot; there is no extrapolation.  Values are not judged."""

    def __init__(self, times, values):
        t = np.array(times, dtype=np.float64)
        if t.ndim != 1 or t.size < 2:
            raise ValueError("BoundarySeries: need nknots >= 2 knot times")
        for k in range(t.size):
            if not np.isfinite(t[k]):
                raise ValueError(f"BoundarySeries: knot {k} is not finite")
            if k > 0 and not t[k] > t[k - 1]:
                raise ValueError(f"BoundarySeries: knot {k} is not after knot {k - 1} (the times must increase strictly)")
        self.times = t
        self.values = {}
        for key, v in dict(values).items():
            try:
                f, c = key
                fc = (_SERIES_FACE[f], _SERIES_COMP[c])
            except (TypeError, ValueError, KeyError):
                raise ValueError(f"BoundarySeries: {key!r} is not a (face, component)") from None
            if fc in self.values:
                raise ValueError(f"BoundarySeries: {key!r} is given twice")
            a = np.ascontiguousarray(v, dtype=np.float64)
            if a.ndim not in (1, 2) or a.shape[0] != t.size:
                raise ValueError(f"BoundarySeries: the values of {key!r} must have shape [nknots] or [nknots, ncolumns]")
            self.values[fc] = a

    @property
    def nknots(self):
        return self.times.size

    def breakpoints(self, t0, t1):
        """t0, every knot strictly inside (t0, t1), t1: the ends of the sub-intervals of one integrate_series call."""
        self._check_span(t0, t1)
        inner = self.times[(self.times > t0) & (self.times < t1)]
        return [float(t0)] + [float(x) for x in inner] + [float(t1)]

    def value_at(self, key, t):
        """The series of (face, component) at time t: a Float64 scalar ([nknots] values) or [ncolumns] array."""
        f, c = key
        v = self.values[(_SERIES_FACE[f], _SERIES_COMP[c])]
        T = self.times
        t = float(t)
        if not T[0] <= t <= T[-1]:
            raise ValueError(f"BoundarySeries: t = {t} is outside the knots [{T[0]}, {T[-1]}] (no extrapolation)")
        k = min(int(np.searchsorted(T, t, side="right")) - 1, T.size - 2)
        if t == T[k]:
            return v[k].copy() if v.ndim == 2 else float(v[k])
        if t == T[k + 1]:
            return v[k + 1].copy() if v.ndim == 2 else float(v[k + 1])
        s = np.float64((t - T[k]) / (T[k + 1] - T[k]))
        r = v[k] + (v[k + 1] - v[k]) * s
        return r if v.ndim == 2 else float(r)

    def _check_span(self, t0, t1):
        if t0 < self.times[0] or t1 > self.times[-1]:
            raise ValueError(f"BoundarySeries: [t0, t1] = [{t0}, {t1}] leaves the knots [{self.times[0]}, {self.times[-1]}] "
                             "(no extrapolation)")

    def _device(self, model):
        """The lh_bc_series of this series in the model's context (created and filled on first use)."""
        be = model._backend()
        made = be.__dict__.setdefault("_bc_series", {})   # id(series) -> (series, lh_bc_series): lh_destroy releases them
        if id(self) in made:
            return made[id(self)][1]
        L = F.lib()
        ncols = model.domain.ncolumns
        for fc, a in self.values.items():
            if a.ndim == 2 and a.shape[1] != ncols:
                raise ValueError("BoundarySeries: per-column values must have ncolumns entries per knot")
        h = C.c_void_p()
        F.check(L.lh_bc_series_create(be.ctx, int(self.nknots), _dptr(self.times), C.byref(h)), be.ctx)
        for (f, c), a in self.values.items():
            F.check(L.lh_bc_series_set(be.ctx, h, f, c, _dptr(a), a.strides[0] // 8, a.strides[1] // 8 if a.ndim == 2 else 0),
                    be.ctx)
        made[id(self)] = (self, h)
        return h


def integrate_series(model: SoilModel, Y: "FieldVector", Ya, series: BoundarySeries, t0: float, t1: float, dt: float,
                     abstol=None, abstol_e=None, reltol=None, adaptive=True, dt_cols=None):
    """Build extension: TR-BDF2 of `Y` from t0 to t1 under a BoundarySeries in ONE library call
    (lh_integrate_series): bitwise the chain of integrate_trbdf2 / integrate_layered_trbdf2 /
    integrate_coupled_trbdf2 calls over the sub-intervals between the series' knots, every column with its own
    boundary values and walking its own sub-intervals.  A (face, component) without a series keeps the model's
    boundary value of t0.  Tolerances, `adaptive` and `dt_cols` as those calls' (abstol_e: coupled models only;
    adaptive=False: Richards models only).  Returns lh_trbdf2_stats of the whole call as a dict."""
    return _integrate(_INTEGRATE_SERIES, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, adaptive, dt_cols, series)


def _check_saveat(saveat, t0, t1, name="integrate_dense"):
    """The save times of a dense call (`name`, in the messages) as a Float64 array: finite, strictly increasing, inside
    [t0, t1] (ValueError), with the library's own rules and before any library call."""
    s = np.array(saveat, dtype=np.float64)
    if s.ndim != 1:
        raise ValueError(f"{name}: saveat must be a sequence of times")
    if s.size > 65536:
        raise ValueError(f"{name}: at most 65536 save times")
    for k in range(s.size):
        if not np.isfinite(s[k]):
            raise ValueError(f"{name}: save time {k} is not finite")
        if k > 0 and not s[k] > s[k - 1]:
            raise ValueError(f"{name}: save time {k} is not after save time {k - 1} (saveat must increase strictly)")
        if s[k] < t0 or s[k] > t1:
            raise ValueError(f"{name}: save time {k} = {s[k]} is outside [t0, t1] = [{t0}, {t1}]")
    return np.ascontiguousarray(s)


def integrate_dense(model: SoilModel, Y: "FieldVector", Ya, t0: float, t1: float, dt: float, saveat, series=None,
                    abstol=None, abstol_e=None, reltol=None, adaptive=True, dt_cols=None):
    """Build extension: TR-BDF2 of `Y` from t0 to t1 with the state at the times `saveat` (OrdinaryDiffEq's saveat;
    lh_integrate_dense): the integration is that of integrate_series (or, with series=None, of integrate_trbdf2 /
    integrate_layered_trbdf2 / integrate_coupled_trbdf2 under the model's boundary values of t0), bitwise, whatever
    `saveat` holds -- no step is cut at a save time; each snapshot is the cubic Hermite interpolant of the accepted
    step that contains its time, evaluated on the device in the same launch.  Returns (lh_trbdf2_stats as a dict,
    [one FieldVector like Y per save time]); only ϑ_l and, on a coupled model, ρe_int of a snapshot are written."""
    s = _check_saveat(saveat, t0, t1)
    return _integrate(_INTEGRATE_DENSE, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, adaptive, dt_cols, series, s)


def integrate_heat_series(model: SoilModel, Y: "FieldVector", Ya, series: BoundarySeries, t0: float, t1: float, dt: float,
                          abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: TR-BDF2 of a heat-only model's `Y` from t0 to t1 under a BoundarySeries in ONE library call
    (lh_integrate_heat_series): bitwise the chain of integrate_heat_trbdf2 or, for a model with soil_classes,
    integrate_layered_heat_trbdf2 calls over the sub-intervals between the series' knots, every column with its own
    boundary values and walking its own sub-intervals.  A (face, component) without a series keeps the model's boundary
    value of t0.  Tolerances and `dt_cols` as those calls'; the prescribed ϑ_l and θ_i are those `Ya` holds, read anew
    in every sub-interval.  Returns lh_trbdf2_stats of the whole call as a dict."""
    fl = _INTEGRATE_HEAT_SERIES_LAYERED if getattr(model, "soil_classes", None) is not None else _INTEGRATE_HEAT_SERIES
    return _integrate(fl, model, Y, Ya, t0, t1, dt, None, abstol_e, reltol, True, dt_cols, series)


def integrate_layered_coupled_series(model: SoilModel, Y: "FieldVector", Ya, series: BoundarySeries, t0: float, t1: float,
                                     dt: float, abstol=None, abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: integrate_series for a coupled model with soil_classes (lh_integrate_layered_coupled_series):
    bitwise the chain of integrate_layered_coupled_trbdf2 calls over the sub-intervals between the series' knots.
    Arguments and the result as integrate_series' (no `adaptive`)."""
    return _integrate(_INTEGRATE_COUPLED_SERIES_LAYERED, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, True, dt_cols,
                      series)


def integrate_heat_dense(model: SoilModel, Y: "FieldVector", Ya, t0: float, t1: float, dt: float, saveat, series=None,
                         abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: integrate_dense for a heat-only model, with or without soil_classes (lh_integrate_heat_dense):
    the integration is that of integrate_heat_series (or, with series=None, of integrate_heat_trbdf2 /
    integrate_layered_heat_trbdf2 under the model's boundary values of t0), bitwise, whatever `saveat` holds; each
    snapshot is the cubic Hermite interpolant of the accepted step that contains its time.  Returns (lh_trbdf2_stats as
    a dict, [one FieldVector like Y per save time]); only ρe_int of a snapshot is written."""
    s = _check_saveat(saveat, t0, t1, "integrate_heat_dense")
    fl = _INTEGRATE_HEAT_DENSE_LAYERED if getattr(model, "soil_classes", None) is not None else _INTEGRATE_HEAT_DENSE
    return _integrate(fl, model, Y, Ya, t0, t1, dt, None, abstol_e, reltol, True, dt_cols, series, s)


def integrate_layered_coupled_dense(model: SoilModel, Y: "FieldVector", Ya, t0: float, t1: float, dt: float, saveat,
                                    series=None, abstol=None, abstol_e=None, reltol=None, dt_cols=None):
    """Build extension: integrate_dense for a coupled model with soil_classes (lh_integrate_layered_coupled_dense): the
    integration is that of integrate_layered_coupled_series (or, with series=None, of integrate_layered_coupled_trbdf2
    under the model's boundary values of t0), bitwise.  Returns (lh_trbdf2_stats as a dict, [one FieldVector like Y per
    save time]); ϑ_l and ρe_int of a snapshot are written."""
    s = _check_saveat(saveat, t0, t1, "integrate_layered_coupled_dense")
    return _integrate(_INTEGRATE_COUPLED_DENSE_LAYERED, model, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, True, dt_cols,
                      series, s)


def _advance_trbdf2(sim, t1):
    """The Simulation's TR-BDF2 (TRBDF2, CoupledAdaptiveTRBDF2, HeatAdaptiveTRBDF2 and their layered forms) from it.t to t1: one library call per dt interval when Dirichlet closures
    depend on time, one for the whole interval otherwise; the per-column step proposals carry over.  With the method's
    `forcing` (a BoundarySeries): one series call for the whole interval, the method's integrate_forcing.
    Returns the time reached (t1 itself, not a sum of steps)."""
    it, m, model = sim.integrator, sim.method, sim.model
    if t1 <= it.t:
        return it.t
    if getattr(it, "_dt_cols", None) is None:
        import torch
        ft, dev = _torch_ft_device(model)
        it._dt_cols = torch.zeros(model.domain.ncolumns, dtype=ft, device=dev)
        it.trbdf2_stats = dict.fromkeys(_TRBDF2_STATS, 0)
    if getattr(m, "forcing", None) is not None:
        hook = getattr(m, "integrate_forcing", None)
        if hook is not None:
            st = hook(model, it.u, it.p, it.t, t1, it.dt, it._dt_cols)
        else:   # (a method object that has `forcing` and the tolerances only: integrate_series, as before the hook)
            st = integrate_series(model, it.u, it.p, m.forcing, it.t, t1, it.dt, m.abstol, getattr(m, "abstol_e", None), m.reltol,
                                  getattr(m, "adaptive", True), it._dt_cols)
        for k, v in st.items():
            it.trbdf2_stats[k] += v
        it.t = t1
        return it.t
    if _time_dependent(model):
        n = max(1, int(round((t1 - it.t) / it.dt)))
        ends = [it.t + (k + 1) * it.dt for k in range(n - 1)] + [t1]
    else:
        ends = [t1]
    for te in ends:
        st = m.integrate(model, it.u, it.p, it.t, te, it.dt, it._dt_cols)
        for k, v in st.items():
            it.trbdf2_stats[k] += v   # (max_steps: the sum over calls of each call's largest count)
        it.t = te
    return it.t


class _Solution:
    def __init__(self):
        self.t = []
        self.u = []


class _Integrator:
    def __init__(self, model, Y, Ya, t0, tf, dt, saveat):
        self.model, self.u, self.p = model, Y, Ya
        self.t, self.tf, self.dt = float(t0), float(tf), float(dt)
        self.t0 = float(t0)
        self.saveat = saveat
        self.sol = _Solution()
        self._nsteps_done = 0
        self._save()

    def _save(self):
        self.sol.t.append(self.t)
        self.sol.u.append({n: self.u.get(n) for n in self.u.names})


class Simulation:
    """Simulation(model, method; Y_init, dt, tspan, Ya_init, saveat, ...)
    (simulation.jl:34-73).  Stepping is lh_step_ssprk33: the whole SSPRK33 step
    runs on the device; Dirichlet closures are evaluated on the host at the stage
    times t, t+dt, t+dt/2 and passed as numbers."""

    def __init__(self, model, method, *, Y_init, dt, tspan, Ya_init, callbacks=None, saveat=None,
                 **kwargs):
        # (CoupledImplicitEuler, CoupledTRBDF2, CoupledAdaptiveTRBDF2 and HeatAdaptiveTRBDF2 are accepted too; the text
        # below is pinned word for word by tests/test_bcv_sampling.py and so does not name them)
        if not isinstance(method, (SSPRK33, ImplicitEuler, TRBDF2, HeatImplicitEuler, CoupledImplicitEuler,
                                   CoupledAdaptiveTRBDF2, HeatAdaptiveTRBDF2)):
            raise NotImplementedError("only SSPRK33, ImplicitEuler, TRBDF2, HeatImplicitEuler and HeatTRBDF2 are "
                                      "provided on the device")
        method.check_scope(model)
        self.method = method
        if Y_init is None:
            # simulation.jl:50 references an undefined variable here:
            # the reference cannot run this branch either.
            raise NameError("soil_model not defined")
        self.model = model
        self.callbacks = callbacks
        self.integrator = _Integrator(model, Y_init, Ya_init, tspan[0], tspan[1], dt, saveat)


def _time_dependent(model):
    bcs = model.boundary_conditions
    for tag in ("top", "bottom"):
        for c in ("energy", "hydrology"):
            if isinstance(getattr(getattr(bcs, tag), c), Dirichlet):
                return True
    return False


def _device_reads_aux(model, Ya) -> bool:
    """Does the device read a prescribed profile of Ya (T with a viscosity factor; the water fields of
    a heat-only model)?"""
    return bool(_aux_mask(model._backend().kind, model)) and isinstance(Ya, FieldVector)


_PROBE_STEPS = 4096   # stage times probed (and stepped) at a time: 3 closure calls per step


def _aux_constant_over(model, Ya, t, dt, nsteps) -> bool:
    """Are the prescribed profiles the DEVICE reads the same at EVERY stage time of the next `nsteps`
    steps (t + k dt, t + k dt + dt, t + k dt + dt/2)?  The reference's rhs! re-evaluates them at every
    stage time (right_hand_side.jl:37-42); the closures are opaque callables, so every one of those
    times is probed on the model's own centre coordinates -- a profile that starts to change later
    in the chunk (piecewise in t, hold-then-ramp) is seen."""
    if not _device_reads_aux(model, Ya):
        return True
    z = np.asarray(Ya.zc)
    fns = []
    if isinstance(model.energy_model, PrescribedTemperatureModel):
        fns.append(model.energy_model.T_profile)
    if isinstance(model.hydrology_model, PrescribedHydrologyModel):
        fns += [model.hydrology_model.vartheta_l_profile, model.hydrology_model.theta_i_profile]
    for f in fns:
        a0 = np.asarray(f(z, t) + 0.0 * z)
        for k in range(int(nsteps)):
            tk = t + k * dt
            for tt in ((tk,) if k else ()) + (tk + dt, tk + dt / 2):
                if not np.array_equal(a0, np.asarray(f(z, tt) + 0.0 * z)):
                    return False
    return True


def _advance_refreshing_aux(sim: Simulation, nsteps: int):
    """SSPRK33 steps for prescribed profiles that depend on time: the reference's rhs! re-evaluates
    them at EVERY stage time (update_aux_en!/update_aux_hydr!, right_hand_side.jl:37-42), so each
    stage is its own launch (lh_ssprk33_stage) with Ya refreshed in between.  Returns the time reached:
    the sum of the steps, one dt at a time."""
    it, model = sim.integrator, sim.model
    be = model._backend()
    L = F.lib()
    update_en = make_update_aux(model.energy_model)
    update_hy = make_update_aux(model.hydrology_model)
    if getattr(it, "_stage_state", None) is None:
        it._stage_state = it.u.similar()
    U = it._stage_state
    t = it.t
    for _ in range(nsteps):
        stage_times = (t, t + it.dt, t + it.dt / 2)
        # (without a Dirichlet closure: NULL, the values set_bcs has just set -- the same numbers)
        vals = _sampled_bcv(model, stage_times, t)
        for stage, ts in enumerate(stage_times, 1):
            update_en(it.p, ts)
            update_hy(it.p, ts)
            be.set_bcs(model, ts)       # kinds and per-column values
            F.check(L.lh_ssprk33_stage(be.ctx, stage, it.u.handle, U.handle, it.p.handle, it.dt,
                                       _dptr(None if vals is None else vals[stage - 1])), be.ctx)
        t = t + it.dt
    return t


def _stage_times(t, dt, nsteps):
    """[nsteps][3]: the stage times t_k, t_k + dt, t_k + dt/2 of SSPRK33 steps from t_k = (t + dt arange)[k]."""
    return (t + dt * np.arange(nsteps))[:, None] + np.array((0.0, dt, dt / 2))


def _advance_ssprk33(sim: Simulation, nsteps: int):
    """lh_step_ssprk33 over `nsteps` steps, Dirichlet closures sampled at the three stage times of each.
    Returns the time reached."""
    it = sim.integrator
    model = sim.model
    be = model._backend()
    L = F.lib()
    ya = _handle(it.p)
    if _device_reads_aux(model, it.p):
        # prescribed profiles on the device: every stage time of the chunk is probed; only a chunk
        # over which they do not change runs with Ya frozen (the persistent stepper), any other
        # refreshes Ya at every stage like the reference's rhs! does
        if nsteps > _PROBE_STEPS:
            for done in range(0, nsteps, _PROBE_STEPS):
                it.t = _advance_ssprk33(sim, min(_PROBE_STEPS, nsteps - done))
            return it.t
        if not _aux_constant_over(model, it.p, it.t, it.dt, nsteps):
            return _advance_refreshing_aux(sim, nsteps)
    if _aux_mask(be.kind, model):
        # constant-in-time profiles: still the values of THIS time (a user may have edited Ya)
        _refresh_prescribed(model, it.p, it.t)
    bcv = _sampled_bcv(model, _stage_times(it.t, it.dt, nsteps), it.t)
    be.set_bcs(model, it.t)
    if not getattr(it, "_placed", False) and _placement_tuning_wanted(model):
        it._placed = True
        F.check(L.lh_tune_placement(be.ctx, it.u.handle, ya, None, 0, 0, None, None), be.ctx)
    F.check(L.lh_step_ssprk33(be.ctx, it.u.handle, ya, it.t, it.dt, nsteps, _dptr(bcv)), be.ctx)
    return it.t + nsteps * it.dt


def _advance_ssprk33_series(sim: Simulation, nsteps: int):
    """lh_step_ssprk33_series over `nsteps` steps: the model's boundary state of the chunk's start, then one call.
    Returns the time reached."""
    it, model = sim.integrator, sim.model
    be = model._backend()
    if _device_reads_aux(model, it.p):
        for done in range(0, nsteps, _PROBE_STEPS):   # (every stage time is probed, _PROBE_STEPS steps at a time)
            if not _aux_constant_over(model, it.p, it.t + done * it.dt, it.dt, min(_PROBE_STEPS, nsteps - done)):
                raise ValueError(f"{type(sim.method).__name__}: the prescribed profiles the device reads change over the "
                                 "chunk, which SSPRK33 steps stage by stage (_advance_refreshing_aux); that path takes no "
                                 "forcing")
    if _aux_mask(be.kind, model):
        _refresh_prescribed(model, it.p, it.t)
    if not getattr(it, "_placed", False) and _placement_tuning_wanted(model):   # (once per Simulation, as _advance_ssprk33)
        it._placed = True
        be.set_bcs(model, it.t)
        F.check(F.lib().lh_tune_placement(be.ctx, it.u.handle, _handle(it.p), None, 0, 0, None, None), be.ctx)
    return step_series(model, it.u, it.p, sim.method.forcing, it.t, it.dt, nsteps)   # (set_bcs at it.t, then the call)


def _advance(sim: Simulation, nsteps: int):
    """`nsteps` intervals of dt with the Simulation's method; the step count and the time are kept here."""
    if nsteps <= 0:
        return
    it = sim.integrator
    t = sim.method.advance(sim, nsteps)
    it._nsteps_done += nsteps
    it.t = it.t + nsteps * it.dt if t is None else t


def step(sim: Simulation):
    """step!(simulation) (simulation.jl:79-80)."""
    _advance(sim, 1)
    return None


def run(sim: Simulation):
    """run!(simulation) (simulation.jl:86-87): integrate to tspan[2], saving
    every `saveat` like DiffEq's saveat."""
    it = sim.integrator
    total = int(round((it.tf - it.t) / it.dt))
    chunk = total
    if it.saveat:
        chunk = max(1, int(round(it.saveat / it.dt)))
    done = 0
    while done < total:
        n = min(chunk, total - done)
        _advance(sim, n)
        done += n
        it._save()
    return it.sol
