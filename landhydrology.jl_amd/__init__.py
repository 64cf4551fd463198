"""landhydrology.jl_amd -- MI355X-native batched soil-column tendency path behind
the LandHydrology.jl SoilModel API.

The directory name contains a dot, so it is loaded through
`__graft_entry__.load_package()` (or tests/conftest.py) under the module name
`landhydrology_jl_amd`.  Compute lives in lib/liblandhydro_hip.so (HIP, gfx950);
this package is the host-side mirror of the reference's Julia interface.
"""
from . import _ffi, case_model, parameterizations, partition, workloads
from ._ffi import LandHydroError, ModelError
from .parameterizations import *  # noqa: F401,F403
from .soil import (BoundarySeries, Column, CoupledAdaptiveTRBDF2, CoupledFactorsImplicitEuler, CoupledFactorsTRBDF2,
                   CoupledImplicitEuler, CoupledTRBDF2, Dirichlet,
                   EarthParameterSet, FactorsImplicitEuler, FactorsTRBDF2, FieldVector, Float32, Float64, FreeDrainage, HeatAdaptiveTRBDF2, HeatImplicitEuler,
                   HeatSeriesTRBDF2, HeatTRBDF2, IceImpedance, ImplicitEuler, LayeredCoupledAdaptiveTRBDF2,
                   LayeredCoupledImplicitEuler, LayeredCoupledSeriesTRBDF2, LayeredCoupledTRBDF2,
                   LayeredHeatAdaptiveTRBDF2, LayeredHeatImplicitEuler, LayeredHeatSeriesTRBDF2, LayeredHeatTRBDF2,
                   LayeredImplicitEuler, LayeredTRBDF2, NoBC, NoEffect,
                   PrescribedAtmosForcing,
                   PrescribedHydrologyModel, PrescribedTemperatureModel, Simulation, SoilColumnBC,
                   SoilClass, SoilClasses, SoilComponentBC, SoilEnergyModel, SoilHydrologyModel, SoilModel, SoilParams,
                   SoilThermal, SeriesSSPRK33, SSPRK33,
                   TemperatureDependentViscosity, TRBDF2, VerticalFlux, boundary_fluxes,
                   compute_turbulent_surface_fluxes, coordinates, default_initial_conditions,
                   initialize_states, integrate_coupled_trbdf2, integrate_dense, integrate_heat_dense, integrate_heat_series,
                   integrate_factors_trbdf2, integrate_heat_trbdf2, integrate_layered_coupled_dense, integrate_layered_coupled_series,
                   integrate_layered_coupled_trbdf2, integrate_layered_heat_trbdf2, integrate_layered_trbdf2, integrate_series, integrate_trbdf2,
                   make_function_space, make_rhs, make_update_aux, run, set_tuning, stable_dt, step, step_adaptive,
                   step_engine, step_implicit, step_series, step_series_engine,
                   step_implicit_coupled, step_implicit_coupled_factors, step_implicit_factors, step_implicit_heat, step_implicit_layered, step_implicit_layered_coupled,
                   step_implicit_layered_heat,
                   tune_placement, vanGenuchten)

__all__ = [n for n in dir() if not n.startswith("_")]
