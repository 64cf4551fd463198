/*
 * landhydro.h -- C ABI of liblandhydro_hip.so: the MI355X (gfx950) batched
 * soil-column tendency path behind LandHydrology.jl's SoilModel API.
 *
 * What it replaces.  LandHydrology.jl has no FFI; its seam is the Julia closure
 *     rhs!(dY, Y, Ya, t) -> dY
 * returned by make_rhs(model::SoilModel) (src/SoilModel/right_hand_side.jl:33-44)
 * and handed to DiffEqBase.ODEProblem (src/Simulations/simulation.jl:58-63).
 * A Julia shim builds the same closure on top of the calls
 * below with ccall.  Every entry point names the reference interface it stands
 * in for (file:line under the reference tree).
 *
 * Conventions
 *   - plain C types only; all entry points return 0 on success or a negative
 *     LH_E* code, never throw; lh_last_error() gives the message (the Julia shim
 *     turns it into error(msg), matching the reference's ArgumentError/error paths).
 *   - a context owns ncols independent columns of nlev cells on ONE device; one
 *     process per GPU (multi-GPU = block partition of columns over processes).
 *   - states are device-resident and owned by the library; host pointers passed
 *     to upload/download are borrowed for the call only.
 *   - cells are indexed bottom -> top (test/SoilModel/coupled.jl:198); host
 *     arrays are addressed a[col*col_stride + lev*lev_stride] (element strides),
 *     so both parent(field)-style level-fastest columns and column-fastest
 *     planes are accepted.
 *   - parameters cross the ABI as double and are rounded to the working type
 *     exactly where the Julia code applies FT(...).
 *   - calls enqueue on the context's HIP stream; lh_download, lh_stable_dt,
 *     lh_get_status and lh_synchronize wait for it.  A context is single-owner
 *     (one host thread at a time), like the reference closure which mutates Ya.
 */
#ifndef LANDHYDRO_H
#define LANDHYDRO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH_VERSION_MAJOR 0
#define LH_VERSION_MINOR 1

/* status codes */
enum {
    LH_OK = 0,
    LH_EINVAL = -1,    /* bad argument (ArgumentError in the reference) */
    LH_ENODEVICE = -2, /* no usable HIP device / HIP runtime failure */
    LH_ENOMEM = -3,
    LH_EMODEL = -4, /* model / boundary-condition combination with no reference method */
    LH_ESTATE = -5  /* state handle lacks a variable this call needs */
};

/* working type FT of SoilModel{FT} (src/SoilModel/models.jl:90-135) */
enum { LH_F32 = 0, LH_F64 = 1 };

/* which make_rhs method (right_hand_side.jl): :118-186, :192-263, :269-369 */
enum {
    LH_MODEL_RICHARDS = 0, /* PrescribedTemperatureModel + SoilHydrologyModel */
    LH_MODEL_HEAT = 1,     /* SoilEnergyModel + PrescribedHydrologyModel      */
    LH_MODEL_COUPLED = 2   /* SoilEnergyModel + SoilHydrologyModel            */
};

/* AbstractBC subtypes, src/SoilModel/boundary_conditions.jl:19-77 */
enum { LH_BC_NONE = 0, LH_BC_FLUX = 1, LH_BC_DIRICHLET = 2, LH_BC_FREE_DRAINAGE = 3 };
/* domain.boundary_tags, src/Domains/domain.jl:31 */
enum { LH_FACE_BOTTOM = 0, LH_FACE_TOP = 1 };
/* SoilComponentBC fields, boundary_conditions.jl:95-101 */
enum { LH_COMP_ENERGY = 0, LH_COMP_HYDROLOGY = 1 };
/* AbstractConductivityFactor, SoilWaterParameterizations.jl:38-65 */
enum { LH_FACTOR_NONE = 0, LH_FACTOR_ON = 1 };

/* variables of Y / dY / Ya (src/SoilModel/initial_conditions.jl:14-17, 85-89) */
enum {
    LH_VAR_VARTHETA_L = 0, /* augmented liquid fraction (Y.soil, or Ya.soil for HEAT) */
    LH_VAR_THETA_I = 1,    /* ice fraction                                             */
    LH_VAR_RHOE_INT = 2,   /* volumetric internal energy                               */
    LH_VAR_T = 3,          /* Ya.soil.T (RICHARDS); diagnostics: temperature           */
    LH_NVARS = 4
};
/* masks for lh_state_create */
#define LH_MASK(var) (1u << (var))
/* diagnostic states reuse the slots: 0 = K, 1 = psi, 2 = kappa, 3 = T */
enum { LH_DIAG_K = 0, LH_DIAG_PSI = 1, LH_DIAG_KAPPA = 2, LH_DIAG_T = 3 };

/* transcendental policy: FAST = the gfx950 log2/exp2 kernels of the product path;
 * LIBM = ocml pow/exp (<= 1 ulp), kept for parity debugging */
enum { LH_MATH_FAST = 0, LH_MATH_LIBM = 1 };

/* per-column parameter ids for lh_set_percol_param (BASELINE config 5) */
enum {
    LH_PC_VG_N = 0,
    LH_PC_VG_ALPHA = 1,
    LH_PC_VG_THETA_R = 2,
    LH_PC_VG_KSAT = 3,
    LH_PC_NU = 4,
    LH_PC_S_S = 5,
    LH_PC_COUNT = 6
};

typedef struct lh_ctx lh_ctx;     /* one SoilModel on one device */
typedef struct lh_state lh_state; /* one FieldVector (Y, dY or Ya) */

/* Column{FT}(zlim, nelements) (src/Domains/domain.jl:12-33) x ncols, plus the
 * SoilModel type parameters that select the method. */
typedef struct {
    int64_t ncols;  /* independent columns owned by this context (>= 1)       */
    int32_t nlev;   /* Column.nelements (>= 1)                                */
    int32_t dtype;  /* LH_F32 | LH_F64                                        */
    double zmin;    /* Column.zlim[1]; zmin < zmax (domain.jl:30)             */
    double zmax;    /* Column.zlim[2]                                         */
    int32_t model;  /* LH_MODEL_*                                             */
    int32_t device; /* HIP device ordinal; -1 = current device                */
    void* stream;   /* hipStream_t to enqueue on; NULL = library-owned stream */
} lh_config;

/* CLIMAParameters constants read by src/SoilModel/SoilHeatParameterizations.jl:12-13
 * (Planet: rho_cloud_liq, rho_cloud_ice, cp_l, cp_i, T_0, LH_f0; Microphysics: K_therm). */
typedef struct {
    double rho_liq, rho_ice, cp_l, cp_i, T_0, LH_f0, K_therm;
} lh_earth_params;

/* SoilParams{FT}, src/SoilModel/parameters.jl:11-43 (physics fields) */
typedef struct {
    double nu, S_s, nu_ss_gravel, nu_ss_om, nu_ss_quartz, rho_c_ds, kappa_solid, rho_p,
        kappa_sat_unfrozen, kappa_sat_frozen, a, b, kappa_dry_parameter;
} lh_soil_params;

/* vanGenuchten{FT}, SoilWaterParameterizations.jl:150-169 (m = 1 - 1/n is derived) */
typedef struct {
    double n, alpha, theta_r, Ksat;
} lh_vg_params;

/* One soil class of a layered soil (build extension: lh_set_soil_classes): the van Genuchten
 * parameters and the two SoilParams fields that lh_set_percol_param can vary per column. */
#define LH_MAX_SOIL_CLASSES 16
typedef struct {
    double n, alpha, theta_r, Ksat, nu, S_s;
} lh_soil_class;
/* The thermal supplement of one soil class (build extension: lh_set_soil_class_thermal): the SoilParams
 * fields a texture changes and the heat path reads.  a, b, kappa_dry_parameter, the earth parameters and
 * the conductivity factors stay scalars of the context. */
typedef struct {
    double rho_c_ds, kappa_solid, rho_p, kappa_sat_unfrozen, kappa_sat_frozen,
           nu_ss_gravel, nu_ss_om, nu_ss_quartz;
} lh_soil_class_thermal;

/* PrescribedAtmosForcing{FT} (boundary_conditions.jl:119-132: the first six fields), the
 * roughness lengths it reads from SoilParams (parameters.jl:38-41), and the CLIMAParameters
 * constants compute_turbulent_surface_fluxes (:553-620) consumes on top of lh_earth_params
 * (Planet: R_v, R_d, grav, cp_d, cp_v, LH_v0, T_triple, press_triple; SubgridScale:
 * von_karman_const).  Inputs, never kernel literals. */
typedef struct {
    double u_atm, theta_atm, z_atm, theta_scale, rho_a_sfc, q_atm;
    double z_0m, z_0s;
    double R_v, R_d, grav, cp_d, cp_v, LH_v0, T_triple, press_triple, von_karman;
} lh_atmos_forcing;

/* ---- lifetime ------------------------------------------------------------ */

/* SoilModel(FT; domain, energy_model, hydrology_model, ...) (models.jl:115-135).
 * Starts with the reference defaults: loam vanGenuchten, default SoilParams,
 * NoEffect factors, NoBC on every face/component; earth parameters must be set
 * before lh_rhs when the model has an energy component. */
int lh_create(lh_ctx** out, const lh_config* cfg);
int lh_destroy(lh_ctx* ctx);
/* message of the last failing call on ctx (ctx == NULL: last lh_create failure) */
const char* lh_last_error(const lh_ctx* ctx);
int lh_version(void);

/* ---- parameters ----------------------------------------------------------- */

int lh_set_earth_params(lh_ctx*, const lh_earth_params*);   /* SoilModel.earth_param_set */
int lh_set_soil_params(lh_ctx*, const lh_soil_params*);     /* SoilModel.soil_param_set  */
int lh_set_vg_params(lh_ctx*, const lh_vg_params*);         /* hydrology.hydraulic_model */
/* per-column override of one parameter (host array of ncols doubles); NULL
 * restores the scalar.  Build extension: the reference has one column. */
int lh_set_percol_param(lh_ctx*, int32_t param_id, const double* host_values);
/* Layered soils.  Build extension: the reference has one SoilParams and one vanGenuchten per model.
 * A soil class is the six numbers lh_set_percol_param knows; a context holds up to LH_MAX_SOIL_CLASSES.
 * nclasses = 0 removes the classes and the class map.  LH_EINVAL for nclasses outside
 * 0 .. LH_MAX_SOIL_CLASSES, for a NULL array, and for fewer classes than the map in place uses.  The call
 * drops the thermal supplement (the count may change), so it is LH_EMODEL while a map is in place on a
 * context that is not LH_MODEL_RICHARDS: remove the map first. */
int lh_set_soil_classes(lh_ctx*, int32_t nclasses, const lh_soil_class* classes);
/* The thermal supplement of the classes (build extension), one entry per class set by lh_set_soil_classes:
 * with it a class map is accepted by LH_MODEL_COUPLED and LH_MODEL_HEAT, whose heat closures then take
 * rho_c_ds, the saturated conductivities, the Kersten exponents, 1 - nu_om and k_dry (from the class's own
 * nu, rho_p, kappa_solid) per cell.  LH_EINVAL, naming both counts, when nclasses is not the number of
 * classes set, and for a NULL array with nclasses > 0.  nclasses = 0 removes the supplement (LH_EMODEL
 * while a map is in place on a model other than LH_MODEL_RICHARDS).  Values are not judged.  A Richards
 * context ignores the supplement.  What a class's constants take from the context's scalars (a,
 * kappa_dry_parameter, K_therm) follows lh_set_soil_params and lh_set_earth_params: these may be called
 * before or after the classes are set. */
int lh_set_soil_class_thermal(lh_ctx*, int32_t nclasses, const lh_soil_class_thermal* classes);
/* The class of every cell (build extension): the byte of (column, level) is
 * host_map[column * col_stride + level * lev_stride], strides in elements as in lh_upload.  NULL removes
 * the map.  LH_EMODEL when no classes are set, and for LH_MODEL_COUPLED / LH_MODEL_HEAT unless the classes
 * carry their thermal supplement (lh_set_soil_class_thermal); LH_EINVAL, naming
 * the first offending (column, level), for a byte >= nclasses.  While a map is set, lh_rhs,
 * lh_ssprk33_stage, lh_step_ssprk33 (fused stages), lh_stable_dt, lh_stable_dt_device, lh_diagnostics
 * and lh_boundary_fluxes evaluate every cell with its class's parameters; they are LH_EMODEL together
 * with a per-column parameter array, LH_MATH_LIBM or a prescribed-atmosphere top, and every other
 * tendency, stepping and tuning entry point (lh_rhs_stable_dt, lh_step_ssprk33_device_dt, the adaptive
 * SSPRK33 calls, the implicit and TR-BDF2 integrators -- lh_step_layered_implicit_euler and
 * lh_integrate_layered_trbdf2 step Richards contexts only, lh_step_layered_heat_implicit and
 * lh_integrate_layered_heat_trbdf2 are the implicit calls of a layered heat-only context,
 * lh_step_layered_coupled_implicit and
 * lh_integrate_layered_coupled_trbdf2 those of a layered coupled context --, lh_tune_placement) is
 * LH_EMODEL.  Without a map nothing changes. */
int lh_set_soil_class_map(lh_ctx*, const uint8_t* host_map, int64_t lev_stride, int64_t col_stride);
/* the number of classes set and whether a class map is in place (build extension); either may be NULL */
int lh_soil_class_info(const lh_ctx*, int32_t* nclasses, int32_t* has_map);
/* whether the classes carry their thermal supplement (build extension) */
int lh_soil_class_thermal_info(const lh_ctx*, int32_t* has_thermal);
/* SoilHydrologyModel.viscosity_factor / .impedance_factor (models.jl:28-33) */
int lh_set_conductivity_factors(lh_ctx*, int32_t viscosity_kind, double gamma, double T_ref,
                                int32_t impedance_kind, double Omega);
/* SoilColumnBC(top = SoilComponentBC(energy=, hydrology=), bottom = ...)
 * (boundary_conditions.jl:95-161).  value = VerticalFlux.flux, or
 * Dirichlet.state_value(t) evaluated by the host shim for the current time;
 * percol_values (ncols doubles) overrides value per column when not NULL. */
int lh_set_bc(lh_ctx*, int32_t face, int32_t component, int32_t kind, double value,
              const double* percol_values);
/* SoilColumnBC(top = PrescribedAtmosForcing{FT}(...), bottom = ...) (boundary_conditions.jl:
 * 119-161, 516-533): the TOP face of every column is driven by Monin-Obukhov surface fluxes
 * computed on the device from the top cell's (vartheta_l, theta_i, T) before every tendency
 * evaluation (compute_turbulent_surface_fluxes, :553-620; kernel in csrc/lh_atmos.hpp); the top
 * entries of lh_set_bc are ignored while it is set.  Only LH_MODEL_COUPLED has a method
 * (SoilEnergyModel + SoilHydrologyModel; LH_EMODEL otherwise, like the reference's MethodError),
 * and only the top face (:523-528).  forcing == NULL removes it.  percol: NULL, or [3][ncols]
 * doubles overriding u_atm, theta_atm, q_atm per column (build extension).  Where the
 * Monin-Obukhov system has no root the fluxes are NaN and bit 1 of lh_get_status is set.
 * PARITY UNPINNED beyond the reference's equilibrium invariant
 * (test/SoilModel/test_prescribed_atmos_bc.jl:75-79): SurfaceFluxes.jl / Thermodynamics.jl are
 * not part of the reference tree. */
int lh_set_atmos_forcing(lh_ctx*, const lh_atmos_forcing* forcing, const double* percol);
/* compute_turbulent_surface_fluxes.(energy, hydrology, model, vartheta_l, theta_i, T) for n
 * top-cell states given as host arrays of doubles (as test_prescribed_atmos_bc.jl:92-100 calls
 * it): heat_flux[n] and water_flux[n] (volume flux, positive upward) in doubles.  Scalar soil
 * and forcing parameters of the context; evaluated on the device.  Synchronises. */
int lh_atmos_surface_fluxes(lh_ctx*, int64_t n, const double* vartheta_l, const double* theta_i,
                            const double* T, double* heat_flux, double* water_flux);
/* 0 (default): bottom-face hydrology Dirichlet flux exactly as the reference
 * writes it (boundary_conditions.jl:395-398); 1: physically consistent sign. */
int lh_set_bottom_sign_consistent(lh_ctx*, int32_t flag);
/* LH_MATH_* (default LH_MATH_FAST; the environment variable LH_MATH=libm
 * selects LH_MATH_LIBM at lh_create) */
int lh_set_math_mode(lh_ctx*, int32_t mode);
/* launch-shape override for measurements, e.g. "block=128" (threads per
 * workgroup: 64, 128, 192 or 256); "" restores the defaults.  The environment
 * variable LH_TUNE is read the same way at lh_create.  Results do not depend
 * on it. */
int lh_set_tuning(lh_ctx*, const char* spec);

/* ---- states ---------------------------------------------------------------- */

/* Fields.FieldVector analogue.  var_mask selects the planes to allocate
 * (LH_MASK(...)); 0 = the prognostic set of the model
 * (initial_conditions.jl:85-89). */
int lh_state_create(lh_ctx*, uint32_t var_mask, lh_state** out);
int lh_state_destroy(lh_ctx*, lh_state*);
/* host -> device / device -> host for one variable, FT elements */
int lh_upload(lh_ctx*, lh_state*, int32_t var, const void* host, int64_t lev_stride,
              int64_t col_stride);
int lh_download(lh_ctx*, const lh_state*, int32_t var, void* host, int64_t lev_stride,
                int64_t col_stride);
/* one level of one variable, FT[ncols] (level 0 = bottom cell, nlev-1 = top cell):
 * what interior_values(X, face, cs) hands to a host-evaluated boundary condition
 * (boundary_conditions.jl:174-186, 516-533) -- ncols values instead of a plane */
int lh_download_level(lh_ctx*, const lh_state*, int32_t var, int32_t level, void* host);
/* A LEVEL-UNIFORM variable: host = FT[nlev], one value per level (bottom first), the same in every
 * column -- what Ya.soil.T .= T_profile.(zc, t) / theta_l_profile / theta_i_profile produce
 * (make_update_aux, right_hand_side.jl:54-81: functions of z and t only) and what an initial
 * condition f(z) gives.  nlev numbers cross PCIe instead of a plane, asynchronously (pinned staging;
 * the call does not wait).  The column kernels take a level-uniform prescribed field of Ya (T of the
 * Richards viscosity factor, vartheta_l and theta_i of the heat-only model) from LDS beside z and
 * read no plane for it (8 B per cell less on the viscosity configuration); every other use
 * (download, a prognostic variable, diagnostics, device pointers) first broadcasts the profile into
 * the plane on the device.  Results are bitwise those of uploading the broadcast plane. */
int lh_upload_profile(lh_ctx*, lh_state*, int32_t var, const void* host_nlev);
int lh_state_fill(lh_ctx*, lh_state*, int32_t var, double value);
int lh_state_copy(lh_ctx*, lh_state* dst, const lh_state* src);
/* zero-copy access: device pointer of a plane and its element strides
 * (column-fastest planes: col_stride == 1). */
int lh_state_device_ptr(lh_ctx*, const lh_state*, int32_t var, void** dptr,
                        int64_t* lev_stride, int64_t* col_stride);
/* While a plane's pointer is out, the caller may write through it at any time, so the library assumes
 * nothing about that plane: its contents are re-read at every launch (never treated as a plane of known
 * zeros, whatever lh_state_fill / lh_state_copy / lh_rhs wrote into it since), and the identically zero
 * d theta_i of a tendency state is re-stored at every lh_rhs.  lh_state_release_ptr ends that: the
 * caller promises not to write through pointers obtained before the call (var = -1: every plane of
 * the state).  Pointers stay valid addresses until the state is destroyed or moved (lh_tune_placement). */
int lh_state_release_ptr(lh_ctx*, lh_state*, int32_t var);
/* coordinates(cs) (right_hand_side.jl:7-8): cell-centre z, nlev doubles */
int lh_coordinates(const lh_ctx*, double* zc_host);

/* ---- the hot path ----------------------------------------------------------- */

/* rhs!(dY, Y, Ya, t) (right_hand_side.jl:37-42).  Ya may be NULL when the model
 * reads no auxiliary field (COUPLED; RICHARDS with NoEffect viscosity).  The
 * prescribed-profile update of make_update_aux (:54-96) is the host shim's job:
 * it uploads Ya when its closures depend on t. */
int lh_rhs(lh_ctx*, double t, const lh_state* Y, const lh_state* Ya, lh_state* dY);

/* lh_rhs plus, from the same pass over the state, this rank's stable-step bound
 * (the rule of lh_stable_dt) left in device memory (one FT value): the input of
 * the RCCL min all-reduce costs no second sweep over the columns.  With a
 * communicator attached (lh_comm_init) that all-reduce is enqueued right behind
 * the launch and the value is the global minimum.  The fused bound accumulates the
 * face diffusivities in Float32 whatever the working type (a safety estimate under
 * a Courant factor): it agrees with lh_stable_dt to 1e-6 relative, and -- a maximum
 * being exact -- does not depend on how the columns are dealt to waves or ranks. */
int lh_rhs_stable_dt(lh_ctx*, double t, const lh_state* Y, const lh_state* Ya, lh_state* dY,
                     double courant, void* dt_device_ft);

/* boundary_fluxes(X, bc::SoilComponentBC, face, model, cs, t) (boundary_conditions.jl:470-489; with a
 * PrescribedAtmosForcing at the top: :516-533) for every column: the pair (f_rhoe_int, f_vartheta_l)
 * of ONE face -- LH_FACE_BOTTOM or LH_FACE_TOP -- from the state of the cell next to it, positive in
 * +z: exactly the two SetValue fluxes the tendency launch uses (same device functions, same bits), for
 * callers that budget water and energy.  Boundary values are those of the last lh_set_bc (the host
 * shim evaluates Dirichlet closures at t first, as for lh_rhs).  f_energy / f_water: ncols doubles
 * each (either may be NULL); NaN where the component has no boundary condition (NoBC: `nothing` in
 * the reference).  Synchronises. */
int lh_boundary_fluxes(lh_ctx*, const lh_state* Y, const lh_state* Ya, double t, int32_t face,
                       double* f_energy, double* f_water);

/* centre fields K, psi, kappa, T of the same pointwise stage
 * (right_hand_side.jl:156-167, 291-314) into a 4-plane state (LH_DIAG_*) */
int lh_diagnostics(lh_ctx*, const lh_state* Y, const lh_state* Ya, lh_state* out);

/* solve(prob, SSPRK33(), dt = dt) (simulation.jl:58-87; coupled.jl:94): nsteps
 * fixed-dt steps, Y advanced in place on the device.  bc_stage_values is NULL or
 * [nsteps][3][2][2] doubles (step, stage, face, component): Dirichlet/flux
 * values at the stage times t, t+dt, t+dt/2. */
int lh_step_ssprk33(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                    int64_t nsteps, const double* bc_stage_values);

/* Which engine lh_step_ssprk33 runs a call of nsteps steps with (no counterpart in the reference;
 * for logs, benches and tests -- results do not depend on it: the engines are bitwise equal):
 * LH_ENGINE_FUSED_STAGES = three fused-stage launches per step (rhs_kernel MODE 1-3),
 * LH_ENGINE_COLUMN_STEPPER = ONE launch of the persistent column stepper for the whole call (state in
 * registers).  per_stage_boundary_values: the call would pass bc_stage_values != NULL.
 * A context with a class map (layered soils) answers LH_ENGINE_COLUMN_STEPPER only for LH_MODEL_RICHARDS with
 * up to 128 levels, no prescribed atmosphere and the tuning persist=2 (LH_TUNE / lh_set_tuning);
 * with the default tuning, for the coupled and heat-only models and above 128 levels it answers
 * LH_ENGINE_FUSED_STAGES.  The answer is what lh_step_ssprk33 does in every case.
 * Returns the engine (>= 0) or a negative LH_E* code. */
enum { LH_ENGINE_FUSED_STAGES = 0, LH_ENGINE_COLUMN_STEPPER = 1 };
int lh_step_engine(const lh_ctx*, int64_t nsteps, int32_t per_stage_boundary_values);

/* Which form of the table-driven 2^(.) the water closures of the next launch take (no counterpart in the
 * reference; for logs, benches and tests): LH_CLOSURE_INTEGER_EXPONENT = the exponent put in place by
 * integer addition, taken while every column (every soil class, while a class map is set) keeps every
 * power a normal number -- an interval test over the scalar parameters, the ranges of the per-column
 * arrays or the class table; LH_CLOSURE_LDEXP = the v_ldexp form, for clay-like ensembles (some
 * m = 1 - 1/n below about 0.07), porosity or alpha out of range, a NaN parameter, or "vgfast=0" in
 * LH_TUNE / lh_set_tuning; LH_CLOSURE_NOT_APPLICABLE = Float32, LH_MODEL_HEAT and LH_MATH_LIBM have one
 * form only (the stepping launches of an LH_MATH_LIBM context run the production math and are given the same
 * decision as without it).  It is the value the launch itself is given.  Returns the form (>= 0) or a negative LH_E* code. */
enum { LH_CLOSURE_LDEXP = 0, LH_CLOSURE_INTEGER_EXPONENT = 1, LH_CLOSURE_NOT_APPLICABLE = 2 };
int lh_closure_form(const lh_ctx*);

/* One stage of that step (OrdinaryDiffEq SSPRK33, Shu-Osher form), for hosts that must refresh
 * Ya between the stage evaluations: the reference's rhs! calls update_aux_en!/update_aux_hydr!
 * with the STAGE time at every evaluation (right_hand_side.jl:37-42, 54-81), so a prescribed
 * T_profile(z, t) / theta_l_profile(z, t) that really depends on t has to be re-evaluated by
 * the host shim and uploaded three times per step:
 *   stage 1 (time t):        U = Y + dt f(Y; Ya)
 *   stage 2 (time t + dt):   U = (3 Y + U + dt f(U; Ya)) / 4
 *   stage 3 (time t + dt/2): Y = (Y + 2 U + 2 dt f(U; Ya)) / 3
 * U: a state with the model's prognostic planes (its theta_i plane is not used: theta_i is read
 * from Y and never changes).  bc_values: NULL or [2][2] doubles (face, component) for this
 * stage.  Three calls are bitwise one lh_step_ssprk33 step with the same Ya. */
int lh_ssprk33_stage(lh_ctx*, int32_t stage, lh_state* Y, lh_state* U, const lh_state* Ya, double dt,
                     const double* bc_values);

/* Placement tuning -- no counterpart in the reference (host arrays have no such
 * effect).  The speed of the column launch on MI355X depends on where in HBM the
 * planes it streams together sit relative to each other (a few discrete rates,
 * up to ~10 % apart, reproducible for a given set of plane slots, also seen by a plain
 * device copy; cause not identified).  This call times the real launch on the
 * data in Y with the WRITTEN planes in up to max_candidates (0 = default 6) different slot
 * sets -- all written planes together, then each on its own -- and keeps the fastest:
 *   dY != NULL: the tendency launch of lh_rhs / lh_rhs_stable_dt writing dY;
 *   dY == NULL: the fused SSPRK33 stages of lh_step_ssprk33* writing the context's
 *               internal stage state (the trial stages run with dt = 0).
 * With LH_PLACE_MOVE_INPUT in flags the planes of Y are then tried in other slots
 * the same way (contents copied).  The values in Y never change; the contents of dY
 * are unspecified afterwards; device pointers obtained earlier from
 * lh_state_device_ptr for a moved state (dY; Y with LH_PLACE_MOVE_INPUT) are
 * stale.  Results of later launches do not depend on the placement.  One-off cost:
 * ~12 launches per candidate and (max_candidates-1) temporary copies of the moved
 * planes, never more than 25 % of the free device memory (LH_TUNE place_mem=PCT).
 * ms_before/ms_after (optional): launch time with the original and the
 * chosen placement.  Synchronises.  Always explicit: no other entry point tunes. */
#define LH_PLACE_MOVE_INPUT 1u
int lh_tune_placement(lh_ctx*, lh_state* Y, const lh_state* Ya, lh_state* dY, int max_candidates,
                      uint32_t flags, float* ms_before, float* ms_after);

/* One SSPRK33 step whose dt is read from DEVICE memory (one FT value, e.g. the
 * output of lh_stable_dt_device after an RCCL min all-reduce): adaptive stepping
 * across ranks without a host round trip.  bc_stage_values: NULL or [3][2][2]. */
int lh_step_ssprk33_device_dt(lh_ctx*, lh_state* Y, const lh_state* Ya, double t,
                              const void* dt_device_ft, const double* bc_stage_values);

/* nsteps ADAPTIVE SSPRK33 steps with nothing leaving the device (build-defined: the reference
 * steps with a fixed user dt, simulation.jl:34-70).  Per step, all on the context's stream:
 *   f(Y) and the stable-step bound of Y in ONE launch (as lh_rhs_stable_dt; the RCCL min over
 *   ranks follows when a communicator is attached); dt = min(bound, dt_max) (dt_max <= 0: no
 *   cap), *elapsed += dt; then stages 2 and 3 -- stage 2 takes (Y, f(Y)) and forms
 *   U1 = Y + dt f(Y) in registers, so f(Y) is evaluated once, not twice: three evaluations of f
 *   per step instead of the four of lh_rhs_stable_dt + lh_step_ssprk33_device_dt, and bitwise
 *   their result.
 * Boundary values are the constants of lh_set_bc (a time-dependent Dirichlet closure needs the
 * stage times on the host: use the per-step calls).  dt_device_ft: one FT in device memory,
 * holds the last step's dt afterwards; elapsed_device_ft: NULL or one FT in device memory that
 * accumulates the simulated time (the caller zeroes it, on a stream ordered before this call: the
 * context's own stream is non-blocking).  A step whose bound is not a positive finite number is
 * taken with dt = 0 and sets bit 2 of lh_get_status.  Does not synchronise. */
int lh_step_ssprk33_adaptive(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double courant,
                             double dt_max, int64_t nsteps, void* dt_device_ft, void* elapsed_device_ft);

/* lh_step_ssprk33_adaptive with the step size HELD for `hold` steps: nchunks chunks of `hold`
 * SSPRK33 steps each (1 <= hold <= 2^20, nchunks >= 0), nothing leaving the device.  Per chunk: the
 * stable-step bound of the current Y (the rule of lh_rhs_stable_dt; the RCCL min over ranks follows
 * when a communicator is attached -- one collective per chunk, not per step), dt formed from it
 * exactly as lh_step_ssprk33_adaptive forms it (dt_max, the dt = 0 fallback and status bit 2
 * included), then `hold` steps at that dt, and *elapsed advanced by `hold` successive += dt.
 * Every column takes the same dt sequence.  Y and the dt of every chunk are bitwise those of: copy
 * Y to Z, lh_step_ssprk33_adaptive(Z, nsteps = 1, dtbuf), then `hold` x
 * lh_step_ssprk33_device_dt(Y, dtbuf); with hold = 1 the call is bitwise
 * lh_step_ssprk33_adaptive(nsteps = nchunks).
 * Where the persistent column stepper serves the call (lh_adaptive_hold_engine) a chunk is ONE
 * launch, which also leaves the bound of the state it ends on: nchunks + 1 heavy launches instead of
 * 3 nchunks hold.  Elsewhere a chunk is the bound's launch plus `hold` x the three fused stages
 * (3 hold + 1 launches, f(Y) evaluated twice for the chunk's first step) and the call ends with
 * one more bound launch: slower than lh_step_ssprk33_adaptive at small `hold` (four launches
 * against three per step at hold = 1), level with it at large `hold`, never faster.  On
 * ensembles of more than 2^20 lanes (ncolumns x nlev rounded up to 64) the stepper serves calls of 3
 * steps and more only, so hold = 1 and hold = 2 take that path there: use hold >= 3, in practice 8
 * and more (the bound's extra closure pass and the launch are paid once per chunk).
 * hold <= 1048576 (2^20; LH_EINVAL above): *elapsed is advanced by a one-thread loop of `hold`
 * additions between two chunks.
 * Overrun flag: after every chunk (the last included) the rank-reduced bound of the state the chunk
 * ENDED on is compared with the dt the chunk used; a bound below that dt, or one that is not a
 * positive finite number, sets bit 5 (value 32) of lh_get_status: the held step exceeded the stable
 * step of the state it produced -- `hold` or `courant` is too aggressive.  The call goes on.
 * dt_device_ft holds the last chunk's dt afterwards.  Boundary values are the constants of
 * lh_set_bc.  Does not synchronise. */
int lh_step_ssprk33_adaptive_hold(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double courant,
                                  double dt_max, int64_t nchunks, int32_t hold,
                                  void* dt_device_ft, void* elapsed_device_ft);

/* Which engine lh_step_ssprk33_adaptive_hold runs the chunks of a call with (as lh_step_engine):
 * LH_ENGINE_COLUMN_STEPPER = one stepper launch per chunk, LH_ENGINE_FUSED_STAGES = 3 hold + 1
 * streamed launches per chunk (more than 128 levels, the Float64 coupled model with conductivity
 * factors on large ensembles, a prescribed atmosphere, LH_TUNE persist=0, and hold < 3 on
 * ensembles of more than 2^20 lanes).
 * Returns the engine (>= 0) or a negative LH_E* code. */
int lh_adaptive_hold_engine(const lh_ctx*, int32_t hold);

/* ---- Adaptive SSPRK33 for LAYERED Richards soils (a class map is set).
 * The scalar calls above keep refusing a context with a map; these three refuse one without
 * (LH_EMODEL, naming the scalar call), any model but Richards, columns of more than 128 levels, a
 * prescribed atmosphere, and what every layered call refuses (per-column parameter arrays,
 * LH_MATH_LIBM) -- all LH_EMODEL; NULL words, courant <= 0, nsteps < 0, nchunks < 0 and a hold outside
 * 1 ... 2^20 are LH_EINVAL.  They have ONE engine, the layered column stepper with the step in
 * device memory and the step bound as its epilogue, and do not consult LH_TUNE persist: that key
 * chooses where there are two engines.  None of them synchronises.
 *
 * lh_layered_step_bound_device: the stable-step bound of Y under `courant` into one FT in device
 * memory -- lh_stable_dt's rule (every cell's slope with its own class's n m, an interior face the sum
 * of its two true conductivities times the larger slope, a Dirichlet face half a cell away) with the
 * slopes and maxima in Float32, as lh_rhs_stable_dt accumulates its own: within 1e-6 (Float64) or
 * 2e-4 (Float32) of lh_stable_dt.  A zero-step launch of the stepper: no plane of Y is written.  The
 * RCCL min over ranks follows when a communicator is attached.  A column whose bound is NaN is left
 * out; a call no column contributes to leaves +inf. */
int lh_layered_step_bound_device(lh_ctx*, const lh_state* Y, const lh_state* Ya, double courant, void* dt_device_ft);

/* nsteps SSPRK33 steps in ONE launch at the step read from device memory (one FT, read once per
 * launch): bitwise lh_step_ssprk33 with the same step by value.  bcv: as in lh_step_ssprk33.  The
 * launch is the bound flavour of the stepper; the bound it leaves is written to a word the context
 * owns and discarded. */
int lh_step_layered_ssprk33_device_dt(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, const void* dt_device_ft,
                                      int64_t nsteps, const double* bcv);

/* lh_step_ssprk33_adaptive_hold for a layered context: nchunks chunks of `hold` steps, nothing
 * leaving the device, one collective per chunk.  The first bound comes from a zero-step launch; per
 * chunk dt is formed from the rank-reduced bound exactly as the scalar call forms it (dt_max, the
 * dt = 0 fallback with status bit 2, *elapsed advanced by `hold` successive += dt, the overrun flag
 * bit 5 for the chunk that ended), then one launch takes `hold` steps and leaves the next bound; the
 * last chunk's bound is checked as well.  Y, every chunk's dt and *elapsed are bitwise those of: per
 * chunk lh_layered_step_bound_device, dt = min(bound, dt_max), lh_step_ssprk33(Y, dt, hold) under
 * LH_TUNE persist=0.  elapsed_device_ft may be NULL.  dt_device_ft holds the last chunk's dt
 * afterwards.  Boundary values are the constants of lh_set_bc. */
int lh_step_layered_ssprk33_adaptive_hold(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double courant,
                                          double dt_max, int64_t nchunks, int32_t hold,
                                          void* dt_device_ft, void* elapsed_device_ft);

/* Backward-Euler steps of a Richards model: per step, Newton on
 * Y - Yn - dt f(Y, t+dt) = 0 with f exactly lh_rhs's tendency, one tridiagonal solve per
 * column and iteration.  bcv: NULL (current boundary values) or nsteps*4 doubles at t_{n+1}.
 * tol <= 0 / max_iter <= 0: defaults.  Asynchronous; non-convergence sets status bit 3.
 * (With a non-NULL bcv the call waits for its launch before it releases the device copy of the
 * values, as lh_step_ssprk33 does.)
 * (Build-defined: the reference hands any OrdinaryDiffEq method to DiffEqBase.init,
 * src/Simulations/simulation.jl:34-73.)  bcv is laid out [nsteps][2 faces][2 components] like one
 * stage of lh_step_ssprk33's.  A column-step converges when max_i |dY_i| <= tol max(|Y_i|, nu)
 * (defaults: tol 1e-10 in Float64, 1e-5 in Float32; max_iter 50); one that does not keeps its last
 * iterate.  Richards models only, without conductivity factors and without a prescribed
 * atmosphere: anything else is LH_EMODEL.  theta_i is constant through the step. */
int lh_step_implicit_euler(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                           int64_t nsteps, const double* bcv, double tol, int32_t max_iter);
/* Of the last lh_step_implicit_euler, lh_step_layered_implicit_euler or lh_step_coupled_implicit call
 * (the water stages of the last): the largest iteration count any column needed and the number of
 * column-steps (TR-BDF2: column-stages) that did not converge (zeros once a later call was refused).
 * Synchronises. */
int lh_implicit_stats(lh_ctx*, int32_t* max_iters, int64_t* unconverged);
/* Of the last lh_step_implicit_euler, lh_step_layered_implicit_euler or lh_step_coupled_implicit call:
 * the Newton iterations summed over all column-steps (divided by ncols * nsteps: the mean per
 * column-step).  Synchronises. */
int lh_implicit_iterations(lh_ctx*, int64_t* iterations);

/* TR-BDF2 of a Richards model from t0 to t1: L-stable, second order, two
 * stages of the form Y - w - d h f(Y) = 0 (d = (2 - sqrt 2)/2), each solved by
 * lh_step_implicit_euler's safeguarded Newton with one tridiagonal solve per iteration.  Every
 * column carries its own step h and its own accept/reject history (no collective): the error
 * estimate (I - d h J)^-1 (b1 z_n + b2 z_g + b3 z_1) of Hosea & Shampine is measured in
 * E = sqrt(mean_i (e_i / (abstol + reltol max(|Y_n,i|, |Y_1,i|)))^2); E <= 1 accepts, and
 * h <- h clamp(0.9 E^(-1/3), 0.2, 5); a stage whose Newton does not converge within 10 iterations
 * rejects the step and h <- h/4.  The last step lands on t1 exactly.  A column fails when h falls
 * below 1e-10 (t1 - t0) or after 100000 attempted steps in one call: it keeps its last accepted
 * state (at an earlier time) and sets status bit 4.
 * dt: the initial step (flags LH_TRBDF2_FIXED: the fixed step, no error control, Newton with
 * lh_step_implicit_euler's defaults; non-convergence sets status bit 3 and the step is kept).
 * abstol, reltol: each one that is 0 takes its own default, 1e-6 and 1e-3 (OrdinaryDiffEq's).
 * dt_cols_device_ft: NULL or ncols FT values in device memory: on entry each column's initial step
 * (<= 0: dt), on exit the controller's proposal for the next call, or 0 for a failed column.  With
 * LH_TRBDF2_FIXED the entries are not read (every column steps by dt) and receive dt.
 * bcv: NULL (lh_set_bc's values) or 8 doubles [t0 | t1][2 faces][2 components], interpolated
 * linearly at every stage time.  Richards models only, without conductivity factors and without a
 * prescribed atmosphere: anything else is LH_EMODEL.  Asynchronous. */
#define LH_TRBDF2_FIXED 1u
int lh_integrate_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                        double abstol, double reltol, uint32_t flags, void* dt_cols_device_ft,
                        const double* bcv);
/* Of the last lh_integrate_trbdf2, lh_integrate_layered_trbdf2, lh_integrate_coupled_trbdf2,
 * lh_integrate_layered_coupled_trbdf2, lh_integrate_heat_trbdf2, lh_integrate_layered_heat_trbdf2 or
 * lh_integrate_series, lh_integrate_heat_series or lh_integrate_layered_coupled_series call (the series
 * calls' counters over their whole interval, see there),
 * LH_TRBDF2_NSTATS counters (zeros once a later call of any of them was refused): accepted steps,
 * rejected steps, Newton iterations (summed over stages and columns), the largest number of
 * attempted steps of any column,
 * failed columns, wave_steps (the sum over waves of 64 x the wave's largest step count: what the
 * slowest lane of each wave costs) and, in fixed-step mode, unconverged stages (0 after
 * lh_integrate_coupled_trbdf2 and lh_integrate_layered_coupled_trbdf2; after the two heat-only calls,
 * which solve every stage exactly, the Newton iterations are 0 as well).  Synchronises. */
#define LH_TRBDF2_NSTATS 7
int lh_trbdf2_stats(lh_ctx*, int64_t* stats);

/* lh_step_implicit_euler and lh_integrate_trbdf2 for layered soils (a class map is set,
 * lh_set_soil_class_map): the same arguments, defaults, bcv layouts, flags,
 * statistics (lh_implicit_stats / lh_implicit_iterations, lh_trbdf2_stats) and status bits 3 and 4.
 * f is lh_rhs's tendency of the same context; the Newton Jacobian takes the two conductivities and the
 * two slopes of a face from its two cells' classes, and the safeguard (half of nu - theta_r per
 * iteration, half way to theta_r, a stop on nu - theta_i) and backward Euler's convergence test
 * max_i |dY_i| <= tol max(|Y_i|, nu) use each cell's own class.
 * LH_EMODEL, in this order: any model but LH_MODEL_RICHARDS, a context without a class map (use the
 * call without `layered`), what
 * every layered call refuses (per-column parameter arrays, LH_MATH_LIBM), conductivity factors other
 * than NoEffect, a prescribed atmosphere.  LH_EINVAL as the scalar calls.  Asynchronous. */
int lh_step_layered_implicit_euler(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                                   int64_t nsteps, const double* bcv, double tol, int32_t max_iter);
int lh_integrate_layered_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1,
                                double dt, double abstol, double reltol, uint32_t flags,
                                void* dt_cols_device_ft, const double* bcv);

/* lh_step_implicit_euler and lh_integrate_trbdf2 for a Richards context whose hydrology has a
 * conductivity factor other than NoEffect (lh_set_conductivity_factors: TemperatureDependentViscosity
 * and / or IceImpedance): the same arguments, defaults, bcv layouts, flags
 * (LH_TRBDF2_FIXED, dt_cols), statistics (lh_implicit_stats / lh_implicit_iterations, lh_trbdf2_stats),
 * scratch planes and status bits 3 and 4; status bit 0 where a Newton step is not finite (a cell with
 * theta_l + theta_i = 0 under the impedance factor has K = NaN, as in the reference).
 * f is lh_rhs's tendency of the same context, K = visc(T) imp(vartheta_l, theta_i) K_NoEffect.  T is
 * whatever Ya holds at the call (a plane, or a level-uniform profile from lh_upload_profile) and is
 * held through the call, as every stepping call holds the prescribed fields; theta_i is constant
 * through the call.  The viscosity factor is then a constant of every cell and the impedance factor a
 * function of the cell's own vartheta_l, so the Newton Jacobian stays tridiagonal:
 *   dK/dvartheta_l = visc imp dK_NoEffect/dvartheta_l + K Omega ln10 theta_i / (theta_l + theta_i)^2,
 * the second term only where vartheta_l < nu - theta_i.  Per-column parameter arrays and LH_MATH_LIBM
 * are served as the plain calls serve them.
 * LH_EINVAL as the plain calls, checked first.  Then LH_EMODEL, in this order: any model but
 * LH_MODEL_RICHARDS, a class map, a context whose factors are both NoEffect (use the call without
 * `factors`), a prescribed atmosphere.  Boundary-value series and dense output do not take these
 * contexts.  Asynchronous. */
int lh_step_factors_implicit_euler(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                                   int64_t nsteps, const double* bcv, double tol, int32_t max_iter);
int lh_integrate_factors_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1,
                                double dt, double abstol, double reltol, uint32_t flags,
                                void* dt_cols_device_ft, const double* bcv);

/* Implicit steps of the heat-only model, SoilEnergyModel + PrescribedHydrologyModel
 * (right_hand_side.jl:192-263).  With vartheta_l and theta_i prescribed the
 * tendency is affine in rhoe_int, so a stage Y - w - c f(Y) = 0 is one tridiagonal solve, exact up to
 * round-off: no Newton iteration, no tolerance, no convergence flag.  The matrix is factored once
 * per call; a step is one forward and one back substitution (flags 0: backward Euler,
 * Y - Yn - dt f(Y, t+dt) = 0) or two of each (LH_HEAT_TRBDF2: fixed-step TR-BDF2, second order and
 * L-stable, gamma = 2 - sqrt 2, the stages at t + gamma dt and t + dt).  Fixed step: no error control.
 * (Build-defined: the reference hands any OrdinaryDiffEq method to DiffEqBase.init,
 * src/Simulations/simulation.jl:34-73.)
 * bcv: NULL (lh_set_bc's values, per-column arrays included) or (nsteps + 1) * 4 doubles
 * [nsteps + 1][2 faces][2 components] at t + k dt, k = 0 .. nsteps; the hydrology entries are
 * ignored.  Backward Euler takes sample k + 1 for step k; TR-BDF2 takes (1 - gamma) v_k + gamma v_k+1
 * for its first stage, v_k+1 for its second and v_k for the tendency at the start of the step.
 * The prescribed vartheta_l and theta_i of Ya are read once per call and held through it.
 * A non-finite result sets status bit 0.  LH_EMODEL for any model but LH_MODEL_HEAT; LH_EINVAL for
 * dt <= 0 or not finite, nsteps < 0 or unknown flag bits; nsteps == 0 does nothing.  Asynchronous.
 * (With a non-NULL bcv the call waits for its launch before it releases the device copy of the
 * values, as lh_step_implicit_euler does.) */
#define LH_HEAT_TRBDF2 1u
int lh_step_heat_implicit(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                          int64_t nsteps, uint32_t flags, const double* bcv);

/* lh_step_heat_implicit for layered soils (a class map with its thermal supplement is set,
 * lh_set_soil_class_thermal + lh_set_soil_class_map): the same arguments, flags
 * (0 or LH_HEAT_TRBDF2), bcv layout and sampling, status bit 0 and asynchrony.  Every cell takes beta,
 * rho_c_s and kappa from its own class; an interior face is (kappa_lo + kappa_hi) whatever the classes of
 * its two cells, a Dirichlet energy face takes kappa from the boundary cell's class: f is lh_rhs's
 * tendency of the same context, still affine in rhoe_int, so a stage stays one exact tridiagonal solve.
 * LH_EINVAL as lh_step_heat_implicit.  LH_EMODEL, in this order: any model but LH_MODEL_HEAT, a context
 * without a class map (lh_step_heat_implicit steps it), what every layered call refuses (per-column
 * parameter arrays, LH_MATH_LIBM).  nsteps == 0 does nothing. */
int lh_step_layered_heat_implicit(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                                  int64_t nsteps, uint32_t flags, const double* bcv);

/* Implicit steps of the coupled model, SoilEnergyModel + SoilHydrologyModel
 * (right_hand_side.jl:269-369).  Without conductivity factors the water
 * tendency does not read rhoe_int and the energy tendency is affine in rhoe_int at fixed vartheta_l,
 * theta_i, so the Jacobian of a stage Y - w - c f(Y) = 0 is block lower-triangular: the water stage
 * is solved by lh_step_implicit_euler's safeguarded Newton, the energy stage by one tridiagonal
 * solve at the new water state -- exactly the monolithic implicit stage, no splitting error.
 * flags 0: backward Euler, Y - Yn - dt f(Y, t+dt) = 0.  LH_COUPLED_TRBDF2: fixed-step TR-BDF2
 * (gamma = 2 - sqrt 2, both stages with the coefficient gamma/2 dt, at t + gamma dt and t + dt); no
 * error control.  (Build-defined: the reference hands any OrdinaryDiffEq method to DiffEqBase.init,
 * src/Simulations/simulation.jl:34-73.)
 * bcv: NULL (lh_set_bc's values, per-column arrays included) or (nsteps + 1) * 4 doubles
 * [nsteps + 1][2 faces][2 components] at t + k dt, k = 0 .. nsteps, both components read.  Backward
 * Euler takes sample k + 1 for step k; TR-BDF2 takes (1 - gamma) v_k + gamma v_k+1 for its first
 * stage, v_k+1 for its second and v_k for the tendency at the start of the call.
 * tol <= 0 / max_iter <= 0: lh_step_implicit_euler's defaults, and its per-column test on the
 * Newton step of the water stage.  A column-stage that does not converge keeps its last iterate,
 * sets status bit 3 and still gets its energy solve at that iterate; a non-finite result sets
 * status bit 0.  lh_implicit_stats / lh_implicit_iterations report the water stages of the call.
 * LH_EINVAL for dt <= 0 or not finite, nsteps < 0 or unknown flag bits; LH_EMODEL for any model but
 * LH_MODEL_COUPLED, for conductivity factors other than NoEffect (the water would read T) and for
 * a prescribed-atmosphere top; nsteps == 0 does nothing.  theta_i is constant through the call.
 * Asynchronous.  (With a non-NULL bcv the call waits for its launch before it releases the device
 * copy of the values, as lh_step_implicit_euler does.) */
#define LH_COUPLED_TRBDF2 1u
int lh_step_coupled_implicit(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                             int64_t nsteps, uint32_t flags, const double* bcv, double tol,
                             int32_t max_iter);

/* lh_step_coupled_implicit for layered soils (a class map with its thermal supplement is set,
 * lh_set_soil_class_thermal + lh_set_soil_class_map): the same arguments, flags
 * (0 or LH_COUPLED_TRBDF2), bcv layout and sampling, tol / max_iter defaults, status bits 0 and 3,
 * lh_implicit_stats / lh_implicit_iterations and asynchrony.  (Build-defined like that call: the
 * reference hands any OrdinaryDiffEq method to DiffEqBase.init, src/Simulations/simulation.jl:34-73.)
 * The water stage is lh_step_layered_implicit_euler's Newton with every cell's own class (vartheta_l
 * after a backward-Euler step is bitwise that call's on a Richards context with the same classes); the
 * energy stage is one tridiagonal solve at the new water state with beta, rho_c_s and kappa of every
 * cell from its own class, the interior face (kappa_lo + kappa_hi) with the advected energy carried by
 * the two cells' own true conductivities, a Dirichlet energy face with kappa from the boundary cell's
 * class: f is lh_rhs's tendency of the same context, and a stage is still solved exactly.
 * LH_EINVAL as lh_step_coupled_implicit.  LH_EMODEL, in this order: any model but LH_MODEL_COUPLED, a
 * context without a class map (lh_step_coupled_implicit steps it; that call keeps refusing a context
 * WITH a map), what every layered call refuses (a prescribed-atmosphere top, per-column parameter
 * arrays, LH_MATH_LIBM), conductivity factors other than NoEffect.  nsteps == 0 does nothing. */
int lh_step_layered_coupled_implicit(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                                     int64_t nsteps, uint32_t flags, const double* bcv, double tol,
                                     int32_t max_iter);

/* lh_step_coupled_implicit for a coupled context whose hydrology has the IceImpedance factor and no
 * viscosity factor (lh_set_conductivity_factors): the same arguments, flags
 * (0 or LH_COUPLED_TRBDF2), bcv layout and sampling, tol / max_iter defaults, status bits 0 and 3,
 * lh_implicit_stats / lh_implicit_iterations, scratch planes and asynchrony.  theta_i is constant and no
 * closure of the water reads T, so the water tendency still does not read rhoe_int and the energy
 * tendency is still affine in it: the impedance scales K, in the water's fluxes and in the advected
 * energy, and the stage Jacobian stays block lower-triangular.  The water stage is
 * lh_step_factors_implicit_euler's Newton (vartheta_l after a backward-Euler step is bitwise that call's
 * on a Richards context with the same hydrology, ice and factor); the energy stage is one tridiagonal
 * solve at the new water state, matrix and right-hand side formed with the same K: f is lh_rhs's
 * tendency of the same context.  Per-column parameter arrays and LH_MATH_LIBM are served as the plain
 * call serves them.
 * LH_EINVAL as lh_step_coupled_implicit, checked first.  Then LH_EMODEL, in this order: any model but
 * LH_MODEL_COUPLED, a class map, a viscosity factor other than NoEffect (the water then reads the unknown
 * T and the stage is no longer block triangular), a context without the impedance factor
 * (lh_step_coupled_implicit steps it), a prescribed-atmosphere top.  nsteps == 0 does nothing. */
int lh_step_coupled_factors_implicit(lh_ctx*, lh_state* Y, const lh_state* Ya, double t, double dt,
                                     int64_t nsteps, uint32_t flags, const double* bcv, double tol,
                                     int32_t max_iter);

/* TR-BDF2 of the coupled model from t0 to t1 with per-column error control:
 * lh_integrate_trbdf2's method and controller over both components, every stage solved as
 * lh_step_coupled_implicit solves it (the water by the safeguarded Newton with lh_integrate_trbdf2's
 * adaptive test, kappa 0.01 within 10 iterations; the energy by one tridiagonal solve at the new
 * vartheta_l).  The error estimate r = b1 h f_n + b2 z_g + b3 z_1 of both components is filtered by
 * the diagonal blocks of I - d h J(Y_1), (I - d h J_ww) e_w = r_w and (I - d h J_ee) e_e = r_e, and
 * measured in E = sqrt((sum_i q_w,i^2 + sum_i q_e,i^2) / (2 nlev)) with
 * q_w = e_w / (abstol + reltol max(|vartheta_l,n|, |vartheta_l,1|)) and
 * q_e = e_e / (abstol_e + reltol max(|rhoe_int,n|, |rhoe_int,1|)).  E <= 1 accepts; step changes, the
 * landing on t1, the step floor and the attempt cap are lh_integrate_trbdf2's.  A column that fails
 * keeps its last accepted vartheta_l and rhoe_int, sets status bit 4 and gets dt_cols = 0; a
 * non-finite accepted result sets status bit 0.
 * abstol, reltol: each one that is 0 takes its own default, 1e-6 and 1e-3.  abstol_e: 0 takes
 * 1e-6 rho_l c_l, the energy of 1e-6 K in water (4.18 J/m^3 with the default earth parameters);
 * rhoe_int passes through 0 at T = T_0, where a water-sized absolute tolerance would pin the step.
 * flags must be 0 (fixed steps: lh_step_coupled_implicit with LH_COUPLED_TRBDF2).  dt_cols_device_ft
 * and bcv as lh_integrate_trbdf2, both components of bcv read.  lh_trbdf2_stats reports the call.
 * LH_EINVAL for t1 < t0, dt <= 0, a negative tolerance, anything not finite, or flags != 0;
 * LH_EMODEL as lh_step_coupled_implicit.  theta_i is constant through the call.  Asynchronous. */
int lh_integrate_coupled_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                                double abstol, double abstol_e, double reltol, uint32_t flags,
                                void* dt_cols_device_ft, const double* bcv);

/* lh_integrate_coupled_trbdf2 for layered soils (a class map with its thermal supplement is set,
 * lh_set_soil_class_thermal + lh_set_soil_class_map): the same arguments,
 * tolerance defaults (abstol_e = 0 takes 1e-6 rho_l c_l), bcv layout, dt_cols in and out, error norm E
 * over both components, controller, step floor and attempt cap, lh_trbdf2_stats, status bits 0 and 4
 * and asynchrony.  Every stage is solved as lh_step_layered_coupled_implicit solves it: the water by
 * lh_integrate_layered_trbdf2's Newton with every cell's own class in the safeguard, the energy by one
 * tridiagonal solve at the new vartheta_l with beta, rho_c_s, kappa and the true conductivity of every
 * cell from its own class.  The error filters are the two diagonal blocks at Y_1 with per-cell
 * constants, the energy's the stage-2 matrix against r_e alone (Dirichlet conductances in the pivots,
 * no boundary offset).  f is lh_rhs's tendency of the same context.
 * flags must be 0 (fixed steps: lh_step_layered_coupled_implicit with LH_COUPLED_TRBDF2).
 * LH_EINVAL as lh_integrate_coupled_trbdf2, checked first.  LH_EMODEL, in this order: any model but
 * LH_MODEL_COUPLED, a context without a class map (lh_integrate_coupled_trbdf2 integrates it; that
 * call keeps refusing a context WITH a map), what every layered call refuses (a prescribed-atmosphere
 * top, per-column parameter arrays, LH_MATH_LIBM), conductivity factors other than NoEffect.  A
 * refused call leaves the statistics zeroed; t1 == t0 does nothing. */
int lh_integrate_layered_coupled_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1,
                                        double dt, double abstol, double abstol_e, double reltol,
                                        uint32_t flags, void* dt_cols_device_ft, const double* bcv);

/* Adaptive TR-BDF2 of the heat-only model, SoilEnergyModel + PrescribedHydrologyModel, each column with
 * its own step (build-defined as lh_integrate_trbdf2).  The tendency is affine in
 * rhoe_int (lh_step_heat_implicit), so both stages of a step are exact tridiagonal solves -- no Newton, no
 * convergence question -- and the Hosea-Shampine estimate is filtered by the stage matrix itself:
 * e = (I - d h A)^-1 (b1 h f_n + b2 z_g + b3 z_1), solved homogeneously against the factorisation of the
 * attempt (Dirichlet conductances in the pivots, no boundary offset);
 * E = sqrt(mean_i (e_i / (abstol_e + reltol max(|rhoe_n,i|, |rhoe_1,i|)))^2), accepted when E <= 1,
 * h <- h clamp(0.9 E^(-1/3), 0.2, 5): lh_integrate_trbdf2's controller, step floor (LH_TRBDF2_HMIN_FRAC)
 * and attempt cap (LH_TRBDF2_MAX_STEPS).  Every other semantic is lh_integrate_coupled_trbdf2's: flags
 * must be 0 (fixed steps: lh_step_heat_implicit with LH_HEAT_TRBDF2); dt is the initial step; dt_cols is
 * NULL or ncols FT values on the device, on entry each column's initial step (0: dt), on exit its next
 * proposal (0: the column failed); bcv is NULL or 8 doubles [t0 | t1][2 faces][2 components], interpolated
 * linearly in double at every stage time and rounded once to FT (hydrology entries are ignored; per-column
 * arrays of lh_set_bc take precedence); reltol = 0 takes 1e-3 and abstol_e = 0 takes 1e-6 rho_l c_l, each
 * on its own; t1 == t0 does nothing; status bit 0 flags a non-finite accepted result, bit 4 a column that
 * hit the step floor or the attempt cap and keeps its last accepted state; lh_trbdf2_stats reports the
 * call (Newton iterations and unconverged stages stay 0).  vartheta_l and theta_i of Ya are read once per
 * call and held through it.  f_n is carried from step to step and a call's first f_n is a fresh
 * tendency, so a call split in two is not bitwise the whole call (as for the other adaptive integrators).
 * LH_EINVAL as lh_integrate_trbdf2, checked first; then LH_EMODEL in lh_step_heat_implicit's order: any
 * model but LH_MODEL_HEAT, the states, a context with a class map.  A refused call leaves the statistics
 * zeroed.  Asynchronous. */
int lh_integrate_heat_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                             double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft,
                             const double* bcv);

/* lh_integrate_heat_trbdf2 for layered soils (a class map with its thermal supplement is set,
 * lh_set_soil_class_thermal + lh_set_soil_class_map): the same arguments,
 * defaults, bcv layout, dt_cols in and out, error norm, controller, lh_trbdf2_stats, status bits 0 and 4
 * and asynchrony, with beta, rho_c_s and kappa of every cell from its own class as
 * lh_step_layered_heat_implicit takes them.  LH_EINVAL as lh_integrate_heat_trbdf2, checked first.
 * LH_EMODEL, in this order: any model but LH_MODEL_HEAT, the states, a context without a class map
 * (lh_integrate_heat_trbdf2 integrates it; that call keeps refusing a context WITH a map), what every
 * layered call refuses (per-column parameter arrays, LH_MATH_LIBM). */
int lh_integrate_layered_heat_trbdf2(lh_ctx*, lh_state* Y, const lh_state* Ya, double t0, double t1,
                                     double dt, double abstol_e, double reltol, uint32_t flags,
                                     void* dt_cols_device_ft, const double* bcv);

/* Per-column boundary-value time series for the TR-BDF2 integrators.
 * A series holds nknots >= 2 knot times, finite and strictly increasing (LH_EINVAL otherwise, the
 * message names the first offending knot), and for any (face, component) the values at the knots,
 * piecewise linear in between: at t in [T_k, T_k+1] the value is
 * v_k + (v_k+1 - v_k) ((t - T_k) / (T_k+1 - T_k)) in double, and exactly v_k on a knot.
 * lh_bc_series_set: the value of (knot k, column c) is values[k*knot_stride + c*col_stride];
 * col_stride == 0 gives every column the same value per knot (stored as nknots doubles).  A
 * per-column table is kept on the device in double, column-fastest with the context's plane
 * stride, whatever the working type.  values == NULL removes that component's series.  Values are
 * not judged.  The call copies the values and synchronises.
 * lh_bc_series_destroy releases the tables (lh_destroy releases the series still alive).
 *
 * lh_integrate_series stands for lh_integrate_trbdf2 (Richards without a class map),
 * lh_integrate_layered_trbdf2 (Richards with one) or lh_integrate_coupled_trbdf2 (coupled without
 * one); anything else is LH_EMODEL.  abstol_e is read by the coupled model only.  With the
 * breakpoints t0, every knot strictly inside (t0, t1) and t1, every column that does not fail gets,
 * BITWISE, the Y, the dt_cols entry and status bit 0 of calling that entry point once per
 * sub-interval [a, b] in order, dt_cols carried from call to call and bcv holding the column's own
 * series values at a and b -- in ONE launch, each column walking its own sub-intervals.  With
 * dt_cols_device_ft == NULL the proposals are carried in a zeroed scratch buffer of the library
 * (the first sub-interval starts every column at dt).  A (face, component) without a series keeps
 * lh_set_bc's value, its per-column array included; one with a series ignores both.  The step
 * floor (1e-10 x the sub-interval) and the cap on attempted steps apply per sub-interval, and the
 * tendency at the start of every sub-interval is evaluated anew.  A column that fails in a
 * sub-interval stops there with its last accepted state, sets status bit 4 and gets dt_cols = 0.
 * lh_trbdf2_stats: accepted, rejected, Newton iterations, failed and unconverged are sums over the
 * sub-intervals; max_steps is the largest total of attempted steps of any column over the whole
 * call and wave_steps the sum over waves of 64 x the wave's largest such total.
 * flags: LH_TRBDF2_FIXED where the entry stood for takes it (steps are clipped at every breakpoint
 * as at t1); 0 for the coupled model.
 * LH_EINVAL: what the entry stood for refuses, t0 < T_0 or t1 > T_last (no extrapolation), a NULL
 * series, a series of another context; t0 == t1 does nothing.  LH_EMODEL: what the entry stood for
 * refuses, in its order; then a series on a component the model does not have (energy on a Richards
 * context) or on a (face, component) whose lh_set_bc kind reads no value (LH_BC_NONE,
 * LH_BC_FREE_DRAINAGE).  After a refused call lh_trbdf2_stats gives zeros.  Asynchronous. */
typedef struct lh_bc_series lh_bc_series;
int lh_bc_series_create(lh_ctx*, int32_t nknots, const double* times, lh_bc_series** out);
int lh_bc_series_set(lh_ctx*, lh_bc_series*, int32_t face, int32_t component, const double* values,
                     int64_t knot_stride, int64_t col_stride);
int lh_bc_series_destroy(lh_ctx*, lh_bc_series*);
int lh_integrate_series(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series*, double t0, double t1,
                        double dt, double abstol, double abstol_e, double reltol, uint32_t flags,
                        void* dt_cols_device_ft);

/* lh_integrate_series' semantics for the heat-only model (no counterpart in the
 * reference, as lh_integrate_series): stands for lh_integrate_heat_trbdf2 (a heat-only context without
 * a class map) or lh_integrate_layered_heat_trbdf2 (with one).  Breakpoints, the bitwise chain (Y, the
 * dt_cols entry, status bit 0 of calling that entry point once per sub-interval in order, dt_cols
 * carried and bcv holding the column's own series values at both ends), dt_cols_device_ft == NULL, the
 * components without a series, the step floor and attempt cap per sub-interval, a failing column and
 * lh_trbdf2_stats are lh_integrate_series' (Newton iterations and unconverged stages stay 0).  flags
 * must be 0.  Every sub-interval starts with that entry point's prologue: the closure sweep of the
 * column and a fresh tendency.  Refusals, in this order: what the entry stood for refuses, in its
 * order and words (arguments first; any model but LH_MODEL_HEAT is LH_EMODEL); a NULL series or one
 * of another context, [t0, t1] beyond the knots (LH_EINVAL); an energy series on a face whose
 * lh_set_bc kind reads no value, then a hydrology series -- a heat-only model has no hydrology
 * component (LH_EMODEL).  A refused call leaves the statistics zeroed; t0 == t1 does nothing.
 * Asynchronous. */
int lh_integrate_heat_series(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series*, double t0, double t1,
                             double dt, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft);

/* lh_integrate_series' semantics for a coupled context with a class map and its thermal supplement
 * (no counterpart in the reference): stands for
 * lh_integrate_layered_coupled_trbdf2, with lh_integrate_series' arguments, breakpoints, bitwise chain,
 * dt_cols handling and statistics (unconverged stages stay 0).  flags must be 0.  Refusals, in this
 * order: what lh_integrate_layered_coupled_trbdf2 refuses, in its order and words (a coupled context
 * without a class map is pointed to lh_integrate_series); then the series' own checks as
 * lh_integrate_series makes them.  A refused call leaves the statistics zeroed; t0 == t1 does nothing.
 * Asynchronous. */
int lh_integrate_layered_coupled_series(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series*, double t0,
                                        double t1, double dt, double abstol, double abstol_e, double reltol,
                                        uint32_t flags, void* dt_cols_device_ft);

/* lh_step_ssprk33 under a per-column boundary-value series (no counterpart in the
 * reference): nsteps fixed-dt SSPRK33 steps from t.  Y and the status word are those of lh_step_ssprk33;
 * the one difference is where the boundary values come from.  A (face, component) for which the series holds
 * a table has, in every column, its value sampled from that column's own piecewise-linear table at every
 * stage time; it reads neither lh_set_bc's value nor its per-column array (the kind stays lh_set_bc's).  A
 * component without a series keeps its value, or its per-column array, for the whole call.
 * Stage times, in double: t_k = t + dt * (double)k; the stages of step k are at t_k, t_k + dt, t_k + dt / 2.
 * The value at a stage time tau is lh_integrate_series' (above): with k the largest index that has
 * T_k <= tau, capped at nknots - 2, exactly v_k or v_k+1 on a knot, v_k + (v_k+1 - v_k) ((tau - T_k) /
 * (T_k+1 - T_k)) in double otherwise, rounded once to the working type.  For a uniform series the call is
 * BITWISE lh_step_ssprk33 with bc_stage_values holding those samples; a column's result depends on its own
 * table only.  The context's boundary state is not modified.
 * Refusals, in this order: lh_step_ssprk33's own, in its order and words under this call's name; a t that
 * is not finite (LH_EINVAL); the series' checks as lh_integrate_series makes them (a NULL series or one of
 * another context, LH_EINVAL; a series on a component the model does not have or whose lh_set_bc kind reads
 * no value, LH_EMODEL); a stage time of the call outside [T_0, T_last] (LH_EINVAL, the message names the
 * time).  nsteps == 0 does nothing after the first three.  Asynchronous.
 * lh_step_series_engine: LH_ENGINE_COLUMN_STEPPER (ONE launch, the wave stepper samples the series itself) for
 * a context without a class map and nlev <= 128 where lh_step_engine(ctx, nsteps, 1) answers the stepper and the
 * ensemble is small (ncols x nlev rounded up to 64 at most 2^20) or the tuning says persist=2;
 * LH_ENGINE_FUSED_STAGES otherwise (columns of more than 128 levels, every context with a class map,
 * a prescribed atmosphere, persist=0, large ensembles under the default tuning): one small launch per step writes the three stages' sampled values
 * per column, and the three fused-stage launches take them where lh_set_bc's per-column arrays go.  The
 * answer is what lh_step_ssprk33_series does in every case; a negative LH_E* for a NULL context or
 * nsteps < 0. */
int lh_step_ssprk33_series(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series*, double t, double dt,
                           int64_t nsteps);
int lh_step_series_engine(const lh_ctx*, int64_t nsteps);

/* Dense output for the adaptive TR-BDF2 integrators (OrdinaryDiffEq's saveat): the
 * integration of lh_integrate_series -- same three families (Richards, Richards with a class map, coupled
 * without one), same arguments, defaults and flags -- with nsave snapshots of the state at save_times,
 * interpolated inside the launch from the steps the columns accept.  series == NULL: no forcing table;
 * the call then stands for lh_integrate_trbdf2 / lh_integrate_layered_trbdf2 / lh_integrate_coupled_trbdf2
 * with bcv == NULL (lh_set_bc's values, per-column arrays included; one sub-interval).
 * The integration does not see the output: Y, dt_cols, the status word and all of lh_trbdf2_stats are
 * BITWISE those of that twin call without output; no step is clipped or restarted at a save time.
 * save_times (host, [nsave]): finite, strictly increasing, t0 <= s_1 and s_nsave <= t1; nsave <= 65536;
 * nsave == 0 with both arrays NULL is the twin call.  snapshots (host, [nsave]): states of this context
 * that hold vartheta_l and, on a coupled context, rhoe_int, each distinct from Y, Ya and one another.
 * Only those planes are written (and marked written).  Snapshot k of a column is written when the column
 * accepts the step t -> t_new (its own doubles) with t < s_k <= t_new: with theta = (s_k - t) / h,
 * y0 = Y_n, y1 = Y_n+1, f0 the step's f_n and f1 = (Y_n+1 - w_2) / (d h),
 *   u = (1 - theta) y0 + theta y1 + theta (theta - 1) ((1 - 2 theta)(y1 - y0) + (theta - 1) h f0 + theta h f1),
 * the coefficients rounded to the working type once and the combination evaluated in it, per cell.
 * theta == 1 gives Y_n+1 bitwise; a snapshot at s_k == t0 is Y as passed.  A rejected step writes nothing.
 * A column that fails (status bit 4) stops as in lh_integrate_series, and every snapshot it has not yet
 * written receives its last accepted state.  A column's snapshots do not depend on the other columns.
 * Refusals: lh_integrate_series' own, in its order and words under this call's name (a heat-only context
 * and a coupled context with a class map are LH_EMODEL), the series' checks only with a series; behind
 * them, all LH_EINVAL and naming the offending index: nsave < 0 or > 65536, a NULL array with nsave > 0,
 * a save time that is not finite, not above its predecessor or outside [t0, t1], a snapshot that is
 * NULL, not a state of this context, Y, Ya or an earlier snapshot, or that lacks a written plane.  A
 * refused call leaves Y, every snapshot and dt_cols untouched and the statistics zeroed.  The two host
 * arrays are copied before the call returns; it waits for its launch. */
int lh_integrate_dense(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series* series, double t0, double t1,
                       double dt, double abstol, double abstol_e, double reltol, uint32_t flags,
                       void* dt_cols_device_ft, int32_t nsave, const double* save_times,
                       lh_state* const* snapshots);

/* lh_integrate_dense's semantics for the heat-only model: the integration of
 * lh_integrate_heat_series -- without or with a class map, same arguments and defaults, flags must be 0 --
 * with nsave snapshots of rhoe_int at save_times, interpolated inside the launch from the steps the
 * columns accept.  series == NULL: no forcing table; the call then stands for lh_integrate_heat_trbdf2 /
 * lh_integrate_layered_heat_trbdf2 with bcv == NULL (one sub-interval).  The integration does not see
 * the output: Y, dt_cols, the status word and all of lh_trbdf2_stats are BITWISE those of that twin call;
 * nsave == 0 with both arrays NULL is the twin call and asynchronous as it.  save_times, the interpolant
 * (f1 = (Y_n+1 - w_2) / (d h) also on the last step of a sub-interval), theta == 1, s_k == t0, rejected
 * steps, a failing column and the independence of the columns are lh_integrate_dense's.  snapshots: states
 * of this context that hold rhoe_int (vartheta_l is not required), each distinct from Y, Ya and one
 * another; only rhoe_int of a snapshot is written (and marked written).
 * Refusals: lh_integrate_heat_series' own, in its order and words under this call's name (any model but
 * LH_MODEL_HEAT is LH_EMODEL), the series' checks only with a series; behind them lh_integrate_dense's
 * checks of the output (LH_EINVAL, naming the offending index).  A refused call leaves Y, every snapshot
 * and dt_cols untouched and the statistics zeroed.  With nsave > 0 the two host arrays are copied before
 * the call returns and it waits for its launch. */
int lh_integrate_heat_dense(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series* series, double t0, double t1,
                            double dt, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft,
                            int32_t nsave, const double* save_times, lh_state* const* snapshots);

/* ... and for a coupled context with a class map and its thermal supplement: the
 * integration of lh_integrate_layered_coupled_series (series == NULL: of lh_integrate_layered_coupled_trbdf2
 * with bcv == NULL) with snapshots of vartheta_l and rhoe_int, both required of a snapshot, both written and
 * marked written.  flags must be 0.  Everything else is lh_integrate_heat_dense's, with
 * lh_integrate_layered_coupled_series' refusals in front (a coupled context without a class map is
 * pointed to lh_integrate_dense). */
int lh_integrate_layered_coupled_dense(lh_ctx*, lh_state* Y, const lh_state* Ya, const lh_bc_series* series, double t0,
                                       double t1, double dt, double abstol, double abstol_e, double reltol,
                                       uint32_t flags, void* dt_cols_device_ft, int32_t nsave,
                                       const double* save_times, lh_state* const* snapshots);

/* Build-defined stable step (the reference uses a fixed user dt):
 * courant*dz^2 / max over owned faces of the face diffusivities
 * ((K_lo+K_hi)/2 * max dpsi/dvl, (kappa_lo+kappa_hi)/2 / min rho_c_s; boundary
 * cells and Dirichlet faces with their own coefficients).
 * _device leaves the FT result in device memory (for an RCCL min all-reduce
 * across ranks without a host round trip); the host form synchronises. */
int lh_stable_dt(lh_ctx*, const lh_state* Y, const lh_state* Ya, double courant,
                 double* dt_host);
int lh_stable_dt_device(lh_ctx*, const lh_state* Y, const lh_state* Ya, double courant,
                        void* dt_device_ft);

/* ---- multi-GPU: block partition + the one collective ------------- */

/* No counterpart in the reference (one column, one process, fixed user dt:
 * src/Simulations/simulation.jl:34-70).  Columns are independent, so an ensemble
 * of ncols_global columns is block-partitioned over ranks (one process and one
 * context per GPU) with no halo and no data-path exchange.  The only collective
 * of the path is the minimum of the ranks' stable-step bounds: ONE FT value,
 * ncclAllReduce(count = 1, ncclMin) over RCCL/xGMI on the context's stream. */

/* columns [*lo, *hi) owned by `rank` of `nranks` (the first ncols_global % nranks
 * ranks own one more); per-column parameter and BC arrays partition the same way */
int lh_block_range(int64_t ncols_global, int32_t rank, int32_t nranks, int64_t* lo, int64_t* hi);

/* ncclGetUniqueId: fills LH_COMM_ID_BYTES bytes on ONE rank; the host ships them
 * to the others (MPI_Bcast, a file, torch.distributed ...) before lh_comm_init */
#define LH_COMM_ID_BYTES 128
int lh_comm_unique_id(void* id_out);
/* ncclCommInitRank on the context's device (collective: every rank calls it).
 * While a communicator is attached, lh_rhs_stable_dt, lh_stable_dt_device and
 * lh_stable_dt deliver the GLOBAL minimum over all ranks (the all-reduce is
 * enqueued on the context's stream behind the local reduction: no host round
 * trip); everything else stays rank-local. */
int lh_comm_init(lh_ctx*, int32_t rank, int32_t nranks, const void* unique_id);
int lh_comm_destroy(lh_ctx*);
/* rank / nranks of the attached communicator (0 / 1 when there is none) */
int lh_comm_info(const lh_ctx*, int32_t* rank, int32_t* nranks);
/* in-place min all-reduce of one FT value in device memory over the attached
 * communicator (no-op without one): for hosts that form their own step bound */
int lh_allreduce_min(lh_ctx*, void* value_device_ft);

/* ---- status / timing -------------------------------------------------------- */

/* bit 0: a non-finite tendency was produced since the last call (the reference would have raised
 * DomainError from `^`), or a non-finite result by lh_step_heat_implicit, lh_step_coupled_implicit
 * or an accepted step of lh_integrate_coupled_trbdf2; bit 1: the Monin-Obukhov system of the
 * prescribed-atmosphere BC had no root in some column; bit 2: a step of lh_step_ssprk33_adaptive
 * found no positive finite step bound (no positive diffusivity anywhere and no dt_max, or a NaN)
 * and was taken with dt = 0; bit 3: an implicit step (lh_step_implicit_euler) did not converge in
 * some column (also the fixed-step mode of lh_integrate_trbdf2); bit 4: a column of
 * lh_integrate_trbdf2, lh_integrate_coupled_trbdf2, lh_integrate_layered_coupled_trbdf2,
 * lh_integrate_heat_trbdf2 or lh_integrate_layered_heat_trbdf2 (or of a series call that stands for
 * one of them) failed
 * (its step fell below the floor or it hit the step cap) and did not reach t1; bit 5: a chunk of lh_step_ssprk33_adaptive_hold held a
 * step that exceeded the stable step of the state it produced; synchronises and clears. */
int lh_get_status(lh_ctx*, uint32_t* flags);
int lh_synchronize(lh_ctx*);
/* Streaming ceiling of the column launch on a given set of planes (measurement aid, no
 * counterpart in the reference): a kernel with rhs_kernel's access pattern and no arithmetic
 * reads the planes of `in` selected by read_mask and writes the planes of `out` selected by
 * write_mask (LH_MASK bits), `reps` launches (<= 0: 20); *ms_per_launch = their average
 * duration by HIP events.  The selected planes of `out` hold unspecified values afterwards.
 * Synchronises. */
int lh_stream_probe(lh_ctx*, const lh_state* in, uint32_t read_mask, lh_state* out, uint32_t write_mask,
                    int reps, float* ms_per_launch);
/* HIP-event stopwatch on the context's stream */
int lh_timer_start(lh_ctx*);
int lh_timer_stop(lh_ctx*, float* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* LANDHYDRO_H */
