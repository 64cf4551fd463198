// lh_device.hpp -- kernel-argument structs shared by the host API (lh_api.hip)
// and the gfx950 kernels (lh_kernels.hip).  Product code: nothing here touches
// the CPU oracle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lh {

enum { MODEL_RICHARDS = 0, MODEL_HEAT = 1, MODEL_COUPLED = 2 };
enum { BC_NONE = 0, BC_FLUX = 1, BC_DIRICHLET = 2, BC_FREE_DRAINAGE = 3 };
enum { FACE_BOTTOM = 0, FACE_TOP = 1 };
enum { COMP_ENERGY = 0, COMP_HYDROLOGY = 1 };
enum { PC_VG_N = 0, PC_VG_ALPHA, PC_VG_THETA_R, PC_VG_KSAT, PC_NU, PC_S_S, PC_COUNT };

// per-column constants derived from vanGenuchten / SoilParams; one set per lane
// (uniform ensembles: computed once on the host, see DevParams::uc)
template <typename FT>
struct ColC {
    FT nu, S_s, theta_r, theta_lim; // theta_lim = theta_r + eps(FT)
    FT n, inv_n, m, inv_m;          // m = 1 - 1/n (SoilWaterParameterizations.jl:167)
    FT alpha_pnn;                   // alpha^(-n)
    FT Ksat;
    FT cgw;                         // cg2 * Ksat: the water flux constant of the column kernels (K is carried without Ksat)
    FT k_dry;                       // SoilHeatParameterizations.jl:280-294
    FT inv_por, inv_S_s, inv_nu;    // 1/(nu - theta_r), 1/S_s, 1/nu
    FT log2_alpha;                  // log2(alpha), for the log-domain psi
    FT l2_por;                      // log2(nu - theta_r) BY THE DEVICE'S OWN log2 (finish_colc): ice lanes
    // exponent multipliers of the log-domain closures, pre-scaled by the exp2 unit
    // of the math policy (MathFast<double>::EXP2_SCALE = 2048, else 1)
    FT e_inv_m, e_m, e_inv_n, e_log2_alpha, e_one; // S*/m, S*m, S*/n, S*log2 alpha, S
    // every power of the water closures stays a normal number for every S >= eps / (nu - theta_r)
    // (set_fast_vg): m >= LH_VG_FAST_MIN_M and moderate alpha, porosity.  Clay-like columns below that
    // (n < 1.075) take the v_ldexp form of 2^(.), which saturates like the reference's pows do.
    int32_t vg_fast;
    int32_t pad_;
};
// smallest m = 1 - 1/n for which S^(1/m) of the driest representable cell stays a normal number
#define LH_VG_FAST_MIN_M 0.07

// Everything a launch needs, already rounded to the working type FT the way the
// Julia constructors round (FT(x)); passed by value as the kernel argument.
template <typename FT>
struct DevParams {
    int64_t ncols;   // columns owned by this context
    int64_t stride;  // elements between consecutive levels of a plane (>= ncols, multiple of 64)
    int32_t nlev;
    int32_t model;
    FT dz;        // (zmax - zmin) / nlev            (domain.jl:64)
    FT inv_dz;    // 1 / dz
    FT half_inv_dz; // (1/2) / dz: the arithmetic-mean factor of InterpolateC2F folded into GradientC2F (exact)
    FT cg2;       // (1/2) / dz^2 = half_inv_dz * inv_dz: the factor of a centre difference that makes a flux a TENDENCY
                  // (host-computed: a product of two kernel arguments would live in VGPRs -- there is no scalar f64 multiply)
    FT half_dz;   // boundary centre-to-face distance (boundary_conditions.jl:196-208)
    const FT* zc; // device array [nlev], coordinates(cs)

    // vanGenuchten{FT} (SoilWaterParameterizations.jl:150-169)
    FT vg_n, vg_alpha, vg_theta_r, vg_Ksat;
    // SoilParams{FT} (parameters.jl:11-43)
    FT nu, S_s, rho_c_ds, kappa_solid, rho_p, kappa_sat_unfrozen, kappa_sat_frozen,
        kappa_dry_parameter, nu_ss_om, b;
    FT kersten_exp_unfrozen; // (1 + nu_om - a*nu_q - nu_g)/2  (SoilHeatParameterizations.jl:165)
    FT kersten_exp_frozen;   // 1 + nu_om                      (:171)
    FT one_minus_om;         // 1 - nu_om                      (:169)
    FT neg_b_log2e_sc;       // -b log2(e) x the exp2 unit of the production math: exp(-b S_r) as one 2^(.)
    // log2 of the saturated conductivities, for kappa_su^(tl/tw) kappa_sf^(ti/tw) as one 2^(.)
    FT l2_kappa_sat_unfrozen, l2_kappa_sat_frozen;
    // CLIMAParameters constants as SoilHeatParameterizations.jl forms them
    FT rho_i, rhocp_l, rhocp_i, T_ref, LH_f0, k_air;
    // conductivity factors (SoilWaterParameterizations.jl:46-126)
    int32_t viscosity_kind, impedance_kind;
    FT gamma, T_ref_visc, Omega;

    ColC<FT> uc; // column constants of the scalar parameters (host-computed)

    // per-column overrides, device arrays [ncols] or nullptr
    const FT* pc[PC_COUNT];
    // boundary conditions [face][component]
    int32_t bc_kind[2][2];
    FT bc_value[2][2];
    const FT* bc_pc[2][2];
    int32_t consistent_bottom_sign;

    uint32_t* status; // device word; bit 0 = non-finite tendency seen
    const double* math_tab; // device copy of the log2/exp2 tables (lh_fastmath.hpp)
    void* dt_out;           // MODE 4: FT-sized device word receiving the stable-step minimum
    int32_t cs_cpb;         // persistent column stepper: columns per workgroup (0 = launcher's choice)
    int32_t seg_len;        // > 0: level-segmented launch, levels per segment (small ensembles)
    int32_t xcd_remap;      // workgroup -> column-block map that gives each XCD one contiguous column range
    // LEVEL-UNIFORM prescribed fields of Ya (lh_upload_profile): FT[nlev] device arrays or nullptr, indexed
    // like Planes::v -- the column kernels stage them in LDS beside z and read no plane for them
    // (Ya.soil.T .= T_profile.(zc, t) is a function of z and t only: right_hand_side.jl:54-62)
    const FT* aux_prof[4];
    int32_t vg_fast_all;    // every column has ColC::vg_fast (host decision: uniform parameters + the ranges of the per-column arrays)
};

// PrescribedAtmosForcing{FT} (boundary_conditions.jl:119-132) plus every constant
// compute_turbulent_surface_fluxes (:553-620) reads, rounded to FT (lh_atmos.hpp)
template <typename FT>
struct AtmosParams {
    FT u_atm, theta_atm, z_atm, theta_scale, rho_a_sfc, q_atm; // PrescribedAtmosForcing{FT}
    FT z_0m, z_0s;                                             // SoilParams.z_0m, z_0s
    FT R_v, R_d, grav, cp_d, cp_v, T_triple, press_triple, von_karman;
    FT cp_l, T_0, rho_liq;   // from the earth parameters of the context
    double cp_v_d, LH_v0_d;  // FT(cp_v (T - T_ref) + LH_v0): formed in Float64, rounded once (:614-615)
    const FT* pc_u;          // per-column u_atm / theta_atm / q_atm or nullptr
    const FT* pc_theta;
    const FT* pc_q;
};

// one FieldVector on the device: up to four planes [nlev][stride]
template <typename FT>
struct Planes {
    FT* v[4];
};

// lh_step_implicit_euler's launch (lh_implicit.hpp)
template <typename FT>
struct ImplicitArgs {
    FT* y;               // vartheta_l plane of Y: the iterate
    const FT* ti;        // theta_i plane (not read by the kernels that know it zero)
    FT* yn;              // scratch planes [nlev][stride]: v_n, c', d'
    FT* cp;
    FT* dp;
    const FT* bcv;       // [nsteps][2 faces][2 components] boundary values at t_{n+1}, or nullptr
    FT dt, tol;
    int32_t max_iter;
    int64_t nsteps;
    int32_t* max_iters;          // largest iteration count of any column-step
    unsigned long long* unconverged; // column-steps that did not converge
    unsigned long long* total_iters; // Newton iterations over all column-steps
};

// lh_step_implicit_euler's and lh_step_coupled_implicit's statistics of one call: the device block the three
// counters of ImplicitArgs / CoupledImplicitArgs point into, and what the host reads back
struct ImplicitStats {
    int32_t max_iters;
    unsigned long long unconverged, total_iters;
};
static_assert(sizeof(ImplicitStats) == 24, "one int32 (padded) and two 64-bit counters");

// lh_step_heat_implicit's launch (lh_heat_implicit.hpp)
template <typename FT>
struct HeatImplicitArgs {
    FT* y;               // rhoe_int plane of Y
    const FT* vl;        // the prescribed vartheta_l and theta_i planes of Ya, read once per call
    const FT* ti;
    FT* a;               // scratch planes [nlev][stride]: the factorisation (G_i-1 / den_i-1, rho_c_s,i / den_i, G_i alpha_i+1 rho_c_s,i / den_i),
    FT* iden;
    FT* cp;
    FT* kc;              // ... coef x the constant of the affine tendency (without the boundary faces' share),
    FT* z;               // ... r' of a forward sweep, TR-BDF2's w2
    FT* ks;              // (TR-BDF2) kappa_i + kappa_i+1, alpha_i = 1 / rho_c_s, beta_i = T(rhoe_int = 0): the tendency
    FT* al;
    FT* be;
    const FT* bcv;       // [nsteps + 1][2 faces][2 components] boundary values at t + k dt, or nullptr
    FT coef;             // dt (backward Euler) or (2 - sqrt 2)/2 dt (both TR-BDF2 stages)
    int64_t nsteps;
};

// lh_step_coupled_implicit's launch (lh_coupled_implicit.hpp); the three counters point into an ImplicitStats block
template <typename FT>
struct CoupledImplicitArgs {
    FT* y;               // vartheta_l plane of Y: the water stage's iterate
    const FT* ti;        // theta_i plane (not read by the kernels that know it zero)
    FT* e;               // rhoe_int plane of Y
    FT* w;               // scratch planes [nlev][stride]: the water stage's w (backward Euler: v_n), c', d' --
    FT* cp;              // ... the last two reused by the energy solve once Newton is finished
    FT* dp;
    FT* yn;              // (TR-BDF2) the water's Y_n and f_n, the energy's f_n and w2
    FT* fn;
    FT* fe;
    FT* we;
    const FT* bcv;       // [nsteps + 1][2 faces][2 components] boundary values at t + k dt, or nullptr
    FT coef;             // dt (backward Euler) or (2 - sqrt 2)/2 dt (both TR-BDF2 stages)
    FT tol;
    int32_t max_iter;
    int64_t nsteps;
    int32_t* max_iters;
    unsigned long long* unconverged;
    unsigned long long* total_iters;
};

// lh_integrate_trbdf2's launch (lh_implicit.hpp)
template <typename FT>
struct Trbdf2Args {
    FT* y;               // vartheta_l plane of Y: the column's state, and the stage iterates
    const FT* ti;        // theta_i plane (not read by the kernels that know it zero)
    FT* yn;              // scratch planes [nlev][stride]: Y_n, f_n, Y_gamma, the stage's w, c', d'
    FT* fn;
    FT* yg;
    FT* w;
    FT* cp;
    FT* dp;
    FT* dt_cols;         // [ncols] per-column step in / proposal out (0: failed), or nullptr
    double t0, t1, dt;   // the call's interval; dt: the initial (adaptive) or the fixed step
    double abstol, reltol;
    double bcv[8];       // [t0 | t1][2 faces][2 components], linear in between (has_bcv)
    int32_t has_bcv;
    int32_t fixed;       // LH_TRBDF2_FIXED: steps of dt, no error control, backward Euler's Newton test
    FT tol;              // (fixed) Newton tolerance and cap, as lh_step_implicit_euler
    int32_t max_iter;
    FT kappa;            // (adaptive) stage Newton test max |delta| / (atol + rtol |Y|) <= kappa ...
    int32_t newton_max;  // ... within newton_max iterations, else the step is rejected
    unsigned long long* stats; // accepted, rejected, Newton iterations, max steps, failed, wave_steps, unconverged
};
// lh_integrate_coupled_trbdf2's launch (lh_coupled_trbdf2.hpp); stats as Trbdf2Args (slot 6 stays 0)
template <typename FT>
struct CoupledTrbdf2Args {
    FT* y;               // vartheta_l plane of Y: the column's state, and the water stages' iterates
    const FT* ti;        // theta_i plane (not read by the kernels that know it zero)
    FT* e;               // rhoe_int plane of Y: the column's state, and the candidate Y_1
    FT* yn;              // scratch planes [nlev][stride], the water's as Trbdf2Args: Y_n, f_n, Y_gamma, the stage's w, c', d'
    FT* fn;
    FT* yg;
    FT* w;
    FT* cp;              // (c', d' also serve the energy solves and both error filters)
    FT* dp;
    FT* en;              // ... and the energy's: Y_n, f_n, Y_gamma, w2
    FT* fe;
    FT* eg;
    FT* we;
    FT* dt_cols;         // [ncols] per-column step in / proposal out (0: failed), or nullptr
    double t0, t1, dt;   // the call's interval and the initial step
    double abstol, abstol_e, reltol;
    double bcv[8];       // [t0 | t1][2 faces][2 components], linear in between (has_bcv)
    int32_t has_bcv;
    FT kappa;            // the water stage's Newton test max |delta| / (atol + rtol |Y|) <= kappa ...
    int32_t newton_max;  // ... within newton_max iterations, else the step is rejected
    unsigned long long* stats; // accepted, rejected, Newton iterations, max steps, failed, wave_steps, 0
};
// one column's counters of a call (reduced over the wave)
struct Trbdf2ColStats {
    unsigned accepted = 0, rejected = 0, iters = 0, steps = 0, failed = 0, unconv = 0;
};

} // namespace lh
