// lh_column_ops.hpp -- what the column kernels share on the device: first the small utilities (math-table
// staging, the implicit kernels' opening, Bits, fmin/fmax, max_nonneg), then the expressions of the SSPRK33
// engines that could move here with rhs_kernel's instructions and every kernel's register, LDS and scratch
// budget unchanged.  What could not, and which tests pin it, is in DESIGN section 4.14.
#pragma once
#include "lh_closures.hpp"

namespace lh {

// Stage the log2/exp2 tables of MathFast<double> in LDS (48 KiB per workgroup);
// every thread of the block must call this before any thread leaves.
template <typename M>
__device__ __forceinline__ MathTables stage_math_tables(const double* gtab, double* lds) {
    MathTables t;
    t.log_tab = lds;
    t.exp_tab = lds + 2 * LOG_TAB_N;
    if (M::uses_tables) {
        for (int i = threadIdx.x; i < MATH_TAB_DOUBLES; i += blockDim.x) lds[i] = gtab[i];
        __syncthreads();
    }
    return t;
}

// The opening the one-lane-per-column implicit kernels (lh_implicit.hpp, lh_heat_implicit.hpp) share:
// the workgroup size ...
template <typename M>
constexpr int implicit_threads() {
    return M::uses_tables ? 512 : 256; // (the Float64 tables take 48 KiB of LDS per workgroup)
}
// ... the math tables staged in LDS (every thread of the workgroup) ...
template <typename M>
__device__ __forceinline__ M implicit_math(const double* math_tab) {
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    return M(stage_math_tables<M>(math_tab, s_tab));
}
// ... and the column this lane owns
__device__ __forceinline__ int64_t implicit_lane_column() { return int64_t(blockIdx.x) * blockDim.x + threadIdx.x; }

// positive IEEE values order like their bit patterns: global minima are integer atomicMin
template <typename FT> struct Bits;
template <> struct Bits<double> { using type = unsigned long long; };
template <> struct Bits<float> { using type = unsigned int; };

__device__ __forceinline__ double fmax_ft(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float fmax_ft(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double fmin_ft(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float fmin_ft(float a, float b) { return __builtin_fminf(a, b); }

// max of two NON-NEGATIVE floats as a signed-integer max of their bit patterns (they order alike;
// -0.0 and negative values lose, a NaN wins and is dropped with its lane at the end): one
// v_max_i32 / v_max3_i32, where fmaxf costs a canonicalising v_max_f32 per operand on top
__device__ __forceinline__ float max_nonneg(float a, float b) {
    return __builtin_bit_cast(float, __builtin_elementwise_max(__builtin_bit_cast(int, a), __builtin_bit_cast(int, b)));
}

// Workgroups are dealt round-robin to the 8 XCDs.  With xcd_remap, workgroup b handles
// column block (b % 8) * (nblocks / 8) + b / 8: each XCD streams one contiguous eighth of
// every plane row instead of every eighth 2-KiB piece.  (The column steppers: neighbouring workgroups
// share the 128-byte lines their 16..64-byte pieces of a plane row lie in, so they must share an L2.)
// Used by both steppers and stream_probe_kernel; rhs_kernel keeps the same lines in its own text.
__device__ __forceinline__ unsigned xcd_block(int xcd_remap) {
    unsigned blk = blockIdx.x;
    if (xcd_remap) {
        const unsigned per = gridDim.x >> 3;
        if (blk < (per << 3)) blk = (blk & 7u) * per + (blk >> 3);
    }
    return blk;
}

// the boundary values of one stage or step: b = (bottom energy, bottom water, top energy, top water)
template <typename FT>
__device__ __forceinline__ void set_stage_boundary_values(DevParams<FT>& P, const FT* b) {
    P.bc_value[FACE_BOTTOM][COMP_ENERGY] = b[0];
    P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = b[1];
    P.bc_value[FACE_TOP][COMP_ENERGY] = b[2];
    P.bc_value[FACE_TOP][COMP_HYDROLOGY] = b[3];
}

// Fluxes are carried in units of the TENDENCY: the arithmetic-mean factor 1/2 of InterpolateC2F,
// the 1/dz of GradientC2F and the 1/dz of DivergenceF2C are one constant cg = (1/2)/dz^2 applied to
// the centre difference, and (production math) the closures return K WITHOUT Ksat, which joins cg in
// the per-column constant of the water flux: two multiplications per cell less than
// F = -(K_lo + K_hi) (dh (1/2)/dz), -(F_hi - F_lo)/dz, a rounding-level regrouping.  Boundary
// fluxes (physical units, boundary_fluxes) are scaled by 1/dz once per column.
// Ksc: the factor that makes a closure K a true conductivity; cgw: the water flux constant.
template <typename FT, typename M>
__device__ __forceinline__ void flux_scales(const DevParams<FT>& P, const ColC<FT>& c, FT& Ksc, FT& cgw) {
    Ksc = M::is_production ? c.Ksat : FT(1);
    cgw = M::is_production ? c.cgw : P.cg2;
}

// The closures of one cell, heat first, then water, then E: T and kappa (HEAT), K WITHOUT Ksat where the
// math is the production one (flux_scales) and -psi (WATER; see head_difference), E = rho_e_int_l K
// (COUPLED).  Ta is the prescribed temperature a Richards cell passes on as T.  With WANT_DT also the
// Float32 terms of the step bound: dpsi = n m d psi / d vl and ircs = 1 / rho_c_s (the reciprocal
// temperature_closure formed); without it both come back 0 and water_closures never writes through &dpsi.
// (Both column steppers and the BOUND epilogue; rhs_kernel keeps the same lines in its own text.)
template <typename FT, typename M, int MODEL, bool FACTORS, bool NOICE, bool WANT_DT>
__device__ __forceinline__ void cell_closures(const M& mm, const DevParams<FT>& P, const ColC<FT>& c, FT vl, FT ti,
                                              FT re, FT Ta, bool vgf, FT& T, FT& kap, FT& K, FT& psi, FT& E,
                                              float& dpsi, float& ircs) {
    constexpr bool WATER = (MODEL != MODEL_HEAT), HEAT = (MODEL != MODEL_RICHARDS);
    FT rcs = FT(1);
    T = Ta;
    kap = FT(0);
    K = psi = E = FT(0);
    dpsi = ircs = 0.0f;
    if (HEAT) {
        T = temperature_closure<FT, M, NOICE>(mm, P, c, vl, ti, re, rcs);
        kap = kappa_closure<FT, M, NOICE>(mm, P, c, vl, ti);
        if (WANT_DT) ircs = float(mm.rcp(rcs));
    }
    if (WATER) {
        water_closures<FT, M, FACTORS, true, WANT_DT, NOICE, M::is_production, HEAT, true>(mm, P, c, vl, ti, T, K, psi, &dpsi, vgf);
        if (HEAT) E = (P.rhocp_l * (T - P.T_ref)) * K; // rho_e_int_l * K (:364)
    }
}

// The fluxes of one interior face, LOWER CELL FIRST (psi_*: -psi): -1/2 (a_lo + a_hi) (x_hi - x_lo)/dz /dz
// with the three constants (and Ksat) folded into the gradient's factor (cgw, cgT: flux_scales).
// (column_sweep_up, lh_implicit.hpp, forms the same water face but keeps h and K_lo + K_hi for its Jacobian.)
// Used by rhs_kernel and the thread-per-cell stepper; the one-wave stepper keeps the same lines in its own text.
template <typename FT, bool WATER, bool HEAT>
__device__ __forceinline__ void interior_face(const FT& K_lo, const FT& psi_lo, const FT& T_lo, const FT& kap_lo,
                                              const FT& E_lo, const FT& K_hi, const FT& psi_hi, const FT& T_hi,
                                              const FT& kap_hi, const FT& E_hi, FT dz, FT cgw, FT cgT, FT& Fw, FT& Fe) {
    Fw = Fe = FT(0);
    FT gh = FT(0);
    if (WATER) {
        gh = head_difference(psi_hi, psi_lo, dz) * cgw;
        Fw = -(K_lo + K_hi) * gh;
    }
    if (HEAT) {
        const FT gT = (T_hi - T_lo) * cgT;
        Fe = -(kap_lo + kap_hi) * gT;
        if (WATER) Fe = Fe - (E_lo + E_hi) * gh;
    }
}

// The SSPRK33 stage values (OrdinaryDiffEq SSPRK33, Shu-Osher form; b = Y, u = the stage state, k = f(u)):
//   stage 0: u + dt k      stage 1: (3 b + u + dt k)/4      stage 2: (b + 2 u + 2 dt k)/3
template <typename FT>
__device__ __forceinline__ FT ssprk33_stage_value(int stage, FT b, FT u, FT k, FT dt) {
    if (stage == 0) return u + dt * k;
    if (stage == 1) return (FT(3) * b + u + dt * k) * FT(0.25);
    // s / 3 as s*(1/3) plus one residual correction: a bare multiply by
    // the rounded 1/3 biases every step by 5.5e-17 and the total mass
    // drifts (1.6e-11 after 138 240 steps); this form is unbiased
    const FT sum = b + FT(2) * u + FT(2) * dt * k;
    const FT q = sum * FT(1.0 / 3.0);
    return fma_ft(fma_ft(FT(-3), q, sum), FT(1.0 / 3.0), q);
}

// ---- the local stable-step bound.  Its face, boundary-cell and per-column terms stay in rhs_kernel MODE 4 and
// in the BOUND epilogue, in the same words: moved into functions they change the register allocation of the
// MODE 4 instantiations, whose device code is held fixed.  The publication is shared:
// dt = courant dz^2 / (max D): dmax = twice the diffusivity, the maximum over whatever the caller reduced
// (x -> fl(c/x) is monotone, so the minimum of the quotients IS the quotient of the maximum; a maximum is
// exact, so the word does not depend on how columns are dealt to lanes, waves or ranks).  A column whose
// maximum is NaN never gets here: the caller drops it (Dj == Dj), it is flagged through P.status; nor does
// dmax = 0 (no column, or no diffusivity at all).
template <typename FT>
__device__ __forceinline__ void bound_publish(const DevParams<FT>& P, FT courant, float dmax) {
    using U = typename Bits<FT>::type;
    const FT best = (FT(2) * courant * P.dz * P.dz) / FT(dmax);
    U b;
    __builtin_memcpy(&b, &best, sizeof(FT));
    // (most bounds are above the minimum already there: a plain read first -- the atomic only
    // when it would change the word; a stale read can only cause a redundant atomic)
    U* word = reinterpret_cast<U*>(P.dt_out);
    if (b < __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMin(word, b);
}

// ---- the two persistent column steppers: the exchange arrays in the dynamic LDS

// exchange arrays of one column, `len` words each: (K, -psi) for the water, (T, kappa) for the heat,
// rho_e_l K for both -- only what the model needs (LDS per workgroup sets how many workgroups a CU holds)
template <int MODEL> constexpr int cs_exchange_arrays() {
    return MODEL == MODEL_COUPLED ? 5 : 2;
}
template <typename FT, int MODEL>
struct StepperLds {
    FT *K, *h, *T, *kap, *E;
    __device__ __forceinline__ StepperLds(FT* base, int len) {
        K = base;
        h = K + len;
        T = (MODEL != MODEL_HEAT) ? h + len : K;
        kap = T + len;
        E = kap + len;
    }
};

} // namespace lh
