// lh_layered_stepper.hpp -- the persistent column stepper of layered soils: column_stepper_wave_kernel for the
// Richards model with the column constants taken per CELL.
//
// One wave per column, lane l owns the CW adjacent cells CW l .. CW l + CW - 1 for all steps of the call, so the
// class of a cell is a per-lane constant of the call: its byte is read once in the prologue.  The class table is
// staged in LDS beside the math tables (stage_class_table) and a cell takes `s_cls[k]` where it uses a field, as
// layered_rhs_kernel does: a register copy of the CW entries (46 VGPRs each in Float64) does not fit the budget
// of any instantiation, see section 4.22.  The stage, face and boundary expressions are layered_rhs_kernel's, so
// a call is bitwise the fused stages.
//
// Two kernels over one text (lh_layered_stepper_body.inc): layered_column_stepper_wave_kernel takes its step by value;
// layered_column_stepper_bound_kernel reads it from device memory and leaves the stable-step bound of the state the
// launch ends on (section 4.23: lh_step_layered_ssprk33_adaptive_hold and its two companions).
//
// A kernel family of its own, in its own translation units (section 4.18's rule): no kernel, DevParams or ColC
// of another header changes.
//
// The launcher's declaration is what lh_api.hip includes; the kernel follows under LH_LAYERED_STEPPER_TU, which
// only lh_kernels_f64_layered_stepper.hip / lh_kernels_f32_layered_stepper.hip define (with LH_LAYERED_TU, for
// stage_class_table and the variant rules of lh_layered.hpp).
#pragma once
#include "lh_layered.hpp"

namespace lh {

// nsteps SSPRK33 steps of a layered Richards ensemble of up to 128 levels in ONE launch;
// bcv: NULL or [nsteps][3][2][2] FT boundary values (step, stage, face, component)
template <typename FT>
void launch_layered_column_stepper(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                   const Planes<FT>& aux, FT dt, int64_t nsteps, const FT* bcv, bool factors, bool noice,
                                   hipStream_t s);

// The BOUND flavour: the step is read from *dt_device once per launch, `courant` is the
// Courant factor, and the launch leaves the stable-step bound of the state it ENDS on in P.dt_out (an FT word the
// caller has set to +inf).  nsteps == 0 is legal: the bound of Y, and no plane of Y is written.
template <typename FT>
void launch_layered_column_stepper_bound(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                         const Planes<FT>& aux, FT courant, const FT* dt_device, int64_t nsteps,
                                         const FT* bcv, bool factors, bool noice, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_STEPPER_TU

namespace lh {

// exchange words of one column: the top cell of every lane (true K, -psi) and the flux of the face below every
// lane's bottom cell, 64 words each
constexpr int LS_EXCHANGE_ARRAYS = 3;

// The variants that exist are layered_rhs_kernel's (production math, NOICE and VGF = false where rhs_kernel has
// them) for one or two cells per lane, each with and without the BOUND epilogue (two kernels over one body).
template <typename M, bool FACTORS, int CW, bool NOICE, bool VGF>
constexpr bool layered_stepper_variant_exists() {
    return layered_variant_exists<M, FACTORS, NOICE, VGF, 1>() && (CW == 1 || CW == 2);
}
// waves per SIMD the compiler is asked to leave room for: cs_wave_min_waves' budgets for the Richards model
template <typename FT, typename M, bool FACTORS, int CW, bool NOICE>
constexpr int layered_stepper_min_waves() {
    return cs_wave_min_waves<FT, MODEL_RICHARDS, FACTORS, false, M, CW, NOICE>();
}
// plane tiles of the prologue: vartheta_l, theta_i unless it is known zero, the aux T with a viscosity factor
static inline int layered_stepper_tiles(bool noice, bool need_Taux) { return 1 + (noice ? 0 : 1) + (need_Taux ? 1 : 0); }

// slope32's clamp once more (lh_closures.hpp): a non-negative Float32 kept finite by an integer minimum of the bits
__device__ __forceinline__ float finite_nonneg(float s) {
    return __builtin_bit_cast(float, __builtin_elementwise_min(__builtin_bit_cast(int, s), 0x7f7fffff));
}

// The two kernels share their text (lh_layered_stepper_body.inc).  By value: `dt` is the step.
template <typename FT, bool FACTORS, typename M, int CW, bool NOICE, bool VGF>
__global__ void __launch_bounds__(1024, (layered_stepper_min_waves<FT, M, FACTORS, CW, NOICE>()))
layered_column_stepper_wave_kernel(const DevParams<FT> P0, const LayeredArgs<FT> L, const Planes<FT> Y,
                                   const Planes<FT> AUX, const FT dt, const int64_t nsteps, const FT* __restrict__ bcv) {
    constexpr bool BOUND = false;
    const FT courant = FT(0); // (the epilogue that reads it is compiled out)
#include "lh_layered_stepper_body.inc"
}

// BOUND (section 4.23): the step is read from *dt_device once per launch, the scalar argument carries the Courant
// factor (as in rhs_kernel MODE 4 and the scalar stepper's BOUND), and after the time loop the stable-step bound of
// the state the launch ends on goes to P.dt_out.  nsteps == 0 is legal: the bound of Y, no plane written.
template <typename FT, bool FACTORS, typename M, int CW, bool NOICE, bool VGF>
__global__ void __launch_bounds__(1024, (layered_stepper_min_waves<FT, M, FACTORS, CW, NOICE>()))
layered_column_stepper_bound_kernel(const DevParams<FT> P0, const LayeredArgs<FT> L, const Planes<FT> Y,
                                    const Planes<FT> AUX, const FT courant, const FT* __restrict__ dt_device,
                                    const int64_t nsteps, const FT* __restrict__ bcv) {
    constexpr bool BOUND = true;
    const FT dt = *dt_device;
#include "lh_layered_stepper_body.inc"
}

template <typename FT>
static void launch_layered_stepper_flavour(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                           const Planes<FT>& aux, FT dt, const FT* dt_device, int64_t nsteps, const FT* bcv,
                                           bool factors, bool noice, hipStream_t s) {
    using M = MathFast<FT>;
    const int cw = (P.nlev + 63) / 64; // (the caller keeps columns of more than 128 levels with the fused stages)
    const bool ni = noice && noice_exists<M>(factors);
    const bool robust = robust_vg_exists<M, MODEL_RICHARDS>() && P.vg_fast_all == 0; // (as launch_layered_rhs)
    const bool need_Taux = factors && P.viscosity_kind;
    // dynamic LDS: the plane tiles of the prologue and the exchange arrays share it
    const size_t ex_words = size_t(LS_EXCHANGE_ARRAYS) * 64;
    const size_t tile_words = size_t(layered_stepper_tiles(ni, need_Taux)) * size_t(P.nlev);
    const size_t dyn_col = (ex_words > tile_words ? ex_words : tile_words) * sizeof(FT);
    with_bool(factors, [&](auto f) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<1, 2>{}, cw, [&](auto w) { with_bool(dt_device != nullptr, [&](auto bd) {
            constexpr bool F = decltype(f)::value, NI = decltype(i)::value, VG = decltype(vg)::value, B = decltype(bd)::value;
            constexpr int CW = decltype(w)::value;
            // (ni and robust are normalised above: the guard only keeps what cannot occur un-instantiated)
            if constexpr (layered_stepper_variant_exists<M, F, CW, NI, VG>()) {
                constexpr auto plain = layered_column_stepper_wave_kernel<FT, F, M, CW, NI, VG>;
                constexpr auto bound = layered_column_stepper_bound_kernel<FT, F, M, CW, NI, VG>;
                unsigned cpb;
                if constexpr (B) cpb = wave_stepper_columns<bound>(P.ncols, dyn_col, nsteps);
                else cpb = wave_stepper_columns<plain>(P.ncols, dyn_col, nsteps);
                if (P.cs_cpb > 0 && (unsigned)P.cs_cpb * 64u <= 1024u) cpb = (unsigned)P.cs_cpb;
                const dim3 g((unsigned)((P.ncols + cpb - 1) / cpb)), b(64u * cpb);
                const unsigned dyn = (unsigned)(cpb * dyn_col);
                if constexpr (B) hipLaunchKernelGGL(bound, g, b, dyn, s, P, L, Y, aux, dt, dt_device, nsteps, bcv);
                else hipLaunchKernelGGL(plain, g, b, dyn, s, P, L, Y, aux, dt, nsteps, bcv);
            }
        }); });
    }); }); });
}

template <typename FT>
void launch_layered_column_stepper(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                   const Planes<FT>& aux, FT dt, int64_t nsteps, const FT* bcv, bool factors, bool noice,
                                   hipStream_t s) {
    launch_layered_stepper_flavour<FT>(P, L, Y, aux, dt, nullptr, nsteps, bcv, factors, noice, s);
}

template <typename FT>
void launch_layered_column_stepper_bound(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                         const Planes<FT>& aux, FT courant, const FT* dt_device, int64_t nsteps,
                                         const FT* bcv, bool factors, bool noice, hipStream_t s) {
    launch_layered_stepper_flavour<FT>(P, L, Y, aux, courant, dt_device, nsteps, bcv, factors, noice, s);
}

#define LH_INSTANTIATE_LAYERED_STEPPER(FT)                                                                            \
    template void launch_layered_column_stepper<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&, \
                                                    const Planes<FT>&, FT, int64_t, const FT*, bool, bool, hipStream_t); \
    template void launch_layered_column_stepper_bound<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&, \
                                                          const Planes<FT>&, FT, const FT*, int64_t, const FT*, bool, bool, \
                                                          hipStream_t);

} // namespace lh
#endif // LH_LAYERED_STEPPER_TU
