// lh_series_stepper.hpp -- lh_step_ssprk33_series: fixed-step SSPRK33 under a per-column boundary-value time
// series (lh_bc_series).
//
// Two device paths, both bitwise lh_step_ssprk33 given the sampled values:
//
//   series_column_stepper_wave_kernel   column_stepper_wave_kernel's text (lh_column_stepper_wave_body.inc) with the
//       boundary values of a stage sampled by the wave itself.  One wave is one column, so a sampled value is
//       wave-uniform: it goes into the wave's private P.bc_value[f][c] through the scalar register file, and the
//       per-column array of a component with a series is never read (series_step_params).  Contexts without a class map,
//       columns of up to 128 levels.
//
//   series_stage_values_kernel          one thread per column writes the sampled values of the three stages of ONE
//       step as FT arrays [3][2][2][stride]; the host points DevParams::bc_pc of the three fused-stage launches of
//       that step at them, so rhs_kernel, layered_rhs_kernel, layered_heat_rhs_kernel and the segmented launches run
//       unchanged.  Every model family, every nlev, layered contexts, the prescribed-atmosphere top.
//
// The knot interval of a stage time is found from the time alone (the stage times of a step are not monotone, a step
// may span several knots, an interval may hold many steps): no cursor is kept anywhere.  The value is series_value of
// lh_series.hpp, in double, rounded once to the working type.
//
// The first part (the launch argument and the launchers' declarations) is what lh_api.hip includes; the kernels follow
// under LH_SERIES_STEPPER_TU, which only lh_kernels_f64_series_stepper.hip / lh_kernels_f32_series_stepper.hip define
// (with LH_SERIES_TU and what it needs, for series_value; no kernel of lh_series.hpp is instantiated there).
#pragma once
#include "lh_series.hpp" // series_value (under LH_SERIES_TU)

namespace lh {

// The table and the call's clock.  Stage `stage` of step `s` is at (t + dt double(s)) + (0, dt, dt / 2)[stage], formed in
// double on both sides (the build does not contract): series_stage_time below is the one statement of it.
// The table is SeriesArgs' packed: a per-column component has its rows P.stride doubles apart and is read at the column,
// a uniform one is nknots doubles, so one bit per component says all that knot_stride and col_varies say there (16
// scalars instead of 30 beside DevParams in the wave stepper's time loop).
struct SeriesStepArgs {
    const double* times;     // [nknots], strictly increasing
    const double* val[2][2]; // [face][component], or nullptr: lh_set_bc's value (and per-column array) stays
    uint32_t percol;         // bit 2 f + c: the component's table is per column
    int32_t nknots;
    double t, dt;
};

__host__ __device__ inline double series_stage_time(double t, double dt, int64_t s, int stage) {
    const double ts = t + dt * double(s);
    return ts + (stage == 0 ? 0.0 : (stage == 1 ? dt : dt / 2));
}

// nsteps SSPRK33 steps of an ensemble of up to 128 levels without a class map in ONE launch
template <typename FT>
void launch_series_column_stepper(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux, FT dt, int64_t nsteps,
                                  const SeriesStepArgs& S, bool factors, bool percol, bool noice, hipStream_t s);

// The sampled values of the three stages of step `step` into out[((stage * 2 + f) * 2 + c) * P.stride + col], for the
// components that have a series (the others' rows are not written)
template <typename FT>
void launch_series_stage_values(const DevParams<FT>& P, const SeriesStepArgs& S, int64_t step, FT* out, hipStream_t s);

} // namespace lh

#ifdef LH_SERIES_STEPPER_TU
#include "lh_kernels_impl.hpp" // the wave stepper's body and what it reads

namespace lh {

// The knot interval of tau: the largest k with T_k <= tau, capped at nknots - 2 (the host has checked T_0 <= tau <= T_last)
__device__ __forceinline__ int series_knot_interval(const double* __restrict__ times, int nknots, double tau) {
    int lo = 0, hi = nknots - 1; // T_lo <= tau; tau < T_hi or hi == nknots - 1
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (times[mid] <= tau) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The same index found by a whole wave: bisection down to a window of 64 knots (none for tables of up to 65 knots),
// then one load per lane and a count of the knots at or before tau.  Every lane of the wave must be here.
__device__ __forceinline__ int series_knot_interval_wave(const double* __restrict__ times, int nknots, double tau, int lane) {
    int lo = 0, hi = nknots - 1; // T_lo <= tau; tau < T_hi or hi == nknots - 1
    while (hi - lo > 64) {
        const int mid = lo + ((hi - lo) >> 1);
        if (times[mid] <= tau) lo = mid;
        else hi = mid;
    }
    const int j = lo + lane;
    const bool at_or_before = j < hi && times[j] <= tau;
    const int k = lo + int(__popcll(__ballot(at_or_before))) - 1; // (T_lo counts: >= lo; <= hi - 1 <= nknots - 2)
    return k < lo ? lo : k;
}

// The value of component (f, c) of column `col` at tau in the knot interval k, rounded once
template <typename FT>
__device__ __forceinline__ FT series_sample(const SeriesStepArgs& S, int64_t stride, int f, int c, int k, double Tk, double Tk1,
                                            double tau, int64_t col) {
    const double* v = S.val[f][c];
    const bool percol = (S.percol >> (2 * f + c)) & 1u;
    const int64_t row = percol ? stride : int64_t(1);
    const int64_t at = int64_t(k) * row + (percol ? col : int64_t(0));
    return FT(series_value(tau, Tk, Tk1, v[at], v[at + row]));
}

// series_params (lh_series.hpp) for this table: a component with a series does not read lh_set_bc's per-column array
template <typename FT>
__device__ __forceinline__ void series_step_params(DevParams<FT>& P, const SeriesStepArgs& S) {
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (S.val[f][c]) P.bc_pc[f][c] = nullptr;
}

// The wave's own sampling: what `if (bcv) set_stage_boundary_values(...)` is in column_stepper_wave_kernel
template <typename FT>
__device__ __forceinline__ void series_stage_boundary_values(DevParams<FT>& P, const SeriesStepArgs& S, int64_t col, int64_t s,
                                                             int stage, int lane) {
    // (the column of a wave is uniform, which the compiler cannot see: said here, the table's addresses are scalars and
    // are not kept in vector registers over the time loop)
    const int64_t wave_col = wave_uniform(col);
    const double tau = series_stage_time(S.t, S.dt, s, stage);
    const int k = __builtin_amdgcn_readfirstlane(series_knot_interval_wave(S.times, S.nknots, tau, lane));
    const double Tk = S.times[k], Tk1 = S.times[k + 1];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (S.val[f][c]) P.bc_value[f][c] = wave_uniform(series_sample<FT>(S, P.stride, f, c, k, Tk, Tk1, tau, wave_col));
}

// The register budgets are the scalar stepper's (cs_wave_min_waves) except where the sampling does not fit them and the
// kernel would spill vector registers its twin does not: the Float64 Richards kernels with one
// cell per lane that read theta_i leave room for 5 waves per SIMD instead of 6 (96 registers instead of 80), and the
// Float64 heat and coupled kernels with two cells per lane, which sit at the 128 registers a 1024-thread workgroup
// allows, are built for workgroups of up to 768 threads (12 columns, the most wave_stepper_columns picks) and 3 waves.
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int CW, bool NOICE>
constexpr int series_stepper_max_threads() {
    return (M::uses_tables && MODEL != MODEL_RICHARDS && CW == 2) ? 768 : 1024;
}
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int CW, bool NOICE>
constexpr int series_stepper_min_waves() {
    if (series_stepper_max_threads<FT, MODEL, FACTORS, PERCOL, M, CW, NOICE>() == 768) return 3;
    if (M::uses_tables && MODEL == MODEL_RICHARDS && CW == 1 && !NOICE) return 5;
    return cs_wave_min_waves<FT, MODEL, FACTORS, PERCOL, M, CW, NOICE>();
}

// column_stepper_wave_kernel under a series: the same body, the step by value, no BOUND epilogue
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int CW, bool NOICE, bool VGF>
__global__ void __launch_bounds__((series_stepper_max_threads<FT, MODEL, FACTORS, PERCOL, M, CW, NOICE>()),
                                  (series_stepper_min_waves<FT, MODEL, FACTORS, PERCOL, M, CW, NOICE>()))
series_column_stepper_wave_kernel(const DevParams<FT> Pk, const Planes<FT> Y, const Planes<FT> AUX, const FT dt_value,
                                  const int64_t nsteps, const SeriesStepArgs S) {
    constexpr bool BOUND = false;
    const FT* const dt_device = nullptr;
    DevParams<FT> P0 = Pk;
    series_step_params(P0, S);
    // a face keeps constant boundary values over the call only if none of its components has a series
#define LH_CSW_FACE_VALUES_FIXED(face) (!S.val[face][COMP_ENERGY] && !S.val[face][COMP_HYDROLOGY])
#define LH_CSW_STAGE_BOUNDARY_VALUES series_stage_boundary_values<FT>(P, S, col, s, stage, l)
#include "lh_column_stepper_wave_body.inc"
#undef LH_CSW_FACE_VALUES_FIXED
#undef LH_CSW_STAGE_BOUNDARY_VALUES
}

template <typename FT>
__global__ void __launch_bounds__(256)
series_stage_values_kernel(const int64_t ncols, const int64_t stride, const SeriesStepArgs S, const int64_t step,
                           FT* __restrict__ out) {
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
#pragma unroll 1
    for (int stage = 0; stage < 3; ++stage) {
        const double tau = series_stage_time(S.t, S.dt, step, stage);
        const int k = series_knot_interval(S.times, S.nknots, tau);
        const double Tk = S.times[k], Tk1 = S.times[k + 1];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (S.val[f][c])
                    out[int64_t((stage * 2 + f) * 2 + c) * stride + col] = series_sample<FT>(S, stride, f, c, k, Tk, Tk1, tau, col);
    }
}

template <typename FT, int MODEL>
static void launch_series_column_stepper_for_model(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux, FT dt,
                                                   int64_t nsteps, const SeriesStepArgs& S, bool factors, bool percol,
                                                   bool noice, hipStream_t s) {
    // launch_column_stepper_for_model's shapes for the wave kernel (the caller keeps taller columns with the fused stages)
    const int cw = (P.nlev + 63) / 64;
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && factors && P.viscosity_kind;
    const int tiles = cs_fetch_tiles(MODEL, noice && !factors, need_Taux);
    const int narr = cs_exchange_arrays<MODEL>() + cs_flux_arrays<MODEL>();
    const size_t ex_words = size_t(narr) * 64 + CS_FACE_WORDS;
    const size_t tile_words = size_t(tiles) * size_t(P.nlev);
    const size_t dyn_col = (ex_words > tile_words ? ex_words : tile_words) * sizeof(FT);
    using M = MathFast<FT>;
    const bool ni = noice && noice_exists<M>(factors);
    const bool robust = robust_vg_exists<M, MODEL>() && P.vg_fast_all == 0;
    with_bool(factors, [&](auto f) { with_bool(percol, [&](auto pc) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<1, 2>{}, cw, [&](auto w) {
            constexpr bool F = decltype(f)::value, PC = decltype(pc)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            constexpr int CW = decltype(w)::value;
            if constexpr ((!NI || noice_exists<M>(F)) && (VG || robust_vg_exists<M, MODEL>())) {
                constexpr auto kernel = series_column_stepper_wave_kernel<FT, MODEL, F, PC, M, CW, NI, VG>;
                unsigned cpb = wave_stepper_columns<kernel>(P.ncols, dyn_col, nsteps);
                constexpr unsigned max_threads = series_stepper_max_threads<FT, MODEL, F, PC, M, CW, NI>();
                if (P.cs_cpb > 0 && (unsigned)P.cs_cpb * 64u <= max_threads) cpb = (unsigned)P.cs_cpb;
                const dim3 g((unsigned)((P.ncols + cpb - 1) / cpb)), b(64u * cpb);
                hipLaunchKernelGGL(kernel, g, b, (unsigned)(cpb * dyn_col), s, P, Y, aux, dt, nsteps, S);
            }
        });
    }); }); }); });
}

template <typename FT>
void launch_series_column_stepper(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux, FT dt, int64_t nsteps,
                                  const SeriesStepArgs& S, bool factors, bool percol, bool noice, hipStream_t s) {
    with_int(model_list{}, P.model, [&](auto m) {
        launch_series_column_stepper_for_model<FT, decltype(m)::value>(P, Y, aux, dt, nsteps, S, factors, percol, noice, s);
    });
}

template <typename FT>
void launch_series_stage_values(const DevParams<FT>& P, const SeriesStepArgs& S, int64_t step, FT* out, hipStream_t s) {
    hipLaunchKernelGGL((series_stage_values_kernel<FT>), grid_for(P.ncols, 256), dim3(256), 0, s, P.ncols, P.stride, S, step, out);
}

#define LH_INSTANTIATE_SERIES_STEPPER(FT)                                                                                     \
    template void launch_series_column_stepper<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&, FT, int64_t,   \
                                                   const SeriesStepArgs&, bool, bool, bool, hipStream_t);                     \
    template void launch_series_stage_values<FT>(const DevParams<FT>&, const SeriesStepArgs&, int64_t, FT*, hipStream_t);

} // namespace lh
#endif // LH_SERIES_STEPPER_TU
