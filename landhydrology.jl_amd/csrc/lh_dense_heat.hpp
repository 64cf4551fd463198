// lh_dense_heat.hpp -- lh_integrate_heat_dense: the adaptive TR-BDF2 of the heat-only model, without and with a class
// map, with output at given times interpolated inside the launch from the steps the columns accept (DESIGN.md
// section 4.30).
//
// lh_dense.hpp's construction on the series kernels of lh_series_heat.hpp: the kernels below are those kernels -- the
// same variants, launch bounds, table stagings and __syncthreads() discipline -- with the bare sub-interval loop
// replaced by dense_walk and heat_trbdf2_column's accepted-step functor a DenseOutput<FT, false> over the rhoe_int
// planes of HeatTrbdf2Args: y (Y_n+1), yn, fn and w (the stage-2 w2, from which the functor forms
// f_n+1 = (Y_n+1 - w2) / (d h) itself, also on the last step of a sub-interval, where the routine skips it).  The
// snapshots' rhoe_int planes travel in DenseArgs::snap_y; snap_e is unused.  Without a series there is one
// sub-interval and no table (lh_integrate_heat_trbdf2 / lh_integrate_layered_heat_trbdf2 with bcv = NULL).
//
// The first part (the launchers' declarations) is what lh_api.hip includes; the kernels follow under
// LH_DENSE_HEAT_TU, which only lh_kernels_f64_dense_heat.hip / lh_kernels_f32_dense_heat.hip define (with
// lh_kernels_f64_series_heat.hip's list and LH_DENSE_OUTPUT_TU for lh_dense.hpp's per-lane pieces).
#pragma once
#include "lh_dense.hpp"
#include "lh_series_heat.hpp"

namespace lh {

// S.times == nullptr: no series (one sub-interval, A as the plain call fills it)
template <typename FT>
void launch_dense_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, const SeriesArgs& S, const DenseArgs<FT>& D,
                              bool percol, int math, hipStream_t s);
template <typename FT>
void launch_dense_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                      const SeriesArgs& S, const DenseArgs<FT>& D, hipStream_t s);

} // namespace lh

#ifdef LH_DENSE_HEAT_TU
#if !defined(LH_DENSE_OUTPUT_TU) || !defined(LH_SERIES_TU) || !defined(LH_LAYERED_HEAT_TRBDF2_TU)
#error "lh_dense_heat.hpp's kernels need lh_dense.hpp's and lh_series.hpp's per-lane pieces and the heat CELLS objects (define LH_DENSE_OUTPUT_TU, LH_SERIES_TU and lh_kernels_f64_layered_heat_trbdf2.hip's list first)"
#endif

namespace lh {

// the heat-only column's output: its one prognostic variable in the place of vartheta_l
template <typename FT>
__device__ __forceinline__ DenseOutput<FT, false> dense_output(const DenseArgs<FT>& D, const DevParams<FT>& P,
                                                               const HeatTrbdf2Args<FT>& A, int64_t col, int& next,
                                                               double& s_next) {
    return {D, A.y, A.yn, A.fn, A.w, nullptr, nullptr, nullptr, nullptr, col, P.stride, P.nlev, next, s_next};
}

// series_heat_trbdf2_kernel's variants and launch bounds
template <typename FT, typename M, bool PERCOL>
__global__ void __launch_bounds__(implicit_threads<M>())
dense_heat_trbdf2_kernel(const DevParams<FT> P, const HeatTrbdf2Args<FT> A, const SeriesArgs S, const DenseArgs<FT> D) {
    const M mm = implicit_math<M>(P.math_tab); // (every thread of the workgroup)
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    bool nonfinite = false;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        const ColC<FT> c = make_colc<FT, M>(Pl, col, PERCOL);
        const HeatCells<FT, M> C{mm, Pl, c, A.vl, A.ti, col};
        dense_walk<FT>(P, A, S, D, col, tot, [&](const HeatTrbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            heat_trbdf2_column<FT>(Pl, B, C, col, st, nonfinite, out);
        });
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats);
}

// series_layered_heat_trbdf2_kernel's: both table stagings and implicit_math hold a __syncthreads(), every thread of
// the workgroup reaches all three, and no lane leaves before the statistics' reduction
template <typename FT>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
dense_layered_heat_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const HeatTrbdf2Args<FT> A,
                                 const SeriesArgs S, const DenseArgs<FT> D) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, false>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    bool nonfinite = false;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        const ThermView<FT> V{s_cls, s_th, L.cls};
        const LayeredHeatCells<FT, M> C{mm, Pl, V, L.any_om != 0, A.vl, A.ti, col};
        dense_walk<FT>(P, A, S, D, col, tot, [&](const HeatTrbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            heat_trbdf2_column<FT>(Pl, B, C, col, st, nonfinite, out);
        });
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT>
void launch_dense_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, const SeriesArgs& S, const DenseArgs<FT>& D,
                              bool percol, int math, hipStream_t s) {
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_bool(percol, [&](auto pc) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((dense_heat_trbdf2_kernel<FT, M, decltype(pc)::value>), grid_for(P.ncols, implicit_threads<M>()),
                           dim3(implicit_threads<M>()), 0, s, P, A, S, D);
    }); });
}

template <typename FT>
void launch_dense_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                      const SeriesArgs& S, const DenseArgs<FT>& D, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    hipLaunchKernelGGL((dense_layered_heat_trbdf2_kernel<FT>), grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S, D);
}

#define LH_INSTANTIATE_DENSE_HEAT(FT)                                                                                        \
    template void launch_dense_heat_trbdf2<FT>(const DevParams<FT>&, const HeatTrbdf2Args<FT>&, const SeriesArgs&,           \
                                               const DenseArgs<FT>&, bool, int, hipStream_t);                                \
    template void launch_dense_layered_heat_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,                     \
                                                       const HeatTrbdf2Args<FT>&, const SeriesArgs&, const DenseArgs<FT>&,   \
                                                       hipStream_t);

} // namespace lh
#endif // LH_DENSE_HEAT_TU
