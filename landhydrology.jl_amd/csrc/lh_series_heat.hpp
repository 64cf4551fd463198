// lh_series_heat.hpp -- lh_integrate_heat_series: the adaptive TR-BDF2 of the heat-only model, without and with a
// class map, driven by a per-column boundary-value time series (lh_bc_series).
//
// lh_series.hpp's construction on heat_trbdf2_column: one launch stands for the chain of lh_integrate_heat_trbdf2 /
// lh_integrate_layered_heat_trbdf2 calls over the sub-intervals between the breakpoints.  Each lane reads its two knot
// values of every (face, component) that has a series, fills a lane-local copy of the launch arguments
// (series_sub_interval) and calls heat_trbdf2_column UNCHANGED with the wrapped kernel's CELLS object -- so Y, the
// step proposals and status bit 0 are bitwise those of the chain by construction.  That includes the column's prologue
// (the closure sweep and the fresh f_n), which every sub-interval runs again: the price of the bitwise chain.
// lh_heat_trbdf2.hpp and lh_layered_heat_trbdf2.hpp are not edited: their kernels keep their instructions.
//
// The first part (the launchers' declarations) is what lh_api.hip includes; the kernels follow under
// LH_SERIES_HEAT_TU, which only lh_kernels_f64_series_heat.hip / lh_kernels_f32_series_heat.hip define (with
// LH_SERIES_TU for lh_series.hpp's per-lane pieces and the layered heat translation units' defines for the CELLS
// objects and the two table stagings).
#pragma once
#include "lh_series.hpp"
#include "lh_layered_heat_trbdf2.hpp" // with it lh_heat_trbdf2.hpp (HeatTrbdf2Args)

namespace lh {

template <typename FT>
void launch_series_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, const SeriesArgs& S, bool percol, int math,
                               hipStream_t s);
template <typename FT>
void launch_series_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                       const SeriesArgs& S, hipStream_t s);

} // namespace lh

#ifdef LH_SERIES_HEAT_TU
#if !defined(LH_SERIES_TU) || !defined(LH_LAYERED_HEAT_TRBDF2_TU)
#error "lh_series_heat.hpp's kernels need lh_series.hpp's per-lane pieces and the heat CELLS objects (define LH_SERIES_TU and lh_kernels_f64_layered_heat_trbdf2.hip's list first)"
#endif

namespace lh {

// heat_trbdf2_kernel's variants and launch bounds.  (The statistics' slots 2 and 6 get the zeros the column leaves
// in iters and unconv.)
template <typename FT, typename M, bool PERCOL>
__global__ void __launch_bounds__(implicit_threads<M>())
series_heat_trbdf2_kernel(const DevParams<FT> P, const HeatTrbdf2Args<FT> A, const SeriesArgs S) {
    const M mm = implicit_math<M>(P.math_tab); // (every thread of the workgroup)
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    bool nonfinite = false;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        const ColC<FT> c = make_colc<FT, M>(Pl, col, PERCOL);
        const HeatCells<FT, M> C{mm, Pl, c, A.vl, A.ti, col};
        HeatTrbdf2Args<FT> B = A;
        for (int j = 0; j < S.nsub; ++j) {
            series_sub_interval(A, S, j, col, B);
            Trbdf2ColStats st;
            heat_trbdf2_column<FT>(Pl, B, C, col, st, nonfinite);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats);
}

// layered_heat_trbdf2_kernel's: both table stagings and implicit_math hold a __syncthreads(), every thread of the
// workgroup reaches all three, and no lane leaves before the statistics' reduction
template <typename FT>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
series_layered_heat_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const HeatTrbdf2Args<FT> A,
                                  const SeriesArgs S) {
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
        HeatTrbdf2Args<FT> B = A;
        for (int j = 0; j < S.nsub; ++j) {
            series_sub_interval(A, S, j, col, B);
            Trbdf2ColStats st;
            heat_trbdf2_column<FT>(Pl, B, C, col, st, nonfinite);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT>
void launch_series_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, const SeriesArgs& S, bool percol, int math,
                               hipStream_t s) {
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_bool(percol, [&](auto pc) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((series_heat_trbdf2_kernel<FT, M, decltype(pc)::value>), grid_for(P.ncols, implicit_threads<M>()),
                           dim3(implicit_threads<M>()), 0, s, P, A, S);
    }); });
}

template <typename FT>
void launch_series_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                       const SeriesArgs& S, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    hipLaunchKernelGGL((series_layered_heat_trbdf2_kernel<FT>), grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S);
}

#define LH_INSTANTIATE_SERIES_HEAT(FT)                                                                                     \
    template void launch_series_heat_trbdf2<FT>(const DevParams<FT>&, const HeatTrbdf2Args<FT>&, const SeriesArgs&, bool,  \
                                                int, hipStream_t);                                                         \
    template void launch_series_layered_heat_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,                  \
                                                        const HeatTrbdf2Args<FT>&, const SeriesArgs&, hipStream_t);

} // namespace lh
#endif // LH_SERIES_HEAT_TU
