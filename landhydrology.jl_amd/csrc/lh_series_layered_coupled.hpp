// lh_series_layered_coupled.hpp -- lh_integrate_layered_coupled_series: the adaptive TR-BDF2 of the coupled model with
// per-cell soil classes driven by a per-column boundary-value time series (lh_bc_series).
//
// lh_series.hpp's construction on layered_coupled_trbdf2_column: one launch stands for the chain of
// lh_integrate_layered_coupled_trbdf2 calls over the sub-intervals between the breakpoints; each lane fills a
// lane-local copy of the launch arguments per sub-interval (series_sub_interval) and calls the column routine
// UNCHANGED, so Y, the step proposals and status bit 0 are bitwise those of the chain by construction.
// lh_layered_coupled_trbdf2.hpp is not edited: its kernels keep their instructions.
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernel follows under
// LH_SERIES_LAYERED_COUPLED_TU, which only lh_kernels_f64_series_layered_coupled.hip /
// lh_kernels_f32_series_layered_coupled.hip define (with LH_SERIES_TU and lh_kernels_f64_layered_coupled_trbdf2.hip's
// list).
#pragma once
#include "lh_series.hpp"
#include "lh_layered_coupled_trbdf2.hpp"

namespace lh {

template <typename FT>
void launch_series_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                          const SeriesArgs& S, bool noice, hipStream_t s);

} // namespace lh

#ifdef LH_SERIES_LAYERED_COUPLED_TU
#if !defined(LH_SERIES_TU) || !defined(LH_LAYERED_COUPLED_TRBDF2_TU)
#error "lh_series_layered_coupled.hpp's kernel needs lh_series.hpp's per-lane pieces and layered_coupled_trbdf2_column (define LH_SERIES_TU and lh_kernels_f64_layered_coupled_trbdf2.hip's list first)"
#endif

namespace lh {

// layered_coupled_trbdf2_kernel's variants, launch bounds and table stagings (every thread of the workgroup reaches
// all three barriers, and no lane leaves before the statistics' reduction)
template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
series_layered_coupled_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const CoupledTrbdf2Args<FT> A,
                                     const SeriesArgs S) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const ClassView<FT> C{s_cls, L.cls};
    const ThermTable<FT> H{s_th, L.any_om != 0};
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    bool nonfinite = false;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        CoupledTrbdf2Args<FT> B = A;
        for (int j = 0; j < S.nsub; ++j) {
            series_sub_interval(A, S, j, col, B);
            Trbdf2ColStats st;
            layered_coupled_trbdf2_column<FT, M, NOICE, VGF>(mm, Pl, C, H, B, col, st, nonfinite);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats); // (slot 6 stays 0: the coupled column counts no unconverged steps)
}

template <typename FT>
void launch_series_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                          const SeriesArgs& S, bool noice, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((series_layered_coupled_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S);
    });
}

#define LH_INSTANTIATE_SERIES_LAYERED_COUPLED(FT)                                                                          \
    template void launch_series_layered_coupled_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,               \
                                                           const CoupledTrbdf2Args<FT>&, const SeriesArgs&, bool, hipStream_t);

} // namespace lh
#endif // LH_SERIES_LAYERED_COUPLED_TU
