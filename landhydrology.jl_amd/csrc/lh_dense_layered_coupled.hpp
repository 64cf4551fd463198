// lh_dense_layered_coupled.hpp -- lh_integrate_layered_coupled_dense: the adaptive TR-BDF2 of the coupled model with
// per-cell soil classes with output at given times, interpolated inside the launch from the steps the columns accept
// (DESIGN.md section 4.30).
//
// lh_dense.hpp's construction on the series kernel of lh_series_layered_coupled.hpp: the kernel below is that kernel
// -- the same variants, launch bounds, table stagings and __syncthreads() discipline -- with the bare sub-interval
// loop replaced by dense_walk and layered_coupled_trbdf2_column's accepted-step functor lh_dense.hpp's
// DenseOutput<FT, true> over the planes of CoupledTrbdf2Args (its energy overload of dense_output, unchanged).
// Without a series there is one sub-interval and no table (lh_integrate_layered_coupled_trbdf2 with bcv = NULL).
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernel follows under
// LH_DENSE_LAYERED_COUPLED_TU, which only lh_kernels_f64_dense_layered_coupled.hip /
// lh_kernels_f32_dense_layered_coupled.hip define (with lh_kernels_f64_series_layered_coupled.hip's list and
// LH_DENSE_OUTPUT_TU for lh_dense.hpp's per-lane pieces).
#pragma once
#include "lh_dense.hpp"
#include "lh_series_layered_coupled.hpp"

namespace lh {

// S.times == nullptr: no series (one sub-interval, A as the plain call fills it)
template <typename FT>
void launch_dense_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                         const SeriesArgs& S, const DenseArgs<FT>& D, bool noice, hipStream_t s);

} // namespace lh

#ifdef LH_DENSE_LAYERED_COUPLED_TU
#if !defined(LH_DENSE_OUTPUT_TU) || !defined(LH_SERIES_TU) || !defined(LH_LAYERED_COUPLED_TRBDF2_TU)
#error "lh_dense_layered_coupled.hpp's kernel needs lh_dense.hpp's and lh_series.hpp's per-lane pieces and layered_coupled_trbdf2_column (define LH_DENSE_OUTPUT_TU, LH_SERIES_TU and lh_kernels_f64_layered_coupled_trbdf2.hip's list first)"
#endif

namespace lh {

// series_layered_coupled_trbdf2_kernel's variants, launch bounds and table stagings (every thread of the workgroup
// reaches all three barriers, and no lane leaves before the statistics' reduction)
template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
dense_layered_coupled_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const CoupledTrbdf2Args<FT> A,
                                    const SeriesArgs S, const DenseArgs<FT> D) {
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
        dense_walk<FT>(P, A, S, D, col, tot, [&](const CoupledTrbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            layered_coupled_trbdf2_column<FT, M, NOICE, VGF>(mm, Pl, C, H, B, col, st, nonfinite, out);
        });
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats); // (slot 6 stays 0: the coupled column counts no unconverged steps)
}

template <typename FT>
void launch_dense_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                         const SeriesArgs& S, const DenseArgs<FT>& D, bool noice, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((dense_layered_coupled_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S, D);
    });
}

#define LH_INSTANTIATE_DENSE_LAYERED_COUPLED(FT)                                                                           \
    template void launch_dense_layered_coupled_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,                \
                                                          const CoupledTrbdf2Args<FT>&, const SeriesArgs&,                 \
                                                          const DenseArgs<FT>&, bool, hipStream_t);

} // namespace lh
#endif // LH_DENSE_LAYERED_COUPLED_TU
