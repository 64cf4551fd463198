// lh_dense.hpp -- lh_integrate_dense: the adaptive TR-BDF2 integrators of lh_integrate_series with output at given
// times, interpolated inside the launch from the steps the columns accept.
//
// The kernels are the series kernels (lh_series.hpp) with one addition: the column routines' accepted-step functor
// (NoStepOutput in lh_implicit.hpp) is a DenseOutput here.  Between the step's ends (Y_n, f_n) and (Y_n+1, f_n+1) -- all
// four in the routine's planes when a step is accepted: yn, fn, y and (y - w) / (d h) -- it evaluates the cubic Hermite
// interpolant at every save time s with t < s <= t_new and stores it into that save time's snapshot planes.  It changes
// nothing the integration reads: no step is cut at a save time, Y, the step proposals, the status word and the
// statistics are bitwise those of the launch without output.  Each lane carries the index of its next save time
// through the whole call, across the sub-intervals of a series; without a series there is one sub-interval and no
// table (lh_integrate_trbdf2 / lh_integrate_layered_trbdf2 / lh_integrate_coupled_trbdf2 with bcv = NULL).
//
// The first part (the launch argument and the launchers' declarations) is what lh_api.hip includes.  The per-lane
// pieces (HermiteCoefficients, DenseOutput, dense_walk) follow under LH_DENSE_OUTPUT_TU, which the dense translation
// units of the other families define too (lh_dense_heat.hpp, lh_dense_layered_coupled.hpp);
// the kernels follow under LH_DENSE_TU, which only lh_kernels_f64_dense.hip / lh_kernels_f32_dense.hip define (with
// LH_SERIES_TU).
#pragma once
#include "lh_series.hpp" // SeriesArgs; with it lh_layered_implicit.hpp (LayeredArgs) and lh_device.hpp

namespace lh {

// The output of one call: nsave times (double, strictly increasing in [t0, t1]) and per written variable a table of
// nsave plane pointers, the snapshot states' planes [nlev][stride]
template <typename FT>
struct DenseArgs {
    const double* times;  // [nsave]
    FT* const* snap_y;    // [nsave] vartheta_l planes
    FT* const* snap_e;    // [nsave] rhoe_int planes (coupled), else nullptr
    int32_t nsave;
};

// S.times == nullptr: no series (one sub-interval, A as the plain call fills it)
template <typename FT>
void launch_dense_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const SeriesArgs& S, const DenseArgs<FT>& D,
                         bool percol, bool noice, int math, hipStream_t s);
template <typename FT>
void launch_dense_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A,
                                 const SeriesArgs& S, const DenseArgs<FT>& D, bool noice, hipStream_t s);
template <typename FT>
void launch_dense_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, const SeriesArgs& S,
                                 const DenseArgs<FT>& D, bool percol, bool noice, int math, hipStream_t s);

} // namespace lh

#if defined(LH_DENSE_TU) || defined(LH_DENSE_OUTPUT_TU)
#ifndef LH_SERIES_TU
#error "lh_dense.hpp's per-lane pieces need lh_series.hpp's (define LH_SERIES_TU first)"
#endif

namespace lh {

// The coefficients of the interpolant at theta = (s - t) / h in (0, 1], each rounded to FT once:
//   u = a0 y0 + a1 y1 + b (c (y1 - y0) + d0 f0 + d1 f1)
// with a0 = 1 - theta, a1 = theta, b = theta (theta - 1), c = 1 - 2 theta, d0 = (theta - 1) h, d1 = theta h
template <typename FT>
struct HermiteCoefficients {
    FT a0, a1, b, c, d0, d1;
    bool end; // theta == 1: Y_n+1 itself
    __device__ __forceinline__ HermiteCoefficients(double theta, double h)
        : a0(FT(1.0 - theta)), a1(FT(theta)), b(FT(theta * (theta - 1.0))), c(FT(1.0 - 2.0 * theta)),
          d0(FT((theta - 1.0) * h)), d1(FT(theta * h)), end(theta == 1.0) {}
    __device__ __forceinline__ FT operator()(FT y0, FT y1, FT f0, FT f1) const {
        const FT u = (a0 * y0 + a1 * y1) + b * ((c * (y1 - y0) + d0 * f0) + d1 * f1);
        return end ? y1 : u;
    }
};

// One lane's output through a call: `next` is the index of its first save time not yet written, `s_next` that time
// (+inf behind the last).  ENERGY: the coupled column, whose rhoe_int is written beside vartheta_l.
template <typename FT, bool ENERGY>
struct DenseOutput {
    const DenseArgs<FT>& D;
    const FT* y;  // Y_n+1 (the state's plane), Y_n, the step's f_n, the stage-2 w
    const FT* yn;
    const FT* fn;
    const FT* w;
    const FT* e;  // ... and the energy's
    const FT* en;
    const FT* fe;
    const FT* we;
    int64_t col, stride;
    int n;
    int& next;
    double& s_next;

    __device__ __forceinline__ void advance() const {
        ++next;
        s_next = next < D.nsave ? D.times[next] : double(INFINITY);
    }
    // the state as it stands into every snapshot up to `upto`: Y as passed (s == t0), or a failed column's kept state
    // (upto = +inf: all that are left -- s_next is +inf behind the last one, so the index bounds the loop, not the time)
    __device__ __forceinline__ void store_state(double upto) const {
        while (next < D.nsave && s_next <= upto) {
            FT* const sy = D.snap_y[next];
            FT* const se = ENERGY ? D.snap_e[next] : nullptr;
            int64_t id = col;
            for (int i = 0; i < n; ++i) {
                sy[id] = y[id];
                if (ENERGY) se[id] = e[id];
                id += stride;
            }
            advance();
        }
    }
    // the accepted step t -> tn of size hh (the column routines' call): the level loop runs only with a save pending
    __device__ __forceinline__ void operator()(double t, double tn, double hh) const {
        if (!(s_next <= tn)) return;
        const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
        const FT inv_dh = FT(1.0 / (dg * hh)); // (f_n+1 = (Y_n+1 - w2) / (d h), as the routines form the next step's f_n)
        do {
            const HermiteCoefficients<FT> H((s_next - t) / hh, hh);
            FT* const sy = D.snap_y[next];
            FT* const se = ENERGY ? D.snap_e[next] : nullptr;
            int64_t id = col;
            for (int i = 0; i < n; ++i) {
                const FT y1 = y[id];
                sy[id] = H(yn[id], y1, fn[id], (y1 - w[id]) * inv_dh);
                if (ENERGY) {
                    const FT e1 = e[id];
                    se[id] = H(en[id], e1, fe[id], (e1 - we[id]) * inv_dh);
                }
                id += stride;
            }
            advance();
        } while (s_next <= tn);
    }
};

template <typename FT>
__device__ __forceinline__ DenseOutput<FT, false> dense_output(const DenseArgs<FT>& D, const DevParams<FT>& P,
                                                               const Trbdf2Args<FT>& A, int64_t col, int& next, double& s_next) {
    return {D, A.y, A.yn, A.fn, A.w, nullptr, nullptr, nullptr, nullptr, col, P.stride, P.nlev, next, s_next};
}
template <typename FT>
__device__ __forceinline__ DenseOutput<FT, true> dense_output(const DenseArgs<FT>& D, const DevParams<FT>& P,
                                                              const CoupledTrbdf2Args<FT>& A, int64_t col, int& next,
                                                              double& s_next) {
    return {D, A.y, A.yn, A.fn, A.w, A.e, A.en, A.fe, A.we, col, P.stride, P.nlev, next, s_next};
}

// The lane's walk through the call's sub-intervals, the three kernels' common text: column(B, st, out) is the
// family's column routine on sub-interval B.  The snapshots at t0 come first; a column that fails stops, and every
// snapshot it has not written receives its kept state.
template <typename FT, typename ARGS, typename COLUMN>
__device__ __forceinline__ void dense_walk(const DevParams<FT>& P, const ARGS& A, const SeriesArgs& S, const DenseArgs<FT>& D,
                                           int64_t col, Trbdf2ColStats& tot, COLUMN&& column) {
    int next = -1;
    double s_next;
    ARGS B = A;
    const auto out = dense_output<FT>(D, P, B, col, next, s_next);
    out.advance();
    out.store_state(A.t0);
    for (int j = 0; j < S.nsub; ++j) {
        if (S.times) series_sub_interval(A, S, j, col, B);
        Trbdf2ColStats st;
        column(B, st, out);
        series_add(tot, st);
        if (st.failed) break;
    }
    if (tot.failed) out.store_state(double(INFINITY));
}

} // namespace lh
#endif // LH_DENSE_TU || LH_DENSE_OUTPUT_TU

#ifdef LH_DENSE_TU

namespace lh {

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
dense_trbdf2_kernel(const DevParams<FT> P, const Trbdf2Args<FT> A, const SeriesArgs S, const DenseArgs<FT> D) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        dense_walk<FT>(P, A, S, D, col, tot, [&](const Trbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, Pl, B, col, st, out);
        });
    }
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
dense_layered_trbdf2_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Trbdf2Args<FT> A, const SeriesArgs S,
                            const DenseArgs<FT> D) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls); // (every thread of the workgroup)
    const ClassView<FT> C{s_cls, L.cls};
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        dense_walk<FT>(P, A, S, D, col, tot, [&](const Trbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            layered_trbdf2_column<FT, M, NOICE, VGF>(mm, Pl, C, B, col, st, out);
        });
    }
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
dense_coupled_trbdf2_kernel(const DevParams<FT> P, const CoupledTrbdf2Args<FT> A, const SeriesArgs S, const DenseArgs<FT> D) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    bool nonfinite = false;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        dense_walk<FT>(P, A, S, D, col, tot, [&](const CoupledTrbdf2Args<FT>& B, Trbdf2ColStats& st, const auto& out) {
            coupled_trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, Pl, B, col, st, nonfinite, out);
        });
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats); // (slot 6 stays 0: the coupled column counts no unconverged steps)
}

template <typename FT>
void launch_dense_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const SeriesArgs& S, const DenseArgs<FT>& D,
                         bool percol, bool noice, int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((dense_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, S, D);
    });
}

template <typename FT>
void launch_dense_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A,
                                 const SeriesArgs& S, const DenseArgs<FT>& D, bool noice, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((dense_layered_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S, D);
    });
}

template <typename FT>
void launch_dense_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, const SeriesArgs& S,
                                 const DenseArgs<FT>& D, bool percol, bool noice, int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((dense_coupled_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, S, D);
    });
}

#define LH_INSTANTIATE_DENSE(FT)                                                                                             \
    template void launch_dense_trbdf2<FT>(const DevParams<FT>&, const Trbdf2Args<FT>&, const SeriesArgs&,                    \
                                          const DenseArgs<FT>&, bool, bool, int, hipStream_t);                               \
    template void launch_dense_layered_trbdf2<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Trbdf2Args<FT>&,       \
                                                  const SeriesArgs&, const DenseArgs<FT>&, bool, hipStream_t);               \
    template void launch_dense_coupled_trbdf2<FT>(const DevParams<FT>&, const CoupledTrbdf2Args<FT>&, const SeriesArgs&,     \
                                                  const DenseArgs<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
#endif // LH_DENSE_TU
