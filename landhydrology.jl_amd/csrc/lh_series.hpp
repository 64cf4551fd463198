// lh_series.hpp -- lh_integrate_series: the adaptive TR-BDF2 integrators driven by a per-column boundary-value
// time series (lh_bc_series).
//
// One launch stands for the chain of calls the host would make, one per sub-interval between the breakpoints
// t0, every knot strictly inside (t0, t1), t1.  Each lane walks its column through the sub-intervals: it reads
// its two knot values of every (face, component) that has a series, fills a lane-local copy of the launch
// arguments (t0, t1, the eight boundary values, has_bcv = 1) and calls trbdf2_column / layered_trbdf2_column /
// coupled_trbdf2_column UNCHANGED -- so Y, the step proposals and the status bits are bitwise those of the
// chain by construction.  Nothing of lh_implicit.hpp, lh_layered_implicit.hpp or lh_coupled_trbdf2.hpp is
// touched: their kernels keep their instructions.
//
// The first part (the table's launch argument and the launchers' declarations) is what lh_api.hip includes;
// the kernels follow under LH_SERIES_TU, which only lh_kernels_f64_series.hip / lh_kernels_f32_series.hip
// define (with LH_LAYERED_TU and LH_LAYERED_IMPLICIT_TU, for the layered column routine).
#pragma once
#include "lh_layered_implicit.hpp" // LayeredArgs; with it lh_device.hpp (DevParams, Trbdf2Args, CoupledTrbdf2Args)

namespace lh {

// The forcing table of one call.  Always double, whatever the working type: the integrators interpolate their
// boundary values in double and round once.  Column-fastest: knot k of a per-column component is the row
// val[f][c] + k * knot_stride[f][c] of ncols doubles (knot_stride = the context's plane stride, col_varies = 1);
// a uniform component is nknots doubles (knot_stride = 1, col_varies = 0).
struct SeriesArgs {
    const double* times;        // [nknots], strictly increasing
    const double* val[2][2];    // [face][component], or nullptr: lh_set_bc's value (and per-column array) stays
    int64_t knot_stride[2][2];
    int32_t col_varies[2][2];
    int32_t k0;                 // the knot interval [T_k0, T_k0+1] that holds t0: sub-interval j lies in k0 + j
    int32_t nsub;               // sub-intervals of the call: interior knots + 1; k0 + nsub <= nknots - 1
};

template <typename FT>
void launch_series_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const SeriesArgs& S, bool percol, bool noice,
                          int math, hipStream_t s);
template <typename FT>
void launch_series_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A,
                                  const SeriesArgs& S, bool noice, hipStream_t s);
template <typename FT>
void launch_series_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, const SeriesArgs& S, bool percol,
                                  bool noice, int math, hipStream_t s);

} // namespace lh

#ifdef LH_SERIES_TU
#include "lh_coupled_trbdf2.hpp" // coupled_trbdf2_column; with it lh_implicit.hpp (trbdf2_column, with_implicit_variant)

namespace lh {

// The value of a series at t in its knot interval [Tk, Tk1] with the knot values vk, vk1: exactly the knot's
// value on a knot, v_k + (v_k+1 - v_k) ((t - T_k) / (T_k+1 - T_k)) in double in between
__device__ __forceinline__ double series_value(double t, double Tk, double Tk1, double vk, double vk1) {
    if (t == Tk) return vk;
    if (t == Tk1) return vk1;
    return vk + (vk1 - vk) * ((t - Tk) / (Tk1 - Tk));
}

// The lane's own parameter block: a (face, component) with a series reads neither lh_set_bc's value (the
// boundary table replaces it) nor its per-column array, which face_bc would let win
template <typename FT>
__device__ __forceinline__ void series_params(DevParams<FT>& P, const SeriesArgs& S) {
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (S.val[f][c]) P.bc_pc[f][c] = nullptr;
}

// Sub-interval j of the call in B (a lane-local copy of the launch's A, whose bcv holds lh_set_bc's values at
// both ends): its ends and the column's boundary values at them.  ARGS: Trbdf2Args, CoupledTrbdf2Args or (lh_series_heat.hpp)
// HeatTrbdf2Args -- any launch argument with t0, t1, bcv[8] and has_bcv, which the launch sets to 1.
template <typename ARGS>
__device__ __forceinline__ void series_sub_interval(const ARGS& A, const SeriesArgs& S, int j, int64_t col, ARGS& B) {
    const int k = S.k0 + j;
    const double Tk = S.times[k], Tk1 = S.times[k + 1];
    const double a = j == 0 ? A.t0 : Tk;
    const double b = j == S.nsub - 1 ? A.t1 : Tk1;
    B.t0 = a;
    B.t1 = b;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double* v = S.val[f][c];
            if (v) {
                const int64_t at = int64_t(k) * S.knot_stride[f][c] + (S.col_varies[f][c] ? col : int64_t(0));
                const double vk = v[at], vk1 = v[at + S.knot_stride[f][c]];
                B.bcv[2 * f + c] = series_value(a, Tk, Tk1, vk, vk1);
                B.bcv[4 + 2 * f + c] = series_value(b, Tk, Tk1, vk, vk1);
            }
        }
}

// One sub-interval's counters added to the call's: sums, and the column's total of attempted steps
__device__ __forceinline__ void series_add(Trbdf2ColStats& tot, const Trbdf2ColStats& st) {
    tot.accepted += st.accepted;
    tot.rejected += st.rejected;
    tot.iters += st.iters;
    tot.steps += st.steps;
    tot.unconv += st.unconv;
    tot.failed = st.failed; // (a failed column stops: the last sub-interval it ran decides)
}

// The statistics epilogue of trbdf2_kernel, layered_trbdf2_kernel and coupled_trbdf2_kernel (every lane of the wave
// gets here, those past the last column with zeros): one atomic per counter and wave
__device__ __forceinline__ void series_reduce_stats(const Trbdf2ColStats& st, uint32_t* status, unsigned long long* s) {
    unsigned long long acc = st.accepted, rej = st.rejected, its = st.iters, fl = st.failed, un = st.unconv;
    unsigned long long mx = st.steps;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        rej += __shfl_xor(rej, off, 64);
        its += __shfl_xor(its, off, 64);
        fl += __shfl_xor(fl, off, 64);
        un += __shfl_xor(un, off, 64);
        const unsigned long long o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(s + 0, acc);
        atomicAdd(s + 1, rej);
        atomicAdd(s + 2, its);
        if (mx > __atomic_load_n(s + 3, __ATOMIC_RELAXED)) atomicMax(s + 3, mx);
        if (fl) {
            atomicOr(status, 16u);
            atomicAdd(s + 4, fl);
        }
        atomicAdd(s + 5, 64ull * mx);
        if (un) {
            atomicOr(status, 8u);
            atomicAdd(s + 6, un);
        }
    }
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
series_trbdf2_kernel(const DevParams<FT> P, const Trbdf2Args<FT> A, const SeriesArgs S) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats tot;
    if (col < P.ncols) {
        DevParams<FT> Pl = P;
        series_params(Pl, S);
        Trbdf2Args<FT> B = A;
        for (int j = 0; j < S.nsub; ++j) {
            series_sub_interval(A, S, j, col, B);
            Trbdf2ColStats st;
            trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, Pl, B, col, st);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
series_layered_trbdf2_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Trbdf2Args<FT> A, const SeriesArgs S) {
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
        Trbdf2Args<FT> B = A;
        for (int j = 0; j < S.nsub; ++j) {
            series_sub_interval(A, S, j, col, B);
            Trbdf2ColStats st;
            layered_trbdf2_column<FT, M, NOICE, VGF>(mm, Pl, C, B, col, st);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    series_reduce_stats(tot, P.status, A.stats);
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
series_coupled_trbdf2_kernel(const DevParams<FT> P, const CoupledTrbdf2Args<FT> A, const SeriesArgs S) {
    const M mm = implicit_math<M>(P.math_tab);
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
            coupled_trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, Pl, B, col, st, nonfinite);
            series_add(tot, st);
            if (st.failed) break;
        }
    }
    if (nonfinite) atomicOr(P.status, 1u);
    series_reduce_stats(tot, P.status, A.stats); // (slot 6 stays 0: the coupled column counts no unconverged steps)
}

template <typename FT>
void launch_series_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const SeriesArgs& S, bool percol, bool noice,
                          int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((series_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, S);
    });
}

template <typename FT>
void launch_series_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A,
                                  const SeriesArgs& S, bool noice, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((series_layered_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A, S);
    });
}

template <typename FT>
void launch_series_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, const SeriesArgs& S, bool percol,
                                  bool noice, int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((series_coupled_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, S);
    });
}

#define LH_INSTANTIATE_SERIES(FT)                                                                                            \
    template void launch_series_trbdf2<FT>(const DevParams<FT>&, const Trbdf2Args<FT>&, const SeriesArgs&, bool, bool, int,  \
                                           hipStream_t);                                                                     \
    template void launch_series_layered_trbdf2<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Trbdf2Args<FT>&,      \
                                                   const SeriesArgs&, bool, hipStream_t);                                    \
    template void launch_series_coupled_trbdf2<FT>(const DevParams<FT>&, const CoupledTrbdf2Args<FT>&, const SeriesArgs&,    \
                                                   bool, bool, int, hipStream_t);

} // namespace lh
#endif // LH_SERIES_TU
