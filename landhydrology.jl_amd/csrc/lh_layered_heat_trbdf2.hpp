// lh_layered_heat_trbdf2.hpp -- adaptive TR-BDF2 (lh_integrate_layered_heat_trbdf2) of a heat-only model with
// per-CELL soil classes and their thermal supplement, on gfx950.
//
// heat_trbdf2_column (lh_heat_trbdf2.hpp: the prologue's stored constants, the factorisation inside stage 1's forward
// sweep, the homogeneous error solve, the controller, one lane per column with its own t and h) with the constants
// of lh_layered_heat_implicit.hpp: the class table and the thermal table in LDS beside the math tables, a cell's
// class byte read from the class plane, and beta, rho_c_s and kappa of a cell from temperature_closure_cls and
// kappa_closure_cls with the cell's own `c` and `th`.  An interior face stays (kappa_lo + kappa_hi) cg2 whatever the
// classes of its two cells; a Dirichlet energy face takes kappa from the boundary cell's own class.  The class plane
// is read in the prologue only: the time loop is the scalar kernel's text.
//
// A kernel family of its own, in its own translation units: lh_layered_heat_implicit.hpp and lh_layered_heat.hpp are
// not edited, so every kernel of theirs keeps its instructions (profiles/heat_trbdf2_manifest.txt).
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernels follow under
// LH_LAYERED_HEAT_TRBDF2_TU, which only lh_kernels_f64_layered_heat_trbdf2.hip / lh_kernels_f32_layered_heat_trbdf2.hip
// define (with LH_LAYERED_TU, LH_LAYERED_HEAT_TU, LH_LAYERED_HEAT_IMPLICIT_TU and LH_HEAT_TRBDF2_TU, for the two table
// stagings, the closures, ThermView and heat_trbdf2_column).
#pragma once
#include "lh_heat_trbdf2.hpp"
#include "lh_layered_heat_implicit.hpp"

namespace lh {

// Production math, theta_i read from Ya (no ice-free variant)
template <typename FT>
void launch_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_HEAT_TRBDF2_TU
#if !defined(LH_LAYERED_HEAT_IMPLICIT_TU) || !defined(LH_HEAT_TRBDF2_TU)
#error "lh_layered_heat_trbdf2.hpp's kernels need ThermView and heat_trbdf2_column (define LH_LAYERED_TU, LH_LAYERED_HEAT_TU, LH_LAYERED_HEAT_IMPLICIT_TU and LH_HEAT_TRBDF2_TU first)"
#endif

namespace lh {

// the constants of a cell from its own class: layered_heat_implicit_column's `cell` and `face`
template <typename FT, typename M>
struct LayeredHeatCells {
    const M& mm;
    const DevParams<FT>& P;
    const ThermView<FT>& C;
    bool any_om;
    const FT* vl;
    const FT* ti;
    int64_t col;
    __device__ __forceinline__ void cell(int64_t id, FT& alpha, FT& beta, FT& kap, FT& rcs) const {
        const unsigned q = C.index(id);
        const ColC<FT>& c = C.tab[q];
        const ThermC<FT>& th = C.th[q];
        const FT v = vl[id], i = ti[id];
        beta = temperature_closure_cls<FT, M, false>(mm, P, c, th, v, i, FT(0), rcs);
        alpha = mm.rcp(rcs);
        kap = kappa_closure_cls<FT, M, false>(mm, P, c, th, any_om, v, i);
    }
    __device__ __forceinline__ FT face_kappa(int face, int64_t id) const {
        if (face_bc(P, face, col).ke != BC_DIRICHLET) return FT(0);
        const unsigned q = C.index(id);
        return kappa_closure_cls<FT, M, false>(mm, P, C.tab[q], C.th[q], any_om, vl[id], ti[id]);
    }
};

// Both table stagings and implicit_math hold a __syncthreads(): every thread of the workgroup reaches all three, and
// no lane leaves before the statistics' reduction (a lane past the last column takes part in it with zeros).
template <typename FT>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
layered_heat_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const HeatTrbdf2Args<FT> A) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, false>(mm, class_args(L), s_cls); // (no water closure: nothing reads l2_por)
    stage_therm_table<FT>(L, s_th);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    bool nonfinite = false;
    if (col < P.ncols) {
        const ThermView<FT> V{s_cls, s_th, L.cls};
        const LayeredHeatCells<FT, M> C{mm, P, V, L.any_om != 0, A.vl, A.ti, col};
        heat_trbdf2_column<FT>(P, A, C, col, st, nonfinite);
    }
    heat_trbdf2_epilogue(st, nonfinite, P.status, A.stats);
}

template <typename FT>
void launch_layered_heat_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatTrbdf2Args<FT>& A,
                                hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    hipLaunchKernelGGL((layered_heat_trbdf2_kernel<FT>), grid_for(P.ncols, block), dim3(block), 0, s, P, L, A);
}

#define LH_INSTANTIATE_LAYERED_HEAT_TRBDF2(FT)                                                               \
    template void launch_layered_heat_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,           \
                                                 const HeatTrbdf2Args<FT>&, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_HEAT_TRBDF2_TU
