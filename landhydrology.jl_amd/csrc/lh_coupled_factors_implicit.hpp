// lh_coupled_factors_implicit.hpp -- backward-Euler and fixed-step TR-BDF2 steps (lh_step_coupled_factors_implicit)
// of the coupled model, SoilEnergyModel + SoilHydrologyModel, whose hydrology has the IceImpedance factor and no
// viscosity factor.
//
// theta_i is constant and with TemperatureDependentViscosity off no closure of the water reads T, so f_w still does
// not read rhoe_int and f_e is still affine in rhoe_int: the impedance scales K, in the water's own fluxes and in the
// advected energy, and nothing else.  The stage Jacobian stays block lower-triangular and a stage is solved exactly by
//   1. the water stage: factors_newton_stage (lh_factors_implicit.hpp) on the coupled state's vartheta_l plane;
//   2. the energy stage: energy_sweep_up<FACTORS = true> (lh_coupled_implicit.hpp), one tridiagonal solve whose
//      advective entries A^lo, A^hi and right-hand side at T = beta carry the same K.
// The stage sequence is coupled_implicit_column's own, instantiated with FACTORS = true; the kernel is
// coupled_implicit_kernel's shape (one lane per column, all steps of a call in one launch, implicit_threads<M>(), its
// statistics reduction).  No NOICE variant: the impedance is a function of theta_i, so the plane is read whatever
// its zero bit says (section 4.32).
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernel follows under
// LH_COUPLED_FACTORS_IMPLICIT_TU, which only lh_kernels_f64_coupled_factors_implicit.hip /
// lh_kernels_f32_coupled_factors_implicit.hip define.
#pragma once
#include "lh_device.hpp"

namespace lh {

// percol, trbdf2, math: as launch_coupled_implicit's
template <typename FT>
void launch_coupled_factors_implicit(const DevParams<FT>& P, const CoupledImplicitArgs<FT>& A, bool percol, bool trbdf2,
                                     int math, hipStream_t s);

} // namespace lh

#ifdef LH_COUPLED_FACTORS_IMPLICIT_TU
// (the two translation units define LH_FACTORS_IMPLICIT_TU as well: that header's device text -- factors_newton_stage,
// factors_sweep_up, factors_face_states -- is then visible, and nothing of it is instantiated here)
#include "lh_factors_implicit.hpp" // (before lh_coupled_implicit.hpp, which only declares what it names of this one)
#include "lh_coupled_implicit.hpp" // coupled_implicit_column, energy_sweep_up

namespace lh {

template <typename FT, typename M, bool PERCOL, bool VGF, bool TRBDF2>
__global__ void __launch_bounds__(implicit_threads<M>())
coupled_factors_implicit_kernel(const DevParams<FT> P, const CoupledImplicitArgs<FT> A) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    FT nf_acc = FT(0);
    if (col < P.ncols)
        coupled_implicit_column<FT, M, PERCOL, false, VGF, TRBDF2, true>(mm, P, A, col, my_max, unconv, total, nf_acc);
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
    // (every lane of the wave gets here, those past the last column with zeros): one atomic per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        total += __shfl_xor(total, off, 64);
        unconv += __shfl_xor(unconv, off, 64);
        const int o = __shfl_xor(my_max, off, 64);
        my_max = o > my_max ? o : my_max;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (unconv) {
            atomicOr(P.status, 8u);
            atomicAdd(A.unconverged, unconv);
        }
        atomicAdd(A.total_iters, total);
        if (my_max > __atomic_load_n(A.max_iters, __ATOMIC_RELAXED)) atomicMax(A.max_iters, my_max);
    }
}

template <typename FT>
void launch_coupled_factors_implicit(const DevParams<FT>& P, const CoupledImplicitArgs<FT>& A, bool percol, bool trbdf2,
                                     int math, hipStream_t s) {
    with_factors_implicit_variant(P, percol, math, [&](auto m, auto pc, auto vg) { with_bool(trbdf2, [&](auto tr) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((coupled_factors_implicit_kernel<FT, M, decltype(pc)::value, decltype(vg)::value, decltype(tr)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    }); });
}

#define LH_INSTANTIATE_COUPLED_FACTORS_IMPLICIT(FT) \
    template void launch_coupled_factors_implicit<FT>(const DevParams<FT>&, const CoupledImplicitArgs<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
#endif // LH_COUPLED_FACTORS_IMPLICIT_TU
