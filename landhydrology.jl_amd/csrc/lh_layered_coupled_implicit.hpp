// lh_layered_coupled_implicit.hpp -- backward-Euler and fixed-step TR-BDF2 steps (lh_step_layered_coupled_implicit)
// of the coupled model, SoilEnergyModel + SoilHydrologyModel, with per-CELL soil classes and their thermal
// supplement.
//
// coupled_implicit_kernel (lh_coupled_implicit.hpp: one lane per column, all steps of a call in one launch, a stage
// solved exactly by the water's Newton followed by one tridiagonal solve for the energy at the new water state) with
// the constants of lh_layered_heat.hpp.  The block structure survives classes: f_w reads K and psi of vartheta_l and
// theta_i with the cell's own class and nothing of rhoe_int, and f_e stays affine in rhoe_int at fixed water
// (T = beta + alpha rhoe_int with the cell's own rho_c_s; kappa reads no temperature).
//   * The water stage is layered_newton_stage (lh_layered_implicit.hpp) on the vartheta_l plane with
//     layered_face_states, the instantiation layered_implicit_euler_kernel takes: vartheta_l after a backward-Euler
//     step is bitwise lh_step_layered_implicit_euler's on the Richards twin.
//   * The energy stage is energy_sweep_up with per-cell constants: beta, rho_c_s and alpha from
//     temperature_closure_cls at rhoe_int = 0, kappa from kappa_closure_cls, K the TRUE conductivity K_r Ksat of the
//     cell's class as layered_sweep_up forms it.  The interior face is layered_heat_rhs_kernel's: conductance
//     (kappa_lo + kappa_hi) cg2, advective parts rho_l c_l K_lo q and rho_l c_l K_hi q with q =
//     head_difference cg2 and the two cells' own conductivities; a Dirichlet energy face takes kappa from the
//     boundary cell's own class (boundary_fluxes_cls).  Column i of the stage matrix still sums to rho_c_s,i, now the
//     cell's own, so the transposed positive-sum recurrence (t_i, pi_i, r'_i) and the back substitution folded to
//     Y = rho_c_s u are lh_coupled_implicit.hpp's.
//
// A kernel family of its own, in its own translation units: lh_coupled_implicit.hpp, lh_layered_implicit.hpp and
// lh_layered_heat.hpp are not touched, so every kernel of theirs keeps its instructions
// (profiles/layered_coupled_implicit_manifest.txt).  The energy sweep and the time loop below are therefore copies of
// energy_sweep_up's and coupled_implicit_column's -- the rule of DESIGN section 4.14: shared text only where the
// existing kernels keep their instruction hashes.
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernels follow under
// LH_LAYERED_COUPLED_IMPLICIT_TU, which only lh_kernels_f64_layered_coupled_implicit.hip /
// lh_kernels_f32_layered_coupled_implicit.hip define (with LH_LAYERED_TU, LH_LAYERED_HEAT_TU and
// LH_LAYERED_IMPLICIT_TU, for the two table stagings, the two heat closures and the water stage).
#pragma once
#include "lh_layered_heat.hpp"
#include "lh_layered_implicit.hpp"

namespace lh {

// NOICE as launch_layered_implicit_euler's; the closure form (VGF) is the host's decision over all classes
// (P.vg_fast_all).  Production math, no conductivity factors.  trbdf2: both stages of a TR-BDF2 step per step
template <typename FT>
void launch_layered_coupled_implicit(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledImplicitArgs<FT>& A,
                                     bool noice, bool trbdf2, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_COUPLED_IMPLICIT_TU
#if !defined(LH_LAYERED_TU) || !defined(LH_LAYERED_HEAT_TU) || !defined(LH_LAYERED_IMPLICIT_TU)
#error "lh_layered_coupled_implicit.hpp's kernels need lh_layered.hpp's, lh_layered_heat.hpp's and lh_layered_implicit.hpp's (define LH_LAYERED_TU, LH_LAYERED_HEAT_TU and LH_LAYERED_IMPLICIT_TU first)"
#endif

namespace lh {

// the thermal table beside a ClassView's class table, and the host's decision on organic matter
template <typename FT>
struct ThermTable {
    const ThermC<FT>* th; // LDS, LH_LAYERED_MAX_CLASSES entries (stage_therm_table)
    bool any_om;
};

// the energy face state of one face at the water state the column holds (boundary_fluxes_cls): kappa of a Dirichlet
// energy face at the face's vartheta_l (the hydrology's Dirichlet value, else the boundary cell's own value) with
// the boundary cell's own class, FaceState::T the boundary value.  The energy reads no water closure of the face.
template <typename FT, typename M, bool NOICE>
__device__ __forceinline__ FaceState<FT> layered_energy_face(const M& mm, const DevParams<FT>& P, const ClassView<FT>& C,
                                                             const ThermTable<FT>& H, int face, int64_t col, int64_t id,
                                                             FT vl_c, FT ti_c) {
    const FaceBC<FT> bc = face_bc(P, face, col);
    FaceState<FT> fs;
    fs.K = fs.psi = fs.kap = fs.T = FT(0);
    if (bc.ke == BC_DIRICHLET) {
        const unsigned q = C.index(id);
        const FT vl_f = bc.kh == BC_DIRICHLET ? bc.vh : vl_c;
        fs.T = bc.ve;
        fs.kap = kappa_closure_cls<FT, M, NOICE>(mm, P, C.at(q), H.th[q], H.any_om, vl_f, ti_c);
    }
    return fs;
}

// energy_sweep_up (lh_coupled_implicit.hpp) with per-cell constants: one upward sweep of the energy equation over
// a column at the water state y (a rolling window of two cells' closures).  SOLVE: row i of the stage matrix and
// r_i = in(i, idx) + coef f_e,i(T = beta), eliminated forward; cp, dp receive the back substitution's
// Y_i = dp_i + cp_i Y_i+1.  Otherwise in(i, idx) is rhoe_int and out(idx, f_e,i) receives the tendency.  SOLVE with
// HOMOG: the same matrix against r_i = in(i, idx) alone (no tendency at T = beta, no boundary offset; the Dirichlet
// conductances stay in the pivots): the error filter of lh_layered_coupled_trbdf2.hpp, as energy_sweep_up's.
template <typename FT, typename M, bool NOICE, bool VGF, bool SOLVE, bool HOMOG = false, typename In, typename Out>
__device__ __forceinline__ void layered_energy_sweep_up(const M& mm, const DevParams<FT>& P, const ClassView<FT>& C,
                                                        const ThermTable<FT>& H, const FaceState<FT>& fsb,
                                                        const FaceState<FT>& fst, int64_t col, const FT* y, const FT* ti,
                                                        FT coef, FT* cp, FT* dp, FT& nf_acc, In&& in, Out&& out) {
    constexpr bool vgf = VGF && M::uses_tables;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    // K (the true conductivity), -psi as the water stage formed them; beta = T(rhoe_int = 0), alpha = 1 / rho_c_s; kappa
    auto cell = [&](int64_t id, FT& K, FT& np, FT& al, FT& be, FT& kap, FT& rcs) {
        const unsigned q = C.index(id);
        const ColC<FT>& c = C.at(q);
        const ThermC<FT>& th = H.th[q];
        const FT v = y[id];
        const FT tiv = NOICE ? FT(0) : ti[id];
        nf_acc = fma_ft(v, FT(0), nf_acc);
        FT Kr = FT(0);
        np = FT(0);
        water_closures<FT, M, false, true, false, NOICE, true, false, true>(mm, P, c, v, tiv, FT(288), Kr, np, nullptr, vgf);
        K = Kr * c.Ksat; // the two cells of a face may differ in Ksat (layered_sweep_up)
        be = temperature_closure_cls<FT, M, NOICE>(mm, P, c, th, v, tiv, FT(0), rcs);
        al = mm.rcp(rcs);
        kap = kappa_closure_cls<FT, M, NOICE>(mm, P, c, th, H.any_om, v, tiv);
    };
    // the energy flux of a boundary face at T_c = beta (the energy reads no water flux of the face)
    auto boundary = [&](const FaceState<FT>& fs, int face, FT be) {
        FT fe, fw;
        boundary_fluxes_from<FT, MODEL_HEAT>(P, fs, face, col, be, FT(0), FT(0), fe, fw);
        return fe * P.inv_dz;
    };
    const FT inv_dzb = FT(2) * P.inv_dz;
    const FT Gb = P.bc_kind[FACE_BOTTOM][COMP_ENERGY] == BC_DIRICHLET ? (fsb.kap * inv_dzb) * P.inv_dz : FT(0);
    const FT Gt = P.bc_kind[FACE_TOP][COMP_ENERGY] == BC_DIRICHLET ? (fst.kap * inv_dzb) * P.inv_dz : FT(0);
    int64_t idx = col;
    FT K, np, al, be, kap, rcs;
    cell(idx, K, np, al, be, kap, rcs);
    FT u = FT(0); // T - beta of the cell (tendency sweep)
    if constexpr (!SOLVE) u = al * in(0, idx);
    FT Flo = FT(0); // (the homogeneous solve reads no flux: the matrix alone)
    if constexpr (!HOMOG) Flo = boundary(fsb, FACE_BOTTOM, be) - Gb * u; // (a Dirichlet face is affine in T_c: - G_b u on top)
    FT p_lo = FT(0), l_lo = FT(0);                        // p_i-1 and l_i
    FT t_prev = FT(0), ipi_prev = FT(0), rp_prev = FT(0); // t, 1 / pi and r' of the cell below
    for (int i = 0; i < n; ++i) {
        FT Fhi = FT(0), p_hi = FT(0), l_up = FT(0);
        FT Ku = FT(0), npu = FT(0), alu = FT(0), beu = FT(0), kapu = FT(0), rcsu = FT(0), uu = FT(0);
        const int64_t idu = idx + stride;
        if (i + 1 < n) {
            cell(idu, Ku, npu, alu, beu, kapu, rcsu);
            // layered_heat_rhs_kernel's interior face: -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2) - (E_lo + E_hi) gh
            const FT gh = head_difference(npu, np, P.dz) * P.cg2;
            const FT ks = kap + kapu;
            if constexpr (SOLVE) {
                if constexpr (!HOMOG) {
                    const FT E = (P.rhocp_l * (be - P.T_ref)) * K, Eu = (P.rhocp_l * (beu - P.T_ref)) * Ku;
                    Fhi = -ks * ((beu - be) * P.cg2) - (E + Eu) * gh;
                }
                const FT g = ks * P.cg2;
                p_hi = coef * (g + (P.rhocp_l * Ku) * gh);
                l_up = coef * (g - (P.rhocp_l * K) * gh);
            } else {
                uu = alu * in(i + 1, idu);
                // T_hi - T_lo without rounding the absolute temperatures (lh_heat_implicit.hpp)
                const FT E = (P.rhocp_l * ((be - P.T_ref) + u)) * K, Eu = (P.rhocp_l * ((beu - P.T_ref) + uu)) * Ku;
                Fhi = -ks * (((uu - u) + (beu - be)) * P.cg2) - (E + Eu) * gh;
            }
        } else if constexpr (!HOMOG) {
            Fhi = boundary(fst, FACE_TOP, be) + Gt * u;
        }
        const FT f = Flo - Fhi; // layered_heat_rhs_kernel's emit
        if constexpr (SOLVE) {
            FT r = in(i, idx);
            if constexpr (!HOMOG) r = r + coef * f;
            FT tp = rcs; // the pivot without the entry below it: a column sum
            if (i == 0) tp = tp + coef * Gb;
            else tp = tp + p_lo * (t_prev * ipi_prev);
            if (i == n - 1) tp = tp + coef * Gt;
            const FT ipi = FT(1) / (tp + l_up);
            const FT rp = r + (l_lo * ipi_prev) * rp_prev;
            const FT ri = rcs * ipi; // folded back to Y = rho_c_s u
            dp[idx] = rp * ri;
            cp[idx] = (p_hi * alu) * ri;
            t_prev = tp;
            ipi_prev = ipi;
            rp_prev = rp;
            p_lo = p_hi;
            l_lo = l_up;
        } else {
            out(idx, f);
        }
        Flo = Fhi;
        K = Ku; np = npu; al = alu; be = beu; kap = kapu; rcs = rcsu; u = uu;
        idx = idu;
    }
}

// coupled_implicit_column (lh_coupled_implicit.hpp) with per-cell constants.  my_max, unconv, total: the water
// stages' Newton statistics; nf_acc becomes NaN once a result is non-finite.
template <typename FT, typename M, bool NOICE, bool VGF, bool TRBDF2>
__device__ __forceinline__ void layered_coupled_implicit_column(const M& mm, DevParams<FT> P, const ClassView<FT>& C,
                                                                const ThermTable<FT>& H, const CoupledImplicitArgs<FT>& A,
                                                                int64_t col, int& my_max, unsigned long long& unconv,
                                                                unsigned long long& total, FT& nf_acc) {
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const int64_t top = int64_t(n - 1) * stride + col;
    const FT coef = A.coef; // dt, or d dt of both TR-BDF2 stages
    FT* const y = A.y;
    FT* const e = A.e;
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    const FT ti_t = NOICE ? FT(0) : A.ti[top];
    // the water stage Y - w - coef f_w(Y) = 0 at the boundary values P holds: layered_newton_stage, as
    // layered_implicit_column
    auto water_stage = [&](auto wfirst) {
        FaceState<FT> fsb, fst;
        layered_face_states<FT, M, NOICE, VGF>(mm, P, C, col, ti_b, ti_t, fsb, fst);
        bool conv;
        const int it = layered_newton_stage<FT, M, NOICE, VGF, decltype(wfirst)::value, false>(
            mm, P, C, fsb, fst, col, y, A.ti, ti_b, A.w, A.cp, A.dp, coef, A.tol, FT(0), FT(0), A.max_iter, conv);
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    };
    auto energy_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        fsb = layered_energy_face<FT, M, NOICE>(mm, P, C, H, FACE_BOTTOM, col, col, y[col], ti_b);
        fst = layered_energy_face<FT, M, NOICE>(mm, P, C, H, FACE_TOP, col, top, y[top], ti_t);
    };
    // the energy stage Y - w - coef f_e(Y) = 0 at the water state y: w = in(i, idx), out(idx, Y_i) top down
    auto energy_stage = [&](auto&& in, auto&& out) {
        FaceState<FT> fsb, fst;
        energy_faces(fsb, fst);
        layered_energy_sweep_up<FT, M, NOICE, VGF, true>(mm, P, C, H, fsb, fst, col, y, A.ti, coef, A.cp, A.dp, nf_acc, in,
                                                         [](int64_t, FT) {});
        FT xnext = FT(0);
        int64_t idx = top;
        for (int i = n - 1; i >= 0; --i) {
            xnext = A.dp[idx] + A.cp[idx] * xnext;
            out(idx, xnext);
            idx -= stride;
        }
    };
    auto store_e = [&](int64_t idx, FT x) {
        e[idx] = x;
        nf_acc = fma_ft(x, FT(0), nf_acc);
    };
    const FT* bv = A.bcv; // sample k: bv[4 k + ..] = bottom energy, bottom water, top energy, top water

    if constexpr (!TRBDF2) {
        for (int64_t s = 0; s < A.nsteps; ++s) {
            if (bv) set_stage_boundary_values(P, bv + (s + 1) * 4);
            water_stage(std::true_type{});
            energy_stage([&](int, int64_t idx) { return e[idx]; }, store_e);
        }
    } else {
        // gamma = 2 - sqrt(2), d = gamma / 2 (coef = d dt), both components:
        //   stage 1: Y_g - w1 - coef f(Y_g, t + gamma dt) = 0,  w1 = Y_n + coef f_n
        //   stage 2: Y_1 - w2 - coef f(Y_1, t + dt) = 0,        w2 = (Y_g - (1-gamma)^2 Y_n) / (gamma (2-gamma))
        // f_n+1 = (Y_1 - w2) / coef is the next step's f_n: one tendency sweep per call, for the first step
        const double gam = 2.0 - 1.4142135623730951;
        const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
        const FT g1 = FT(gam), g0 = FT(1.0 - gam);
        const FT inv_coef = FT(1) / coef;
        FT* const yn = A.yn;
        FT* const fn = A.fn;
        FT* const fe = A.fe;
        FT* const we = A.we;
        FT* const w = A.w;
        {
            if (bv) set_stage_boundary_values(P, bv);
            FaceState<FT> fsb, fst;
            layered_face_states<FT, M, NOICE, VGF>(mm, P, C, col, ti_b, ti_t, fsb, fst);
            layered_sweep_up<FT, M, NOICE, VGF, false>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
                                                       [&](int64_t idx, FT, FT f) { fn[idx] = f; return FT(0); });
            FaceState<FT> eb, et;
            energy_faces(eb, et);
            layered_energy_sweep_up<FT, M, NOICE, VGF, false>(mm, P, C, H, eb, et, col, y, A.ti, coef, nullptr, nullptr, nf_acc,
                                                              [&](int, int64_t idx) { return e[idx]; },
                                                              [&](int64_t idx, FT f) { fe[idx] = f; });
        }
        for (int64_t s = 0; s < A.nsteps; ++s) {
            // stage 1: the water's Y_n and w1 (the guess is Y_n); boundary values (1 - gamma) v_k + gamma v_k+1
            int64_t idx = col;
            for (int i = 0; i < n; ++i) {
                const FT v = y[idx];
                yn[idx] = v;
                w[idx] = v + coef * fn[idx];
                idx += stride;
            }
            if (bv) {
                const FT* b0 = bv + s * 4;
                const FT* b1 = b0 + 4;
                P.bc_value[FACE_BOTTOM][COMP_ENERGY] = g0 * b0[0] + g1 * b1[0];
                P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = g0 * b0[1] + g1 * b1[1];
                P.bc_value[FACE_TOP][COMP_ENERGY] = g0 * b0[2] + g1 * b1[2];
                P.bc_value[FACE_TOP][COMP_HYDROLOGY] = g0 * b0[3] + g1 * b1[3];
            }
            water_stage(std::false_type{});
            // the energy's Y_g is not kept: the back substitution leaves w2 (rhoe_int still holds Y_n)
            energy_stage([&](int, int64_t id) { return e[id] + coef * fe[id]; },
                         [&](int64_t id, FT x) { we[id] = (x - c_yn * e[id]) * c_w2; });
            // stage 2: the guess is Y_g
            idx = col;
            for (int i = 0; i < n; ++i) {
                w[idx] = (y[idx] - c_yn * yn[idx]) * c_w2;
                idx += stride;
            }
            if (bv) set_stage_boundary_values(P, bv + (s + 1) * 4);
            water_stage(std::false_type{});
            energy_stage([&](int, int64_t id) { return we[id]; }, store_e);
            if (s + 1 < A.nsteps) { // f_n+1 = z_1 / h
                idx = col;
                for (int i = 0; i < n; ++i) {
                    fn[idx] = (y[idx] - w[idx]) * inv_coef;
                    fe[idx] = (e[idx] - we[idx]) * inv_coef;
                    idx += stride;
                }
            }
        }
    }
}

// implicit_math and both table stagings hold a __syncthreads(): every thread of the workgroup reaches all of them,
// and no lane leaves before the last one.  A lane past the last column does not return either: it skips the column
// and takes part in the wave's reduction of the Newton statistics with zeros (coupled_implicit_kernel).
template <typename FT, bool NOICE, bool VGF, bool TRBDF2>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
layered_coupled_implicit_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const CoupledImplicitArgs<FT> A) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, class_args(L), s_cls); // (as layered_implicit_euler_kernel: the same l2_por)
    stage_therm_table<FT>(L, s_th);
    const ClassView<FT> C{s_cls, L.cls};
    const ThermTable<FT> H{s_th, L.any_om != 0};
    const int64_t col = implicit_lane_column();
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    FT nf_acc = FT(0);
    if (col < P.ncols) layered_coupled_implicit_column<FT, M, NOICE, VGF, TRBDF2>(mm, P, C, H, A, col, my_max, unconv, total, nf_acc);
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
void launch_layered_coupled_implicit(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledImplicitArgs<FT>& A,
                                     bool noice, bool trbdf2, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) { with_bool(trbdf2, [&](auto tr) {
        hipLaunchKernelGGL((layered_coupled_implicit_kernel<FT, decltype(ni)::value, decltype(vg)::value, decltype(tr)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A);
    }); });
}

#define LH_INSTANTIATE_LAYERED_COUPLED_IMPLICIT(FT)                                                                 \
    template void launch_layered_coupled_implicit<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,             \
                                                      const CoupledImplicitArgs<FT>&, bool, bool, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_COUPLED_IMPLICIT_TU
