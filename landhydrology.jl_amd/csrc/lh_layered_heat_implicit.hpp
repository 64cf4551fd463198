// lh_layered_heat_implicit.hpp -- backward-Euler and fixed-step TR-BDF2 steps (lh_step_layered_heat_implicit) of
// a heat-only model with per-CELL soil classes and their thermal supplement.
//
// heat_implicit_kernel (lh_heat_implicit.hpp: one lane per column, all steps of a call in one launch, the stage
// matrix factored once per call without a subtraction) with the constants of lh_layered_heat.hpp: the class
// table and the thermal table in LDS beside the math tables, a cell's class byte read from the class plane, and
// beta, rho_c_s and kappa of a cell from temperature_closure_cls and kappa_closure_cls with the cell's own `c`
// and `th`.  An interior face stays (kappa_lo + kappa_hi) cg2, whatever the classes of its two cells
// (layered_heat_rhs_kernel's face); a Dirichlet energy face takes kappa from the boundary cell's own class
// (boundary_fluxes_cls).  The class plane is read in the prologue only: the time loop touches the planes the
// scalar kernel touches, so "solved" means solved against lh_rhs of the same context.
//
// A kernel family of its own, in its own translation units: lh_heat_implicit.hpp and lh_layered_heat.hpp are not
// touched, so every kernel of theirs keeps its instructions (profiles/layered_heat_implicit_manifest.txt).  The
// elimination and the time loop below are therefore copies of heat_implicit_column's -- the rule of DESIGN
// section 4.14: shared text only where the existing kernels keep their instruction hashes.
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernels follow under
// LH_LAYERED_HEAT_IMPLICIT_TU, which only lh_kernels_f64_layered_heat_implicit.hip /
// lh_kernels_f32_layered_heat_implicit.hip define (with LH_LAYERED_TU and LH_LAYERED_HEAT_TU, for
// stage_class_table, stage_therm_table and the two closures).
#pragma once
#include "lh_layered_heat.hpp"

namespace lh {

// Production math, theta_i read from Ya (no ice-free variant); trbdf2: both stages of a TR-BDF2 step per step
template <typename FT>
void launch_layered_heat_implicit(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatImplicitArgs<FT>& A,
                                  bool trbdf2, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_HEAT_IMPLICIT_TU
#if !defined(LH_LAYERED_TU) || !defined(LH_LAYERED_HEAT_TU)
#error "lh_layered_heat_implicit.hpp's kernels need lh_layered.hpp's and lh_layered_heat.hpp's (define LH_LAYERED_TU and LH_LAYERED_HEAT_TU first)"
#endif
#include "lh_heat_implicit.hpp" // heat_boundary_flux

namespace lh {

// what a lane needs to find a cell's constants: the two tables in LDS and the class plane
template <typename FT>
struct ThermView {
    const ColC<FT>* tab;  // LDS, LH_LAYERED_MAX_CLASSES entries (stage_class_table)
    const ThermC<FT>* th; // LDS, LH_LAYERED_MAX_CLASSES entries (stage_therm_table)
    const uint8_t* cls;   // class plane [nlev][stride]; pad columns hold class 0
    __device__ __forceinline__ unsigned index(int64_t id) const { return cls[id] & unsigned(LH_LAYERED_MAX_CLASSES - 1); }
};

// heat_implicit_column (lh_heat_implicit.hpp) with per-cell constants; nf_acc becomes NaN once a result is
// non-finite.
template <typename FT, typename M, bool TRBDF2>
__device__ __forceinline__ void layered_heat_implicit_column(const M& mm, DevParams<FT> P, const ThermView<FT>& C,
                                                             bool any_om, const HeatImplicitArgs<FT>& A, int64_t col,
                                                             FT& nf_acc) {
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const int64_t top = int64_t(n - 1) * stride + col;
    const FT coef = A.coef; // dt, or d dt of both TR-BDF2 stages
    FT* const y = A.y;
    FT* const z = A.z;

    // ---------------- prologue: the closures of every cell (once), the factorisation of the stage matrix
    // T of rhoe_int = 0 is the offset beta; alpha is the reciprocal temperature_closure_cls itself forms
    auto cell = [&](int64_t id, FT& alpha, FT& beta, FT& kap, FT& rcs) {
        const unsigned q = C.index(id);
        const ColC<FT>& c = C.tab[q];
        const ThermC<FT>& th = C.th[q];
        const FT vl = A.vl[id], ti = A.ti[id];
        beta = temperature_closure_cls<FT, M, false>(mm, P, c, th, vl, ti, FT(0), rcs);
        alpha = mm.rcp(rcs);
        kap = kappa_closure_cls<FT, M, false>(mm, P, c, th, any_om, vl, ti);
    };
    // the Dirichlet face states read the prescribed boundary cell only, with that cell's own class
    // (boundary_fluxes_cls): kappa(face) is a constant of the call, FaceState::T follows the boundary value (faces_at)
    auto face = [&](int f, int64_t id) {
        FaceState<FT> fs;
        fs.K = fs.psi = fs.kap = fs.T = FT(0);
        const unsigned q = C.index(id);
        if (face_bc(P, f, col).ke == BC_DIRICHLET)
            fs.kap = kappa_closure_cls<FT, M, false>(mm, P, C.tab[q], C.th[q], any_om, A.vl[id], A.ti[id]);
        return fs;
    };
    FaceState<FT> fsb = face(FACE_BOTTOM, col);
    FaceState<FT> fst = face(FACE_TOP, top);
    const FT inv_dzb = FT(2) * P.inv_dz;
    const FT Gb = P.bc_kind[FACE_BOTTOM][COMP_ENERGY] == BC_DIRICHLET ? (fsb.kap * inv_dzb) * P.inv_dz : FT(0);
    const FT Gt = P.bc_kind[FACE_TOP][COMP_ENERGY] == BC_DIRICHLET ? (fst.kap * inv_dzb) * P.inv_dz : FT(0);
    FT beta_b, beta_t = FT(0); // beta of the two boundary cells
    {
        FT al, be, kap, rc, be_lo = FT(0);
        cell(col, al, be, kap, rc);
        beta_b = be;
        FT g_lo = FT(0);                      // g of the face below the cell (interior faces)
        FT s_prev = FT(0), iden_prev = FT(0); // s and 1 / den of the cell below
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            FT al_u = FT(0), be_u = FT(0), kap_u = FT(0), rc_u = FT(0), ks = FT(0), g_hi = FT(0);
            if (i + 1 < n) {
                cell(idx + stride, al_u, be_u, kap_u, rc_u);
                ks = kap + kap_u;     // layered_heat_rhs_kernel's interior face: -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2)
                g_hi = ks * P.cg2;
            }
            const FT G_lo = coef * g_lo, G_hi = coef * g_hi;
            FT sp = rc; // the pivot without G_hi: positive terms only
            if (i == 0) sp = sp + coef * Gb;
            else sp = sp + G_lo * (s_prev * iden_prev);
            if (i == n - 1) sp = sp + coef * Gt;
            const FT iden = FT(1) / (sp + G_hi);
            const FT ri = rc * iden;
            FT k = FT(0); // (the boundary faces' share is added per stage: it carries the boundary value)
            if (i > 0) k = g_lo * (be_lo - be);
            if (i + 1 < n) k = k + g_hi * (be_u - be);
            A.a[idx] = i > 0 ? G_lo * iden_prev : FT(0);
            A.iden[idx] = ri;
            A.cp[idx] = (G_hi * al_u) * ri;
            A.kc[idx] = coef * k;
            if constexpr (TRBDF2) {
                A.ks[idx] = ks;
                A.al[idx] = al;
                A.be[idx] = be;
            }
            s_prev = sp;
            iden_prev = iden;
            beta_t = be;
            g_lo = g_hi; be_lo = be;
            al = al_u; be = be_u; kap = kap_u; rc = rc_u;
            idx += stride;
        }
    }

    // ---------------- from here on heat_implicit_column's text: the class plane is not read again
    // boundary values of one time: lh_set_bc's constants, or the two energy entries of a bcv sample
    // (per-column arrays take precedence inside face_bc, as everywhere)
    auto faces_at = [&](FT vb, FT vt) {
        if (A.bcv) {
            P.bc_value[FACE_BOTTOM][COMP_ENERGY] = vb;
            P.bc_value[FACE_TOP][COMP_ENERGY] = vt;
        }
        fsb.T = face_state_T<FT, MODEL_HEAT>(P, FACE_BOTTOM, col, FT(0));
        fst.T = face_state_T<FT, MODEL_HEAT>(P, FACE_TOP, col, FT(0));
    };
    // coef x the boundary faces' share of the affine constant: their fluxes at T_c = beta
    auto boundary_constants = [&](FT& kb, FT& kt) {
        kb = coef * heat_boundary_flux<FT>(P, fsb, FACE_BOTTOM, col, beta_b);
        kt = -(coef * heat_boundary_flux<FT>(P, fst, FACE_TOP, col, beta_t));
    };
    // forward elimination, r_i = w(i, idx) + kc_i + the boundary constants: r'_i = r_i + (G_i-1 / den_i-1) r'_i-1 to z
    auto forward = [&](FT kb, FT kt, auto&& w) {
        FT dprev = FT(0);
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            FT r = w(i, idx) + A.kc[idx];
            if (i == 0) r = r + kb;
            if (i == n - 1) r = r + kt;
            dprev = r + A.a[idx] * dprev;
            z[idx] = dprev;
            idx += stride;
        }
    };
    // back substitution Y_i = r'_i rho_c_s,i / den_i + (G_i alpha_i+1 rho_c_s,i / den_i) Y_i+1, top down; out(idx, Y_i) stores
    auto backward = [&](auto&& out) {
        FT xnext = FT(0);
        int64_t idx = top;
        for (int i = n - 1; i >= 0; --i) {
            xnext = z[idx] * A.iden[idx] + A.cp[idx] * xnext;
            out(idx, xnext);
            idx -= stride;
        }
    };
    auto store_y = [&](int64_t idx, FT x) {
        y[idx] = x;
        nf_acc = fma_ft(x, FT(0), nf_acc);
    };

    const FT* bv = A.bcv; // sample k: bv[4 k + 0] bottom energy, bv[4 k + 2] top energy
    if constexpr (!TRBDF2) {
        for (int64_t s = 0; s < A.nsteps; ++s) {
            if (bv) faces_at(bv[4 * (s + 1)], bv[4 * (s + 1) + 2]);
            else faces_at(FT(0), FT(0));
            FT kb, kt;
            boundary_constants(kb, kt);
            forward(kb, kt, [&](int, int64_t idx) { return y[idx]; });
            backward(store_y);
        }
    } else {
        // gamma = 2 - sqrt(2), d = gamma / 2 (coef = d dt):
        //   stage 1: (I - coef A) Y_g = Y_n + coef f(Y_n, t) + coef b(t + gamma dt)
        //   stage 2: (I - coef A) Y_1 = w2 + coef b(t + dt),  w2 = (Y_g - (1-gamma)^2 Y_n) / (gamma (2-gamma))
        // f(Y_n, t) is layered_heat_rhs_kernel's tendency (its faces, its grouping), evaluated in stage 1's forward
        // sweep from the planes of the prologue: a step is a function of (Y_n, the boundary values) alone, so a
        // call split in two gives the same bits
        const double gam = 2.0 - 1.4142135623730951;
        const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
        const FT g1 = FT(gam), g0 = FT(1.0 - gam);
        for (int64_t s = 0; s < A.nsteps; ++s) {
            FT vb0 = FT(0), vt0 = FT(0), vb1 = FT(0), vt1 = FT(0);
            if (bv) {
                vb0 = bv[4 * s]; vt0 = bv[4 * s + 2];
                vb1 = bv[4 * (s + 1)]; vt1 = bv[4 * (s + 1) + 2];
            }
            // the tendency at t, with T = alpha rhoe + beta kept apart as (alpha rhoe) and beta (heat_implicit_column)
            faces_at(vb0, vt0);
            const FT fb_n = heat_boundary_flux<FT>(P, fsb, FACE_BOTTOM, col, beta_b);
            const FT ft_n = heat_boundary_flux<FT>(P, fst, FACE_TOP, col, beta_t);
            FT kb, kt;
            faces_at(g0 * vb0 + g1 * vb1, g0 * vt0 + g1 * vt1);
            boundary_constants(kb, kt);
            {
                FT ay = A.al[col] * y[col], be = A.be[col];
                FT Flo = fb_n - Gb * ay;
                forward(kb, kt, [&](int i, int64_t idx) {
                    FT Fhi, ayu = FT(0), beu = FT(0);
                    if (i + 1 < n) {
                        const int64_t idu = idx + stride;
                        ayu = A.al[idu] * y[idu];
                        beu = A.be[idu];
                        Fhi = -A.ks[idx] * (((ayu - ay) + (beu - be)) * P.cg2);
                    } else {
                        Fhi = ft_n + Gt * ay;
                    }
                    const FT f = Flo - Fhi; // the tendency kernel's emit
                    Flo = Fhi;
                    ay = ayu;
                    be = beu;
                    return y[idx] + coef * f;
                });
            }
            backward([&](int64_t idx, FT x) { z[idx] = (x - c_yn * y[idx]) * c_w2; }); // Y_g -> w2
            faces_at(vb1, vt1);
            boundary_constants(kb, kt);
            forward(kb, kt, [&](int, int64_t idx) { return z[idx]; });
            backward(store_y);
        }
    }
}

// Both table stagings and implicit_math hold a __syncthreads(): every thread of the workgroup reaches all three
// before the lanes past the last column leave.
template <typename FT, typename M, bool TRBDF2>
__global__ void __launch_bounds__(implicit_threads<M>())
layered_heat_implicit_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const HeatImplicitArgs<FT> A) {
    static_assert(M::is_production, "the layered kernels exist for the production math only");
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, false>(mm, class_args(L), s_cls); // (no water closure: nothing reads l2_por)
    stage_therm_table<FT>(L, s_th);
    const int64_t col = implicit_lane_column();
    if (col >= P.ncols) return;
    const ThermView<FT> C{s_cls, s_th, L.cls};
    FT nf_acc = FT(0);
    layered_heat_implicit_column<FT, M, TRBDF2>(mm, P, C, L.any_om != 0, A, col, nf_acc);
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
}

template <typename FT>
void launch_layered_heat_implicit(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const HeatImplicitArgs<FT>& A,
                                  bool trbdf2, hipStream_t s) {
    using M = MathFast<FT>;
    constexpr int block = implicit_threads<M>();
    with_bool(trbdf2, [&](auto tr) {
        hipLaunchKernelGGL((layered_heat_implicit_kernel<FT, M, decltype(tr)::value>), grid_for(P.ncols, block), dim3(block), 0,
                           s, P, L, A);
    });
}

#define LH_INSTANTIATE_LAYERED_HEAT_IMPLICIT(FT)                                                                  \
    template void launch_layered_heat_implicit<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,              \
                                                   const HeatImplicitArgs<FT>&, bool, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_HEAT_IMPLICIT_TU
