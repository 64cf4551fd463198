// lh_heat_implicit.hpp -- backward-Euler and fixed-step TR-BDF2 steps (lh_step_heat_implicit) of the
// heat-only model, SoilEnergyModel + PrescribedHydrologyModel (right_hand_side.jl:192-263), on gfx950.
//
// With vartheta_l and theta_i prescribed, rho_c_s and kappa are constants of a call, T is affine in
// rhoe_int (T_i = alpha_i rhoe_i + beta_i, alpha_i = 1 / rho_c_s) and every energy face gives a flux
// affine in its cells' T.  So f(Y, t) = A Y + b(t), a stage equation Y - w - c f(Y) = 0 is the
// tridiagonal system (I - c A) Y = w + c b(t), and A does not depend on the boundary VALUES: the matrix
// is factored once per call, and a stage is one forward and one back substitution.  No Newton iteration, no
// convergence flag.
//
// One lane owns one column (every per-level access of a wave is one coalesced row), all steps of a call
// run in one launch, as implicit_euler_kernel.  With G_i = c (kappa_i + kappa_i+1) cg2
// the conductance of the face above cell i (rhs_kernel's grouping: lower cell first, (1/2)/dz^2 folded) and
// G_b, G_t = c kappa_face (2/dz)(1/dz) those of Dirichlet boundary faces (0 for the other kinds), the stage
// in u_i = alpha_i Y_i is the symmetric system
//   rho_c_s,i u_i + G_i-1 (u_i - u_i-1) + G_i (u_i - u_i+1) [+ G_b u_0] [+ G_t u_n-1] = r_i,
//   r_i = w_i + c [g_i-1 (beta_i-1 - beta_i) + g_i (beta_i+1 - beta_i)] + c (boundary flux at T_c = beta),
// the bracket a constant of the call (plane kc), the boundary term a constant of the stage.  G / rho_c_s is
// 1e3..1e4 at a thousand stable steps, so the textbook pivot b_i - a_i c'_i-1 cancels that many eps away
// (in Float32 nothing of the "1" of I - c A, which carries the conserved energy, is left).  The
// elimination here has no subtraction: with s_i the pivot without its upper conductance,
//   s_0 = rho_c_s,0 + G_b,   s_i = rho_c_s,i + G_i-1 s_i-1 / den_i-1 [+ G_t],   den_i = s_i + G_i,
//   forward r'_i = r_i + (G_i-1 / den_i-1) r'_i-1,   back u_i = (r'_i + G_i u_i+1) / den_i
// -- sums and products of positive numbers only, so the solve is accurate to a few eps per level whatever
// the step (the matrix is an M-matrix: its inverse is non-negative).  Stored per cell, folded back to
// Y = rho_c_s u: the multiplier G_i-1 / den_i-1, rho_c_s,i / den_i and G_i alpha_i+1 rho_c_s,i / den_i.
#pragma once
#include "lh_kernels_impl.hpp" // grid_for; with it lh_column_ops.hpp (implicit_threads, implicit_math, implicit_lane_column),
                               // lh_closures.hpp, lh_launch.hpp, lh_dispatch.hpp (with_bool), lh_fastmath.hpp (with_math)
                               // and lh_device.hpp (HeatImplicitArgs)

namespace lh {

// the energy flux of one boundary face in tendency units, as rhs_kernel forms it: boundary_fluxes_from / dz
template <typename FT>
__device__ __forceinline__ FT heat_boundary_flux(const DevParams<FT>& P, const FaceState<FT>& fs, int face, int64_t col,
                                                 FT T_c) {
    FT fe, fw;
    boundary_fluxes_from<FT, MODEL_HEAT>(P, fs, face, col, T_c, FT(0), FT(0), fe, fw);
    return fe * P.inv_dz;
}

// One column (lane) through the prologue and all steps of the call; nf_acc becomes NaN once a result is
// non-finite.
template <typename FT, typename M, bool PERCOL, bool TRBDF2>
__device__ __forceinline__ void heat_implicit_column(const M& mm, DevParams<FT> P, const HeatImplicitArgs<FT>& A,
                                                     int64_t col, FT& nf_acc) {
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const int64_t top = int64_t(n - 1) * stride + col;
    const FT coef = A.coef; // dt, or d dt of both TR-BDF2 stages
    const ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    FT* const y = A.y;
    FT* const z = A.z;

    // ---------------- prologue: the closures of every cell (once), the factorisation of the stage matrix
    // T of rhoe_int = 0 is the offset beta; alpha is the reciprocal temperature_closure itself forms
    auto cell = [&](int64_t id, FT& alpha, FT& beta, FT& kap, FT& rcs) {
        const FT vl = A.vl[id], ti = A.ti[id];
        beta = temperature_closure<FT, M>(mm, P, c, vl, ti, FT(0), rcs);
        alpha = M::is_production ? mm.rcp(rcs) : FT(1) / rcs;
        kap = kappa_closure<FT, M>(mm, P, c, vl, ti);
    };
    // the Dirichlet face states read the prescribed boundary cell only: kappa(face) is a constant of the
    // call, FaceState::T follows the boundary value (faces_at)
    FaceState<FT> fsb = face_state<FT, M, MODEL_HEAT, false>(mm, P, c, FACE_BOTTOM, col, A.vl[col], A.ti[col], FT(0));
    FaceState<FT> fst = face_state<FT, M, MODEL_HEAT, false>(mm, P, c, FACE_TOP, col, A.vl[top], A.ti[top], FT(0));
    const FT inv_dzb = FT(2) * P.inv_dz;
    const FT Gb = P.bc_kind[FACE_BOTTOM][COMP_ENERGY] == BC_DIRICHLET ? (fsb.kap * inv_dzb) * P.inv_dz : FT(0);
    const FT Gt = P.bc_kind[FACE_TOP][COMP_ENERGY] == BC_DIRICHLET ? (fst.kap * inv_dzb) * P.inv_dz : FT(0);
    FT beta_b, beta_t = FT(0); // beta of the two boundary cells
    {
        FT al, be, kap, rc, be_lo = FT(0);
        cell(col, al, be, kap, rc);
        beta_b = be;
        FT g_lo = FT(0);                     // g of the face below the cell (interior faces)
        FT s_prev = FT(0), iden_prev = FT(0); // s and 1 / den of the cell below
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            FT al_u = FT(0), be_u = FT(0), kap_u = FT(0), rc_u = FT(0), ks = FT(0), g_hi = FT(0);
            if (i + 1 < n) {
                cell(idx + stride, al_u, be_u, kap_u, rc_u);
                ks = kap + kap_u;     // rhs_kernel's interior face: -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2)
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
        // f(Y_n, t) is rhs_kernel's tendency (its faces, its grouping), evaluated in stage 1's forward sweep
        // from the planes of the prologue: a step is a function of (Y_n, the boundary values) alone, so a
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
            // the tendency at t.  With T = alpha rhoe + beta, a face reads T_hi - T_lo as (alpha rhoe)_hi -
            // (alpha rhoe)_lo plus the constant beta_hi - beta_lo, and a Dirichlet face is its flux at T_c = beta
            // minus G alpha rhoe: rhs_kernel's fluxes without rounding the absolute temperatures (|T - beta| is
            // some 10 K where T is near 280 K: in Float32 the difference keeps four more bits)
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
                    const FT f = Flo - Fhi; // rhs_kernel's emit
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

template <typename FT, typename M, bool PERCOL, bool TRBDF2>
__global__ void __launch_bounds__(implicit_threads<M>())
heat_implicit_kernel(const DevParams<FT> P, const HeatImplicitArgs<FT> A) {
    const M mm = implicit_math<M>(P.math_tab); // (every thread of the workgroup)
    const int64_t col = implicit_lane_column();
    if (col >= P.ncols) return;
    FT nf_acc = FT(0);
    heat_implicit_column<FT, M, PERCOL, TRBDF2>(mm, P, A, col, nf_acc);
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
}

template <typename FT>
void launch_heat_implicit(const DevParams<FT>& P, const HeatImplicitArgs<FT>& A, bool percol, bool trbdf2, int math,
                          hipStream_t s) {
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_bool(percol, [&](auto pc) { with_bool(trbdf2, [&](auto tr) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((heat_implicit_kernel<FT, M, decltype(pc)::value, decltype(tr)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    }); }); });
}

#define LH_INSTANTIATE_HEAT_IMPLICIT(FT) \
    template void launch_heat_implicit<FT>(const DevParams<FT>&, const HeatImplicitArgs<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
