// lh_heat_trbdf2.hpp -- adaptive TR-BDF2 (lh_integrate_heat_trbdf2) of the heat-only model, SoilEnergyModel +
// PrescribedHydrologyModel, on gfx950.
//
// The method is trbdf2_column's (lh_implicit.hpp: the two stages, z = (Y - w) / d, the Hosea-Shampine estimate,
// the controller, one lane per column with its own t and h in double) on heat_implicit_column's linear algebra
// (lh_heat_implicit.hpp): with vartheta_l and theta_i prescribed the tendency is affine in rhoe_int,
// f(Y, t) = A Y + b(t), so a stage Y - w - c f(Y) = 0 with c = d hh is the tridiagonal system
// (I - c A) Y = w + c b(t): one exact solve, no Newton, no convergence question.  The error filter is that same
// matrix, e = (I - c A)^-1 (b1 hh f_n + b2 z_g + b3 z_1), solved homogeneously (no affine constant, no boundary
// constants, the Dirichlet conductances in the pivots): nothing of the stage Jacobian is dropped.
//
// Prologue, once per call and column: heat_implicit_column's closure sweep stores what does not depend on the step --
// rho_c_s, alpha = 1 / rho_c_s, the face sums kappa_i + kappa_i+1 and the affine constant
// k_i = g_i-1 (beta_i-1 - beta_i) + g_i (beta_i+1 - beta_i) WITHOUT its coef -- and, in the same sweep, the fresh
// tendency f_n(Y, t0) in heat_implicit_column's beta-difference form (so no plane of beta is kept: the sweep is
// beta's only reader).  The two Dirichlet conductances and the boundary cells' beta stay in registers.
//
// Per attempt c changes, so the no-subtraction elimination of section 4.15,
//   s_0 = rho_c_s,0 + c G_b,   s_i = rho_c_s,i + G_i-1 s_i-1 / den_i-1 [+ c G_t],   den_i = s_i + G_i,
// is recomputed inside stage 1's forward sweep (sums and products of positives only) and the three numbers the
// later sweeps read are stored per cell: the multiplier G_i-1 / den_i-1, rho_c_s,i / den_i and
// G_i alpha_i+1 rho_c_s,i / den_i.  Stage 2 and the error solve reuse them: all three systems have the same matrix.
//
// Plane passes per cell and attempt (FT words): stage 1 up 6 reads (Y, f_n, rho_c_s, kappa sum, k, alpha) + 5 writes
// (Y_n, the three of the factorisation, r'), down 4 + 2 (Y_g, w2); stage 2 up 3 + 1, down 3 + 1 (Y_1); error up 6 + 1,
// down 5 + 0; an accepted step 2 + 1 (f_n+1 = z_1 / hh), a rejected one 1 + 1 (Y restored from Y_n): 40 words,
// 320 bytes in Float64.
//
// A step is not bitwise splittable across calls: f_n is carried from step to step (first same as last) and a call's
// first f_n is a fresh tendency, as for the other adaptive integrators.
//
// heat_trbdf2_column takes the per-cell constants from a CELLS object, so the layered twin
// (lh_layered_heat_trbdf2.hpp) runs this text with class tables in LDS.  lh_heat_implicit.hpp is not edited.
//
// The first part (arguments, the launcher's declaration) is what lh_api.hip includes; the kernels follow under
// LH_HEAT_TRBDF2_TU, which only lh_kernels_f64_heat_trbdf2.hip / lh_kernels_f32_heat_trbdf2.hip (and the layered
// twin's translation units) define.
#pragma once
#include "lh_launch.hpp"

namespace lh {

// lh_integrate_heat_trbdf2's and lh_integrate_layered_heat_trbdf2's launch
template <typename FT>
struct HeatTrbdf2Args {
    FT* y;               // rhoe_int plane of Y: the column's state, and the candidate Y_1
    const FT* vl;        // vartheta_l and theta_i planes of Ya (prescribed: read by the prologue only)
    const FT* ti;
    FT* rc;              // scratch planes [nlev][stride], of the prologue: rho_c_s, alpha, kappa_i + kappa_i+1, k
    FT* al;
    FT* ks;
    FT* k;
    FT* a;               // ... of an attempt's factorisation: G_i-1 / den_i-1, rho_c_s / den, G alpha_i+1 rho_c_s / den
    FT* iden;
    FT* cp;
    FT* yn;              // ... and of the time loop: Y_n, f_n, Y_gamma, w2, r' of a forward sweep
    FT* fn;
    FT* yg;
    FT* w;
    FT* z;
    FT* dt_cols;         // [ncols] per-column step in / proposal out (0: failed), or nullptr
    double t0, t1, dt;   // the call's interval and the initial step
    double abstol_e, reltol;
    double bcv[8];       // [t0 | t1][2 faces][2 components], linear in between (has_bcv); hydrology entries unread
    int32_t has_bcv;
    unsigned long long* stats; // accepted, rejected, 0, max steps, failed, wave_steps, 0
};

template <typename FT>
void launch_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, bool percol, int math, hipStream_t s);

} // namespace lh

#ifdef LH_HEAT_TRBDF2_TU
#include "lh_heat_implicit.hpp" // heat_boundary_flux; with it lh_kernels_impl.hpp, lh_column_ops.hpp, lh_closures.hpp
#include "lh_implicit.hpp"      // trbdf2_clip, trbdf2_control, trbdf2_next_step

namespace lh {

// One column (lane) from t0 to t1.  CELLS: cell(id, alpha, beta, kappa, rho_c_s) of one cell and face_kappa(face, id),
// kappa of a Dirichlet energy face's state (0 for the other kinds).  nonfinite: an accepted result was not finite.
// output: the accepted-step functor (NoStepOutput in lh_implicit.hpp; lh_dense_heat.hpp's launches pass a DenseOutput).
template <typename FT, typename CELLS, typename OUT = NoStepOutput>
__device__ __forceinline__ void heat_trbdf2_column(const DevParams<FT>& P0, const HeatTrbdf2Args<FT>& A, const CELLS& C,
                                                   int64_t col, Trbdf2ColStats& st, bool& nonfinite, OUT output = OUT()) {
    DevParams<FT> P = P0; // (the lane's own: its boundary values are those of its own stage times)
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const int64_t top = int64_t(n - 1) * stride + col;
    const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
    const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
    const FT b1 = FT((1.0 - 1.4142135623730951) / 3.0), b2 = FT(1.0 / 3.0), b3 = FT((1.4142135623730951 - 2.0) / 3.0);
    const FT inv_d = FT(1.0 / dg);
    const FT atol_e = FT(A.abstol_e), rtol = FT(A.reltol);
    FT* const y = A.y;
    FT* const yn = A.yn;
    FT* const fn = A.fn;
    FT* const yg = A.yg;
    FT* const w = A.w;
    FT* const z = A.z;

    // the Dirichlet face states read the prescribed boundary cell only: kappa(face) is a constant of the call,
    // FaceState::T follows the boundary value (faces_at)
    FaceState<FT> fsb, fst;
    fsb.K = fsb.psi = fsb.T = FT(0);
    fst = fsb;
    fsb.kap = C.face_kappa(FACE_BOTTOM, col);
    fst.kap = C.face_kappa(FACE_TOP, top);
    const FT inv_dzb = FT(2) * P.inv_dz;
    const FT Gb = P.bc_kind[FACE_BOTTOM][COMP_ENERGY] == BC_DIRICHLET ? (fsb.kap * inv_dzb) * P.inv_dz : FT(0);
    const FT Gt = P.bc_kind[FACE_TOP][COMP_ENERGY] == BC_DIRICHLET ? (fst.kap * inv_dzb) * P.inv_dz : FT(0);
    // boundary values at time t: linear in t between the call's two ends, in double, rounded once (or lh_set_bc's
    // constants; per-column arrays take precedence inside face_bc, as everywhere)
    auto faces_at = [&](double t) {
        if (A.has_bcv) {
            const double s = A.t1 > A.t0 ? (t - A.t0) / (A.t1 - A.t0) : 1.0;
            P.bc_value[FACE_BOTTOM][COMP_ENERGY] = FT(A.bcv[0] + (A.bcv[4] - A.bcv[0]) * s);
            P.bc_value[FACE_TOP][COMP_ENERGY] = FT(A.bcv[2] + (A.bcv[6] - A.bcv[2]) * s);
        }
        fsb.T = face_state_T<FT, MODEL_HEAT>(P, FACE_BOTTOM, col, FT(0));
        fst.T = face_state_T<FT, MODEL_HEAT>(P, FACE_TOP, col, FT(0));
    };

    // ---------------- prologue: the closures of every cell (once), what does not depend on the step, and f_n(Y, t0)
    // in heat_implicit_column's form: with T = alpha rhoe + beta a face reads T_hi - T_lo as (alpha rhoe)_hi -
    // (alpha rhoe)_lo plus the constant beta_hi - beta_lo, a Dirichlet face is its flux at T_c = beta minus G alpha rhoe
    faces_at(A.t0);
    FT beta_b, beta_t = FT(0); // beta of the two boundary cells
    {
        FT al, be, kap, rc, be_lo = FT(0);
        C.cell(col, al, be, kap, rc);
        beta_b = be;
        FT ay = al * y[col];
        FT Flo = heat_boundary_flux<FT>(P, fsb, FACE_BOTTOM, col, beta_b) - Gb * ay;
        FT g_lo = FT(0); // g of the face below the cell (interior faces)
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            FT al_u = FT(0), be_u = FT(0), kap_u = FT(0), rc_u = FT(0), ks = FT(0), g_hi = FT(0), ay_u = FT(0), Fhi;
            if (i + 1 < n) {
                C.cell(idx + stride, al_u, be_u, kap_u, rc_u);
                ks = kap + kap_u; // rhs_kernel's interior face: -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2)
                g_hi = ks * P.cg2;
                ay_u = al_u * y[idx + stride];
                Fhi = -ks * (((ay_u - ay) + (be_u - be)) * P.cg2);
            } else {
                Fhi = heat_boundary_flux<FT>(P, fst, FACE_TOP, col, be) + Gt * ay;
            }
            fn[idx] = Flo - Fhi; // rhs_kernel's emit
            FT k = FT(0);        // (the boundary faces' share is added per stage: it carries the boundary value)
            if (i > 0) k = g_lo * (be_lo - be);
            if (i + 1 < n) k = k + g_hi * (be_u - be);
            A.rc[idx] = rc;
            A.al[idx] = al;
            A.ks[idx] = ks;
            A.k[idx] = k;
            beta_t = be;
            Flo = Fhi;
            g_lo = g_hi; be_lo = be;
            al = al_u; be = be_u; kap = kap_u; rc = rc_u; ay = ay_u;
            idx += stride;
        }
    }

    // c x the boundary faces' share of the affine constant at the boundary values P holds: their fluxes at T_c = beta
    auto boundary_constants = [&](FT c, FT& kb, FT& kt) {
        kb = c * heat_boundary_flux<FT>(P, fsb, FACE_BOTTOM, col, beta_b);
        kt = -(c * heat_boundary_flux<FT>(P, fst, FACE_TOP, col, beta_t));
    };
    // forward elimination with the stored multipliers, r'_i = r(i, idx) + (G_i-1 / den_i-1) r'_i-1 to z
    auto forward = [&](auto&& r) {
        FT dprev = FT(0);
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            dprev = r(i, idx) + A.a[idx] * dprev;
            z[idx] = dprev;
            idx += stride;
        }
    };
    // back substitution x_i = r'_i rho_c_s,i / den_i + (G_i alpha_i+1 rho_c_s,i / den_i) x_i+1, top down
    auto backward = [&](auto&& out) {
        FT xnext = FT(0);
        int64_t idx = top;
        for (int i = n - 1; i >= 0; --i) {
            xnext = z[idx] * A.iden[idx] + A.cp[idx] * xnext;
            out(idx, xnext);
            idx -= stride;
        }
    };

    double t = A.t0;
    double h = A.dt;
    if (A.dt_cols) {
        const double h0 = double(A.dt_cols[col]);
        if (h0 > 0) h = h0;
    }
    const double hmin = LH_TRBDF2_HMIN_FRAC * (A.t1 - A.t0);
    bool failed = false;
    while (t < A.t1) {
        if (st.accepted + st.rejected >= LH_TRBDF2_MAX_STEPS) { failed = true; break; } // (attempted steps)
        double hh;
        const bool clip = trbdf2_clip(t, A.t1, h, hh); // land on t1 exactly
        const FT c = FT(dg * hh);
        FT kb, kt;
        // stage 1: (I - c A) Y_g = Y_n + c f_n + c b(t + gamma hh).  The sweep factors the matrix of this attempt,
        // keeps Y_n and eliminates in one pass
        faces_at(t + gam * hh);
        boundary_constants(c, kb, kt);
        {
            const FT cGb = c * Gb, cGt = c * Gt;
            FT dprev = FT(0), s_prev = FT(0), iden_prev = FT(0), G_lo = FT(0);
            int64_t idx = col;
            for (int i = 0; i < n; ++i) {
                const FT rc = A.rc[idx];
                const FT G_hi = c * (A.ks[idx] * P.cg2); // (the top cell's kappa sum is 0)
                const FT al_u = i + 1 < n ? A.al[idx + stride] : FT(0);
                FT sp = rc; // the pivot without G_hi: positive terms only
                if (i == 0) sp = sp + cGb;
                else sp = sp + G_lo * (s_prev * iden_prev);
                if (i == n - 1) sp = sp + cGt;
                const FT iden = FT(1) / (sp + G_hi);
                const FT ri = rc * iden;
                const FT a = i > 0 ? G_lo * iden_prev : FT(0);
                A.a[idx] = a;
                A.iden[idx] = ri;
                A.cp[idx] = (G_hi * al_u) * ri;
                const FT v = y[idx];
                yn[idx] = v;
                FT r = (v + c * fn[idx]) + c * A.k[idx];
                if (i == 0) r = r + kb;
                if (i == n - 1) r = r + kt;
                dprev = r + a * dprev;
                z[idx] = dprev;
                s_prev = sp;
                iden_prev = iden;
                G_lo = G_hi;
                idx += stride;
            }
        }
        backward([&](int64_t idx, FT x) { // Y_g and w2 = (Y_g - (1-gamma)^2 Y_n) / (gamma (2-gamma))
            yg[idx] = x;
            w[idx] = (x - c_yn * yn[idx]) * c_w2;
        });
        // stage 2: (I - c A) Y_1 = w2 + c b(t + hh); the candidate goes to rhoe_int's own plane
        faces_at(t + hh);
        boundary_constants(c, kb, kt);
        forward([&](int i, int64_t idx) {
            FT r = w[idx] + c * A.k[idx];
            if (i == 0) r = r + kb;
            if (i == n - 1) r = r + kt;
            return r;
        });
        backward([&](int64_t idx, FT x) { y[idx] = x; });
        // the error estimate: (I - c A) e = b1 hh f_n + b2 z_g + b3 z_1 against the same factorisation, homogeneous;
        // the norm accumulates in double during the back substitution
        const FT hf = FT(hh);
        forward([&](int, int64_t idx) {
            const FT f0 = fn[idx];
            const FT zg = (yg[idx] - (yn[idx] + c * f0)) * inv_d;
            const FT z1 = (y[idx] - w[idx]) * inv_d;
            return b1 * (hf * f0) + b2 * zg + b3 * z1;
        });
        double sum = 0.0;
        backward([&](int64_t idx, FT ev) {
            const FT v0 = yn[idx], v1 = y[idx];
            const FT a0 = v0 < FT(0) ? -v0 : v0;
            const FT a1 = v1 < FT(0) ? -v1 : v1;
            const double q = double(ev) / double(atol_e + rtol * (a0 > a1 ? a0 : a1));
            sum += q * q;
        });
        double fac;
        const bool accept = trbdf2_control(sqrt(sum / n), fac);
        if (accept) {
            ++st.accepted;
            output(t, clip ? A.t1 : t + hh, hh); // (before t moves and f_n is overwritten: w is still w2)
            t = clip ? A.t1 : t + hh; // (assigned: the column lands on t1 exactly)
            h = trbdf2_next_step(h, hh, fac, clip);
            // the accepted result's finiteness and f_n+1 = z_1 / hh where a next step follows
            const bool more = t < A.t1;
            const FT inv_dh = FT(1.0 / (dg * hh));
            int64_t idx = col;
            for (int i = 0; i < n; ++i) {
                const FT v = y[idx];
                if (more) fn[idx] = (v - w[idx]) * inv_dh;
                nonfinite = nonfinite || !(v - v == FT(0)); // (inf - inf and NaN - NaN are NaN)
                idx += stride;
            }
        } else {
            ++st.rejected;
            int64_t idx = col;
            for (int i = 0; i < n; ++i) { // back to the last accepted state
                y[idx] = yn[idx];
                idx += stride;
            }
            h = hh * fac;
            if (!(h >= hmin)) { failed = true; break; }
        }
    }
    st.steps = st.accepted + st.rejected;
    st.failed = failed ? 1u : 0u;
    if (A.dt_cols) A.dt_cols[col] = failed ? FT(0) : FT(h);
}

// trbdf2_kernel's epilogue (lh_implicit.hpp) without the Newton counters: every lane of the wave gets here, those
// past the last column with zeros; one atomic per counter and wave
__device__ __forceinline__ void heat_trbdf2_epilogue(const Trbdf2ColStats& st, bool nonfinite, unsigned* status,
                                                     unsigned long long* s) {
    if (nonfinite) atomicOr(status, 1u);
    unsigned long long acc = st.accepted, rej = st.rejected, fl = st.failed;
    unsigned long long mx = st.steps;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        rej += __shfl_xor(rej, off, 64);
        fl += __shfl_xor(fl, off, 64);
        const unsigned long long o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(s + 0, acc);
        atomicAdd(s + 1, rej);
        if (mx > __atomic_load_n(s + 3, __ATOMIC_RELAXED)) atomicMax(s + 3, mx);
        if (fl) {
            atomicOr(status, 16u);
            atomicAdd(s + 4, fl);
        }
        atomicAdd(s + 5, 64ull * mx);
    }
}

// the constants of a cell of a model without soil classes: heat_implicit_column's `cell` and face states
template <typename FT, typename M>
struct HeatCells {
    const M& mm;
    const DevParams<FT>& P;
    const ColC<FT>& c;
    const FT* vl;
    const FT* ti;
    int64_t col;
    __device__ __forceinline__ void cell(int64_t id, FT& alpha, FT& beta, FT& kap, FT& rcs) const {
        const FT v = vl[id], i = ti[id];
        beta = temperature_closure<FT, M>(mm, P, c, v, i, FT(0), rcs); // T of rhoe_int = 0 is the offset beta
        alpha = M::is_production ? mm.rcp(rcs) : FT(1) / rcs;
        kap = kappa_closure<FT, M>(mm, P, c, v, i);
    }
    __device__ __forceinline__ FT face_kappa(int face, int64_t id) const {
        return face_state<FT, M, MODEL_HEAT, false>(mm, P, c, face, col, vl[id], ti[id], FT(0)).kap;
    }
};

template <typename FT, typename M, bool PERCOL>
__global__ void __launch_bounds__(implicit_threads<M>())
heat_trbdf2_kernel(const DevParams<FT> P, const HeatTrbdf2Args<FT> A) {
    const M mm = implicit_math<M>(P.math_tab); // (every thread of the workgroup)
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    bool nonfinite = false;
    if (col < P.ncols) {
        const ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
        const HeatCells<FT, M> C{mm, P, c, A.vl, A.ti, col};
        heat_trbdf2_column<FT>(P, A, C, col, st, nonfinite);
    }
    heat_trbdf2_epilogue(st, nonfinite, P.status, A.stats);
}

template <typename FT>
void launch_heat_trbdf2(const DevParams<FT>& P, const HeatTrbdf2Args<FT>& A, bool percol, int math, hipStream_t s) {
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_bool(percol, [&](auto pc) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((heat_trbdf2_kernel<FT, M, decltype(pc)::value>), grid_for(P.ncols, implicit_threads<M>()),
                           dim3(implicit_threads<M>()), 0, s, P, A);
    }); });
}

#define LH_INSTANTIATE_HEAT_TRBDF2(FT) \
    template void launch_heat_trbdf2<FT>(const DevParams<FT>&, const HeatTrbdf2Args<FT>&, bool, int, hipStream_t);

} // namespace lh
#endif // LH_HEAT_TRBDF2_TU
