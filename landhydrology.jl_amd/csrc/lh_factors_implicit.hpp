// lh_factors_implicit.hpp -- backward Euler (lh_step_factors_implicit_euler) and adaptive TR-BDF2
// (lh_integrate_factors_trbdf2) of a Richards model whose hydrology has conductivity factors other than
// NoEffect: TemperatureDependentViscosity and / or IceImpedance.
//
// The one-lane-per-column kernels of lh_implicit.hpp (same workgroup size, math tables, lane-to-column map,
// statistics reduction, safeguard, stall rule, TR-BDF2 stages, error estimate and controller) with
//   K = visc(T) imp(vartheta_l, theta_i) K_NoEffect.
// T is prescribed (Ya.soil.T, a plane or a level-uniform profile) and theta_i never changes, so the viscosity
// factor is a constant of every cell during a call, the impedance factor depends on the cell's own vartheta_l
// only, and the stage Jacobian stays tridiagonal: only dK / dvartheta_l gains a term (factor_slopes).  f is
// rhs_kernel's FACTORS tendency expression for expression (the same water_closures instantiation, face_state
// with the boundary cell's T), so "solved" means solved against lh_rhs of the same context.
//
// A kernel family of its own, in its own translation units: lh_implicit.hpp is not touched, so every kernel of
// its keeps its instructions (profiles/factors_implicit_manifest.txt).  The sweep and the drivers below are
// therefore copies of column_sweep_up, newton_stage, implicit_column and trbdf2_column with the cell's T read
// and the factors' slope added -- the rule of DESIGN section 4.14: shared text only where the existing kernels
// keep their instruction hashes.  No NOICE variant: the impedance factor is a function of theta_i, so (as
// rhs_kernel with factors) the plane is read whatever its zero bit says; a known-zero plane reads zeros.
//
// The first part (the launchers' declarations) is what lh_api.hip includes; the kernels follow under
// LH_FACTORS_IMPLICIT_TU, which only lh_kernels_f64_factors_implicit.hip / lh_kernels_f32_factors_implicit.hip
// define.
#pragma once
#include "lh_device.hpp"

namespace lh {

// T: the prescribed temperature plane of Ya [nlev][stride]; NULL where no cell's T is read (no viscosity factor) or
// where it comes from the level-uniform profile P.aux_prof[LH_VAR_T].  percol, math: as launch_implicit_euler's.
template <typename FT>
void launch_factors_implicit_euler(const DevParams<FT>& P, const ImplicitArgs<FT>& A, const FT* T, bool percol, int math,
                                   hipStream_t s);
template <typename FT>
void launch_factors_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const FT* T, bool percol, int math,
                           hipStream_t s);

} // namespace lh

#ifdef LH_FACTORS_IMPLICIT_TU
#include "lh_implicit.hpp" // water_slopes, boundary_flux_slope, ColumnSolve, the safeguard's and the controller's constants

namespace lh {

// where a cell's prescribed T comes from: nothing (no viscosity factor: no closure reads T), the level-uniform
// profile (a wave-uniform read) or the plane
template <typename FT>
struct PrescribedT {
    const FT* prof;  // [nlev] or nullptr
    const FT* plane; // [nlev][stride] or nullptr
    bool need;
    __device__ __forceinline__ PrescribedT(const DevParams<FT>& P, const FT* T)
        : prof(P.aux_prof[3]), plane(T), need(P.viscosity_kind != 0) {}
    __device__ __forceinline__ FT at(int i, int64_t idx) const {
        if (!need) return FT(288);
        return prof ? prof[i] : plane[idx];
    }
};

// dK / dvartheta_l with the factors, from the slope dK of K_NoEffect (in the units K is carried in, water_slopes)
// and K itself (with the factors).  With F = visc imp, theta_l = min(vartheta_l, nu - theta_i):
//   dK/dvl = F dK_NoEffect/dvl + K Omega ln10 theta_i / (theta_l + theta_i)^2,
// the second term only where vartheta_l < nu - theta_i (on and above it theta_l is constant: the side psi's slope
// takes there).  The impedance reads the RAW vartheta_l as water_closures does, so a cell clamped at theta_r + eps
// has dK_NoEffect = 0 and still this term.  theta_i = 0: F's impedance part is 1 and the term 0;
// theta_l + theta_i = 0: NaN, as K.  In Float32 whatever FT is: it only enters the Jacobian.
template <typename FT>
__device__ __forceinline__ FT factor_slopes(const DevParams<FT>& P, const ColC<FT>& c, FT vl, FT ti, FT T, FT K, FT dK) {
    using MF = MathFast<float>;
    float F = 1.0f, g = 0.0f;
    if (P.viscosity_kind) F = MF::exp2(float(P.gamma * (T - P.T_ref_visc)) * 1.4426950408889634f);
    if (P.impedance_kind) {
        const FT nu_eff = c.nu - ti;
        const bool below = vl < nu_eff;
        const float tif = float(ti);
        const float itw = MF::rcp(float(below ? vl : nu_eff) + tif);
        const float Om = float(P.Omega);
        F = F * MF::exp2((-Om * (tif * itw)) * 3.3219280948873623f);
        if (below) g = (Om * 2.302585092994046f) * tif * itw * itw;
    }
    return FT(F) * dK + K * FT(g);
}

// column_sweep_up (lh_implicit.hpp) with conductivity factors: every cell's T is read, the closures are
// rhs_kernel's FACTORS instantiation, and dK takes factor_slopes.  row(idx, v_i, f_i) returns R_i; with JAC row i
// of J = I - coef df/dv is formed and eliminated forward (c'_i, d'_i of J x = -R to cp, dp).
template <typename FT, typename M, bool PERCOL, bool VGF, bool JAC, typename Row>
__device__ __forceinline__ void factors_sweep_up(const M& mm, const DevParams<FT>& P,
                                                 const ColumnSolve<FT, M, PERCOL, false>& S, const FaceState<FT>& fsb,
                                                 const FaceState<FT>& fst, int64_t col, const FT* y, const FT* ti,
                                                 const PrescribedT<FT>& Tp, FT coef, FT* cp, FT* dp, Row&& row) {
    constexpr bool RELK = ColumnSolve<FT, M, PERCOL, false>::RELK;
    constexpr bool vgf = VGF && M::uses_tables;
    const ColC<FT>& c = S.c;
    const FT Ksc = S.Ksc, cgw = S.cgw;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    auto closures = [&](FT v, FT tiv, FT T, FT& K, FT& np, FT& dK, FT& dn) {
        water_closures<FT, M, true, true, false, false, RELK, false, true>(mm, P, c, v, tiv, T, K, np, nullptr, vgf);
        if constexpr (JAC) {
            float dkr, dnf;
            water_slopes<FT, false>(c, v, tiv, np, dkr, dnf);
            dK = factor_slopes<FT>(P, c, v, tiv, T, K, FT(dkr) * (RELK ? FT(1) : c.Ksat)); // in the units of K
            dn = FT(dnf);
        }
    };
    int64_t idx = col;
    FT v = y[idx];
    FT Tc = Tp.at(0, idx);
    FT K, np, dK = FT(0), dn = FT(0);
    closures(v, ti[idx], Tc, K, np, dK, dn);
    FT Flo, dFlo_lo = FT(0), dFlo_c = FT(0);
    {
        FT fe, fw;
        boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fsb, FACE_BOTTOM, col, Tc, K * Ksc, -np, fe, fw);
        Flo = fw * P.inv_dz;
        if constexpr (JAC) dFlo_c = boundary_flux_slope<FT>(P, fsb, FACE_BOTTOM, dK * Ksc, dn) * P.inv_dz;
    }
    FT cp_prev = FT(0), dp_prev = FT(0);
    for (int i = 0; i < n; ++i) {
        FT Fhi, dFhi_c = FT(0), dFhi_u = FT(0);
        FT vu = FT(0), Tu = Tc, Ku = FT(0), npu = FT(0), dKu = FT(0), dnu = FT(0);
        const int64_t idu = idx + stride;
        if (i + 1 < n) {
            vu = y[idu];
            Tu = Tp.at(i + 1, idu);
            closures(vu, ti[idu], Tu, Ku, npu, dKu, dnu);
            // interior_face's water flux (lh_column_ops.hpp), h and K_lo + K_hi kept for the Jacobian rows
            const FT h = head_difference(npu, np, P.dz);
            const FT Ks = K + Ku;
            Fhi = -Ks * (h * cgw);
            if constexpr (JAC) {
                dFhi_c = -cgw * (dK * h + Ks * dn);
                dFhi_u = -cgw * (dKu * h - Ks * dnu);
            }
        } else {
            FT fe, fw;
            boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fst, FACE_TOP, col, Tc, K * Ksc, -np, fe, fw);
            Fhi = fw * P.inv_dz;
            if constexpr (JAC) dFhi_c = boundary_flux_slope<FT>(P, fst, FACE_TOP, dK * Ksc, dn) * P.inv_dz;
        }
        const FT R = row(idx, v, Flo - Fhi); // f_i = F_lo - F_hi, rhs_kernel's emit
        if constexpr (JAC) {
            const FT a = -coef * dFlo_lo;
            const FT b = FT(1) - coef * (dFlo_c - dFhi_c);
            const FT cc = coef * dFhi_u;
            const FT den = b - a * cp_prev;
            const FT cpi = cc / den;
            const FT dpi = (-R - a * dp_prev) / den;
            cp[idx] = cpi;
            dp[idx] = dpi;
            cp_prev = cpi;
            dp_prev = dpi;
        }
        // slide the window: the face above becomes the face below
        Flo = Fhi;
        dFlo_lo = dFhi_c;
        dFlo_c = dFhi_u;
        v = vu; Tc = Tu; K = Ku; np = npu; dK = dKu; dn = dnu;
        idx = idu;
    }
}

// newton_stage (lh_implicit.hpp) on factors_sweep_up.  nonfinite: a Newton step that is NaN in some cell (a cell with
// theta_l + theta_i = 0 under the impedance factor has K = NaN, as in the reference) -- status bit 0.
template <typename FT, typename M, bool PERCOL, bool VGF, bool WFIRST, bool ADAPT>
__device__ __forceinline__ int factors_newton_stage(const M& mm, const DevParams<FT>& P,
                                                    const ColumnSolve<FT, M, PERCOL, false>& S, const FaceState<FT>& fsb,
                                                    const FaceState<FT>& fst, int64_t col, FT* y, const FT* ti,
                                                    const PrescribedT<FT>& Tp, FT* w, FT* cp, FT* dp, FT coef, FT tol,
                                                    FT atol, FT rtol, int max_iter, bool& conv, bool& nonfinite,
                                                    FT kappa = FT(0)) {
    const ColC<FT>& c = S.c;
    const int n = P.nlev;
    const FT dmax = S.dmax, floor_r = S.floor_r;
    conv = false;
    int it = 0;
    FT lam = FT(1);          // step length of the safeguard (see LH_IMPLICIT_STALL)
    FT dprev = FT(INFINITY); // largest |Newton step| of the previous iteration
    while (it < max_iter && !conv) {
        auto row = [&](int64_t idx, FT v, FT f) {
            FT vn;
            if (WFIRST && it == 0) { vn = v; w[idx] = v; } else vn = w[idx];
            return (v - vn) - coef * f;
        };
        factors_sweep_up<FT, M, PERCOL, VGF, true>(mm, P, S, fsb, fst, col, y, ti, Tp, coef, cp, dp, row);
        FT dnext = FT(0);
        bool ok = true;
        FT dbig = FT(0);
        for (int i = n - 1; i >= 0; --i) {
            const int64_t id = int64_t(i) * P.stride + col;
            const FT d = dp[id] - cp[id] * dnext; // (c'_{n-1} = 0)
            dnext = d;
            const FT vo = y[id];
            const FT du = fmin_ft(fmax_ft(lam * d, -dmax), dmax);
            FT vnew = vo + du;
            const FT fl = floor_r + FT(0.5) * (vo - floor_r);
            if (vo > floor_r) vnew = vnew < fl ? fl : vnew; // at most half way down to theta_r
            else vnew = vnew < vo ? vo : vnew;              // (at or below it already: no further)
            const FT nue = c.nu - ti[id];                   // the saturation kink: stop on it from below
            if (vo < nue && vnew > nue) vnew = nue;
            y[id] = vnew;
            // judged on the Newton step itself: a step the safeguard cut short is not convergence
            const FT av = vnew < FT(0) ? -vnew : vnew;
            const FT ad = d < FT(0) ? -d : d;
            if (ADAPT) ok = ok && (ad <= kappa * (atol + rtol * av));
            else ok = ok && (ad <= tol * fmax_ft(av, c.nu));
            dbig = ad > dbig ? ad : dbig;
        }
        if (dnext != dnext) nonfinite = true; // (a NaN anywhere in the column reaches the bottom of the back substitution)
        conv = ok;
        lam = (dbig > FT(LH_IMPLICIT_STALL) * dprev) ? fmax_ft(FT(0.5) * lam, FT(1.0 / 16)) : fmin_ft(FT(2) * lam, FT(1));
        dprev = dbig;
        ++it;
    }
    return it;
}

// the two Dirichlet face states of a column, with the boundary cells' T (rhs_kernel's boundary_fluxes hands its
// face_state the boundary cell's T, and the oracle does the same)
template <typename FT, typename M, bool PERCOL, bool VGF>
__device__ __forceinline__ void factors_face_states(const M& mm, const DevParams<FT>& P,
                                                    const ColumnSolve<FT, M, PERCOL, false>& S, int64_t col, FT ti_b,
                                                    FT ti_t, FT T_b, FT T_t, FaceState<FT>& fsb, FaceState<FT>& fst) {
    constexpr bool vgf = VGF && M::uses_tables;
    fsb = face_state<FT, M, MODEL_RICHARDS, true, false>(mm, P, S.c, FACE_BOTTOM, col, FT(0), ti_b, T_b, vgf);
    fst = face_state<FT, M, MODEL_RICHARDS, true, false>(mm, P, S.c, FACE_TOP, col, FT(0), ti_t, T_t, vgf);
}

// implicit_column (lh_implicit.hpp)
template <typename FT, typename M, bool PERCOL, bool VGF>
__device__ __forceinline__ void factors_implicit_column(const M& mm, DevParams<FT> P, const ImplicitArgs<FT>& A,
                                                        const PrescribedT<FT>& Tp, int64_t col, int& my_max,
                                                        unsigned long long& unconv, unsigned long long& total,
                                                        bool& nonfinite) {
    const ColumnSolve<FT, M, PERCOL, false> S(mm, P, col);
    const int64_t top = int64_t(P.nlev - 1) * P.stride + col;
    const FT ti_b = A.ti[col], ti_t = A.ti[top];
    const FT T_b = Tp.at(0, col), T_t = Tp.at(P.nlev - 1, top);
    for (int64_t s = 0; s < A.nsteps; ++s) {
        if (A.bcv) set_stage_boundary_values(P, A.bcv + s * 4);
        FaceState<FT> fsb, fst;
        factors_face_states<FT, M, PERCOL, VGF>(mm, P, S, col, ti_b, ti_t, T_b, T_t, fsb, fst);
        bool conv;
        const int it = factors_newton_stage<FT, M, PERCOL, VGF, true, false>(
            mm, P, S, fsb, fst, col, A.y, A.ti, Tp, A.yn, A.cp, A.dp, A.dt, A.tol, FT(0), FT(0), A.max_iter, conv, nonfinite);
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    }
}

template <typename FT, typename M, bool PERCOL, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
factors_implicit_euler_kernel(const DevParams<FT> P, const ImplicitArgs<FT> A, const FT* __restrict__ T) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    const PrescribedT<FT> Tp(P, T);
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    bool nonfinite = false;
    if (col < P.ncols) factors_implicit_column<FT, M, PERCOL, VGF>(mm, P, A, Tp, col, my_max, unconv, total, nonfinite);
    if (nonfinite) atomicOr(P.status, 1u);
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

// trbdf2_column (lh_implicit.hpp): the stages, the error estimate and the controller are its own, unchanged
template <typename FT, typename M, bool PERCOL, bool VGF>
__device__ __forceinline__ void factors_trbdf2_column(const M& mm, DevParams<FT> P, const Trbdf2Args<FT>& A,
                                                      const PrescribedT<FT>& Tp, int64_t col, Trbdf2ColStats& st,
                                                      bool& nonfinite) {
    const ColumnSolve<FT, M, PERCOL, false> S(mm, P, col);
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
    const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
    const FT b1 = FT((1.0 - 1.4142135623730951) / 3.0), b2 = FT(1.0 / 3.0), b3 = FT((1.4142135623730951 - 2.0) / 3.0);
    const FT inv_d = FT(1.0 / dg);
    const FT atol = FT(A.abstol), rtol = FT(A.reltol);
    const int64_t top = int64_t(n - 1) * stride + col;
    const FT ti_b = A.ti[col], ti_t = A.ti[top];
    const FT T_b = Tp.at(0, col), T_t = Tp.at(n - 1, top);
    FaceState<FT> fsb, fst;
    // boundary values at time t: linear in t between the call's two ends (or lh_set_bc's constants)
    auto faces_at = [&](double t) {
        if (A.has_bcv) {
            const double s = A.t1 > A.t0 ? (t - A.t0) / (A.t1 - A.t0) : 1.0;
            P.bc_value[FACE_BOTTOM][COMP_ENERGY] = FT(A.bcv[0] + (A.bcv[4] - A.bcv[0]) * s);
            P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = FT(A.bcv[1] + (A.bcv[5] - A.bcv[1]) * s);
            P.bc_value[FACE_TOP][COMP_ENERGY] = FT(A.bcv[2] + (A.bcv[6] - A.bcv[2]) * s);
            P.bc_value[FACE_TOP][COMP_HYDROLOGY] = FT(A.bcv[3] + (A.bcv[7] - A.bcv[3]) * s);
        }
        factors_face_states<FT, M, PERCOL, VGF>(mm, P, S, col, ti_b, ti_t, T_b, T_t, fsb, fst);
    };
    FT* const y = A.y;
    FT* const yn = A.yn;
    FT* const fn = A.fn;
    FT* const yg = A.yg;
    FT* const w = A.w;
    const FT tol = A.tol;
    const int max_iter = A.fixed ? A.max_iter : A.newton_max;
    const FT kappa = A.kappa;
    // f_n of the first step: one tendency sweep at (Y, t0)
    faces_at(A.t0);
    factors_sweep_up<FT, M, PERCOL, VGF, false>(mm, P, S, fsb, fst, col, y, A.ti, Tp, FT(0), nullptr, nullptr,
                                                [&](int64_t idx, FT, FT f) { fn[idx] = f; return FT(0); });
    double t = A.t0;
    double h = A.dt;
    if (A.dt_cols && !A.fixed) { // (fixed mode: steps of exactly dt, whatever the buffer holds)
        const double h0 = double(A.dt_cols[col]);
        if (h0 > 0) h = h0;
    }
    const double hmin = LH_TRBDF2_HMIN_FRAC * (A.t1 - A.t0);
    bool failed = false;
    unsigned steps = 0;
    while (t < A.t1) {
        if (steps >= LH_TRBDF2_MAX_STEPS) { failed = true; break; }
        ++steps;
        double hh;
        const bool clip = trbdf2_clip(t, A.t1, h, hh);
        const FT dh = FT(dg * hh);
        // stage 1: Y_n and w1 = Y_n + d h f_n; the guess is Y_n
        for (int i = 0; i < n; ++i) {
            const int64_t id = int64_t(i) * stride + col;
            const FT v = y[id];
            yn[id] = v;
            w[id] = v + dh * fn[id];
        }
        faces_at(t + gam * hh);
        bool conv;
        int it = factors_newton_stage<FT, M, PERCOL, VGF, false, true>(mm, P, S, fsb, fst, col, y, A.ti, Tp, w, A.cp, A.dp, dh,
                                                                      tol, atol, rtol, max_iter, conv, nonfinite, kappa);
        st.iters += unsigned(it);
        bool newton_ok = conv;
        if (!conv && A.fixed) ++st.unconv;
        if (conv || A.fixed) {
            // stage 2: Y_g and w2; the guess is Y_g
            for (int i = 0; i < n; ++i) {
                const int64_t id = int64_t(i) * stride + col;
                const FT v = y[id];
                yg[id] = v;
                w[id] = (v - c_yn * yn[id]) * c_w2;
            }
            faces_at(t + hh);
            it = factors_newton_stage<FT, M, PERCOL, VGF, false, true>(mm, P, S, fsb, fst, col, y, A.ti, Tp, w, A.cp, A.dp, dh,
                                                                      tol, atol, rtol, max_iter, conv, nonfinite, kappa);
            st.iters += unsigned(it);
            newton_ok = conv;
            if (!conv && A.fixed) ++st.unconv;
        }
        double fac = 0.25; // (a stage that did not converge)
        bool accept = A.fixed != 0;
        if (!A.fixed && newton_ok) {
            // the error estimate: rhs b1 h f_n + b2 z_g + b3 z_1 and J re-formed at Y_1 (the stage-2 face states)
            const FT hf = FT(hh);
            auto rhs = [&](int64_t idx, FT v) {
                const FT f0 = fn[idx], v0 = yn[idx];
                const FT zg = (yg[idx] - (v0 + dh * f0)) * inv_d;
                const FT z1 = (v - w[idx]) * inv_d;
                return b1 * (hf * f0) + b2 * zg + b3 * z1;
            };
            factors_sweep_up<FT, M, PERCOL, VGF, true>(mm, P, S, fsb, fst, col, y, A.ti, Tp, dh, A.cp, A.dp,
                                                       [&](int64_t idx, FT v, FT) { return -rhs(idx, v); });
            FT enext = FT(0);
            double sum = 0.0;
            for (int i = n - 1; i >= 0; --i) {
                const int64_t id = int64_t(i) * stride + col;
                const FT e = A.dp[id] - A.cp[id] * enext;
                enext = e;
                const FT a0 = yn[id] < FT(0) ? -yn[id] : yn[id];
                const FT a1 = y[id] < FT(0) ? -y[id] : y[id];
                const double q = double(e) / double(atol + rtol * (a0 > a1 ? a0 : a1));
                sum += q * q;
            }
            const double E = sqrt(sum / n);
            accept = trbdf2_control(E, fac);
        }
        if (accept) {
            ++st.accepted;
            t = clip ? A.t1 : t + hh; // (assigned: the column lands on t1 exactly)
            if (!A.fixed) h = trbdf2_next_step(h, hh, fac, clip);
            if (t < A.t1) { // f_{n+1} = z_1 / h for the next step
                const FT inv_dh = FT(1.0 / (dg * hh));
                for (int i = 0; i < n; ++i) {
                    const int64_t id = int64_t(i) * stride + col;
                    fn[id] = (y[id] - w[id]) * inv_dh;
                }
            }
        } else {
            ++st.rejected;
            for (int i = 0; i < n; ++i) { // back to the last accepted state
                const int64_t id = int64_t(i) * stride + col;
                y[id] = yn[id];
            }
            h = hh * fac;
            if (!(h >= hmin)) { failed = true; break; }
        }
    }
    st.steps = steps;
    st.failed = failed ? 1u : 0u;
    if (A.dt_cols) A.dt_cols[col] = failed ? FT(0) : FT(h);
}

template <typename FT, typename M, bool PERCOL, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
factors_trbdf2_kernel(const DevParams<FT> P, const Trbdf2Args<FT> A, const FT* __restrict__ T) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    const PrescribedT<FT> Tp(P, T);
    Trbdf2ColStats st;
    bool nonfinite = false;
    if (col < P.ncols) factors_trbdf2_column<FT, M, PERCOL, VGF>(mm, P, A, Tp, col, st, nonfinite);
    if (nonfinite) atomicOr(P.status, 1u);
    // (every lane of the wave gets here, those past the last column with zeros): one atomic per counter and wave
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
        unsigned long long* s = A.stats;
        atomicAdd(s + 0, acc);
        atomicAdd(s + 1, rej);
        atomicAdd(s + 2, its);
        if (mx > __atomic_load_n(s + 3, __ATOMIC_RELAXED)) atomicMax(s + 3, mx);
        if (fl) {
            atomicOr(P.status, 16u);
            atomicAdd(s + 4, fl);
        }
        atomicAdd(s + 5, 64ull * mx);
        if (un) {
            atomicOr(P.status, 8u);
            atomicAdd(s + 6, un);
        }
    }
}

// f(type_c<M>, PERCOL, VGF) for the variant a launch of either kernel takes: with_implicit_variant's axes without
// NOICE.  MathLibm has no tables for VGF to mean anything (spelled VGF = false), and neither has MathFast<float>
// (spelled VGF = true: its VGF = false kernels would be the same code and are not instantiated).
template <typename FT, typename F>
inline void with_factors_implicit_variant(const DevParams<FT>& P, bool percol, int math, F&& f) {
    const bool libm = math == MATH_LIBM;
    const bool vg = !libm && !(sizeof(FT) == 8 && P.vg_fast_all == 0);
    with_math<FT>(libm, [&](auto m) { with_bool(percol, [&](auto pc) { with_bool(vg, [&](auto v) {
        using M = typename decltype(m)::type;
        if constexpr (M::is_production ? (decltype(v)::value || M::uses_tables) : !decltype(v)::value) f(m, pc, v);
    }); }); });
}

template <typename FT>
void launch_factors_implicit_euler(const DevParams<FT>& P, const ImplicitArgs<FT>& A, const FT* T, bool percol, int math,
                                   hipStream_t s) {
    with_factors_implicit_variant(P, percol, math, [&](auto m, auto pc, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((factors_implicit_euler_kernel<FT, M, decltype(pc)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, T);
    });
}

template <typename FT>
void launch_factors_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, const FT* T, bool percol, int math,
                           hipStream_t s) {
    with_factors_implicit_variant(P, percol, math, [&](auto m, auto pc, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((factors_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A, T);
    });
}

#define LH_INSTANTIATE_FACTORS_IMPLICIT(FT)                                                                          \
    template void launch_factors_implicit_euler<FT>(const DevParams<FT>&, const ImplicitArgs<FT>&, const FT*, bool, \
                                                    int, hipStream_t);                                              \
    template void launch_factors_trbdf2<FT>(const DevParams<FT>&, const Trbdf2Args<FT>&, const FT*, bool, int,      \
                                            hipStream_t);

} // namespace lh
#endif // LH_FACTORS_IMPLICIT_TU
