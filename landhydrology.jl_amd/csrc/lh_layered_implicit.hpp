// lh_layered_implicit.hpp -- backward Euler (lh_step_layered_implicit_euler) and adaptive TR-BDF2
// (lh_integrate_layered_trbdf2) of a Richards model with per-CELL soil classes.
//
// The one-lane-per-column kernels of lh_implicit.hpp (same workgroup size, math tables, lane-to-column map,
// statistics reduction, safeguard, stall rule, TR-BDF2 stages, error estimate and controller) with the column
// constants of lh_layered.hpp: the class table in LDS, a cell's class byte read from the class plane, and
// `c` a reference into the table.  f is layered_rhs_kernel's tendency expression for expression (relative K
// times the cell's own Ksat, the interior face -(K_lo + K_hi) (head_difference cg2), the boundary faces with
// the boundary cell's class), so "solved" means solved against lh_rhs of the same context; the Jacobian row
// of a face takes the two conductivities and the two slopes of its cells separately.
//
// A kernel family of its own, in its own translation units: lh_implicit.hpp and lh_layered.hpp are not
// touched, so every kernel of theirs keeps its instructions (profiles/layered_implicit_manifest.txt).  The
// sweeps and the drivers below are therefore copies of column_sweep_up, newton_stage, implicit_column and
// trbdf2_column with `S.c` replaced by the cell's entry -- the rule of DESIGN section 4.14: shared text only
// where the existing kernels keep their instruction hashes.
//
// The first part (the launchers' declarations) is what lh_api.hip includes; the kernels follow under
// LH_LAYERED_IMPLICIT_TU, which only lh_kernels_f64_layered_implicit.hip / lh_kernels_f32_layered_implicit.hip
// define (with LH_LAYERED_TU, for stage_class_table).
#pragma once
#include "lh_layered.hpp"

namespace lh {

// NOICE as launch_implicit_euler's; the closure form (VGF) is the host's decision over all classes
// (P.vg_fast_all), as launch_layered_rhs takes it.  Production math, no conductivity factors.
template <typename FT>
void launch_layered_implicit_euler(const DevParams<FT>& P, const LayeredArgs<FT>& L, const ImplicitArgs<FT>& A, bool noice,
                                   hipStream_t s);
template <typename FT>
void launch_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A, bool noice,
                           hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_IMPLICIT_TU
#include "lh_implicit.hpp" // water_slopes, boundary_flux_slope, the safeguard's and the controller's constants

namespace lh {

// what a lane needs to find a cell's constants: the table in LDS and the class plane
template <typename FT>
struct ClassView {
    const ColC<FT>* tab;  // LDS, LH_LAYERED_MAX_CLASSES entries (stage_class_table)
    const uint8_t* cls;   // class plane [nlev][stride]
    __device__ __forceinline__ unsigned index(int64_t id) const { return cls[id] & unsigned(LH_LAYERED_MAX_CLASSES - 1); }
    __device__ __forceinline__ const ColC<FT>& at(unsigned k) const { return tab[k]; }
};

// column_sweep_up (lh_implicit.hpp) with per-cell constants: the rolling window of two cells carries the
// class INDEX of a cell (k, ku), not its entry.  K is the TRUE conductivity (K_r c.Ksat) and the interior
// face is layered_rhs_kernel's; row(idx, v_i, f_i) returns R_i; with JAC row i of J = I - coef df/dv is
// formed and eliminated forward (c'_i, d'_i of J x = -R to cp, dp).
template <typename FT, typename M, bool NOICE, bool VGF, bool JAC, typename Row>
__device__ __forceinline__ void layered_sweep_up(const M& mm, const DevParams<FT>& P, const ClassView<FT>& C,
                                                 const FaceState<FT>& fsb, const FaceState<FT>& fst, int64_t col,
                                                 const FT* y, const FT* ti, FT ti_b, FT coef, FT* cp, FT* dp, Row&& row) {
    constexpr bool vgf = VGF && M::uses_tables;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const FT T = FT(288); // (read by nothing: no conductivity factors on this path)
    auto closures = [&](unsigned kc, FT v, FT tiv, FT& K, FT& np, FT& dK, FT& dn) {
        const ColC<FT>& c = C.at(kc);
        FT Kr = FT(0);
        np = FT(0);
        water_closures<FT, M, false, true, false, NOICE, true, false, true>(mm, P, c, v, tiv, T, Kr, np, nullptr, vgf);
        K = Kr * c.Ksat; // the true conductivity: the two cells of a face may differ in Ksat
        if constexpr (JAC) {
            float dkr, dnf;
            water_slopes<FT, NOICE>(c, v, tiv, np, dkr, dnf);
            dK = FT(dkr) * c.Ksat;
            dn = FT(dnf);
        }
    };
    int64_t idx = col;
    unsigned k = C.index(idx);
    FT v = y[idx];
    FT K, np, dK = FT(0), dn = FT(0);
    closures(k, v, NOICE ? FT(0) : ti_b, K, np, dK, dn);
    FT Flo, dFlo_lo = FT(0), dFlo_c = FT(0);
    {
        FT fe, fw;
        boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fsb, FACE_BOTTOM, col, T, K, -np, fe, fw);
        Flo = fw * P.inv_dz;
        if constexpr (JAC) dFlo_c = boundary_flux_slope<FT>(P, fsb, FACE_BOTTOM, dK, dn) * P.inv_dz;
    }
    FT cp_prev = FT(0), dp_prev = FT(0);
    for (int i = 0; i < n; ++i) {
        FT Fhi, dFhi_c = FT(0), dFhi_u = FT(0);
        FT vu = FT(0), Ku = FT(0), npu = FT(0), dKu = FT(0), dnu = FT(0);
        unsigned ku = k;
        const int64_t idu = idx + stride;
        if (i + 1 < n) {
            vu = y[idu];
            ku = C.index(idu);
            closures(ku, vu, NOICE ? FT(0) : ti[idu], Ku, npu, dKu, dnu);
            // layered_rhs_kernel's interior face, lower cell first; h and K_lo + K_hi kept for the Jacobian rows
            const FT h = head_difference(npu, np, P.dz);
            const FT Ks = K + Ku;
            Fhi = -Ks * (h * P.cg2);
            if constexpr (JAC) {
                dFhi_c = -P.cg2 * (dK * h + Ks * dn);
                dFhi_u = -P.cg2 * (dKu * h - Ks * dnu);
            }
        } else {
            FT fe, fw;
            boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fst, FACE_TOP, col, T, K, -np, fe, fw);
            Fhi = fw * P.inv_dz;
            if constexpr (JAC) dFhi_c = boundary_flux_slope<FT>(P, fst, FACE_TOP, dK, dn) * P.inv_dz;
        }
        const FT R = row(idx, v, Flo - Fhi); // f_i = F_lo - F_hi, layered_rhs_kernel's emit
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
        v = vu; K = Ku; np = npu; dK = dKu; dn = dnu; k = ku;
        idx = idu;
    }
}

// newton_stage (lh_implicit.hpp) with the safeguard and the convergence test per cell: dmax = 1/2 (nu - theta_r),
// the floor theta_r, the kink nu - theta_i and the scale tol max(|v_i|, nu) are the cell's class's.
template <typename FT, typename M, bool NOICE, bool VGF, bool WFIRST, bool ADAPT>
__device__ __forceinline__ int layered_newton_stage(const M& mm, const DevParams<FT>& P, const ClassView<FT>& C,
                                                    const FaceState<FT>& fsb, const FaceState<FT>& fst, int64_t col,
                                                    FT* y, const FT* ti, FT ti_b, FT* w, FT* cp, FT* dp, FT coef, FT tol,
                                                    FT atol, FT rtol, int max_iter, bool& conv, FT kappa = FT(0)) {
    const int n = P.nlev;
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
        layered_sweep_up<FT, M, NOICE, VGF, true>(mm, P, C, fsb, fst, col, y, ti, ti_b, coef, cp, dp, row);
        FT dnext = FT(0);
        bool ok = true;
        FT dbig = FT(0);
        for (int i = n - 1; i >= 0; --i) {
            const int64_t id = int64_t(i) * P.stride + col;
            const ColC<FT>& c = C.at(C.index(id));
            const FT floor_r = c.theta_r;
            const FT dmax = FT(LH_IMPLICIT_DMAX_FRAC) * (c.nu - floor_r);
            const FT d = dp[id] - cp[id] * dnext; // (c'_{n-1} = 0)
            dnext = d;
            const FT vo = y[id];
            const FT du = fmin_ft(fmax_ft(lam * d, -dmax), dmax);
            FT vnew = vo + du;
            const FT fl = floor_r + FT(0.5) * (vo - floor_r);
            if (vo > floor_r) vnew = vnew < fl ? fl : vnew; // at most half way down to theta_r
            else vnew = vnew < vo ? vo : vnew;              // (at or below it already: no further)
            const FT nue = NOICE ? c.nu : c.nu - ti[id];    // the saturation kink: stop on it from below
            if (vo < nue && vnew > nue) vnew = nue;
            y[id] = vnew;
            // judged on the Newton step itself: a step the safeguard cut short is not convergence
            const FT av = vnew < FT(0) ? -vnew : vnew;
            const FT ad = d < FT(0) ? -d : d;
            if (ADAPT) ok = ok && (ad <= kappa * (atol + rtol * av));
            else ok = ok && (ad <= tol * fmax_ft(av, c.nu));
            dbig = ad > dbig ? ad : dbig;
        }
        conv = ok;
        lam = (dbig > FT(LH_IMPLICIT_STALL) * dprev) ? fmax_ft(FT(0.5) * lam, FT(1.0 / 16)) : fmin_ft(FT(2) * lam, FT(1));
        dprev = dbig;
        ++it;
    }
    return it;
}

// the two Dirichlet face states of a column: the boundary cells' own class entries
template <typename FT, typename M, bool NOICE, bool VGF>
__device__ __forceinline__ void layered_face_states(const M& mm, const DevParams<FT>& P, const ClassView<FT>& C, int64_t col,
                                                    FT ti_b, FT ti_t, FaceState<FT>& fsb, FaceState<FT>& fst) {
    constexpr bool vgf = VGF && M::uses_tables;
    const FT T = FT(288);
    const int64_t top = int64_t(P.nlev - 1) * P.stride + col;
    fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, C.at(C.index(col)), FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
    fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, C.at(C.index(top)), FACE_TOP, col, FT(0), ti_t, T, vgf);
}

// implicit_column (lh_implicit.hpp)
template <typename FT, typename M, bool NOICE, bool VGF>
__device__ __forceinline__ void layered_implicit_column(const M& mm, DevParams<FT> P, const ClassView<FT>& C,
                                                        const ImplicitArgs<FT>& A, int64_t col, int& my_max,
                                                        unsigned long long& unconv, unsigned long long& total) {
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    const FT ti_t = NOICE ? FT(0) : A.ti[int64_t(P.nlev - 1) * P.stride + col];
    for (int64_t s = 0; s < A.nsteps; ++s) {
        if (A.bcv) set_stage_boundary_values(P, A.bcv + s * 4);
        FaceState<FT> fsb, fst;
        layered_face_states<FT, M, NOICE, VGF>(mm, P, C, col, ti_b, ti_t, fsb, fst);
        bool conv;
        const int it = layered_newton_stage<FT, M, NOICE, VGF, true, false>(
            mm, P, C, fsb, fst, col, A.y, A.ti, ti_b, A.yn, A.cp, A.dp, A.dt, A.tol, FT(0), FT(0), A.max_iter, conv);
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    }
}

template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
layered_implicit_euler_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const ImplicitArgs<FT> A) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls); // (every thread of the workgroup)
    const ClassView<FT> C{s_cls, L.cls};
    const int64_t col = implicit_lane_column();
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    if (col < P.ncols) layered_implicit_column<FT, M, NOICE, VGF>(mm, P, C, A, col, my_max, unconv, total);
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
template <typename FT, typename M, bool NOICE, bool VGF, typename OUT = NoStepOutput>
__device__ __forceinline__ void layered_trbdf2_column(const M& mm, DevParams<FT> P, const ClassView<FT>& C,
                                                      const Trbdf2Args<FT>& A, int64_t col, Trbdf2ColStats& st,
                                                      OUT output = OUT()) {
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
    const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
    const FT b1 = FT((1.0 - 1.4142135623730951) / 3.0), b2 = FT(1.0 / 3.0), b3 = FT((1.4142135623730951 - 2.0) / 3.0);
    const FT inv_d = FT(1.0 / dg);
    const FT atol = FT(A.abstol), rtol = FT(A.reltol);
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    const FT ti_t = NOICE ? FT(0) : A.ti[int64_t(n - 1) * stride + col];
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
        layered_face_states<FT, M, NOICE, VGF>(mm, P, C, col, ti_b, ti_t, fsb, fst);
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
    layered_sweep_up<FT, M, NOICE, VGF, false>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
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
        int it = layered_newton_stage<FT, M, NOICE, VGF, false, true>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, w, A.cp, A.dp,
                                                                      dh, tol, atol, rtol, max_iter, conv, kappa);
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
            it = layered_newton_stage<FT, M, NOICE, VGF, false, true>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, w, A.cp, A.dp,
                                                                      dh, tol, atol, rtol, max_iter, conv, kappa);
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
            layered_sweep_up<FT, M, NOICE, VGF, true>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, dh, A.cp, A.dp,
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
            output(t, clip ? A.t1 : t + hh, hh);
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

template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
layered_trbdf2_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Trbdf2Args<FT> A) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls); // (every thread of the workgroup)
    const ClassView<FT> C{s_cls, L.cls};
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    if (col < P.ncols) layered_trbdf2_column<FT, M, NOICE, VGF>(mm, P, C, A, col, st);
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

// f(NOICE, VGF) as launch_layered_rhs chooses them without conductivity factors
template <typename FT, typename F>
inline void with_layered_implicit_variant(const DevParams<FT>& P, bool noice, F&& f) {
    using M = MathFast<FT>;
    const bool ni = noice && noice_exists<M>(false);
    const bool robust = robust_vg_exists<M, MODEL_RICHARDS>() && P.vg_fast_all == 0;
    with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        // (robust is normalised above: the guard only keeps what cannot occur un-instantiated)
        if constexpr (decltype(vg)::value || robust_vg_exists<M, MODEL_RICHARDS>()) f(i, vg);
    }); });
}

template <typename FT>
void launch_layered_implicit_euler(const DevParams<FT>& P, const LayeredArgs<FT>& L, const ImplicitArgs<FT>& A, bool noice,
                                   hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((layered_implicit_euler_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A);
    });
}

template <typename FT>
void launch_layered_trbdf2(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Trbdf2Args<FT>& A, bool noice,
                           hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((layered_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, block), dim3(block), 0, s, P, L, A);
    });
}

#define LH_INSTANTIATE_LAYERED_IMPLICIT(FT)                                                                         \
    template void launch_layered_implicit_euler<FT>(const DevParams<FT>&, const LayeredArgs<FT>&,                   \
                                                    const ImplicitArgs<FT>&, bool, hipStream_t);                    \
    template void launch_layered_trbdf2<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Trbdf2Args<FT>&,    \
                                            bool, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_IMPLICIT_TU
