// lh_implicit.hpp -- backward-Euler steps (lh_step_implicit_euler) and adaptive TR-BDF2
// (lh_integrate_trbdf2, below) of the Richards model on gfx950.  Both solve stage equations
// Y - w - coef f(Y) = 0 with the same Newton (newton_stage); backward Euler's is w = v_n, coef = dt.
//
// Per step and column, Newton on R(v) = v - v_n - dt f(v) = 0, where f is EXACTLY the tendency of
// rhs_kernel (the same water_closures, face expressions and boundary_fluxes, in the same order), and
// J = I - dt df/dv is tridiagonal: f_i reads cells i-1, i, i+1 only.  One lane owns one column (every
// per-level access of a wave is one coalesced row), all steps run in one launch.
// One Newton iteration is two sweeps over the column:
//   upward:   closures of cell i+1 (a rolling window of two cells in registers), row i of J and R,
//             forward elimination; c'_i, d'_i go to two scratch planes
//   downward: back substitution, the safeguarded update of the iterate (in Y's plane), and the lane's
//             convergence test max_i |delta_i| <= tol max(|v_i|, nu) on the Newton step delta
// v_n lives in a third scratch plane, written by the first upward sweep of the step.
// The Jacobian is approximate (slopes in Float32, water_slopes); R always uses the exact f.
#pragma once
#include "lh_kernels_impl.hpp" // grid_for; with it lh_column_ops.hpp (implicit_math, fmin_ft / fmax_ft), lh_closures.hpp, lh_launch.hpp,
                               // lh_dispatch.hpp (with_bool), lh_fastmath.hpp (with_math) and lh_device.hpp (ImplicitArgs, Trbdf2Args)

namespace lh {


// Newton's safeguard: the applied change of a cell is at most
// LH_IMPLICIT_DMAX_FRAC (nu - theta_r), a cell moves at most half of its distance to theta_r (and not
// down at all from theta_r or below), and a cell that crosses the saturation kink nu_eff = nu - theta_i
// from below stops on it
#define LH_IMPLICIT_DMAX_FRAC 0.5
// per column: when the largest Newton step of an iteration is more than LH_IMPLICIT_STALL times the
// previous one, the next update is scaled by half the current factor (down to 1/16); after a step that
// did shrink the factor doubles back towards 1
#define LH_IMPLICIT_STALL 0.9
// TR-BDF2 (lh_integrate_trbdf2)
// (the stage's Newton test max |delta| / (atol + rtol |Y|) <= kappa and its iteration cap are Trbdf2Args
// fields: defaults and measurements in lh_api.hip and DESIGN section 4.13)
#define LH_TRBDF2_MAX_STEPS 100000    // attempted steps per column and call before the column fails
#define LH_TRBDF2_HMIN_FRAC 1e-10     // a column whose h falls below this x (t1 - t0) fails

// d K_r / d vl (relative conductivity) and d(-psi) / d vl of one cell, in Float32 whatever FT is:
// they only enter the Jacobian.  With t = S^(1/m), w = 1 - t, inner = 1 - w^m:
//   K_r = sqrt(S) inner^2,  dK_r/dS = K_r / (2 S) + 2 sqrt(S) inner w^(m-1) t / S
//   -dpsi/dvl = -|psi| / (n m w (vl - theta_r))   (the slope of the step bound, slope32)
// and 1/S_s on the saturated branch.  A clamped (bone-dry) cell has constant K and psi.
template <typename FT, bool NOICE>
__device__ __forceinline__ void water_slopes(const ColC<FT>& c, FT vl, FT ti, FT npsi, float& dkr, float& dnpsi) {
    using MF = MathFast<float>;
    dkr = 0.0f;
    dnpsi = 0.0f;
    if (!(vl > c.theta_lim)) return;
    const float num = float(vl - c.theta_r);
    const float m = float(c.m), inv_m = float(c.inv_m);
    const float S = num * float(c.inv_por);
    float w = 0.0f;
    if (S < 1.0f) {
        const float t = MF::exp2(MF::log2(S) * inv_m);
        w = fmaxf(1.0f - t, 1e-7f);
        const float wm = MF::exp2(MF::log2(w) * m);
        const float inner = 1.0f - wm;
        const float sS = MF::sqrt(S);
        const float iS = MF::rcp(S);
        dkr = float(c.inv_por) * (0.5f * sS * inner * inner * iS + 2.0f * sS * inner * wm * t * MF::rcp(w) * iS);
    }
    const FT nu_eff = NOICE ? c.nu : c.nu - ti;
    const float por_e = float(nu_eff - c.theta_r);
    if (num < por_e) {
        float we = w;
        if (!NOICE && nu_eff != c.nu) we = 1.0f - MF::exp2(MF::log2(num * MF::rcp(por_e)) * inv_m);
        we = fmaxf(we, 1e-7f);
        dnpsi = -float(npsi) * MF::rcp(float(c.n) * m * we * num);
    } else {
        dnpsi = -float(c.inv_S_s);
    }
}

// d f_w / d vl_c of one boundary face (physical units, as boundary_fluxes_from returns f_w): a flux
// is constant, free drainage is -K_c, a Dirichlet face has the constant K_f, psi_f of its face state
template <typename FT>
__device__ __forceinline__ FT boundary_flux_slope(const DevParams<FT>& P, const FaceState<FT>& fs, int face,
                                                  FT dK_c, FT dnpsi_c) {
    const int kh = face == FACE_BOTTOM ? P.bc_kind[FACE_BOTTOM][COMP_HYDROLOGY] : P.bc_kind[FACE_TOP][COMP_HYDROLOGY];
    const FT inv_dzb = FT(2) * P.inv_dz;
    if (kh == BC_FREE_DRAINAGE) return -dK_c;
    if (kh == BC_DIRICHLET) {
        // psi_c = -npsi_c: bottom (either sign convention) K_f dnpsi / (dz/2), top -K_f dnpsi / (dz/2)
        return face == FACE_BOTTOM ? fs.K * dnpsi_c * inv_dzb : -fs.K * dnpsi_c * inv_dzb;
    }
    return FT(0);
}

// Which <M, PERCOL, NOICE, VGF> of implicit_euler_kernel / trbdf2_kernel exist: every one of the production
// math (noice_exists, no conductivity factors here), and one per PERCOL of MathLibm, which reads theta_i
// and has no tables for VGF to mean anything -- it is spelled NOICE = false, VGF = false.
template <typename M>
constexpr bool implicit_variant_exists(bool noice, bool vgf) { return M::is_production || (!noice && !vgf); }

// f(type_c<M>, PERCOL, NOICE, VGF) for the variant a launch of either kernel takes
template <typename FT, typename F>
inline void with_implicit_variant(const DevParams<FT>& P, bool percol, bool noice, int math, F&& f) {
    const bool libm = math == MATH_LIBM;
    const bool ni = noice && !libm;
    // clay-like Float64 ensembles: the v_ldexp form, as rhs_kernel.  (The Float32 VGF = false kernels are
    // instantiated and never chosen: MathFast<float> has no tables, they are the VGF = true code.)
    const bool vg = !libm && !(sizeof(FT) == 8 && P.vg_fast_all == 0);
    with_math<FT>(libm, [&](auto m) { with_bool(percol, [&](auto pc) { with_bool(ni, [&](auto i) { with_bool(vg, [&](auto v) {
        if constexpr (implicit_variant_exists<typename decltype(m)::type>(decltype(i)::value, decltype(v)::value)) f(m, pc, i, v);
    }); }); }); });
}

// The column's constants of one solve: ColC, the K and conductance scales of rhs_kernel's
// instantiation, the safeguard's bound
template <typename FT, typename M, bool PERCOL, bool NOICE>
struct ColumnSolve {
    static constexpr bool RELK = M::is_production; // K without Ksat, as rhs_kernel carries it
    ColC<FT> c;
    FT Ksc, cgw, dmax, floor_r;
    __device__ __forceinline__ ColumnSolve(const M& mm, const DevParams<FT>& P, int64_t col) {
        c = make_colc<FT, M>(P, col, PERCOL);
        if (!NOICE) finish_colc<FT, M>(mm, c);
        flux_scales<FT, M>(P, c, Ksc, cgw);
        dmax = FT(LH_IMPLICIT_DMAX_FRAC) * (c.nu - c.theta_r);
        floor_r = c.theta_r;
    }
};

// One upward sweep over a column at the iterate y: the closures of cell i+1 in a rolling window of two
// cells, the face fluxes exactly as rhs_kernel forms them, and f_i = F_lo - F_hi.  row(idx, v_i, f_i)
// returns R_i; with JAC the sweep also forms row i of J = I - coef df/dv and eliminates forward
// (c'_i, d'_i of J x = -R to cp, dp); without it, row only sees f (the tendency).
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, bool JAC, typename Row>
__device__ __forceinline__ void column_sweep_up(const M& mm, const DevParams<FT>& P,
                                                const ColumnSolve<FT, M, PERCOL, NOICE>& S, const FaceState<FT>& fsb,
                                                const FaceState<FT>& fst, int64_t col, const FT* y, const FT* ti,
                                                FT ti_b, FT coef, FT* cp, FT* dp, Row&& row) {
    constexpr bool RELK = ColumnSolve<FT, M, PERCOL, NOICE>::RELK;
    constexpr bool vgf = VGF && M::uses_tables;
    const ColC<FT>& c = S.c;
    const FT Ksc = S.Ksc, cgw = S.cgw;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const FT T = FT(288); // (read by nothing: no conductivity factors on this path)
    auto closures = [&](FT v, FT tiv, FT& K, FT& np, FT& dK, FT& dn) {
        water_closures<FT, M, false, true, false, NOICE, RELK, false, true>(mm, P, c, v, tiv, T, K, np, nullptr, vgf);
        if constexpr (JAC) {
            float dkr, dnf;
            water_slopes<FT, NOICE>(c, v, tiv, np, dkr, dnf);
            dK = FT(dkr) * (RELK ? FT(1) : c.Ksat); // in the units of K
            dn = FT(dnf);
        }
    };
    int64_t idx = col;
    FT v = y[idx];
    FT K, np, dK = FT(0), dn = FT(0);
    closures(v, NOICE ? FT(0) : ti_b, K, np, dK, dn);
    FT Flo, dFlo_lo = FT(0), dFlo_c = FT(0);
    {
        FT fe, fw;
        boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fsb, FACE_BOTTOM, col, T, K * Ksc, -np, fe, fw);
        Flo = fw * P.inv_dz;
        if constexpr (JAC) dFlo_c = boundary_flux_slope<FT>(P, fsb, FACE_BOTTOM, dK * Ksc, dn) * P.inv_dz;
    }
    FT cp_prev = FT(0), dp_prev = FT(0);
    for (int i = 0; i < n; ++i) {
        FT Fhi, dFhi_c = FT(0), dFhi_u = FT(0);
        FT vu = FT(0), tiu = FT(0), Ku = FT(0), npu = FT(0), dKu = FT(0), dnu = FT(0);
        const int64_t idu = idx + stride;
        if (i + 1 < n) {
            vu = y[idu];
            tiu = NOICE ? FT(0) : ti[idu];
            closures(vu, tiu, Ku, npu, dKu, dnu);
            // interior_face's water flux (lh_column_ops.hpp), h and K_lo + K_hi kept for the Jacobian rows:
            // -(K_lo + K_hi) ((npsi_lo - npsi_hi) + dz) cgw
            const FT h = head_difference(npu, np, P.dz);
            const FT Ks = K + Ku;
            Fhi = -Ks * (h * cgw);
            if constexpr (JAC) {
                dFhi_c = -cgw * (dK * h + Ks * dn);
                dFhi_u = -cgw * (dKu * h - Ks * dnu);
            }
        } else {
            FT fe, fw;
            boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fst, FACE_TOP, col, T, K * Ksc, -np, fe, fw);
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
        v = vu; K = Ku; np = npu; dK = dKu; dn = dnu;
        idx = idu;
    }
}

// The Newton solve of one stage equation Y - w - coef f(Y) = 0 in one column: backward Euler's
// (w = v_n, coef = dt) and both TR-BDF2 stages'.  y holds the initial guess and receives the iterate;
// with WFIRST the first upward sweep copies y into w (backward Euler's v_n).  Convergence, per column:
// backward Euler's max_i |delta_i| <= tol max(|v_i|, nu), or with ADAPT
// max_i |delta_i| / (atol + rtol |v_i|) <= kappa.  Returns the iteration count.
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, bool WFIRST, bool ADAPT>
__device__ __forceinline__ int newton_stage(const M& mm, const DevParams<FT>& P,
                                            const ColumnSolve<FT, M, PERCOL, NOICE>& S, const FaceState<FT>& fsb,
                                            const FaceState<FT>& fst, int64_t col, FT* y, const FT* ti, FT ti_b,
                                            FT* w, FT* cp, FT* dp, FT coef, FT tol, FT atol, FT rtol, int max_iter,
                                            bool& conv, FT kappa = FT(0)) {
    const ColC<FT>& c = S.c;
    const int n = P.nlev;
    const FT dmax = S.dmax, floor_r = S.floor_r;
    conv = false;
    int it = 0;
    FT lam = FT(1);                 // step length of the safeguard (see LH_IMPLICIT_STALL)
    FT dprev = FT(INFINITY);        // largest |Newton step| of the previous iteration
    while (it < max_iter && !conv) {
        // ---------------- upward sweep
        auto row = [&](int64_t idx, FT v, FT f) {
            FT vn;
            if (WFIRST && it == 0) { vn = v; w[idx] = v; } else vn = w[idx];
            return (v - vn) - coef * f;
        };
        column_sweep_up<FT, M, PERCOL, NOICE, VGF, true>(mm, P, S, fsb, fst, col, y, ti, ti_b, coef, cp, dp, row);
        // ---------------- downward sweep
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
            // the saturation kink: a cell that crosses nu_eff from below stops on it (psi' has no
            // bound just below, and a Newton step across it oscillates)
            const FT nue = NOICE ? c.nu : c.nu - ti[id];
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
        // a Newton step that has not shrunk (a cycle across the saturation kink): shorten the next
        // one; while the steps shrink, full steps again -- near the solution every step is a full
        // Newton step and the convergence stays quadratic
        lam = (dbig > FT(LH_IMPLICIT_STALL) * dprev) ? fmax_ft(FT(0.5) * lam, FT(1.0 / 16)) : fmin_ft(FT(2) * lam, FT(1));
        dprev = dbig;
        ++it;
    }
    return it;
}

// One column (lane) through all steps of the call: the column's largest iteration count, its
// unconverged steps and its total iterations are returned for the launch's statistics.
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__device__ __forceinline__ void implicit_column(const M& mm, DevParams<FT> P, const ImplicitArgs<FT>& A, int64_t col,
                                                int& my_max, unsigned long long& unconv, unsigned long long& total) {
    constexpr bool vgf = VGF && M::uses_tables;
    const ColumnSolve<FT, M, PERCOL, NOICE> S(mm, P, col);
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const FT T = FT(288); // (read by nothing: no conductivity factors on this path)
    for (int64_t s = 0; s < A.nsteps; ++s) {
        if (A.bcv) set_stage_boundary_values(P, A.bcv + s * 4);
        // The Dirichlet face states read the boundary value and the boundary cell's theta_i only
        // (no conductivity factors): constants of the step -- boundary_fluxes is face_state +
        // boundary_fluxes_from, so the fluxes are bitwise its own
        const FT ti_b = NOICE ? FT(0) : A.ti[col];
        const FT ti_t = NOICE ? FT(0) : A.ti[int64_t(n - 1) * stride + col];
        const FaceState<FT> fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
        const FaceState<FT> fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_TOP, col, FT(0), ti_t, T, vgf);
        bool conv;
        const int it = newton_stage<FT, M, PERCOL, NOICE, VGF, true, false>(
            mm, P, S, fsb, fst, col, A.y, A.ti, ti_b, A.yn, A.cp, A.dp, A.dt, A.tol, FT(0), FT(0), A.max_iter, conv);
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    }
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
implicit_euler_kernel(const DevParams<FT> P, const ImplicitArgs<FT> A) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    if (col < P.ncols) implicit_column<FT, M, PERCOL, NOICE, VGF>(mm, P, A, col, my_max, unconv, total);
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
void launch_implicit_euler(const DevParams<FT>& P, const ImplicitArgs<FT>& A, bool percol, bool noice, int math,
                           hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((implicit_euler_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    });
}

// ---------------------------------------------------------------------------------------------------
// TR-BDF2 (lh_integrate_trbdf2): per column and step, with gamma = 2 - sqrt(2),
// d = gamma/2, h the column's step and f the tendency above,
//   stage 1 (trapezoid): Y_g - w1 - d h f(Y_g) = 0,  w1 = Y_n + d h f_n               at t + gamma h
//   stage 2 (BDF2):      Y_1 - w2 - d h f(Y_1) = 0,  w2 = (Y_g - (1-gamma)^2 Y_n) / (gamma (2-gamma))  at t + h
// both solved by newton_stage.  The stage derivatives come from the converged stage equations,
// z = (Y - w) / d, and f_{n+1} = z_1 / h is the next step's f_n (first same as last).  Error estimate
// (Hosea & Shampine 1996): e = (I - d h J(Y_1))^-1 (b1 h f_n + b2 z_g + b3 z_1), one more upward sweep
// at Y_1 and a back substitution that only accumulates the norm
//   E = sqrt(mean_i (e_i / (atol + rtol max(|Y_n,i|, |Y_1,i|)))^2);
// accepted when E <= 1, h <- h clamp(0.9 E^(-1/3), 0.2, 5); a stage whose Newton does not converge in
// A.newton_max iterations rejects the step with h <- h/4.  Each lane carries its own t and h
// (double) and its own accept/reject history: no collective.

// The step controller's scalar arithmetic, for trbdf2_column and layered_trbdf2_column (lh_coupled_trbdf2.hpp keeps
// its own lines: its kernels move through these calls).  The step taken from t with the proposal
// h: the rest of the interval where h reaches t1 to round-off (the column then lands on t1 exactly) ...
__device__ __forceinline__ bool trbdf2_clip(double t, double t1, double h, double& hh) {
    const bool clip = t + h * (1.0 + 1e-10) >= t1;
    hh = clip ? t1 - t : h;
    return clip;
}
// ... whether a step with error norm E is accepted, and the factor 0.9 E^(-1/3) in [0.2, 5] its size changes by ...
__device__ __forceinline__ bool trbdf2_control(double E, double& fac) {
    fac = 0.9 * pow(E, -1.0 / 3.0);
    fac = fac != fac ? 0.2 : fmin(fmax(fac, 0.2), 5.0);
    return E <= 1.0;
}
// ... and the proposal after an accepted step of hh: a clipped step that could have grown does not shrink h
__device__ __forceinline__ double trbdf2_next_step(double h, double hh, double fac, bool clip) {
    return (clip && fac >= 1.0) ? fmax(hh * fac, h) : hh * fac;
}

// What the column routines (here, lh_layered_implicit.hpp, lh_coupled_trbdf2.hpp, lh_heat_trbdf2.hpp,
// lh_layered_coupled_trbdf2.hpp) hand an accepted step t -> t_new of size hh to, before f_n is overwritten: nothing,
// for every launch but those of the dense calls (lh_dense.hpp, lh_dense_heat.hpp, lh_dense_layered_coupled.hpp), whose
// functor interpolates the output that falls into the step
struct NoStepOutput {
    __device__ __forceinline__ void operator()(double, double, double) const {}
};

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, typename OUT = NoStepOutput>
__device__ __forceinline__ void trbdf2_column(const M& mm, DevParams<FT> P, const Trbdf2Args<FT>& A, int64_t col,
                                              Trbdf2ColStats& st, OUT output = OUT()) {
    constexpr bool vgf = VGF && M::uses_tables;
    const ColumnSolve<FT, M, PERCOL, NOICE> S(mm, P, col);
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const FT T = FT(288);
    const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
    const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
    const FT b1 = FT((1.0 - 1.4142135623730951) / 3.0), b2 = FT(1.0 / 3.0), b3 = FT((1.4142135623730951 - 2.0) / 3.0);
    const FT inv_d = FT(1.0 / dg);
    const FT atol = FT(A.abstol), rtol = FT(A.reltol);
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    const FT ti_t = NOICE ? FT(0) : A.ti[int64_t(n - 1) * stride + col];
    FaceState<FT> fsb, fst;
    // boundary values at time t: linear in t between the call's two ends (or lh_set_bc's constants), and
    // the Dirichlet face states of them
    auto faces_at = [&](double t) {
        if (A.has_bcv) {
            const double s = A.t1 > A.t0 ? (t - A.t0) / (A.t1 - A.t0) : 1.0;
            P.bc_value[FACE_BOTTOM][COMP_ENERGY] = FT(A.bcv[0] + (A.bcv[4] - A.bcv[0]) * s);
            P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = FT(A.bcv[1] + (A.bcv[5] - A.bcv[1]) * s);
            P.bc_value[FACE_TOP][COMP_ENERGY] = FT(A.bcv[2] + (A.bcv[6] - A.bcv[2]) * s);
            P.bc_value[FACE_TOP][COMP_HYDROLOGY] = FT(A.bcv[3] + (A.bcv[7] - A.bcv[3]) * s);
        }
        fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
        fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_TOP, col, FT(0), ti_t, T, vgf);
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
    column_sweep_up<FT, M, PERCOL, NOICE, VGF, false>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
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
    auto restore = [&]() { // back to the last accepted state
        for (int i = 0; i < n; ++i) {
            const int64_t id = int64_t(i) * stride + col;
            y[id] = yn[id];
        }
    };
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
        int it = newton_stage<FT, M, PERCOL, NOICE, VGF, false, true>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, w, A.cp,
                                                                       A.dp, dh, tol, atol, rtol, max_iter, conv, kappa);
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
            it = newton_stage<FT, M, PERCOL, NOICE, VGF, false, true>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, w, A.cp,
                                                                       A.dp, dh, tol, atol, rtol, max_iter, conv, kappa);
            st.iters += unsigned(it);
            newton_ok = conv;
            if (!conv && A.fixed) ++st.unconv;
        }
        double fac = 0.25; // (a stage that did not converge)
        bool accept = A.fixed != 0;
        if (!A.fixed && newton_ok) {
            // the error estimate: rhs b1 h f_n + b2 z_g + b3 z_1 and J re-formed at Y_1 (the stage-2 face
            // states).  (Tried: the factorisation of stage 2's last Newton iteration kept for this solve -- two
            // more planes, no closures in the sweep -- measured 4-8 % slower and removed)
            const FT hf = FT(hh);
            auto rhs = [&](int64_t idx, FT v) {
                const FT f0 = fn[idx], v0 = yn[idx];
                const FT zg = (yg[idx] - (v0 + dh * f0)) * inv_d;
                const FT z1 = (v - w[idx]) * inv_d;
                return b1 * (hf * f0) + b2 * zg + b3 * z1;
            };
            column_sweep_up<FT, M, PERCOL, NOICE, VGF, true>(
                mm, P, S, fsb, fst, col, y, A.ti, ti_b, dh, A.cp, A.dp,
                [&](int64_t idx, FT v, FT) { return -rhs(idx, v); }); // (R = -rhs: the sweep solves J e = -R)
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
            restore();
            h = hh * fac;
            if (!(h >= hmin)) { failed = true; break; }
        }
    }
    st.steps = steps;
    st.failed = failed ? 1u : 0u;
    if (A.dt_cols) A.dt_cols[col] = failed ? FT(0) : FT(h);
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
trbdf2_kernel(const DevParams<FT> P, const Trbdf2Args<FT> A) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    if (col < P.ncols) trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, P, A, col, st);
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

template <typename FT>
void launch_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, bool percol, bool noice, int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    });
}

#define LH_INSTANTIATE_IMPLICIT(FT)                                                                                  \
    template void launch_implicit_euler<FT>(const DevParams<FT>&, const ImplicitArgs<FT>&, bool, bool, int, hipStream_t); \
    template void launch_trbdf2<FT>(const DevParams<FT>&, const Trbdf2Args<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
