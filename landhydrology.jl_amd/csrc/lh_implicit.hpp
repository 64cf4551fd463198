// lh_implicit.hpp -- backward-Euler steps of the Richards model on gfx950 (lh_step_implicit_euler).
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
#include "lh_closures.hpp"
// (included after lh_kernels_impl.hpp: grid_for, stage_math_tables, fmin_ft / fmax_ft; ImplicitArgs is in lh_device.hpp)

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

template <typename M>
constexpr int implicit_threads() {
    return M::uses_tables ? 512 : 256; // (the Float64 tables take 48 KiB of LDS per workgroup)
}

// One column (lane) through all steps of the call: the column's largest iteration count, its
// unconverged steps and its total iterations are returned for the launch's statistics.
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__device__ __forceinline__ void implicit_column(const M& mm, DevParams<FT> P, const ImplicitArgs<FT>& A, int64_t col,
                                                int& my_max, unsigned long long& unconv, unsigned long long& total) {
    constexpr bool RELK = M::is_production; // K without Ksat, as rhs_kernel carries it
    constexpr bool vgf = VGF && M::uses_tables;
    ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    if (!NOICE) finish_colc<FT, M>(mm, c);
    const FT Ksc = RELK ? c.Ksat : FT(1);
    const FT cgw = RELK ? c.cgw : P.cg2;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const FT T = FT(288); // (read by nothing: no conductivity factors on this path)
    const FT dt = A.dt;
    const FT dmax = FT(LH_IMPLICIT_DMAX_FRAC) * (c.nu - c.theta_r);
    const FT floor_r = c.theta_r;

    auto closures = [&](FT v, FT tiv, FT& K, FT& np, FT& dK, FT& dn) {
        water_closures<FT, M, false, true, false, NOICE, RELK, false, true>(mm, P, c, v, tiv, T, K, np, nullptr, vgf);
        float dkr, dnf;
        water_slopes<FT, NOICE>(c, v, tiv, np, dkr, dnf);
        dK = FT(dkr) * (RELK ? FT(1) : c.Ksat); // in the units of K
        dn = FT(dnf);
    };

    for (int64_t s = 0; s < A.nsteps; ++s) {
        if (A.bcv) {
            const FT* b = A.bcv + s * 4;
            P.bc_value[FACE_BOTTOM][COMP_ENERGY] = b[0];
            P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = b[1];
            P.bc_value[FACE_TOP][COMP_ENERGY] = b[2];
            P.bc_value[FACE_TOP][COMP_HYDROLOGY] = b[3];
        }
        // The Dirichlet face states read the boundary value and the boundary cell's theta_i only
        // (no conductivity factors): constants of the step -- boundary_fluxes is face_state +
        // boundary_fluxes_from, so the fluxes are bitwise its own
        const FT ti_b = NOICE ? FT(0) : A.ti[col];
        const FT ti_t = NOICE ? FT(0) : A.ti[int64_t(n - 1) * stride + col];
        const FaceState<FT> fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, c, FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
        const FaceState<FT> fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, c, FACE_TOP, col, FT(0), ti_t, T, vgf);
        bool conv = false;
        int it = 0;
        FT lam = FT(1);                 // step length of the safeguard (see LH_IMPLICIT_STALL)
        FT dprev = FT(INFINITY);        // largest |Newton step| of the previous iteration
        while (it < A.max_iter && !conv) {
            // ---------------- upward sweep
            int64_t idx = col;
            FT v = A.y[idx];
            FT tic = NOICE ? FT(0) : ti_b;
            FT vn;
            if (it == 0) { vn = v; A.yn[idx] = v; } else vn = A.yn[idx];
            FT K, np, dK, dn;
            closures(v, tic, K, np, dK, dn);
            FT Flo, dFlo_lo = FT(0), dFlo_c;
            {
                FT fe, fw;
                boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fsb, FACE_BOTTOM, col, T, K * Ksc, -np, fe, fw);
                Flo = fw * P.inv_dz;
                dFlo_c = boundary_flux_slope<FT>(P, fsb, FACE_BOTTOM, dK * Ksc, dn) * P.inv_dz;
            }
            FT cp_prev = FT(0), dp_prev = FT(0);
            for (int i = 0; i < n; ++i) {
                FT Fhi, dFhi_c, dFhi_u = FT(0);
                FT vu = FT(0), vnu = FT(0), tiu = FT(0), Ku = FT(0), npu = FT(0), dKu = FT(0), dnu = FT(0);
                const int64_t idu = idx + stride;
                if (i + 1 < n) {
                    vu = A.y[idu];
                    tiu = NOICE ? FT(0) : A.ti[idu];
                    if (it == 0) { vnu = vu; A.yn[idu] = vu; } else vnu = A.yn[idu];
                    closures(vu, tiu, Ku, npu, dKu, dnu);
                    // rhs_kernel's interior face: -(K_lo + K_hi) ((npsi_lo - npsi_hi) + dz) cgw
                    const FT h = head_difference(npu, np, P.dz);
                    const FT Ks = K + Ku;
                    Fhi = -Ks * (h * cgw);
                    dFhi_c = -cgw * (dK * h + Ks * dn);
                    dFhi_u = -cgw * (dKu * h - Ks * dnu);
                } else {
                    FT fe, fw;
                    boundary_fluxes_from<FT, MODEL_RICHARDS>(P, fst, FACE_TOP, col, T, K * Ksc, -np, fe, fw);
                    Fhi = fw * P.inv_dz;
                    dFhi_c = boundary_flux_slope<FT>(P, fst, FACE_TOP, dK * Ksc, dn) * P.inv_dz;
                }
                const FT R = (v - vn) - dt * (Flo - Fhi); // f_i = F_lo - F_hi, rhs_kernel's emit
                const FT a = -dt * dFlo_lo;
                const FT b = FT(1) - dt * (dFlo_c - dFhi_c);
                const FT cc = dt * dFhi_u;
                const FT den = b - a * cp_prev;
                const FT cpi = cc / den;
                const FT dpi = (-R - a * dp_prev) / den;
                A.cp[idx] = cpi;
                A.dp[idx] = dpi;
                cp_prev = cpi;
                dp_prev = dpi;
                // slide the window: the face above becomes the face below
                Flo = Fhi;
                dFlo_lo = dFhi_c;
                dFlo_c = dFhi_u;
                v = vu; vn = vnu; K = Ku; np = npu; dK = dKu; dn = dnu;
                idx = idu;
            }
            // ---------------- downward sweep
            FT dnext = FT(0);
            bool ok = true;
            FT dbig = FT(0);
            for (int i = n - 1; i >= 0; --i) {
                const int64_t id = int64_t(i) * stride + col;
                const FT d = A.dp[id] - A.cp[id] * dnext; // (c'_{n-1} = 0)
                dnext = d;
                const FT vo = A.y[id];
                const FT du = fmin_ft(fmax_ft(lam * d, -dmax), dmax);
                FT vnew = vo + du;
                const FT fl = floor_r + FT(0.5) * (vo - floor_r);
                if (vo > floor_r) vnew = vnew < fl ? fl : vnew; // at most half way down to theta_r
                else vnew = vnew < vo ? vo : vnew;              // (at or below it already: no further)
                // the saturation kink: a cell that crosses nu_eff from below stops on it (psi' has no
                // bound just below, and a Newton step across it oscillates)
                const FT nue = NOICE ? c.nu : c.nu - A.ti[id];
                if (vo < nue && vnew > nue) vnew = nue;
                A.y[id] = vnew;
                // judged on the Newton step itself: a step the safeguard cut short is not convergence
                const FT scale = fmax_ft(vnew < FT(0) ? -vnew : vnew, c.nu);
                const FT ad = d < FT(0) ? -d : d;
                ok = ok && (ad <= A.tol * scale);
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
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    }
}

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
implicit_euler_kernel(const DevParams<FT> P, const ImplicitArgs<FT> A) {
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab)); // (every thread)
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
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
    const bool ni = noice && math != MATH_LIBM;
    const bool robust = P.vg_fast_all == 0;
#define LH_IE(MATH, PC, NI, VG)                                                                          \
    hipLaunchKernelGGL((implicit_euler_kernel<FT, MATH, PC, NI, VG>), grid_for(P.ncols, implicit_threads<MATH>()), \
                       dim3(implicit_threads<MATH>()), 0, s, P, A)
#define LH_IE_PC(MATH, NI, VG)                 \
    do {                                       \
        if (percol) LH_IE(MATH, true, NI, VG); \
        else LH_IE(MATH, false, NI, VG);       \
    } while (0)
    if (math == MATH_LIBM) {
        LH_IE_PC(MathLibm<FT>, false, false);
    } else if (sizeof(FT) == 8 && robust) { // clay-like ensembles: the v_ldexp form, as rhs_kernel
        if (ni) LH_IE_PC(MathFast<FT>, true, false);
        else LH_IE_PC(MathFast<FT>, false, false);
    } else {
        if (ni) LH_IE_PC(MathFast<FT>, true, true);
        else LH_IE_PC(MathFast<FT>, false, true);
    }
#undef LH_IE_PC
#undef LH_IE
}

#define LH_INSTANTIATE_IMPLICIT(FT) \
    template void launch_implicit_euler<FT>(const DevParams<FT>&, const ImplicitArgs<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
