// lh_atmos.hpp -- the prescribed-atmosphere top boundary condition on the device (gfx950).
//
// boundary_fluxes(X, bc::PrescribedAtmosForcing, :top, ...) and compute_turbulent_surface_fluxes
// (src/SoilModel/boundary_conditions.jl:516-533, 553-620): from the top cell's (vartheta_l,
// theta_i, T) and the prescribed atmospheric state, the heat flux and the water volume flux
// through the soil surface by Monin-Obukhov similarity.  One lane per column, evaluated in place
// on the device-resident state (no host hop); the two per-column fluxes land in context-owned
// arrays that the column kernel consumes as per-column VerticalFlux values at the top face.
//
// PARITY UNPINNED beyond the reference's equilibrium invariant (test_prescribed_atmos_bc.jl:75-79,
// :138-141): the function's own lines are followed op for op, but the three calls it makes into
// SurfaceFluxes.jl 0.1 / Thermodynamics.jl 0.5 -- packages that are not under the reference
// tree -- are restated from their published forms:
//   q_vap_saturation_generic(param_set, T, rho, Liquid()):
//       p_sat = press_triple (T/T_triple)^(dcp/R_v) exp((LH_v0 - dcp T_0)/R_v (1/T_triple - 1/T)),
//       dcp = cp_v - cp_l;  q_sat = p_sat / (rho R_v T)
//   cp_m(param_set, PhasePartition(q)) = cp_d + (cp_v - cp_d) q
//   surface_conditions(..., DGScheme()): Businger universal functions as in Nishizawa & Kitamura
//       (2018) Eqs. A1-A6 (a = 4.7, Pr_0 = 0.74, gamma_m = 15, gamma_h = 9), point form
//           x*_i = (kappa/pi_i) dx_i / (ln(z/z0_i) - psi_i(z/L) + psi_i(z0_i/L)),
//           L = -u*^3 theta_scale / (kappa g (-u* theta*)).
//       u* and theta* are explicit in s = 1/L and q* does not feed back, so the package's
//       4-unknown Newton problem (residual tolerance sqrt(eps)) is the scalar equation
//           G(s) = kappa g theta*(s) / (u*(s)^2 theta_scale) - s = 0,
//       solved here by bracketing + Illinois regula falsi to rounding level.  Neutral
//       (theta_atm == T): s = 0 and theta* = 0 exactly.  No root (bulk Richardson number past
//       1/a): NaN fluxes and status bit 1 -- the reference's Newton iteration does not converge
//       there either.
#pragma once
#include "lh_closures.hpp"
#include "lh_dispatch.hpp"

namespace lh {

namespace atm {

__device__ __forceinline__ double xlog(double x) { return ::log(x); }
__device__ __forceinline__ float xlog(float x) { return ::logf(x); }
__device__ __forceinline__ double xexp(double x) { return ::exp(x); }
__device__ __forceinline__ float xexp(float x) { return ::expf(x); }
__device__ __forceinline__ double xpow(double x, double y) { return ::pow(x, y); }
__device__ __forceinline__ float xpow(float x, float y) { return ::powf(x, y); }
__device__ __forceinline__ double xsqrt(double x) { return ::sqrt(x); }
__device__ __forceinline__ float xsqrt(float x) { return ::sqrtf(x); }
__device__ __forceinline__ double xatan(double x) { return ::atan(x); }
__device__ __forceinline__ float xatan(float x) { return ::atanf(x); }
__device__ __forceinline__ double xabs(double x) { return ::fabs(x); }
__device__ __forceinline__ float xabs(float x) { return ::fabsf(x); }

template <typename FT>
__device__ inline FT psi_m(FT zeta) {
    if (zeta < FT(0)) {
        const FT f = xsqrt(xsqrt(FT(1) - FT(15) * zeta));
        return xlog((FT(1) + f) * (FT(1) + f) * (FT(1) + f * f) / FT(8)) - FT(2) * xatan(f) +
               FT(3.14159265358979323846) / FT(2);
    }
    return -FT(4.7) * zeta;
}
template <typename FT>
__device__ inline FT psi_h(FT zeta) {
    if (zeta < FT(0)) {
        const FT f = xsqrt(FT(1) - FT(9) * zeta);
        return FT(2) * xlog((FT(1) + f) / FT(2));
    }
    return -FT(4.7) * zeta / FT(0.74);
}

template <typename FT>
struct Problem {
    FT kappa, g, z, z0m, z0s, lm, lh, du, dth, th_scale;
    __device__ FT ustar(FT s) const { return kappa * du / (lm - psi_m<FT>(z * s) + psi_m<FT>(z0m * s)); }
    __device__ FT scalar_coeff(FT s) const { // x* / (x_in - x_s) for theta and q
        return (kappa / FT(0.74)) / (lh - psi_h<FT>(z * s) + psi_h<FT>(z0s * s));
    }
    __device__ FT residual(FT s) const {
        const FT us = ustar(s);
        const FT ts = scalar_coeff(s) * dth;
        return kappa * g * ts / (us * us * th_scale) - s;
    }
};

// s = 1/L of the Monin-Obukhov system; false when no sign change is found
template <typename FT>
__device__ inline bool solve(const Problem<FT>& p, FT& s_out) {
    s_out = FT(0);
    if (p.dth == FT(0) || p.du == FT(0)) return true; // neutral (or calm: no turbulent flux at all)
    FT a = FT(0), Ga = p.residual(a);
    if (Ga == FT(0)) return true;
    FT b = (p.dth > FT(0) ? FT(1) : FT(-1)) / (FT(100) * p.z); // the reference's guess: L = 100 z_atm
    FT Gb = p.residual(b);
    int it = 0;
    while ((Gb > FT(0)) == (Ga > FT(0)) && Gb != FT(0)) {
        if (++it > 200 || !(xabs(b) < FT(1e30))) return false;
        a = b;
        Ga = Gb;
        b = b * FT(2);
        Gb = p.residual(b);
    }
    if (Gb == FT(0)) {
        s_out = b;
        return true;
    }
    int side = 0;
    for (it = 0; it < 200; ++it) { // Illinois
        FT c = (a * Gb - b * Ga) / (Gb - Ga);
        if (!((c > a) == (c < b) && c != a && c != b)) c = (a + b) / FT(2);
        const FT Gc = p.residual(c);
        if (Gc == FT(0)) {
            a = b = c;
            break;
        }
        if ((Gc > FT(0)) == (Gb > FT(0))) {
            b = c;
            Gb = Gc;
            if (side == -1) Ga = Ga / FT(2);
            side = -1;
        } else {
            a = c;
            Ga = Gc;
            if (side == +1) Gb = Gb / FT(2);
            side = +1;
        }
        if (xabs(b - a) <= FT(4) * Limits<FT>::eps() * xabs(b)) break;
    }
    s_out = (xabs(Ga) < xabs(Gb)) ? a : b;
    return true;
}

// compute_turbulent_surface_fluxes for one top-cell state; false = no Monin-Obukhov root
template <typename FT>
__device__ inline bool surface_fluxes(const AtmosParams<FT>& A, const ColC<FT>& c, FT u_atm, FT theta_atm,
                                      FT q_atm, FT vl, FT ti, FT T, FT& heat_flux, FT& water_flux) {
    // :573-583 -- specific humidity of the pore air at the surface
    const FT dcp = A.cp_v - A.cp_l;
    const FT p_sat = A.press_triple * xpow(T / A.T_triple, dcp / A.R_v) *
                     xexp((FT(A.LH_v0_d) - dcp * A.T_0) / A.R_v * (FT(1) / A.T_triple - FT(1) / T));
    const FT q_sat = p_sat / (A.rho_a_sfc * A.R_v * T);
    const FT nu_eff = c.nu - ti;                                   // :577
    const FT tl = liquid_fraction(vl, nu_eff);                     // :578
    // effective_saturation(nu_eff, theta_l, theta_r), clamped at 1 (:579)
    const FT safe = !(tl <= c.theta_lim) ? tl : c.theta_lim;
    FT S = (safe - c.theta_r) / (nu_eff - c.theta_r);
    if (S > FT(1)) S = FT(1);
    // matric_potential(hm, S), SoilWaterParameterizations.jl:196-200, pow for pow
    const FT psi = -xpow((xpow(S, -c.inv_m) - FT(1)) * c.alpha_pnn, c.inv_n);
    const FT correction = xexp(A.grav * psi / A.R_v / T);          // :581
    const FT q_surf = q_sat * correction;                          // :582
    // :584-603 -- x_s = [0, T, q_surf], x_in = [u_atm, theta_atm, q_atm], z_0 = [z_0m, z_0s, z_0s]
    Problem<FT> P;
    P.kappa = A.von_karman;
    P.g = A.grav;
    P.z = A.z_atm;
    P.z0m = A.z_0m;
    P.z0s = A.z_0s;
    P.lm = xlog(P.z / P.z0m);
    P.lh = xlog(P.z / P.z0s);
    P.du = u_atm - FT(0);
    P.dth = theta_atm - T;
    P.th_scale = A.theta_scale;
    FT s;
    if (!solve(P, s)) {
        heat_flux = water_flux = FT(NAN);
        return false;
    }
    const FT ustar = P.ustar(s);
    const FT ch = P.scalar_coeff(s);
    const FT tstar = ch * P.dth;
    const FT qstar = ch * (q_atm - q_surf);
    // :605-619
    const FT cpm = A.cp_d + (A.cp_v - A.cp_d) * q_surf; // cp_m(param_set, PhasePartition(q_surf))
    const FT h_d = A.cp_d * (T - A.T_0) + A.R_d * A.T_0;
    const FT E = -A.rho_a_sfc * ustar * qstar;
    const FT dse = -cpm * A.rho_a_sfc * ustar * tstar - h_d * E;
    const FT vse = FT(A.cp_v_d * double(T - A.T_0) + A.LH_v0_d) * E;
    water_flux = E / A.rho_liq;
    heat_flux = dse + vse;
    return true;
}

} // namespace atm

// One lane per column: the top cell's state -> the two top-face fluxes.
//   from_state: (vl, ti, rhoe) point at the TOP ROWS of the state's planes and T is formed by
//               temperature_from_rhoe_int (the coupled model's centre value, :291-293);
//   else:       (vl, ti, third) are plain arrays [n] of (vartheta_l, theta_i, T) -- the direct
//               evaluation behind lh_atmos_surface_fluxes.
template <typename FT, bool PERCOL>
__global__ void __launch_bounds__(256)
atmos_flux_kernel(const DevParams<FT> P, const AtmosParams<FT> A, const int64_t n, const bool from_state,
                  const FT* __restrict__ vl, const FT* __restrict__ ti, const FT* __restrict__ third,
                  FT* __restrict__ out_heat, FT* __restrict__ out_water) {
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= n) return;
    using M = MathLibm<FT>;
    const M mm;
    // per-column soil only exists for a context's own columns (from_state)
    const ColC<FT> c = make_colc<FT, M>(P, from_state ? col : 0, PERCOL && from_state);
    const FT v = vl[col], t = ti ? ti[col] : FT(0);
    FT T = third[col];
    if (from_state) {
        FT rcs;
        T = temperature_closure<FT, M>(mm, P, c, v, t, third[col], rcs);
    }
    const FT u_atm = (from_state && A.pc_u) ? A.pc_u[col] : A.u_atm;
    const FT th_atm = (from_state && A.pc_theta) ? A.pc_theta[col] : A.theta_atm;
    const FT q_atm = (from_state && A.pc_q) ? A.pc_q[col] : A.q_atm;
    FT fh, fw;
    if (!atm::surface_fluxes<FT>(A, c, u_atm, th_atm, q_atm, v, t, T, fh, fw)) atomicOr(P.status, 2u);
    out_heat[col] = fh;
    out_water[col] = fw;
}

template <typename FT>
void launch_atmos_flux(const DevParams<FT>& P, const AtmosParams<FT>& A, int64_t n, bool from_state, bool percol,
                       const FT* vl, const FT* ti, const FT* third, FT* out_heat, FT* out_water, hipStream_t s) {
    dim3 g((unsigned)((n + 255) / 256)), b(256);
    with_bool(percol, [&](auto pc) {
        hipLaunchKernelGGL((atmos_flux_kernel<FT, decltype(pc)::value>), g, b, 0, s, P, A, n, from_state, vl, ti, third, out_heat, out_water);
    });
}

} // namespace lh
