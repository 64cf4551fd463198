// lh_coupled_implicit.hpp -- backward-Euler and fixed-step TR-BDF2 steps (lh_step_coupled_implicit) of the
// coupled model, SoilEnergyModel + SoilHydrologyModel (right_hand_side.jl:269-369), on gfx950.
//
// Without conductivity factors the coupled tendency f = (f_w, f_e) has a block lower-triangular Jacobian:
// f_w does not read rhoe_int (K and psi depend on vartheta_l and theta_i only), and f_e is AFFINE in rhoe_int at
// fixed vartheta_l, theta_i (T = beta + alpha rhoe_int with alpha = 1 / rho_c_s; kappa reads no temperature; the
// advected energy rho_l c_l (T - T_ref) K grad h and the energy boundary fluxes are affine in T).  A stage
// equation Y - w - c f(Y) = 0 is therefore solved EXACTLY by
//   1. the water stage: newton_stage (lh_implicit.hpp) on the vartheta_l plane, the Richards closures and faces;
//   2. the energy stage: one tridiagonal solve at the new vartheta_l, re-formed every stage.
// One lane owns one column (every per-level access of a wave is one coalesced row), all steps of a call run
// in one launch, as implicit_euler_kernel.
//
// The energy stage in u_i = alpha_i Y_i = T_i - beta_i.  With g_i = (kappa_i + kappa_i+1) cg2 the conductance
// of the face above cell i, q_i = ((-psi_i) - (-psi_i+1) + dz) cgw its head gradient (rhs_kernel's grouping) and
// A_i^lo = rho_l c_l K_i q_i, A_i^hi = rho_l c_l K_i+1 q_i, that face's flux is
//   Fe_i = -g_i (T_i+1 - T_i) - A_i^lo (T_i - T_ref) - A_i^hi (T_i+1 - T_ref),
// and row i of the stage matrix is (-l_i, d_i, -p_i) with
//   p_i = c (g_i + A_i^hi)   (row i, column i+1),     l_i+1 = c (g_i - A_i^lo)   (row i+1, column i),
//   d_i = rho_c_s,i + p_i-1 + l_i+1 [+ c G_b] [+ c G_t]:
// every COLUMN of the matrix sums to rho_c_s,i (+ the Dirichlet conductances) -- that is the conservation of
// energy, and in column sums the advective parts cancel exactly: the water's divergence, which makes the ROW
// sums sign-indefinite, does not appear.  So the subtraction-free elimination of lh_heat_implicit.hpp carries
// over in its transposed form: with t_i the pivot without the entry below it,
//   t_0 = rho_c_s,0 + c G_b,   t_i = rho_c_s,i + p_i-1 t_i-1 / pi_i-1 [+ c G_t],   pi_i = t_i + l_i+1,
//   forward r'_i = r_i + (l_i / pi_i-1) r'_i-1,   back u_i = (r'_i + p_i u_i+1) / pi_i.
// g +- A is one rounding of a conductance with a perturbation of relative size <= 5e-4 (measured), not a
// cancellation; everything else is sums and products of positive numbers while p, l >= 0 (cell Peclet
// number below 2: an M-matrix), and exactly Thomas' algorithm otherwise.
// r_i = w_i + c f_e,i(T = beta): the tendency at u = 0, rhs_kernel's faces with T replaced by beta.
#pragma once
#include "lh_implicit.hpp" // newton_stage, column_sweep_up, ColumnSolve, with_implicit_variant

namespace lh {

// The water stage of a context with the impedance factor (coupled_implicit_column<FACTORS = true>): defined in
// lh_factors_implicit.hpp, which lh_coupled_factors_implicit.hpp includes before this header; declared here so that
// the one stage sequence below can name them.  No other translation unit instantiates that branch.
template <typename FT>
struct PrescribedT;
template <typename FT, typename M, bool PERCOL, bool VGF>
__device__ __forceinline__ void factors_face_states(const M& mm, const DevParams<FT>& P,
                                                    const ColumnSolve<FT, M, PERCOL, false>& S, int64_t col, FT ti_b,
                                                    FT ti_t, FT T_b, FT T_t, FaceState<FT>& fsb, FaceState<FT>& fst);
template <typename FT, typename M, bool PERCOL, bool VGF, bool WFIRST, bool ADAPT>
__device__ __forceinline__ int factors_newton_stage(const M& mm, const DevParams<FT>& P,
                                                    const ColumnSolve<FT, M, PERCOL, false>& S, const FaceState<FT>& fsb,
                                                    const FaceState<FT>& fst, int64_t col, FT* y, const FT* ti,
                                                    const PrescribedT<FT>& Tp, FT* w, FT* cp, FT* dp, FT coef, FT tol,
                                                    FT atol, FT rtol, int max_iter, bool& conv, bool& nonfinite, FT kappa);
template <typename FT, typename M, bool PERCOL, bool VGF, bool JAC, typename Row>
__device__ __forceinline__ void factors_sweep_up(const M& mm, const DevParams<FT>& P,
                                                 const ColumnSolve<FT, M, PERCOL, false>& S, const FaceState<FT>& fsb,
                                                 const FaceState<FT>& fst, int64_t col, const FT* y, const FT* ti,
                                                 const PrescribedT<FT>& Tp, FT coef, FT* cp, FT* dp, Row&& row);

// One upward sweep of the energy equation over a column at the water state y (a rolling window of two
// cells' closures).  SOLVE: row i of the stage matrix and r_i = in(i, idx) + coef f_e,i(T = beta), eliminated
// forward; cp, dp receive the back substitution's Y_i = dp_i + cp_i Y_i+1.  Otherwise in(i, idx) is rhoe_int
// and out(idx, f_e,i) receives the tendency.  SOLVE with HOMOG: the same matrix against r_i = in(i, idx) alone (no
// tendency at T = beta, no boundary offset): the error filter of lh_coupled_trbdf2.hpp.  FACTORS: K with the
// conductivity factors (the impedance; no viscosity, so no closure reads T), in the matrix's advective entries and
// in the right-hand side alike (lh_coupled_factors_implicit.hpp).
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, bool SOLVE, bool HOMOG = false, bool FACTORS = false,
          typename In, typename Out>
__device__ __forceinline__ void energy_sweep_up(const M& mm, const DevParams<FT>& P,
                                                const ColumnSolve<FT, M, PERCOL, NOICE>& S, const FaceState<FT>& fsb,
                                                const FaceState<FT>& fst, int64_t col, const FT* y, const FT* ti,
                                                FT coef, FT* cp, FT* dp, FT& nf_acc, In&& in, Out&& out) {
    constexpr bool RELK = ColumnSolve<FT, M, PERCOL, NOICE>::RELK;
    constexpr bool vgf = VGF && M::uses_tables;
    const ColC<FT>& c = S.c;
    const FT Ksc = S.Ksc, cgw = S.cgw;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    // K, -psi as the water stage formed them; beta = T(rhoe_int = 0), alpha = 1 / rho_c_s; kappa
    auto cell = [&](int64_t id, FT& K, FT& np, FT& al, FT& be, FT& kap, FT& rcs) {
        const FT v = y[id];
        const FT tiv = NOICE ? FT(0) : ti[id];
        nf_acc = fma_ft(v, FT(0), nf_acc);
        water_closures<FT, M, FACTORS, true, false, NOICE, RELK, false, true>(mm, P, c, v, tiv, FT(288), K, np, nullptr, vgf);
        be = temperature_closure<FT, M, NOICE>(mm, P, c, v, tiv, FT(0), rcs);
        al = M::is_production ? mm.rcp(rcs) : FT(1) / rcs;
        kap = kappa_closure<FT, M, NOICE>(mm, P, c, v, tiv);
    };
    const FT inv_dzb = FT(2) * P.inv_dz;
    const FT Gb = P.bc_kind[FACE_BOTTOM][COMP_ENERGY] == BC_DIRICHLET ? (fsb.kap * inv_dzb) * P.inv_dz : FT(0);
    const FT Gt = P.bc_kind[FACE_TOP][COMP_ENERGY] == BC_DIRICHLET ? (fst.kap * inv_dzb) * P.inv_dz : FT(0);
    int64_t idx = col;
    FT K, np, al, be, kap, rcs;
    cell(idx, K, np, al, be, kap, rcs);
    FT u = FT(0); // T - beta of the cell (tendency sweep)
    if constexpr (!SOLVE) u = al * in(0, idx);
    FT Flo = FT(0);
    if constexpr (!HOMOG) { // (the homogeneous solve reads no flux: the matrix alone)
        FT fe, fw; // the boundary face at T_c = beta (a Dirichlet face is affine in T_c: - G_b u on top)
        boundary_fluxes_from<FT, MODEL_COUPLED>(P, fsb, FACE_BOTTOM, col, be, K * Ksc, -np, fe, fw);
        Flo = fe * P.inv_dz - Gb * u;
    }
    FT p_lo = FT(0), l_lo = FT(0);                      // p_i-1 and l_i
    FT t_prev = FT(0), ipi_prev = FT(0), rp_prev = FT(0); // t, 1 / pi and r' of the cell below
    for (int i = 0; i < n; ++i) {
        FT Fhi = FT(0), p_hi = FT(0), l_up = FT(0);
        FT Ku = FT(0), npu = FT(0), alu = FT(0), beu = FT(0), kapu = FT(0), rcsu = FT(0), uu = FT(0);
        const int64_t idu = idx + stride;
        if (i + 1 < n) {
            cell(idu, Ku, npu, alu, beu, kapu, rcsu);
            // interior_face's energy flux (lh_column_ops.hpp): -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2) - (E_lo + E_hi) gh
            const FT gh = head_difference(npu, np, P.dz) * cgw;
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
            FT fe, fw;
            boundary_fluxes_from<FT, MODEL_COUPLED>(P, fst, FACE_TOP, col, be, K * Ksc, -np, fe, fw);
            Fhi = fe * P.inv_dz + Gt * u;
        }
        const FT f = Flo - Fhi; // rhs_kernel's emit
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

// One column (lane) through all steps of the call.  my_max, unconv, total: the water stages' Newton statistics;
// nf_acc becomes NaN once a result is non-finite.  FACTORS (with NOICE = false): the context has the impedance factor
// and no viscosity factor -- the water stage is lh_factors_implicit.hpp's, K of the energy stage
// carries the factor, and the stage sequence is this one.
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, bool TRBDF2, bool FACTORS = false>
__device__ __forceinline__ void coupled_implicit_column(const M& mm, DevParams<FT> P, const CoupledImplicitArgs<FT>& A,
                                                        int64_t col, int& my_max, unsigned long long& unconv,
                                                        unsigned long long& total, FT& nf_acc) {
    constexpr bool vgf = VGF && M::uses_tables;
    const ColumnSolve<FT, M, PERCOL, NOICE> S(mm, P, col);
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const int64_t top = int64_t(n - 1) * stride + col;
    static_assert(!(FACTORS && NOICE), "the impedance factor reads theta_i: no NOICE variant");
    const FT T = FT(288); // (read by nothing: no viscosity factor on either path)
    const FT coef = A.coef; // dt, or d dt of both TR-BDF2 stages
    FT* const y = A.y;
    FT* const e = A.e;
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    const FT ti_t = NOICE ? FT(0) : A.ti[top];
    // the water stage Y - w - coef f_w(Y) = 0 at the boundary values P holds: newton_stage, as implicit_column
    // the Richards face states at the boundary values P holds, as implicit_column
    auto water_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        if constexpr (FACTORS) {
            factors_face_states<FT, M, PERCOL, VGF>(mm, P, S, col, ti_b, ti_t, T, T, fsb, fst);
        } else {
            fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
            fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_TOP, col, FT(0), ti_t, T, vgf);
        }
    };
    auto water_stage = [&](auto wfirst) {
        FaceState<FT> fsb, fst;
        water_faces(fsb, fst);
        bool conv;
        int it;
        if constexpr (FACTORS) {
            // (PrescribedT::need is false: at() returns before it reads a pointer.  The plane it is given is one the
            // kernel holds anyway, not a literal NULL: a constant null base behind `need` crashes the optimizer of
            // ROCm 7.2's clang in SimplifyCFG.)
            const PrescribedT<FT> Tp(P, A.ti);
            bool nonfinite = false;
            it = factors_newton_stage<FT, M, PERCOL, VGF, decltype(wfirst)::value, false>(
                mm, P, S, fsb, fst, col, y, A.ti, Tp, A.w, A.cp, A.dp, coef, A.tol, FT(0), FT(0), A.max_iter, conv, nonfinite, FT(0));
            if (nonfinite) nf_acc = FT(NAN);
        } else {
            it = newton_stage<FT, M, PERCOL, NOICE, VGF, decltype(wfirst)::value, false>(
                mm, P, S, fsb, fst, col, y, A.ti, ti_b, A.w, A.cp, A.dp, coef, A.tol, FT(0), FT(0), A.max_iter, conv);
        }
        my_max = it > my_max ? it : my_max;
        total += unsigned(it);
        if (!conv) ++unconv;
    };
    // the energy face states at the water state y: kappa of a Dirichlet energy face at the face's vartheta_l (the
    // hydrology's Dirichlet value, else the boundary cell's new value), FaceState::T the boundary value.
    // (face_state<MODEL_COUPLED> also evaluates the water closure of a Dirichlet hydrology face, which the energy does
    // not read; face_state<MODEL_HEAT> on a hand-picked vartheta_l avoids that and cost 8-24 bytes of scratch per lane)
    auto energy_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        fsb = face_state<FT, M, MODEL_COUPLED, FACTORS, NOICE>(mm, P, S.c, FACE_BOTTOM, col, y[col], ti_b, FT(0), vgf);
        fst = face_state<FT, M, MODEL_COUPLED, FACTORS, NOICE>(mm, P, S.c, FACE_TOP, col, y[top], ti_t, FT(0), vgf);
    };
    // the energy stage Y - w - coef f_e(Y) = 0 at the water state y: w = in(i, idx), out(idx, Y_i) top down
    auto energy_stage = [&](auto&& in, auto&& out) {
        FaceState<FT> fsb, fst;
        energy_faces(fsb, fst);
        energy_sweep_up<FT, M, PERCOL, NOICE, VGF, true, false, FACTORS>(mm, P, S, fsb, fst, col, y, A.ti, coef, A.cp, A.dp,
                                                                         nf_acc, in, [](int64_t, FT) {});
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
            water_faces(fsb, fst);
            auto to_fn = [&](int64_t idx, FT, FT f) { fn[idx] = f; return FT(0); };
            if constexpr (FACTORS)
                factors_sweep_up<FT, M, PERCOL, VGF, false>(mm, P, S, fsb, fst, col, y, A.ti, PrescribedT<FT>(P, A.ti), FT(0),
                                                            nullptr, nullptr, to_fn);
            else
                column_sweep_up<FT, M, PERCOL, NOICE, VGF, false>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
                                                                  to_fn);
            FaceState<FT> eb, et;
            energy_faces(eb, et);
            energy_sweep_up<FT, M, PERCOL, NOICE, VGF, false, false, FACTORS>(mm, P, S, eb, et, col, y, A.ti, coef, nullptr, nullptr,
                                                                              nf_acc, [&](int, int64_t idx) { return e[idx]; },
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
                const FT m[4] = {g0 * b0[0] + g1 * b1[0], g0 * b0[1] + g1 * b1[1], g0 * b0[2] + g1 * b1[2], g0 * b0[3] + g1 * b1[3]};
                P.bc_value[FACE_BOTTOM][COMP_ENERGY] = m[0];
                P.bc_value[FACE_BOTTOM][COMP_HYDROLOGY] = m[1];
                P.bc_value[FACE_TOP][COMP_ENERGY] = m[2];
                P.bc_value[FACE_TOP][COMP_HYDROLOGY] = m[3];
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

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, bool TRBDF2>
__global__ void __launch_bounds__(implicit_threads<M>())
coupled_implicit_kernel(const DevParams<FT> P, const CoupledImplicitArgs<FT> A) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    int my_max = 0;
    unsigned long long unconv = 0, total = 0;
    FT nf_acc = FT(0);
    if (col < P.ncols) coupled_implicit_column<FT, M, PERCOL, NOICE, VGF, TRBDF2>(mm, P, A, col, my_max, unconv, total, nf_acc);
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
void launch_coupled_implicit(const DevParams<FT>& P, const CoupledImplicitArgs<FT>& A, bool percol, bool noice,
                             bool trbdf2, int math, hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) { with_bool(trbdf2, [&](auto tr) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((coupled_implicit_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value, decltype(tr)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    }); });
}

#define LH_INSTANTIATE_COUPLED_IMPLICIT(FT) \
    template void launch_coupled_implicit<FT>(const DevParams<FT>&, const CoupledImplicitArgs<FT>&, bool, bool, bool, int, hipStream_t);

} // namespace lh
