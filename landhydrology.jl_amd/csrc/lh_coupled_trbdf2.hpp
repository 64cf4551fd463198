// lh_coupled_trbdf2.hpp -- adaptive TR-BDF2 (lh_integrate_coupled_trbdf2) of the coupled model,
// SoilEnergyModel + SoilHydrologyModel without conductivity factors, on gfx950.
//
// The method is trbdf2_column's (lh_implicit.hpp) on both components, every stage the block-triangular solve
// of coupled_implicit_column (lh_coupled_implicit.hpp): with gamma = 2 - sqrt(2), d = gamma / 2 and h the
// column's step,
//   stage 1: Y_g - w1 - d h f(Y_g, t + gamma h) = 0,  w1 = Y_n + d h f_n
//   stage 2: Y_1 - w2 - d h f(Y_1, t + h) = 0,        w2 = (Y_g - (1-gamma)^2 Y_n) / (gamma (2-gamma))
// the water by newton_stage in its adaptive mode, then the energy by one tridiagonal solve at the new
// vartheta_l; z = (Y - w) / d, f_n+1 = z_1 / h.  The error estimate filters r = b1 h f_n + b2 z_g + b3 z_1 by the
// two diagonal blocks of I - d h J(Y_1) (the eigenvalues of a block-triangular matrix are those of its
// diagonal blocks; d h J_ew e_w is dropped):
//   water:  (I - d h J_ww) e_w = r_w     trbdf2_column's error sweep
//   energy: (I - d h J_ee) e_e = r_e     the stage-2 energy matrix against r_e alone (energy_sweep_up<HOMOG>):
//           never the difference of two stage solutions of size |rhoe_int|
//   E = sqrt((sum_i q_w,i^2 + sum_i q_e,i^2) / (2 nlev)),  q_w = e_w / (abstol + reltol max(|v_n|, |v_1|)),
//                                                           q_e = e_e / (abstol_e + reltol max(|rhoe_n|, |rhoe_1|))
// and trbdf2_column's controller.  One lane owns one column with its own t and h (double): no collective.
// Planes: the water's six of trbdf2_column (Y_n, f_n, Y_g, w, c', d') and four of the energy (Y_n, f_n, Y_g, w2);
// rhoe_int's own plane receives the candidate Y_1 and is restored from Y_n by a reject.
#pragma once
#include "lh_coupled_implicit.hpp" // energy_sweep_up; with it lh_implicit.hpp (newton_stage, column_sweep_up, ColumnSolve)

namespace lh {

// One column (lane) from t0 to t1.  nonfinite: an accepted result was not finite.
template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF, typename OUT = NoStepOutput>
__device__ __forceinline__ void coupled_trbdf2_column(const M& mm, const DevParams<FT>& P0, const CoupledTrbdf2Args<FT>& A,
                                                      int64_t col, Trbdf2ColStats& st, bool& nonfinite, OUT output = OUT()) {
    constexpr bool vgf = VGF && M::uses_tables;
    DevParams<FT> P = P0; // (the lane's own: its boundary values are those of its own stage times)
    const ColumnSolve<FT, M, PERCOL, NOICE> S(mm, P, col);
    const int n = P.nlev;
    const int64_t stride = P.stride;
    // (what only a face state or a sweep's start reads is formed there, not carried through the Newton iterations)
    auto top = [&]() { return int64_t(n - 1) * stride + col; };
    const FT T = FT(288); // (read by nothing: no conductivity factors on this path)
    const double gam = 2.0 - 1.4142135623730951, dg = 0.5 * gam;
    const FT c_yn = FT((1.0 - gam) * (1.0 - gam)), c_w2 = FT(1.0 / (gam * (2.0 - gam)));
    const FT b1 = FT((1.0 - 1.4142135623730951) / 3.0), b2 = FT(1.0 / 3.0), b3 = FT((1.4142135623730951 - 2.0) / 3.0);
    const FT inv_d = FT(1.0 / dg);
    const FT atol = FT(A.abstol), atol_e = FT(A.abstol_e), rtol = FT(A.reltol);
    const FT ti_b = NOICE ? FT(0) : A.ti[col];
    auto ti_t = [&]() { return NOICE ? FT(0) : A.ti[top()]; };
    FT* const y = A.y;
    FT* const e = A.e;
    FT* const yn = A.yn;
    FT* const fn = A.fn;
    FT* const yg = A.yg;
    FT* const w = A.w;
    FT* const en = A.en;
    FT* const fe = A.fe;
    FT* const eg = A.eg;
    FT* const we = A.we;
    // boundary values at time t: linear in t between the call's two ends (or lh_set_bc's constants), as
    // trbdf2_column's faces_at.  One component at a time, each assigned whole from the launch's constants and t:
    // the energy's values are set after the water stage of the same time, so they are not live through Newton.
    auto values_at = [&](double t, int comp) {
        const double s = A.t1 > A.t0 ? (t - A.t0) / (A.t1 - A.t0) : 1.0;
        P.bc_value[FACE_BOTTOM][comp] = A.has_bcv ? FT(A.bcv[comp] + (A.bcv[4 + comp] - A.bcv[comp]) * s) : P0.bc_value[FACE_BOTTOM][comp];
        P.bc_value[FACE_TOP][comp] = A.has_bcv ? FT(A.bcv[2 + comp] + (A.bcv[6 + comp] - A.bcv[2 + comp]) * s) : P0.bc_value[FACE_TOP][comp];
    };
    // the face states at the boundary values P holds, as coupled_implicit_column: the water's read the boundary
    // value and the boundary cell's theta_i only, the energy's the water state y
    auto water_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        fsb = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_BOTTOM, col, FT(0), ti_b, T, vgf);
        fst = face_state<FT, M, MODEL_RICHARDS, false, NOICE>(mm, P, S.c, FACE_TOP, col, FT(0), ti_t(), T, vgf);
    };
    auto energy_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        fsb = face_state<FT, M, MODEL_COUPLED, false, NOICE>(mm, P, S.c, FACE_BOTTOM, col, y[col], ti_b, FT(0), vgf);
        fst = face_state<FT, M, MODEL_COUPLED, false, NOICE>(mm, P, S.c, FACE_TOP, col, y[top()], ti_t(), FT(0), vgf);
    };
    // the water stage Y - w - dh f_w(Y) = 0 at the boundary values P holds; false: Newton did not converge
    auto water_stage = [&](double ts, FT dh) {
        values_at(ts, COMP_HYDROLOGY);
        FaceState<FT> fsb, fst;
        water_faces(fsb, fst);
        bool conv;
        const int it = newton_stage<FT, M, PERCOL, NOICE, VGF, false, true>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, w, A.cp, A.dp,
                                                                             dh, FT(0), atol, rtol, A.newton_max, conv, A.kappa);
        st.iters += unsigned(it);
        return conv;
    };
    // one energy solve at the water state y and the boundary values P holds: the stage Y - in - dh f_e(Y) = 0, or
    // with HOMOG (I - dh J_ee) x = in; out(idx, x_i) top down.  (The sweep's own non-finite fold sees every
    // attempt: only accepted results count here, so it goes to a local.)
    auto energy_solve = [&](auto homog, double ts, FT dh, auto&& in, auto&& out) {
        values_at(ts, COMP_ENERGY);
        FaceState<FT> fsb, fst;
        energy_faces(fsb, fst);
        FT nf = FT(0);
        energy_sweep_up<FT, M, PERCOL, NOICE, VGF, true, decltype(homog)::value>(mm, P, S, fsb, fst, col, y, A.ti, dh, A.cp, A.dp, nf,
                                                                                 in, [](int64_t, FT) {});
        FT xnext = FT(0);
        int64_t idx = top();
        for (int i = n - 1; i >= 0; --i) {
            xnext = A.dp[idx] + A.cp[idx] * xnext;
            out(idx, xnext);
            idx -= stride;
        }
    };

    // f_n of the first step: one tendency sweep per component at (Y, t0)
    values_at(A.t0, COMP_HYDROLOGY);
    values_at(A.t0, COMP_ENERGY);
    {
        FaceState<FT> fsb, fst;
        water_faces(fsb, fst);
        column_sweep_up<FT, M, PERCOL, NOICE, VGF, false>(mm, P, S, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
                                                          [&](int64_t idx, FT, FT f) { fn[idx] = f; return FT(0); });
        FaceState<FT> eb, et;
        energy_faces(eb, et);
        FT nf = FT(0);
        energy_sweep_up<FT, M, PERCOL, NOICE, VGF, false>(mm, P, S, eb, et, col, y, A.ti, FT(0), nullptr, nullptr, nf,
                                                           [&](int, int64_t idx) { return e[idx]; },
                                                           [&](int64_t idx, FT f) { fe[idx] = f; });
    }
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
        const bool clip = t + h * (1.0 + 1e-10) >= A.t1; // land on t1 exactly
        const double hh = clip ? A.t1 - t : h;
        const FT dh = FT(dg * hh);
        // stage 1: Y_n of both components and the water's w1; the guess is Y_n
        int64_t idx = col;
        for (int i = 0; i < n; ++i) {
            const FT v = y[idx];
            yn[idx] = v;
            w[idx] = v + dh * fn[idx];
            en[idx] = e[idx];
            idx += stride;
        }
        bool newton_ok = water_stage(t + gam * hh, dh);
        if (newton_ok) {
            energy_solve(std::false_type{}, t + gam * hh, dh, [&](int, int64_t id) { return en[id] + dh * fe[id]; },
                         [&](int64_t id, FT x) { eg[id] = x; });
            // stage 2: Y_g and w2; the guess is Y_g
            idx = col;
            for (int i = 0; i < n; ++i) {
                const FT v = y[idx];
                yg[idx] = v;
                w[idx] = (v - c_yn * yn[idx]) * c_w2;
                idx += stride;
            }
            newton_ok = water_stage(t + hh, dh);
        }
        double fac = 0.25; // (a water stage that did not converge)
        bool accept = false;
        if (newton_ok) {
            energy_solve(std::false_type{}, t + hh, dh,
                         [&](int, int64_t id) {
                             const FT x = (eg[id] - c_yn * en[id]) * c_w2;
                             we[id] = x;
                             return x;
                         },
                         [&](int64_t id, FT x) { e[id] = x; });
            // the error estimate, one component after the other (only the sum crosses): the water's as
            // trbdf2_column, J_ww re-formed at Y_1 and the stage-2 face states ...
            const FT hf = FT(hh);
            double sum = 0.0;
            {
                FaceState<FT> fsb, fst;
                water_faces(fsb, fst);
                column_sweep_up<FT, M, PERCOL, NOICE, VGF, true>(
                    mm, P, S, fsb, fst, col, y, A.ti, ti_b, dh, A.cp, A.dp, [&](int64_t id, FT v, FT) {
                        const FT f0 = fn[id], v0 = yn[id];
                        const FT zg = (yg[id] - (v0 + dh * f0)) * inv_d;
                        const FT z1 = (v - w[id]) * inv_d;
                        return -(b1 * (hf * f0) + b2 * zg + b3 * z1); // (R = -rhs: the sweep solves J e = -R)
                    });
                FT enext = FT(0);
                idx = top();
                for (int i = n - 1; i >= 0; --i) {
                    const FT ev = A.dp[idx] - A.cp[idx] * enext;
                    enext = ev;
                    const FT a0 = yn[idx] < FT(0) ? -yn[idx] : yn[idx];
                    const FT a1 = y[idx] < FT(0) ? -y[idx] : y[idx];
                    const double q = double(ev) / double(atol + rtol * (a0 > a1 ? a0 : a1));
                    sum += q * q;
                    idx -= stride;
                }
            }
            // ... the energy's against the stage-2 energy matrix, homogeneous
            energy_solve(std::true_type{}, t + hh, dh,
                         [&](int, int64_t id) {
                             const FT f0 = fe[id];
                             const FT zg = (eg[id] - (en[id] + dh * f0)) * inv_d;
                             const FT z1 = (e[id] - we[id]) * inv_d;
                             return b1 * (hf * f0) + b2 * zg + b3 * z1;
                         },
                         [&](int64_t id, FT ev) {
                             const FT a0 = en[id] < FT(0) ? -en[id] : en[id];
                             const FT a1 = e[id] < FT(0) ? -e[id] : e[id];
                             const double q = double(ev) / double(atol_e + rtol * (a0 > a1 ? a0 : a1));
                             sum += q * q;
                         });
            const double E = sqrt(sum / (2.0 * n));
            fac = 0.9 * pow(E, -1.0 / 3.0);
            fac = fac != fac ? 0.2 : fmin(fmax(fac, 0.2), 5.0);
            accept = E <= 1.0;
        }
        if (accept) {
            ++st.accepted;
            output(t, clip ? A.t1 : t + hh, hh);
            t = clip ? A.t1 : t + hh; // (assigned: the column lands on t1 exactly)
            h = (clip && fac >= 1.0) ? fmax(hh * fac, h) : hh * fac;
            // the accepted result's finiteness and, as trbdf2_column, f_n+1 = z_1 / h where a next step follows
            const bool more = t < A.t1;
            const FT inv_dh = FT(1.0 / (dg * hh));
            idx = col;
            for (int i = 0; i < n; ++i) {
                const FT v = y[idx], x = e[idx];
                if (more) {
                    fn[idx] = (v - w[idx]) * inv_dh;
                    fe[idx] = (x - we[idx]) * inv_dh;
                }
                nonfinite = nonfinite || !(v - v == FT(0)) || !(x - x == FT(0)); // (inf - inf and NaN - NaN are NaN)
                idx += stride;
            }
        } else {
            ++st.rejected;
            idx = col;
            for (int i = 0; i < n; ++i) { // back to the last accepted state
                y[idx] = yn[idx];
                e[idx] = en[idx];
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

template <typename FT, typename M, bool PERCOL, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<M>())
coupled_trbdf2_kernel(const DevParams<FT> P, const CoupledTrbdf2Args<FT> A) {
    const M mm = implicit_math<M>(P.math_tab);
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    bool nonfinite = false;
    if (col < P.ncols) coupled_trbdf2_column<FT, M, PERCOL, NOICE, VGF>(mm, P, A, col, st, nonfinite);
    if (nonfinite) atomicOr(P.status, 1u);
    // (every lane of the wave gets here, those past the last column with zeros): one atomic per counter and wave
    unsigned long long acc = st.accepted, rej = st.rejected, its = st.iters, fl = st.failed;
    unsigned long long mx = st.steps;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        rej += __shfl_xor(rej, off, 64);
        its += __shfl_xor(its, off, 64);
        fl += __shfl_xor(fl, off, 64);
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
    }
}

template <typename FT>
void launch_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, bool percol, bool noice, int math,
                           hipStream_t s) {
    with_implicit_variant(P, percol, noice, math, [&](auto m, auto pc, auto ni, auto vg) {
        using M = typename decltype(m)::type;
        hipLaunchKernelGGL((coupled_trbdf2_kernel<FT, M, decltype(pc)::value, decltype(ni)::value, decltype(vg)::value>),
                           grid_for(P.ncols, implicit_threads<M>()), dim3(implicit_threads<M>()), 0, s, P, A);
    });
}

#define LH_INSTANTIATE_COUPLED_TRBDF2(FT) \
    template void launch_coupled_trbdf2<FT>(const DevParams<FT>&, const CoupledTrbdf2Args<FT>&, bool, bool, int, hipStream_t);

} // namespace lh
