// lh_layered_coupled_trbdf2.hpp -- adaptive TR-BDF2 (lh_integrate_layered_coupled_trbdf2) of the coupled model,
// SoilEnergyModel + SoilHydrologyModel, with per-CELL soil classes and their thermal supplement, on gfx950
// (DESIGN.md section 4.26).
//
// coupled_trbdf2_column (lh_coupled_trbdf2.hpp: the stages, the error estimate over both components, the controller,
// one lane per column with its own t and h) with the per-cell constants of lh_layered_coupled_implicit.hpp:
//   * a water stage is layered_newton_stage in its adaptive mode (lh_layered_implicit.hpp) with layered_face_states,
//     the water's error filter layered_sweep_up<JAC> at Y_1 with the stage-2 face states, as layered_trbdf2_column;
//   * an energy stage is one layered_energy_sweep_up<SOLVE> at the new vartheta_l with layered_energy_face, the
//     energy's error filter the same sweep with HOMOG: the stage-2 matrix against r_e alone.
// The class table and the thermal table stay in LDS and a cell's entry is read where it is used, so no instantiation
// keeps per-class constants in registers across the time loop (profiles/layered_coupled_trbdf2_kernel_regs.txt).
//
// A kernel family of its own, in its own translation units: no existing kernel changes its instructions
// (profiles/layered_coupled_trbdf2_manifest.txt); the time loop below is therefore a copy of coupled_trbdf2_column's
// -- the rule of DESIGN section 4.14.
//
// The first part (the launcher's declaration) is what lh_api.hip includes; the kernels follow under
// LH_LAYERED_COUPLED_TRBDF2_TU, which only lh_kernels_f64_layered_coupled_trbdf2.hip /
// lh_kernels_f32_layered_coupled_trbdf2.hip define (with LH_LAYERED_TU, LH_LAYERED_HEAT_TU, LH_LAYERED_IMPLICIT_TU and
// LH_LAYERED_COUPLED_IMPLICIT_TU, for the two table stagings, the closures, the water stage and the energy sweep).
#pragma once
#include "lh_layered_coupled_implicit.hpp"

namespace lh {

// NOICE and the closure form (VGF) as launch_layered_coupled_implicit's.  Production math, no conductivity factors.
template <typename FT>
void launch_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                   bool noice, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_COUPLED_TRBDF2_TU
#ifndef LH_LAYERED_COUPLED_IMPLICIT_TU
#error "lh_layered_coupled_trbdf2.hpp's kernels need lh_layered_coupled_implicit.hpp's sweeps (define LH_LAYERED_TU, LH_LAYERED_HEAT_TU, LH_LAYERED_IMPLICIT_TU and LH_LAYERED_COUPLED_IMPLICIT_TU first)"
#endif

namespace lh {

// One column (lane) from t0 to t1: coupled_trbdf2_column with per-cell constants.  nonfinite: an accepted result
// was not finite.  output: the accepted-step functor, as coupled_trbdf2_column's.
template <typename FT, typename M, bool NOICE, bool VGF, typename OUT = NoStepOutput>
__device__ __forceinline__ void layered_coupled_trbdf2_column(const M& mm, const DevParams<FT>& P0, const ClassView<FT>& C,
                                                              const ThermTable<FT>& H, const CoupledTrbdf2Args<FT>& A,
                                                              int64_t col, Trbdf2ColStats& st, bool& nonfinite,
                                                              OUT output = OUT()) {
    DevParams<FT> P = P0; // (the lane's own: its boundary values are those of its own stage times)
    const int n = P.nlev;
    const int64_t stride = P.stride;
    // (what only a face state or a sweep's start reads is formed there, not carried through the Newton iterations)
    auto top = [&]() { return int64_t(n - 1) * stride + col; };
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
    // boundary values at time t: linear in t between the call's two ends (or lh_set_bc's constants).  One component at
    // a time, each assigned whole from the launch's constants and t just before the phase that reads it: the energy's
    // values are set after the water stage of the same time, so they are not live through Newton.
    auto values_at = [&](double t, int comp) {
        const double s = A.t1 > A.t0 ? (t - A.t0) / (A.t1 - A.t0) : 1.0;
        P.bc_value[FACE_BOTTOM][comp] = A.has_bcv ? FT(A.bcv[comp] + (A.bcv[4 + comp] - A.bcv[comp]) * s) : P0.bc_value[FACE_BOTTOM][comp];
        P.bc_value[FACE_TOP][comp] = A.has_bcv ? FT(A.bcv[2 + comp] + (A.bcv[6 + comp] - A.bcv[2 + comp]) * s) : P0.bc_value[FACE_TOP][comp];
    };
    // the face states at the boundary values P holds, as layered_coupled_implicit_column: the water's read the
    // boundary value and the boundary cell's theta_i and class only, the energy's the water state y
    auto water_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        layered_face_states<FT, M, NOICE, VGF>(mm, P, C, col, ti_b, ti_t(), fsb, fst);
    };
    auto energy_faces = [&](FaceState<FT>& fsb, FaceState<FT>& fst) {
        fsb = layered_energy_face<FT, M, NOICE>(mm, P, C, H, FACE_BOTTOM, col, col, y[col], ti_b);
        fst = layered_energy_face<FT, M, NOICE>(mm, P, C, H, FACE_TOP, col, top(), y[top()], ti_t());
    };
    // the water stage Y - w - dh f_w(Y) = 0 at the boundary values P holds; false: Newton did not converge
    auto water_stage = [&](double ts, FT dh) {
        values_at(ts, COMP_HYDROLOGY);
        FaceState<FT> fsb, fst;
        water_faces(fsb, fst);
        bool conv;
        const int it = layered_newton_stage<FT, M, NOICE, VGF, false, true>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, w, A.cp, A.dp, dh,
                                                                            FT(0), atol, rtol, A.newton_max, conv, A.kappa);
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
        layered_energy_sweep_up<FT, M, NOICE, VGF, true, decltype(homog)::value>(mm, P, C, H, fsb, fst, col, y, A.ti, dh, A.cp, A.dp,
                                                                                 nf, in, [](int64_t, FT) {});
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
        layered_sweep_up<FT, M, NOICE, VGF, false>(mm, P, C, fsb, fst, col, y, A.ti, ti_b, FT(0), nullptr, nullptr,
                                                   [&](int64_t idx, FT, FT f) { fn[idx] = f; return FT(0); });
        FaceState<FT> eb, et;
        energy_faces(eb, et);
        FT nf = FT(0);
        layered_energy_sweep_up<FT, M, NOICE, VGF, false>(mm, P, C, H, eb, et, col, y, A.ti, FT(0), nullptr, nullptr, nf,
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
        double hh;
        const bool clip = trbdf2_clip(t, A.t1, h, hh); // land on t1 exactly
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
            // layered_trbdf2_column, J_ww re-formed at Y_1 and the stage-2 face states ...
            const FT hf = FT(hh);
            double sum = 0.0;
            {
                FaceState<FT> fsb, fst;
                water_faces(fsb, fst);
                layered_sweep_up<FT, M, NOICE, VGF, true>(
                    mm, P, C, fsb, fst, col, y, A.ti, ti_b, dh, A.cp, A.dp, [&](int64_t id, FT v, FT) {
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
            accept = trbdf2_control(sqrt(sum / (2.0 * n)), fac);
        }
        if (accept) {
            ++st.accepted;
            output(t, clip ? A.t1 : t + hh, hh); // (before t moves and f_n, f_e are overwritten)
            t = clip ? A.t1 : t + hh; // (assigned: the column lands on t1 exactly)
            h = trbdf2_next_step(h, hh, fac, clip);
            // the accepted result's finiteness and, as layered_trbdf2_column, f_n+1 = z_1 / h where a next step follows
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

// implicit_math and both table stagings hold a __syncthreads(): every thread of the workgroup reaches all of them,
// and no lane leaves before the last one.  A lane past the last column does not return either: it skips the column
// and takes part in the wave's reduction of the statistics with zeros (layered_coupled_implicit_kernel).
template <typename FT, bool NOICE, bool VGF>
__global__ void __launch_bounds__(implicit_threads<MathFast<FT>>())
layered_coupled_trbdf2_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const CoupledTrbdf2Args<FT> A) {
    using M = MathFast<FT>;
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm = implicit_math<M>(P.math_tab);
    stage_class_table<FT, M, !NOICE>(mm, class_args(L), s_cls); // (as layered_coupled_implicit_kernel: the same l2_por)
    stage_therm_table<FT>(L, s_th);
    const ClassView<FT> C{s_cls, L.cls};
    const ThermTable<FT> H{s_th, L.any_om != 0};
    const int64_t col = implicit_lane_column();
    Trbdf2ColStats st;
    bool nonfinite = false;
    if (col < P.ncols) layered_coupled_trbdf2_column<FT, M, NOICE, VGF>(mm, P, C, H, A, col, st, nonfinite);
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
void launch_layered_coupled_trbdf2(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const CoupledTrbdf2Args<FT>& A,
                                   bool noice, hipStream_t s) {
    constexpr int block = implicit_threads<MathFast<FT>>();
    with_layered_implicit_variant(P, noice, [&](auto ni, auto vg) {
        hipLaunchKernelGGL((layered_coupled_trbdf2_kernel<FT, decltype(ni)::value, decltype(vg)::value>), grid_for(P.ncols, block),
                           dim3(block), 0, s, P, L, A);
    });
}

#define LH_INSTANTIATE_LAYERED_COUPLED_TRBDF2(FT)                                                                   \
    template void launch_layered_coupled_trbdf2<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,               \
                                                    const CoupledTrbdf2Args<FT>&, bool, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_COUPLED_TRBDF2_TU
