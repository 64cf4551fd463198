// lh_layered_heat.hpp -- layered soils for the coupled and the heat-only model: per-CELL soil classes with a
// thermal supplement.  The tendency, its fused SSPRK33 stages, the diagnostics, the
// boundary fluxes and the step bound.
//
// A class's thermal supplement (lh_set_soil_class_thermal) is what a texture changes and the heat path reads:
// rho_c_ds, the saturated conductivities, the Kersten exponents and 1 - nu_om, turned by the host into a
// ThermC<FT> with the arithmetic make_params applies to the scalars; the class's ColC<FT> carries nu, 1/nu and
// its own k_dry.  Both tables are staged in LDS; a cell takes `c = s_cls[k]` and `th = s_th[k]`.
//
// A kernel family of its own, in its own translation units, with its own argument struct: DevParams, ColC,
// LayeredArgs and every kernel of lh_kernels_impl.hpp and lh_layered.hpp stay byte for byte what they are
// (tools/kernel_manifest.py, profiles/layered_heat_manifest.txt).  The heat closures below are twins of
// kappa_closure_log / temperature_closure / face_state (lh_closures.hpp) that read the thermal constants from
// the cell's ThermC instead of DevParams, in the same operation order.
//
// The first part (the argument struct and the launchers' declarations) is what lh_api.hip includes; the kernels
// follow under LH_LAYERED_HEAT_TU, which only lh_kernels_f64_layered_heat.hip / lh_kernels_f32_layered_heat.hip define.
#pragma once
#include "lh_layered.hpp"

namespace lh {

// the thermal constants of one class: eight words (a Float64 table of 16 is 1 KiB of LDS)
template <typename FT>
struct ThermC {
    FT rho_c_ds;
    FT kappa_sat_unfrozen, kappa_sat_frozen;
    FT l2_kappa_sat_unfrozen, l2_kappa_sat_frozen; // log2 of the two, as DevParams holds them
    FT kersten_exp_unfrozen, kersten_exp_frozen;   // (1 + nu_om - a nu_q - nu_g)/2, 1 + nu_om
    FT one_minus_om;                               // 1 - nu_om
};

// what only the layered heat kernels read
template <typename FT>
struct LayeredHeatArgs {
    const uint8_t* cls;       // class plane [nlev][stride] bytes, column fastest; pad columns hold class 0
    const ColC<FT>* table;    // device array [ncls]; k_dry from the class's own nu, rho_p, kappa_solid
    const ThermC<FT>* therm;  // device array [ncls]
    int32_t ncls;             // 1 .. LH_LAYERED_MAX_CLASSES
    int32_t any_om;           // some class has one_minus_om != 1 (host decision: one uniform branch per cell)
};

// model: MODEL_COUPLED or MODEL_HEAT.  mode 0: the tendency into `out`; 1..3: the fused SSPRK33 stages of an
// unsegmented step.  The closure form (VGF) is the host's decision over all classes, handed over in P.vg_fast_all.
template <typename FT>
void launch_layered_heat_rhs(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                             const Planes<FT>& aux, const Planes<FT>& base, const Planes<FT>& out, FT dt, int mode,
                             int model, bool factors, bool noice, hipStream_t s);
template <typename FT>
void launch_layered_heat_diag(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                              const Planes<FT>& aux, const Planes<FT>& out, int model, hipStream_t s);
template <typename FT>
void launch_layered_heat_boundary_fluxes(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                                         const Planes<FT>& aux, int face, FT* out_e, FT* out_w, int model, bool factors,
                                         hipStream_t s);
// *out_ft must hold +inf (the minimum's neutral element) when the launch starts
template <typename FT>
void launch_layered_heat_stable_dt(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                                   const Planes<FT>& aux, FT courant, void* out_ft, int model, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_HEAT_TU
#ifndef LH_LAYERED_TU
#error "lh_layered_heat.hpp's kernels need lh_layered.hpp's (define LH_LAYERED_TU first)"
#endif

namespace lh {

// ------------------------------------------------------------ the two tables in LDS

template <typename FT>
__device__ __forceinline__ LayeredArgs<FT> class_args(const LayeredHeatArgs<FT>& L) {
    LayeredArgs<FT> A;
    A.cls = L.cls;
    A.table = L.table;
    A.ncls = L.ncls;
    A.pad_ = 0;
    return A;
}

// the thermal table beside the class table (stage_class_table): LH_LAYERED_MAX_CLASSES entries whatever the
// class count, entries past it repeat the last class.  Every thread of the workgroup must call this.
template <typename FT>
__device__ __forceinline__ void stage_therm_table(const LayeredHeatArgs<FT>& L, ThermC<FT>* s_th) {
    static_assert(sizeof(ThermC<FT>) % 4 == 0, "the table is copied in 32-bit words");
    constexpr unsigned W = sizeof(ThermC<FT>) / 4;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(L.therm);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_th);
    const unsigned last = unsigned(L.ncls) - 1u;
    for (unsigned i = threadIdx.x; i < W * LH_LAYERED_MAX_CLASSES; i += blockDim.x) {
        const unsigned e = i / W, w = i - e * W;
        dst[i] = src[(e < last ? e : last) * W + w];
    }
    __syncthreads();
}

// ------------------------------------------------------------ the heat closures with a cell's own constants

// kappa_closure_log with the thermal constants of the cell's class.  any_om: some class has organic matter
// (uniform); a lane whose own class has none keeps d itself, as the scalar closure does.
template <typename FT, typename M, bool NOICE>
__device__ __forceinline__ FT kappa_closure_cls(const M& mm, const DevParams<FT>& P, const ColC<FT>& c,
                                                const ThermC<FT>& th, bool any_om, FT vl, FT ti) {
    static_assert(M::is_production, "the layered kernels exist for the production math only");
    constexpr FT SC = FT(M::EXP2_SCALE);
    const FT nu_eff = NOICE ? c.nu : c.nu - ti;
    const FT tl = liquid_fraction(vl, nu_eff);
    const FT tw = NOICE ? tl : tl + ti;
    const FT S_r = tw * c.inv_nu;
    const bool unfrozen = NOICE || ti < Limits<FT>::eps();
    const FT e_sel = unfrozen ? th.kersten_exp_unfrozen * SC : th.kersten_exp_frozen * SC;
    FT K_e;
    if constexpr (M::uses_tables) {
        K_e = mm.exp2_scaled(mm.log2(S_r > FT(0) ? S_r : FT(1)) * e_sel);
        K_e = (S_r > FT(0)) ? K_e : ((S_r == FT(0)) ? FT(0) : FT(NAN));
    } else {
        K_e = mm.exp2_scaled(mm.log2(S_r) * e_sel);
    }
    if (unfrozen) {
        const FT e = mm.exp2_scaled(S_r * P.neg_b_log2e_sc);
        const FT a = mm.pow_neg3(FT(1) + e);
        const FT h = (FT(1) - S_r) * FT(0.5);
        const FT d = a - h * h * h;
        FT dp = d;
        if (any_om) {
            const FT dq = mm.pow(d, th.one_minus_om);
            dp = (th.one_minus_om != FT(1)) ? dq : d;
            asm volatile("" : "+v"(dp));
        }
        K_e = K_e * dp;
    }
    FT k_sat = th.kappa_sat_unfrozen;
    if (!NOICE && ti != FT(0)) {
        const FT itw = mm.rcp(tw);
        k_sat = mm.exp2_scaled(((tl * (th.l2_kappa_sat_unfrozen * SC) + ti * (th.l2_kappa_sat_frozen * SC)) * itw));
    }
    k_sat = (tw < Limits<FT>::eps()) ? FT(0) : k_sat;
    return K_e * k_sat + (FT(1) - K_e) * c.k_dry;
}

// temperature_closure with the class's rho_c_ds
template <typename FT, typename M, bool NOICE>
__device__ __forceinline__ FT temperature_closure_cls(const M& mm, const DevParams<FT>& P, const ColC<FT>& c,
                                                      const ThermC<FT>& th, FT vl, FT ti, FT rhoe, FT& rho_c_s) {
    const FT nu_eff = NOICE ? c.nu : c.nu - ti;
    const FT tl = liquid_fraction(vl, nu_eff);
    rho_c_s = NOICE ? th.rho_c_ds + tl * P.rhocp_l : th.rho_c_ds + tl * P.rhocp_l + ti * P.rhocp_i;
    const FT num = NOICE ? rhoe : rhoe + ti * P.rho_i * P.LH_f0;
    return P.T_ref + num * mm.rcp(rho_c_s);
}

// face_state with the BOUNDARY CELL's own thermal class in the kappa of a Dirichlet energy face, and
// boundary_fluxes on top of it (boundary_fluxes_from is shared)
template <typename FT, typename M, int MODEL, bool FACTORS, bool NOICE>
__device__ __forceinline__ void boundary_fluxes_cls(const M& mm, const DevParams<FT>& P, const ColC<FT>& c,
                                                    const ThermC<FT>& th, bool any_om, int face, int64_t col, FT vl_c,
                                                    FT ti_c, FT T_c, FT K_c, FT psi_c, FT& f_e, FT& f_w,
                                                    FT* K_face, FT* kappa_face, bool vgfast) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    const FaceBC<FT> bc = face_bc(P, face, col);
    FaceState<FT> fs;
    fs.K = fs.psi = fs.kap = FT(0);
    FT vl_f = vl_c;
    fs.T = T_c;
    if (bc.ke == BC_DIRICHLET) fs.T = bc.ve;
    if (WATER && bc.kh == BC_DIRICHLET) vl_f = bc.vh;
    if (bc.ke == BC_DIRICHLET) fs.kap = kappa_closure_cls<FT, M, NOICE>(mm, P, c, th, any_om, vl_f, ti_c);
    if (WATER && bc.kh == BC_DIRICHLET)
        water_closures<FT, M, FACTORS, true, false, NOICE>(mm, P, c, vl_f, ti_c, fs.T, fs.K, fs.psi, nullptr, vgfast);
    if (K_face && WATER && bc.kh == BC_DIRICHLET) *K_face = fs.K;
    if (kappa_face && bc.ke == BC_DIRICHLET) *kappa_face = fs.kap;
    boundary_fluxes_from<FT, MODEL>(P, fs, face, col, T_c, K_c, psi_c, f_e, f_w);
}

// ------------------------------------------------------------ which variants exist, and their launch shape

// as layered_variant_exists; the heat-only model has no water closures, so neither conductivity factors nor a
// second closure form
template <typename M, int MODEL, bool FACTORS, bool NOICE, bool VGF, int MODE>
constexpr bool layered_heat_variant_exists() {
    if (!M::is_production || MODE < 0 || MODE > 3) return false;
    if (MODEL == MODEL_HEAT) return !FACTORS && VGF;
    return (!NOICE || noice_exists<M>(FACTORS)) && (VGF || robust_vg_exists<M, MODEL_COUPLED>());
}
// Waves per SIMD the register allocator leaves room for (profiles/layered_heat_kernel_regs.txt).  Float64: the
// 512-thread workgroups hold 53 120 bytes of LDS, three per CU; every instantiation is asked for 4 waves (128
// VGPRs), which all of them fit without scratch.  Float32 (two columns per lane, each with its own two table
// entries) is left to the compiler.
template <typename FT, typename M>
constexpr int layered_heat_min_waves() { return M::uses_tables ? 4 : 1; }

// ------------------------------------------------------------ the tendency and its fused stages
//
// layered_rhs_kernel's march (one lane per CPL columns, bottom to top, PF levels in flight, the class byte in
// the prefetch ring, every face formed once, lower cell first, and differenced) for the coupled and the
// heat-only model.  In tendency units, with the TRUE conductivity K = Ksat K_r of each cell's own class:
//   F'w = -(K_lo + K_hi) (head_difference(-psi_hi, -psi_lo, dz) cg2)                                  (coupled)
//   F'e = -(kappa_lo + kappa_hi) ((T_hi - T_lo) cg2) - (E_lo + E_hi) (head_difference(...) cg2),
//         E = (rhocp_l (T - T_ref)) K;                                     heat-only: the kappa term alone
// i.e. interior_face with cgw = cgT = cg2.  The heat-only model reads vartheta_l and theta_i from Ya.
// MODE as rhs_kernel: 0 the tendency, 1..3 the SSPRK33 stages; the stage state may be updated in place.
template <typename FT, int MODEL, bool FACTORS, typename M, int MODE, bool NOICE, bool VGF>
__global__ void __launch_bounds__((layered_threads<M>()), (layered_heat_min_waves<FT, M>()))
layered_heat_rhs_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                        const Planes<FT> BASE, const Planes<FT> OUT, const FT dt) {
    static_assert(MODEL == MODEL_COUPLED || MODEL == MODEL_HEAT, "the Richards model has lh_layered.hpp");
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    using CFG = typename DefaultCfg<FT>::type;
    constexpr int CPL = CFG::CPL, PF = CFG::PF;
    constexpr bool TEND = (MODE == 0);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, WATER && !NOICE>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const bool any_om = L.any_om != 0;

    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col0 = (int64_t(blk) * blockDim.x + threadIdx.x) * CPL;
    if (col0 >= P.ncols) return;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const unsigned lane_byte = (unsigned)col0 * (unsigned)sizeof(FT);
    const unsigned row_bytes = (unsigned)(stride * (int64_t)sizeof(FT));
    auto rload = [&](const FT* row, FT (&out)[CPL]) { bload<FT, CPL, false>(row, row_bytes, lane_byte, out); };
    auto rstore = [&](FT* row, const FT (&in)[CPL]) { bstore<FT, CPL, false>(row, row_bytes, lane_byte, in); };

    // uniform row pointers (level 0); the heat-only model reads the prescribed water fields from Ya, the fused
    // stages of the coupled one read theta_i from BASE (= Y)
    const FT* r_vl = WATER ? IN.v[0] : AUX.v[0];
    const FT* r_ti = NOICE ? nullptr : (WATER ? (TEND ? IN.v[1] : BASE.v[1]) : AUX.v[1]);
    const FT* r_re = IN.v[2];
    const uint8_t* r_cls = L.cls;
    const FT* b_vl = ((MODE == 2 || MODE == 3) && WATER) ? BASE.v[0] : nullptr;
    const FT* b_re = (MODE == 2 || MODE == 3) ? BASE.v[2] : nullptr;
    FT* o_vl = WATER ? OUT.v[0] : nullptr;
    FT* o_re = OUT.v[2];

    int64_t colj[CPL]; // column index clamped into [0, ncols): pad lanes reuse the last column
#pragma unroll
    for (int j = 0; j < CPL; ++j) colj[j] = col0 + j < P.ncols ? col0 + j : P.ncols - 1;

    constexpr bool vgf = VGF && M::uses_tables;
    FT vl[CPL], ti[CPL], re[CPL];
    FT vl_n[PF][CPL], ti_n[PF][CPL], re_n[PF][CPL];
    unsigned kc = 0u, kc_n[PF];              // class bytes of the current cell / of the levels in flight
    FT vl_p[CPL], re_p[CPL];                 // previous cell's state (fused stages)
    FT K_p[CPL], psi_p[CPL], T_p[CPL], kap_p[CPL], E_p[CPL]; // TRUE conductivity, -psi, T, kappa, rho_e_l K of the previous cell
    FT Fw_lo[CPL], Fe_lo[CPL];
    FT nf_acc = FT(0);                       // += 0 * tendency: NaN once any tendency is non-finite
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        K_p[j] = psi_p[j] = T_p[j] = kap_p[j] = E_p[j] = Fw_lo[j] = Fe_lo[j] = FT(0);
        vl_p[j] = re_p[j] = FT(0);
        vl[j] = ti[j] = re[j] = FT(0);
    }
    auto fetch = [&](int slot) {
        rload(r_vl, vl_n[slot]);
        kc_n[slot] = cload<CPL>(r_cls, (unsigned)stride, (unsigned)col0);
        if (!NOICE) rload(r_ti, ti_n[slot]);
        rload(r_re, re_n[slot]);
        r_vl += stride;
        r_cls += stride;
        if (!NOICE) r_ti += stride;
        r_re += stride;
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) vl_n[k][j] = ti_n[k][j] = re_n[k][j] = FT(0);
        kc_n[k] = 0u;
        if (k < n) fetch(k);
    }

    // emit the result of the cell the OUT/BASE row pointers address (rhs_kernel's emit)
    auto emit = [&](const FT (&Fw_hi)[CPL], const FT (&Fe_hi)[CPL], const FT (&u_vl)[CPL], const FT (&u_re)[CPL]) {
        FT dvl[CPL], dre[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            dvl[j] = WATER ? Fw_lo[j] - Fw_hi[j] : FT(0); // -(F_hi - F_lo), fluxes in tendency units
            dre[j] = Fe_lo[j] - Fe_hi[j];
            if (CPL == 1 || col0 + j < P.ncols) {
                if (WATER) nf_acc = fma_ft(dvl[j], FT(0), nf_acc);
                nf_acc = fma_ft(dre[j], FT(0), nf_acc);
            }
        }
        if (TEND) {
            if (WATER) rstore(o_vl, dvl); // (d theta_i = 0: the plane is kept zero by the host side)
            rstore(o_re, dre);
        } else {
            auto stage = [&](const FT* brow, FT* orow, const FT (&u)[CPL], const FT (&k)[CPL]) {
                constexpr int STAGE = MODE == 1 ? 0 : (MODE == 3 ? 2 : 1);
                FT b[CPL] = {}, r[CPL];
                if (MODE == 2 || MODE == 3) rload(brow, b);
#pragma unroll
                for (int j = 0; j < CPL; ++j) r[j] = ssprk33_stage_value<FT>(STAGE, b[j], u[j], k[j], dt);
                rstore(orow, r);
            };
            if (WATER) stage(b_vl, o_vl, u_vl, dvl);
            stage(b_re, o_re, u_re, dre);
        }
        if (WATER) {
            o_vl += stride;
            if (MODE == 2 || MODE == 3) b_vl += stride;
        }
        o_re += stride;
        if (MODE == 2 || MODE == 3) b_re += stride;
    };

    for (int i0 = 0; i0 < n; i0 += PF) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int i = i0 + k;
        if (PF > 1 && i >= n) break;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl[j] = vl_n[k][j];
            ti[j] = NOICE ? FT(0) : ti_n[k][j];
            re[j] = re_n[k][j];
        }
        kc = kc_n[k];
        if (i + PF < n) fetch(k); // keep PF levels in flight ahead of the one computed
        FT K[CPL], psi[CPL], T[CPL], kap[CPL], E[CPL]; // (psi[], psi_p[] hold -psi: see head_difference)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const unsigned q = class_of(kc, j);
            const ColC<FT>& c = s_cls[q];
            const ThermC<FT>& th = s_th[q];
            FT rcs;
            K[j] = psi[j] = E[j] = FT(0);
            T[j] = temperature_closure_cls<FT, M, NOICE>(mm, P, c, th, vl[j], ti[j], re[j], rcs);
            kap[j] = kappa_closure_cls<FT, M, NOICE>(mm, P, c, th, any_om, vl[j], ti[j]);
            if (WATER) {
                FT Kr = FT(0);
                water_closures<FT, M, FACTORS, true, false, NOICE, true, true, true>(mm, P, c, vl[j], ti[j], T[j], Kr, psi[j],
                                                                                     nullptr, vgf);
                K[j] = Kr * c.Ksat;                              // the true conductivity: the two cells of a face may differ in Ksat
                E[j] = (P.rhocp_l * (T[j] - P.T_ref)) * K[j];    // rho_e_int_l * K (:364)
            }
        }
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const unsigned q = class_of(kc, j);
                boundary_fluxes_cls<FT, M, MODEL, FACTORS, NOICE>(mm, P, s_cls[q], s_th[q], any_om, FACE_BOTTOM, colj[j], vl[j],
                                                                  ti[j], T[j], K[j], -psi[j], Fe_lo[j], Fw_lo[j], nullptr,
                                                                  nullptr, vgf);
                Fe_lo[j] = Fe_lo[j] * P.inv_dz;
                Fw_lo[j] = Fw_lo[j] * P.inv_dz;
            }
        } else {
            FT Fw[CPL], Fe[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                interior_face<FT, WATER, true>(K_p[j], psi_p[j], T_p[j], kap_p[j], E_p[j], K[j], psi[j], T[j], kap[j], E[j],
                                               P.dz, P.cg2, P.cg2, Fw[j], Fe[j]);
            emit(Fw, Fe, vl_p, re_p); // cell i-1
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                Fw_lo[j] = Fw[j];
                Fe_lo[j] = Fe[j];
            }
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl_p[j] = vl[j];
            re_p[j] = re[j];
            K_p[j] = K[j];
            psi_p[j] = psi[j];
            T_p[j] = T[j];
            kap_p[j] = kap[j];
            E_p[j] = E[j];
        }
      }
    }
    {   // the top face of the column: the top cell's own class
        FT Fw[CPL], Fe[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const unsigned q = class_of(kc, j);
            boundary_fluxes_cls<FT, M, MODEL, FACTORS, NOICE>(mm, P, s_cls[q], s_th[q], any_om, FACE_TOP, colj[j], vl[j], ti[j],
                                                              T_p[j], K_p[j], -psi_p[j], Fe[j], Fw[j], nullptr, nullptr, vgf);
            Fe[j] = Fe[j] * P.inv_dz;
            Fw[j] = Fw[j] * P.inv_dz;
        }
        emit(Fw, Fe, vl_p, re_p);
    }
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
}

// ------------------------------------------------------------ the twins of diag / boundary_flux / stable_dt
// The same loops as diag_kernel, boundary_flux_kernel and stable_dt_kernel for the coupled and the heat-only
// model, with `c` and `th` taken per cell from the LDS tables.

template <typename FT, int MODEL, typename M>
__global__ void __launch_bounds__(256)
layered_heat_diag_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                         const Planes<FT> OUT) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, WATER>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    const bool any_om = L.any_om != 0;
    const bool vgf = M::uses_tables && P.vg_fast_all != 0;
    const FT* p_vl = WATER ? IN.v[0] : AUX.v[0];
    const FT* p_ti = WATER ? IN.v[1] : AUX.v[1];
    for (int i = 0; i < P.nlev; ++i) {
        const int64_t o = int64_t(i) * P.stride + col;
        const unsigned q = L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1);
        const ColC<FT>& c = s_cls[q];
        const ThermC<FT>& th = s_th[q];
        const FT vl = p_vl[o], ti = p_ti[o];
        FT K = FT(0), psi = FT(0), rcs;
        const FT T = temperature_closure_cls<FT, M, false>(mm, P, c, th, vl, ti, IN.v[2][o], rcs);
        const FT kap = kappa_closure_cls<FT, M, false>(mm, P, c, th, any_om, vl, ti);
        if (WATER) water_closures<FT, M, true>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
        OUT.v[0][o] = K;
        OUT.v[1][o] = psi;
        OUT.v[2][o] = kap;
        OUT.v[3][o] = T;
    }
}

// (f_rhoe_int, f_vartheta_l) of one face of every column, from the device functions and the closure
// instantiation layered_heat_rhs_kernel uses (K without Ksat times the boundary cell's Ksat; the kappa of a
// Dirichlet energy face from the boundary cell's own thermal class): the same bits
template <typename FT, int MODEL, bool FACTORS, typename M>
__global__ void __launch_bounds__(256)
layered_heat_boundary_flux_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const Planes<FT> IN,
                                  const Planes<FT> AUX, const int face, FT* out_e, FT* out_w) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, WATER>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    const int64_t o = int64_t(face == FACE_BOTTOM ? 0 : P.nlev - 1) * P.stride + col;
    const unsigned q = L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1);
    const ColC<FT>& c = s_cls[q];
    const ThermC<FT>& th = s_th[q];
    const bool any_om = L.any_om != 0;
    const bool vgf = M::uses_tables && P.vg_fast_all != 0;
    const FT vl = (WATER ? IN.v[0] : AUX.v[0])[o], ti = (WATER ? IN.v[1] : AUX.v[1])[o];
    FT K = FT(0), psi = FT(0), rcs;
    const FT T = temperature_closure_cls<FT, M, false>(mm, P, c, th, vl, ti, IN.v[2][o], rcs);
    if (WATER) {
        water_closures<FT, M, FACTORS, true, false, false, true, true>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
        K = K * c.Ksat;
    }
    FT fe, fw;
    boundary_fluxes_cls<FT, M, MODEL, FACTORS, false>(mm, P, c, th, any_om, face, col, vl, ti, T, K, psi, fe, fw, nullptr,
                                                      nullptr, vgf);
    // (selects between the two faces' entries: an indexed read of the by-value block would put it into scratch)
    const bool bot = (face == FACE_BOTTOM);
    if ((bot ? P.bc_kind[FACE_BOTTOM][COMP_ENERGY] : P.bc_kind[FACE_TOP][COMP_ENERGY]) == BC_NONE) fe = FT(NAN);
    if ((bot ? P.bc_kind[FACE_BOTTOM][COMP_HYDROLOGY] : P.bc_kind[FACE_TOP][COMP_HYDROLOGY]) == BC_NONE) fw = FT(NAN);
    out_e[col] = fe;
    out_w[col] = fw;
}

// stable_dt_kernel's rule with `c` and `th` per cell: the water coefficient as layered_stable_dt_kernel forms
// it; the heat coefficient of an interior face is (kappa_lo + kappa_hi)/2 over the smaller rho_c_s of the two
// cells; boundary cells and Dirichlet faces as stable_dt_kernel (the face state's kappa from the cell's class)
template <typename FT, int MODEL, typename M>
__global__ void __launch_bounds__(256)
layered_heat_stable_dt_kernel(const DevParams<FT> P, const LayeredHeatArgs<FT> L, const Planes<FT> IN,
                              const Planes<FT> AUX, const FT courant, typename Bits<FT>::type* out_bits) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    using U = typename Bits<FT>::type;
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    __shared__ ThermC<FT> s_th[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, WATER>(mm, class_args(L), s_cls);
    stage_therm_table<FT>(L, s_th);
    const bool any_om = L.any_om != 0;
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    FT best = FT(INFINITY);
    if (col < P.ncols) {
        const FT* p_vl = WATER ? IN.v[0] : AUX.v[0];
        const FT* p_ti = WATER ? IN.v[1] : AUX.v[1];
        const FT cdz2 = courant * P.dz * P.dz;
        const int n = P.nlev;
        FT K_p = FT(0), dpsi_p = FT(0), kap_p = FT(0), rcs_p = FT(1);
        for (int i = 0; i < n; ++i) {
            const int64_t o = int64_t(i) * P.stride + col;
            const unsigned q = L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1);
            const ColC<FT>& c = s_cls[q];
            const ThermC<FT>& th = s_th[q];
            const FT vl = p_vl[o], ti = p_ti[o];
            FT K = FT(0), dpsi = FT(0), rcs = FT(1);
            const FT Tc = temperature_closure_cls<FT, M, false>(mm, P, c, th, vl, ti, IN.v[2][o], rcs);
            if (WATER) {
                FT psi;
                water_closures<FT, M, true>(mm, P, c, vl, ti, Tc, K, psi);
                const FT nu_eff = c.nu - ti;
                const FT vls = !(vl <= c.theta_lim) ? vl : c.theta_lim;
                const FT Se = (vls - c.theta_r) / (nu_eff - c.theta_r);
                const FT u = mm.pow(Se, -c.inv_m) - FT(1);
                if (Se <= FT(1) && u > FT(0))
                    dpsi = fabs(psi) * (u + FT(1)) / (c.n * c.m * u * Se * (nu_eff - c.theta_r));
                else
                    dpsi = FT(1) / c.S_s;
            }
            const FT kap = kappa_closure_cls<FT, M, false>(mm, P, c, th, any_om, vl, ti);
            FT D = FT(0);
            if (i == 0 || i == n - 1) { // boundary cells: their own coefficients
                D = K * dpsi;
                if (kap / rcs > D) D = kap / rcs;
                // Dirichlet faces sit half a cell away and use the face state's coefficients
                for (int face = 0; face < 2; ++face) {
                    if ((face == FACE_BOTTOM) != (i == 0) && n > 1) continue;
                    const FaceBC<FT> bc = face_bc(P, face, col);
                    const FT vl_f = (WATER && bc.kh == BC_DIRICHLET) ? bc.vh : vl;
                    const FT T_f = (bc.ke == BC_DIRICHLET) ? bc.ve : Tc; // as boundary_fluxes
                    if (WATER && bc.kh == BC_DIRICHLET) {
                        FT K_f, psi_f;
                        water_closures<FT, M, true, false>(mm, P, c, vl_f, ti, T_f, K_f, psi_f);
                        const FT Db = FT(2) * (K_f > K ? K_f : K) * dpsi;
                        if (Db > D) D = Db;
                    }
                    if (bc.ke == BC_DIRICHLET) {
                        const FT kf = kappa_closure_cls<FT, M, false>(mm, P, c, th, any_om, vl_f, ti);
                        const FT Db = FT(2) * (kf > kap ? kf : kap) / rcs;
                        if (Db > D) D = Db;
                    }
                }
            }
            if (i > 0) { // interior face: arithmetic-mean coefficients as in the stencil
                const FT Dw = (K_p + K) * FT(0.5) * (dpsi_p > dpsi ? dpsi_p : dpsi);
                const FT DT = (kap_p + kap) * FT(0.5) / (rcs_p < rcs ? rcs_p : rcs);
                if (Dw > D) D = Dw;
                if (DT > D) D = DT;
            }
            if (D > FT(0)) {
                const FT dtc = cdz2 / D;
                if (dtc < best) best = dtc;
            }
            K_p = K;
            dpsi_p = dpsi;
            kap_p = kap;
            rcs_p = rcs;
        }
    }
    // wave64 reduction, then one atomic per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const FT other = __shfl_down(best, off, 64);
        if (other < best) best = other;
    }
    if ((threadIdx.x & 63) == 0 && best < FT(INFINITY)) {
        U b;
        __builtin_memcpy(&b, &best, sizeof(FT));
        if (b < __atomic_load_n(out_bits, __ATOMIC_RELAXED)) atomicMin(out_bits, b);
    }
}

// ------------------------------------------------------------ launchers

// the two models of this family (anything but the heat-only model is the coupled one)
using heat_models = int_list<MODEL_HEAT, MODEL_COUPLED>;

template <typename FT>
void launch_layered_heat_rhs(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                             const Planes<FT>& aux, const Planes<FT>& base, const Planes<FT>& out, FT dt, int mode,
                             int model, bool factors, bool noice, hipStream_t s) {
    using M = MathFast<FT>;
    using CFG = typename DefaultCfg<FT>::type;
    const bool water = model != MODEL_HEAT;
    const bool fa = water && factors; // (the heat-only model has no water closures: nothing reads the factors)
    const bool ni = noice && noice_exists<M>(fa);
    const bool robust = water && robust_vg_exists<M, MODEL_COUPLED>() && P.vg_fast_all == 0; // (as launch_rhs_model)
    constexpr int block = layered_threads<M>();
    const dim3 g = grid_for((P.ncols + CFG::CPL - 1) / CFG::CPL, block), b(block);
    with_int(heat_models{}, model, [&](auto mo) { with_bool(fa, [&](auto f) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<1, 2, 3, 0>{}, mode, [&](auto md) {
            constexpr int MO = decltype(mo)::value, MODE = decltype(md)::value;
            constexpr bool F = decltype(f)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            // (fa, ni and robust are normalised above: the guard only keeps what cannot occur un-instantiated)
            if constexpr (layered_heat_variant_exists<M, MO, F, NI, VG, MODE>())
                hipLaunchKernelGGL((layered_heat_rhs_kernel<FT, MO, F, M, MODE, NI, VG>), g, b, 0, s, P, L, in, aux, base, out, dt);
        });
    }); }); }); });
}

template <typename FT>
void launch_layered_heat_diag(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                              const Planes<FT>& aux, const Planes<FT>& out, int model, hipStream_t s) {
    with_int(heat_models{}, model, [&](auto mo) {
        hipLaunchKernelGGL((layered_heat_diag_kernel<FT, decltype(mo)::value, MathFast<FT>>), grid_for(P.ncols, 256), dim3(256),
                           0, s, P, L, in, aux, out);
    });
}

template <typename FT>
void launch_layered_heat_boundary_fluxes(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                                         const Planes<FT>& aux, int face, FT* out_e, FT* out_w, int model, bool factors,
                                         hipStream_t s) {
    const bool fa = model != MODEL_HEAT && factors;
    with_int(heat_models{}, model, [&](auto mo) { with_bool(fa, [&](auto f) {
        constexpr int MO = decltype(mo)::value;
        constexpr bool F = decltype(f)::value;
        if constexpr (MO != MODEL_HEAT || !F)
            hipLaunchKernelGGL((layered_heat_boundary_flux_kernel<FT, MO, F, MathFast<FT>>), grid_for(P.ncols, 256), dim3(256), 0,
                               s, P, L, in, aux, face, out_e, out_w);
    }); });
}

template <typename FT>
void launch_layered_heat_stable_dt(const DevParams<FT>& P, const LayeredHeatArgs<FT>& L, const Planes<FT>& in,
                                   const Planes<FT>& aux, FT courant, void* out_ft, int model, hipStream_t s) {
    using U = typename Bits<FT>::type;
    with_int(heat_models{}, model, [&](auto mo) {
        hipLaunchKernelGGL((layered_heat_stable_dt_kernel<FT, decltype(mo)::value, MathFast<FT>>), grid_for(P.ncols, 256),
                           dim3(256), 0, s, P, L, in, aux, courant, reinterpret_cast<U*>(out_ft));
    });
}

#define LH_INSTANTIATE_LAYERED_HEAT(FT)                                                                                  \
    template void launch_layered_heat_rhs<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&, const Planes<FT>&,       \
                                              const Planes<FT>&, const Planes<FT>&, const Planes<FT>&, FT, int, int,     \
                                              bool, bool, hipStream_t);                                                  \
    template void launch_layered_heat_diag<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&, const Planes<FT>&,      \
                                               const Planes<FT>&, const Planes<FT>&, int, hipStream_t);                  \
    template void launch_layered_heat_boundary_fluxes<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&,              \
                                                          const Planes<FT>&, const Planes<FT>&, int, FT*, FT*, int,      \
                                                          bool, hipStream_t);                                            \
    template void launch_layered_heat_stable_dt<FT>(const DevParams<FT>&, const LayeredHeatArgs<FT>&, const Planes<FT>&, \
                                                    const Planes<FT>&, FT, void*, int, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_HEAT_TU
