// lh_layered.hpp -- layered soils: per-CELL soil classes for the Richards tendency, its fused SSPRK33
// stages, the diagnostics, the boundary fluxes and the step bound.
//
// A soil class is the six numbers lh_set_percol_param knows (van Genuchten n, alpha, theta_r, Ksat, and
// nu, S_s), turned by the host into a ColC<FT> with the arithmetic of the scalar parameters; a context holds
// at most LH_LAYERED_MAX_CLASSES of them.  The class map is one byte per cell, a plane [nlev][stride] with the
// column index fastest like every other plane: a wave reads 64 consecutive bytes per level.  The kernels stage
// the class table in LDS beside the math tables and take `const ColC<FT>& c = s_cls[k]` per cell.
//
// This is a kernel family of its own, in its own translation units, with its own argument struct:
// DevParams, ColC and every kernel of lh_kernels_impl.hpp stay byte for byte what they are
// (tools/kernel_manifest.py, profiles/layered_manifest.txt).
//
// The first part (the argument struct and the launchers' declarations) is what lh_api.hip includes; the
// kernels follow under LH_LAYERED_TU, which only lh_kernels_f64_layered.hip / lh_kernels_f32_layered.hip define.
#pragma once
#include "lh_device.hpp"

namespace lh {

constexpr int LH_LAYERED_MAX_CLASSES = 16; // LH_MAX_SOIL_CLASSES of landhydro.h

// what only the layered kernels read
template <typename FT>
struct LayeredArgs {
    const uint8_t* cls;      // class plane [nlev][stride] bytes, column fastest; pad columns hold class 0
    const ColC<FT>* table;   // device array [ncls], host arithmetic; l2_por is finished on the device
    int32_t ncls;            // 1 .. LH_LAYERED_MAX_CLASSES
    int32_t pad_;
};

// mode 0: the tendency into `out`; 1..3: the fused SSPRK33 stages of an unsegmented step (rhs_kernel's modes).
// The closure form (VGF) is the host's decision over all classes, handed over in P.vg_fast_all.
template <typename FT>
void launch_layered_rhs(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in, const Planes<FT>& aux,
                        const Planes<FT>& base, const Planes<FT>& out, FT dt, int mode, bool factors, bool noice,
                        hipStream_t s);
template <typename FT>
void launch_layered_diag(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in, const Planes<FT>& aux,
                         const Planes<FT>& out, hipStream_t s);
template <typename FT>
void launch_layered_boundary_fluxes(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in,
                                    const Planes<FT>& aux, int face, FT* out_e, FT* out_w, bool factors, hipStream_t s);
// *out_ft must hold +inf (the minimum's neutral element) when the launch starts
template <typename FT>
void launch_layered_stable_dt(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in,
                              const Planes<FT>& aux, FT courant, void* out_ft, hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_TU
#include "lh_kernels_impl.hpp"

namespace lh {

// ------------------------------------------------------------ class table and class bytes

// The class table in LDS: LH_LAYERED_MAX_CLASSES entries whatever the class count (entries past it repeat the
// last class, so a class byte masked to four bits never leaves the table), copied word by word by the whole
// workgroup.  FINISH: the kernel reads theta_i, so every entry gets the device's own log2(nu - theta_r)
// (finish_colc), once per workgroup.  Every thread of the workgroup must call this, after the math tables.
template <typename FT, typename M, bool FINISH>
__device__ __forceinline__ void stage_class_table(const M& mm, const LayeredArgs<FT>& L, ColC<FT>* s_cls) {
    static_assert(sizeof(ColC<FT>) % 4 == 0, "the table is copied in 32-bit words");
    constexpr unsigned W = sizeof(ColC<FT>) / 4;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(L.table);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_cls);
    const unsigned last = unsigned(L.ncls) - 1u;
    for (unsigned i = threadIdx.x; i < W * LH_LAYERED_MAX_CLASSES; i += blockDim.x) {
        const unsigned e = i / W, w = i - e * W;
        dst[i] = src[(e < last ? e : last) * W + w];
    }
    __syncthreads();
    if (FINISH) {
        if (threadIdx.x < LH_LAYERED_MAX_CLASSES) finish_colc<FT, M>(mm, s_cls[threadIdx.x]);
        __syncthreads();
    }
}

// the class bytes of this lane's CPL adjacent columns at one level, packed low byte first: a buffer load like
// bload (uniform row pointer, 32-bit lane offset, reads past the row give 0)
template <int CPL>
__device__ __forceinline__ unsigned cload(const uint8_t* row, unsigned row_bytes, unsigned lane_byte) {
    static_assert(CPL == 1 || CPL == 2, "one or two class bytes per lane");
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(row), 0, row_bytes, 0x00020000);
    if constexpr (CPL == 1) return __builtin_amdgcn_raw_buffer_load_b8(rs, lane_byte, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b16(rs, lane_byte, 0, 0);
}
__device__ __forceinline__ unsigned class_of(unsigned packed, int j) {
    return (packed >> (8 * j)) & unsigned(LH_LAYERED_MAX_CLASSES - 1);
}

// ------------------------------------------------------------ which variants exist, and their launch shape

// NOICE and VGF = false as for rhs_kernel (noice_exists, robust_vg_exists); the math policy is the production
// one only (a class map with LH_MATH_LIBM is refused); modes 0..3 (no step bound, no stage from k1)
template <typename M, bool FACTORS, bool NOICE, bool VGF, int MODE>
constexpr bool layered_variant_exists() {
    return M::is_production && (!NOICE || noice_exists<M>(FACTORS)) && (VGF || robust_vg_exists<M, MODEL_RICHARDS>()) &&
           MODE >= 0 && MODE <= 3;
}
// Threads per workgroup: the Float64 math tables take 48 KiB of LDS per workgroup and the class table 2.9 KiB
// more, so three 512-thread workgroups share a CU's 160 KiB (6 waves per SIMD); Float32 keeps 256.
template <typename M>
constexpr int layered_threads() { return M::uses_tables ? 512 : 256; }
// Waves per SIMD the register allocator leaves room for.  Float64: the ice-free kernel without conductivity
// factors fits the 80 VGPRs of 6 waves; the ones that read theta_i keep what they need up to 128 (4 waves).
// Float32 carries two columns per lane, each with its own class entry: left to the compiler.
template <typename FT, typename M, bool FACTORS, bool NOICE>
constexpr int layered_min_waves() {
    if (!M::uses_tables) return 1;
    return (NOICE && !FACTORS) ? 6 : 4;
}

// ------------------------------------------------------------ the tendency and its fused stages
//
// rhs_kernel's march for the Richards model (one lane per CPL columns, bottom to top, PF levels in flight,
// every face flux formed once and differenced) with the column constants taken per CELL: the class byte
// travels in the prefetch ring with vartheta_l, and `c` is a reference into the LDS table.
// water_closures is rhs_kernel's instantiation (relative K, -psi); the interior face is
//   F' = -(Ksat_lo K_r,lo + Ksat_hi K_r,hi) (head_difference(-psi_hi, -psi_lo, dz) cg2), lower cell first,
// the arithmetic mean of the two TRUE conductivities, which is the reference's InterpolateC2F whatever the two
// cells' classes are.  The boundary faces call boundary_fluxes with the boundary cell's own class entry.
// MODE as rhs_kernel: 0 the tendency, 1..3 the SSPRK33 stages; the stage state may be updated in place (a lane
// reads its own column only, ahead of what it writes).
template <typename FT, bool FACTORS, typename M, int MODE, bool NOICE, bool VGF>
__global__ void __launch_bounds__((layered_threads<M>()), (layered_min_waves<FT, M, FACTORS, NOICE>()))
layered_rhs_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                   const Planes<FT> BASE, const Planes<FT> OUT, const FT dt) {
    using CFG = typename DefaultCfg<FT>::type;
    constexpr int CPL = CFG::CPL, PF = CFG::PF;
    constexpr bool TEND = (MODE == 0);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls);

    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col0 = (int64_t(blk) * blockDim.x + threadIdx.x) * CPL;
    if (col0 >= P.ncols) return;
    const int n = P.nlev;
    const int64_t stride = P.stride;
    const unsigned lane_byte = (unsigned)col0 * (unsigned)sizeof(FT);
    const unsigned row_bytes = (unsigned)(stride * (int64_t)sizeof(FT));
    auto rload = [&](const FT* row, FT (&out)[CPL]) { bload<FT, CPL, false>(row, row_bytes, lane_byte, out); };
    auto rstore = [&](FT* row, const FT (&in)[CPL]) { bstore<FT, CPL, false>(row, row_bytes, lane_byte, in); };

    // uniform row pointers (level 0); the fused stages read theta_i from BASE (= Y)
    const FT* r_vl = IN.v[0];
    const FT* r_ti = NOICE ? nullptr : (TEND ? IN.v[1] : BASE.v[1]);
    const bool need_Taux = FACTORS && P.viscosity_kind;
    const FT* r_Ta = need_Taux ? AUX.v[3] : nullptr;
    const uint8_t* r_cls = L.cls;
    const FT* b_vl = (MODE == 2 || MODE == 3) ? BASE.v[0] : nullptr;
    FT* o_vl = OUT.v[0];

    int64_t colj[CPL]; // column index clamped into [0, ncols): pad lanes reuse the last column
#pragma unroll
    for (int j = 0; j < CPL; ++j) colj[j] = col0 + j < P.ncols ? col0 + j : P.ncols - 1;

    constexpr bool vgf = VGF && M::uses_tables;
    FT vl[CPL], ti[CPL], Ta[CPL];
    FT vl_n[PF][CPL], ti_n[PF][CPL], Ta_n[PF][CPL];
    unsigned kc = 0u, kc_n[PF]; // class bytes of the current cell / of the levels in flight
    FT vl_p[CPL];               // previous cell's state (fused stages)
    FT K_p[CPL], psi_p[CPL];    // TRUE conductivity and -psi of the previous cell
    FT Fw_lo[CPL];
    FT nf_acc = FT(0);          // += 0 * tendency: NaN once any tendency is non-finite
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        K_p[j] = psi_p[j] = Fw_lo[j] = vl_p[j] = FT(0);
        vl[j] = ti[j] = FT(0);
        Ta[j] = FT(288); // PrescribedTemperatureModel default (models.jl:53)
    }
    auto fetch = [&](int slot) {
        rload(r_vl, vl_n[slot]);
        kc_n[slot] = cload<CPL>(r_cls, (unsigned)stride, (unsigned)col0);
        if (!NOICE) rload(r_ti, ti_n[slot]);
        if (need_Taux) rload(r_Ta, Ta_n[slot]);
        r_vl += stride;
        r_cls += stride;
        if (!NOICE) r_ti += stride;
        if (need_Taux) r_Ta += stride;
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl_n[k][j] = ti_n[k][j] = FT(0);
            Ta_n[k][j] = FT(288);
        }
        kc_n[k] = 0u;
        if (k < n) fetch(k);
    }

    // emit the result of the cell the OUT/BASE row pointers address (rhs_kernel's emit)
    auto emit = [&](const FT (&Fw_hi)[CPL], const FT (&u_vl)[CPL]) {
        FT dvl[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            dvl[j] = Fw_lo[j] - Fw_hi[j]; // -(F_hi - F_lo), fluxes in tendency units
            if (CPL == 1 || col0 + j < P.ncols) nf_acc = fma_ft(dvl[j], FT(0), nf_acc);
        }
        if (TEND) {
            rstore(o_vl, dvl); // (d theta_i = 0: the plane is kept zero by the host side)
        } else {
            constexpr int STAGE = MODE == 1 ? 0 : (MODE == 3 ? 2 : 1);
            FT b[CPL] = {}, r[CPL];
            if (MODE == 2 || MODE == 3) rload(b_vl, b);
#pragma unroll
            for (int j = 0; j < CPL; ++j) r[j] = ssprk33_stage_value<FT>(STAGE, b[j], u_vl[j], dvl[j], dt);
            rstore(o_vl, r);
        }
        o_vl += stride;
        if (MODE == 2 || MODE == 3) b_vl += stride;
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
            Ta[j] = Ta_n[k][j];
        }
        kc = kc_n[k];
        if (i + PF < n) fetch(k); // keep PF levels in flight ahead of the one computed
        FT K[CPL], psi[CPL];      // (psi[], psi_p[] hold -psi: see head_difference)
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const ColC<FT>& c = s_cls[class_of(kc, j)];
            FT Kr = FT(0);
            psi[j] = FT(0);
            water_closures<FT, M, FACTORS, true, false, NOICE, true, false, true>(mm, P, c, vl[j], ti[j], Ta[j], Kr, psi[j],
                                                                                  nullptr, vgf);
            K[j] = Kr * c.Ksat; // the true conductivity: the two cells of a face may differ in Ksat
        }
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const ColC<FT>& c = s_cls[class_of(kc, j)];
                FT Fe;
                boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, c, FACE_BOTTOM, colj[j], vl[j], ti[j], Ta[j],
                                                                       K[j], -psi[j], Fe, Fw_lo[j], nullptr, nullptr, vgf);
                Fw_lo[j] = Fw_lo[j] * P.inv_dz;
            }
        } else {
            FT Fw[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j) Fw[j] = -(K_p[j] + K[j]) * (head_difference(psi[j], psi_p[j], P.dz) * P.cg2);
            emit(Fw, vl_p); // cell i-1
#pragma unroll
            for (int j = 0; j < CPL; ++j) Fw_lo[j] = Fw[j];
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl_p[j] = vl[j];
            K_p[j] = K[j];
            psi_p[j] = psi[j];
        }
      }
    }
    {   // the top face of the column: the top cell's own class
        FT Fw[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const ColC<FT>& c = s_cls[class_of(kc, j)];
            FT Fe;
            boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, c, FACE_TOP, colj[j], vl[j], ti[j], Ta[j], K_p[j],
                                                                   -psi_p[j], Fe, Fw[j], nullptr, nullptr, vgf);
            Fw[j] = Fw[j] * P.inv_dz;
        }
        emit(Fw, vl_p);
    }
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
}

// ------------------------------------------------------------ the twins of diag / boundary_flux / stable_dt
// The same loops as diag_kernel, boundary_flux_kernel and stable_dt_kernel for the Richards model, with `c`
// taken per cell from the LDS table.

template <typename FT, typename M>
__global__ void __launch_bounds__(256)
layered_diag_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                    const Planes<FT> OUT) {
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, true>(mm, L, s_cls);
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    const bool need_Taux = P.viscosity_kind != 0;
    const bool vgf = M::uses_tables && P.vg_fast_all != 0;
    for (int i = 0; i < P.nlev; ++i) {
        const int64_t o = int64_t(i) * P.stride + col;
        const ColC<FT>& c = s_cls[L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1)];
        const FT vl = IN.v[0][o], ti = IN.v[1][o];
        const FT T = need_Taux ? AUX.v[3][o] : FT(288);
        FT K = FT(0), psi = FT(0);
        water_closures<FT, M, true>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
        OUT.v[0][o] = K;
        OUT.v[1][o] = psi;
        OUT.v[2][o] = FT(0);
        OUT.v[3][o] = T;
    }
}

// (f_rhoe_int, f_vartheta_l) of one face of every column, from the device functions and the closure
// instantiation layered_rhs_kernel uses (K without Ksat times the boundary cell's Ksat): the same bits
template <typename FT, bool FACTORS, typename M>
__global__ void __launch_bounds__(256)
layered_boundary_flux_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                             const int face, FT* out_e, FT* out_w) {
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, true>(mm, L, s_cls);
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    const int64_t o = int64_t(face == FACE_BOTTOM ? 0 : P.nlev - 1) * P.stride + col;
    const ColC<FT>& c = s_cls[L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1)];
    const bool vgf = M::uses_tables && P.vg_fast_all != 0;
    const bool need_Taux = FACTORS && P.viscosity_kind;
    const FT vl = IN.v[0][o], ti = IN.v[1][o];
    const FT T = need_Taux ? AUX.v[3][o] : FT(288);
    FT K = FT(0), psi = FT(0);
    water_closures<FT, M, FACTORS, true, false, false, true>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
    K = K * c.Ksat;
    FT fe, fw;
    boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, false>(mm, P, c, face, col, vl, ti, T, K, psi, fe, fw, nullptr, nullptr, vgf);
    // (selects between the two faces' entries: an indexed read of the by-value block would put it into scratch)
    const bool bot = (face == FACE_BOTTOM);
    if ((bot ? P.bc_kind[FACE_BOTTOM][COMP_ENERGY] : P.bc_kind[FACE_TOP][COMP_ENERGY]) == BC_NONE) fe = FT(NAN);
    if ((bot ? P.bc_kind[FACE_BOTTOM][COMP_HYDROLOGY] : P.bc_kind[FACE_TOP][COMP_HYDROLOGY]) == BC_NONE) fw = FT(NAN);
    out_e[col] = fe;
    out_w[col] = fw;
}

// min over cells of courant dz^2 / (K dpsi/dvl): stable_dt_kernel's rule with every cell's own n m in its
// slope, and on an interior face the mean of the two true conductivities times the larger slope
template <typename FT, typename M>
__global__ void __launch_bounds__(256)
layered_stable_dt_kernel(const DevParams<FT> P, const LayeredArgs<FT> L, const Planes<FT> IN, const Planes<FT> AUX,
                         const FT courant, typename Bits<FT>::type* out_bits) {
    using U = typename Bits<FT>::type;
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    stage_class_table<FT, M, true>(mm, L, s_cls);
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    FT best = FT(INFINITY);
    if (col < P.ncols) {
        const FT cdz2 = courant * P.dz * P.dz;
        const int n = P.nlev;
        FT K_p = FT(0), dpsi_p = FT(0);
        for (int i = 0; i < n; ++i) {
            const int64_t o = int64_t(i) * P.stride + col;
            const ColC<FT>& c = s_cls[L.cls[o] & (LH_LAYERED_MAX_CLASSES - 1)];
            const FT vl = IN.v[0][o], ti = IN.v[1][o];
            const FT Tc = P.viscosity_kind ? AUX.v[3][o] : FT(288);
            FT K = FT(0), dpsi = FT(0), psi;
            water_closures<FT, M, true>(mm, P, c, vl, ti, Tc, K, psi);
            const FT nu_eff = c.nu - ti;
            const FT vls = !(vl <= c.theta_lim) ? vl : c.theta_lim;
            const FT Se = (vls - c.theta_r) / (nu_eff - c.theta_r);
            const FT u = mm.pow(Se, -c.inv_m) - FT(1);
            if (Se <= FT(1) && u > FT(0))
                dpsi = fabs(psi) * (u + FT(1)) / (c.n * c.m * u * Se * (nu_eff - c.theta_r));
            else
                dpsi = FT(1) / c.S_s;
            FT D = FT(0);
            if (i == 0 || i == n - 1) { // boundary cells: their own coefficients
                D = K * dpsi;
                // Dirichlet faces sit half a cell away and use the face state's coefficients
                for (int face = 0; face < 2; ++face) {
                    if ((face == FACE_BOTTOM) != (i == 0) && n > 1) continue;
                    if (P.bc_kind[face][COMP_HYDROLOGY] != BC_DIRICHLET) continue;
                    FT vh = P.bc_value[face][COMP_HYDROLOGY];
                    if (P.bc_pc[face][COMP_HYDROLOGY]) vh = P.bc_pc[face][COMP_HYDROLOGY][col];
                    FT K_f, psi_f;
                    water_closures<FT, M, true, false>(mm, P, c, vh, ti, Tc, K_f, psi_f);
                    const FT Db = FT(2) * (K_f > K ? K_f : K) * dpsi;
                    if (Db > D) D = Db;
                }
            }
            if (i > 0) { // interior face: arithmetic-mean conductivity as in the stencil
                const FT Dw = (K_p + K) * FT(0.5) * (dpsi_p > dpsi ? dpsi_p : dpsi);
                if (Dw > D) D = Dw;
            }
            if (D > FT(0)) {
                const FT dtc = cdz2 / D;
                if (dtc < best) best = dtc;
            }
            K_p = K;
            dpsi_p = dpsi;
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

template <typename FT>
void launch_layered_rhs(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in, const Planes<FT>& aux,
                        const Planes<FT>& base, const Planes<FT>& out, FT dt, int mode, bool factors, bool noice,
                        hipStream_t s) {
    using M = MathFast<FT>;
    using CFG = typename DefaultCfg<FT>::type;
    const bool ni = noice && noice_exists<M>(factors);
    const bool robust = robust_vg_exists<M, MODEL_RICHARDS>() && P.vg_fast_all == 0; // (as launch_rhs_model)
    constexpr int block = layered_threads<M>();
    const dim3 g = grid_for((P.ncols + CFG::CPL - 1) / CFG::CPL, block), b(block);
    with_bool(factors, [&](auto f) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<1, 2, 3, 0>{}, mode, [&](auto md) {
            constexpr bool F = decltype(f)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            constexpr int MODE = decltype(md)::value;
            // (ni and robust are normalised above: the guard only keeps what cannot occur un-instantiated)
            if constexpr (layered_variant_exists<M, F, NI, VG, MODE>())
                hipLaunchKernelGGL((layered_rhs_kernel<FT, F, M, MODE, NI, VG>), g, b, 0, s, P, L, in, aux, base, out, dt);
        });
    }); }); });
}

template <typename FT>
void launch_layered_diag(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in, const Planes<FT>& aux,
                         const Planes<FT>& out, hipStream_t s) {
    hipLaunchKernelGGL((layered_diag_kernel<FT, MathFast<FT>>), grid_for(P.ncols, 256), dim3(256), 0, s, P, L, in, aux, out);
}

template <typename FT>
void launch_layered_boundary_fluxes(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in,
                                    const Planes<FT>& aux, int face, FT* out_e, FT* out_w, bool factors, hipStream_t s) {
    with_bool(factors, [&](auto f) {
        hipLaunchKernelGGL((layered_boundary_flux_kernel<FT, decltype(f)::value, MathFast<FT>>), grid_for(P.ncols, 256),
                           dim3(256), 0, s, P, L, in, aux, face, out_e, out_w);
    });
}

template <typename FT>
void launch_layered_stable_dt(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& in,
                              const Planes<FT>& aux, FT courant, void* out_ft, hipStream_t s) {
    using U = typename Bits<FT>::type;
    hipLaunchKernelGGL((layered_stable_dt_kernel<FT, MathFast<FT>>), grid_for(P.ncols, 256), dim3(256), 0, s, P, L, in, aux,
                       courant, reinterpret_cast<U*>(out_ft));
}

#define LH_INSTANTIATE_LAYERED(FT)                                                                                     \
    template void launch_layered_rhs<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&,              \
                                         const Planes<FT>&, const Planes<FT>&, const Planes<FT>&, FT, int, bool, bool, \
                                         hipStream_t);                                                                 \
    template void launch_layered_diag<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&,             \
                                          const Planes<FT>&, const Planes<FT>&, hipStream_t);                          \
    template void launch_layered_boundary_fluxes<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&,  \
                                                     const Planes<FT>&, int, FT*, FT*, bool, hipStream_t);             \
    template void launch_layered_stable_dt<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&,        \
                                               const Planes<FT>&, FT, void*, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_TU
