// lh_layered_stepper.hpp -- the persistent column stepper of layered soils: column_stepper_wave_kernel for the
// Richards model with the column constants taken per CELL.
//
// One wave per column, lane l owns the CW adjacent cells CW l .. CW l + CW - 1 for all steps of the call, so the
// class of a cell is a per-lane constant of the call: its byte is read once in the prologue.  The class table is
// staged in LDS beside the math tables (stage_class_table) and a cell takes `s_cls[k]` where it uses a field, as
// layered_rhs_kernel does: a register copy of the CW entries (46 VGPRs each in Float64) does not fit the budget
// of any instantiation, see section 4.22.  The stage, face and boundary expressions are layered_rhs_kernel's, so
// a call is bitwise the fused stages.
//
// A kernel family of its own, in its own translation units (section 4.18's rule): no kernel, DevParams or ColC
// of another header changes.
//
// The launcher's declaration is what lh_api.hip includes; the kernel follows under LH_LAYERED_STEPPER_TU, which
// only lh_kernels_f64_layered_stepper.hip / lh_kernels_f32_layered_stepper.hip define (with LH_LAYERED_TU, for
// stage_class_table and the variant rules of lh_layered.hpp).
#pragma once
#include "lh_layered.hpp"

namespace lh {

// nsteps SSPRK33 steps of a layered Richards ensemble of up to 128 levels in ONE launch;
// bcv: NULL or [nsteps][3][2][2] FT boundary values (step, stage, face, component)
template <typename FT>
void launch_layered_column_stepper(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                   const Planes<FT>& aux, FT dt, int64_t nsteps, const FT* bcv, bool factors, bool noice,
                                   hipStream_t s);

} // namespace lh

#ifdef LH_LAYERED_STEPPER_TU

namespace lh {

// exchange words of one column: the top cell of every lane (true K, -psi) and the flux of the face below every
// lane's bottom cell, 64 words each
constexpr int LS_EXCHANGE_ARRAYS = 3;

// The variants that exist are layered_rhs_kernel's (production math, NOICE and VGF = false where rhs_kernel has
// them) for one or two cells per lane; there is no BOUND variant.
template <typename M, bool FACTORS, int CW, bool NOICE, bool VGF>
constexpr bool layered_stepper_variant_exists() {
    return layered_variant_exists<M, FACTORS, NOICE, VGF, 1>() && (CW == 1 || CW == 2);
}
// waves per SIMD the compiler is asked to leave room for: cs_wave_min_waves' budgets for the Richards model
template <typename FT, typename M, bool FACTORS, int CW, bool NOICE>
constexpr int layered_stepper_min_waves() {
    return cs_wave_min_waves<FT, MODEL_RICHARDS, FACTORS, false, M, CW, NOICE>();
}
// plane tiles of the prologue: vartheta_l, theta_i unless it is known zero, the aux T with a viscosity factor
static inline int layered_stepper_tiles(bool noice, bool need_Taux) { return 1 + (noice ? 0 : 1) + (need_Taux ? 1 : 0); }

template <typename FT, bool FACTORS, typename M, int CW, bool NOICE, bool VGF>
__global__ void __launch_bounds__(1024, (layered_stepper_min_waves<FT, M, FACTORS, CW, NOICE>()))
layered_column_stepper_wave_kernel(const DevParams<FT> P0, const LayeredArgs<FT> L, const Planes<FT> Y,
                                   const Planes<FT> AUX, const FT dt, const int64_t nsteps, const FT* __restrict__ bcv) {
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    __shared__ ColC<FT> s_cls[LH_LAYERED_MAX_CLASSES];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int n = P0.nlev; // <= 64 CW (the launcher's choice of CW)
    const int slot = int(threadIdx.x) >> 6; // column of this workgroup
    const int l = int(threadIdx.x) & 63;    // lane = CW adjacent cells
    const int cpb = int(blockDim.x) >> 6;
    // per column: (true K, -psi) of every lane's top cell and the flux of the face below its bottom cell
    FT* sK = reinterpret_cast<FT*>(s_dyn) + size_t(slot) * (LS_EXCHANGE_ARRAYS * 64);
    FT* sh = sK + 64;
    FT* sFw = sh + 64;
    const M mm(stage_math_tables<M>(P0.math_tab, s_tab));
    stage_class_table<FT, M, !NOICE>(mm, L, s_cls); // (ends on a workgroup barrier)
    DevParams<FT> P = P0; // boundary values change per stage
    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col_raw = int64_t(blk) * cpb + slot;
    const bool have = col_raw < P.ncols;
    const int64_t col = have ? col_raw : P.ncols - 1; // spare slots shadow the last column
    constexpr bool vgf = VGF && M::uses_tables;
    const bool need_Taux = FACTORS && P.viscosity_kind;
    // planes are column-fastest, lanes here level-fastest: through LDS tiles [cpb][n] (column_stepper_kernel)
    FT* tiles = reinterpret_cast<FT*>(s_dyn);
    const int64_t col_first = int64_t(blk) * cpb;
    const int tile_n = n * cpb;
    auto request = [&](const FT* plane, int k) {
        for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
            const int lev = e / cpb, cs = e - lev * cpb;
            if (col_first + cs < P.ncols) tiles[k * tile_n + cs * n + lev] = plane[int64_t(lev) * P.stride + col_first + cs];
        }
    };
    constexpr int TILE_TI = 1, TILE_TA = NOICE ? 1 : 2;
    request(Y.v[0], 0);
    if (!NOICE) request(Y.v[1], TILE_TI);
    if (need_Taux) request(AUX.v[3], TILE_TA);
    __syncthreads();
    FT y_vl[CW], ti[CW], Ta[CW];
    unsigned kc[CW]; // the class of the lane's cells: constants of the call
    bool act[CW];    // the cell exists (and the column does)
#pragma unroll
    for (int q = 0; q < CW; ++q) {
        const int i = CW * l + q;
        const int ic = i < n ? i : n - 1;
        act[q] = i < n && have;
        y_vl[q] = have ? tiles[slot * n + ic] : FT(0);
        ti[q] = NOICE ? FT(0) : (have ? tiles[TILE_TI * tile_n + slot * n + ic] : FT(0)); // NOICE: the plane is known to be all zeros
        Ta[q] = need_Taux ? (have ? tiles[TILE_TA * tile_n + slot * n + ic] : FT(288)) : FT(288);
        // one byte per cell per call, read where it lies (the column fastest: a lane's bytes are `stride` apart)
        kc[q] = unsigned(L.cls[int64_t(ic) * P.stride + col]) & unsigned(LH_LAYERED_MAX_CLASSES - 1);
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
    const int lt = (n - 1) / CW, qt = (n - 1) - lt * CW; // lane and slot of the top cell
    const bool at_bottom = (l == 0), at_top = (l == lt);
    // the class of the boundary cell this lane owns (the bottom lane: cell 0; the top cell's slot qt is uniform)
    unsigned kb = kc[0];
    if (!at_bottom) {
#pragma unroll
        for (int q = 1; q < CW; ++q)
            if (q == qt) kb = kc[q];
    }
    unsigned kt = kc[0]; // (a column of <= CW cells: the bottom lane owns the top cell as well)
#pragma unroll
    for (int q = 1; q < CW; ++q)
        if (q == qt) kt = kc[q];
    FT nf_acc = FT(0);
    for (int64_t s = 0; s < nsteps; ++s) {
        FT u_vl[CW]; // the stage state
#pragma unroll
        for (int q = 0; q < CW; ++q) u_vl[q] = y_vl[q];
#pragma unroll 1
        for (int stage = 0; stage < 3; ++stage) {
            if (bcv) set_stage_boundary_values(P, bcv + (s * 3 + stage) * 4);
            FT K[CW], psi[CW]; // the TRUE conductivity and -psi (see head_difference)
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const ColC<FT>& c = s_cls[kc[q]];
                FT Kr = FT(0);
                psi[q] = FT(0);
                water_closures<FT, M, FACTORS, true, false, NOICE, true, false, true>(mm, P, c, u_vl[q], ti[q], Ta[q], Kr, psi[q],
                                                                                      nullptr, vgf);
                K[q] = Kr * c.Ksat; // the two cells of a face may differ in Ksat
            }
            // the lane's top cell, for the lane above
            sK[l] = K[CW - 1];
            sh[l] = psi[CW - 1];
            wave_sync();
            // boundary faces: the lane with the bottom cell and the lane with the top cell go through
            // boundary_fluxes TOGETHER (one divergent pass, not two, when both faces need closures)
            FT Fw_b = FT(0), Fw_t = FT(0);
            if (at_bottom || at_top) {
                FT bv = u_vl[0], bti = ti[0], bT = Ta[0], bK = K[0], bpsi = psi[0];
                if (!at_bottom) {
#pragma unroll
                    for (int q = 1; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = Ta[q]; bK = K[q]; bpsi = psi[q]; }
                }
                FT fe, fw;
                boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, s_cls[kb], at_bottom ? FACE_BOTTOM : FACE_TOP, col, bv,
                                                                       bti, bT, bK, -bpsi, fe, fw, nullptr, nullptr, vgf);
                fw = fw * P.inv_dz;
                if (at_bottom) Fw_b = fw;
                else Fw_t = fw;
                if (at_bottom && at_top) { // a column of <= CW cells: the same lane owns both faces
#pragma unroll
                    for (int q = 0; q < CW; ++q)
                        if (q == qt) { bv = u_vl[q]; bti = ti[q]; bT = Ta[q]; bK = K[q]; bpsi = psi[q]; }
                    boundary_fluxes<FT, M, MODEL_RICHARDS, FACTORS, NOICE>(mm, P, s_cls[kt], FACE_TOP, col, bv, bti, bT, bK, -bpsi, fe,
                                                                           Fw_t, nullptr, nullptr, vgf);
                    Fw_t = Fw_t * P.inv_dz;
                }
            }
            // F[q]: the face below the lane's cell q; F[CW]: the face above its top cell.  Every interior face once,
            // lower cell first, with layered_rhs_kernel's line.
            FT Fw[CW + 1];
#pragma unroll
            for (int q = 0; q <= CW; ++q) Fw[q] = FT(0);
            if (at_bottom) Fw[0] = Fw_b;
            else Fw[0] = -(sK[l - 1] + K[0]) * (head_difference(psi[0], sh[l - 1], P.dz) * P.cg2);
#pragma unroll
            for (int q = 1; q < CW; ++q) Fw[q] = -(K[q - 1] + K[q]) * (head_difference(psi[q], psi[q - 1], P.dz) * P.cg2);
            // the face above the lane's top cell is the face below the next lane's bottom cell
            sFw[l] = Fw[0];
            wave_sync();
            if (l < 63) Fw[CW] = sFw[l + 1];
            if (at_top) { // the face above the column's top cell (slot qt) is the boundary
#pragma unroll
                for (int q = 0; q < CW; ++q)
                    if (q == qt) Fw[q + 1] = Fw_t;
            }
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const FT dvl = Fw[q] - Fw[q + 1];
                if (act[q]) nf_acc = fma_ft(dvl, FT(0), nf_acc);
                u_vl[q] = ssprk33_stage_value<FT>(stage, y_vl[q], u_vl[q], dvl, dt);
            }
            wave_sync(); // the neighbours have read this stage's LDS values
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) y_vl[q] = u_vl[q];
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
#pragma unroll
    for (int q = 0; q < CW; ++q) {
        const int i = CW * l + q;
        if (i < n) tiles[slot * n + i] = y_vl[q];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
        const int lev = e / cpb, cs = e - lev * cpb;
        if (col_first + cs < P.ncols) Y.v[0][int64_t(lev) * P.stride + col_first + cs] = tiles[cs * n + lev];
    }
    if (have && nf_acc != nf_acc) atomicOr(P.status, 1u);
}

template <typename FT>
void launch_layered_column_stepper(const DevParams<FT>& P, const LayeredArgs<FT>& L, const Planes<FT>& Y,
                                   const Planes<FT>& aux, FT dt, int64_t nsteps, const FT* bcv, bool factors, bool noice,
                                   hipStream_t s) {
    using M = MathFast<FT>;
    const int cw = (P.nlev + 63) / 64; // (the caller keeps columns of more than 128 levels with the fused stages)
    const bool ni = noice && noice_exists<M>(factors);
    const bool robust = robust_vg_exists<M, MODEL_RICHARDS>() && P.vg_fast_all == 0; // (as launch_layered_rhs)
    const bool need_Taux = factors && P.viscosity_kind;
    // dynamic LDS: the plane tiles of the prologue and the exchange arrays share it
    const size_t ex_words = size_t(LS_EXCHANGE_ARRAYS) * 64;
    const size_t tile_words = size_t(layered_stepper_tiles(ni, need_Taux)) * size_t(P.nlev);
    const size_t dyn_col = (ex_words > tile_words ? ex_words : tile_words) * sizeof(FT);
    with_bool(factors, [&](auto f) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<1, 2>{}, cw, [&](auto w) {
            constexpr bool F = decltype(f)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            constexpr int CW = decltype(w)::value;
            // (ni and robust are normalised above: the guard only keeps what cannot occur un-instantiated)
            if constexpr (layered_stepper_variant_exists<M, F, CW, NI, VG>()) {
                constexpr auto kernel = layered_column_stepper_wave_kernel<FT, F, M, CW, NI, VG>;
                unsigned cpb = wave_stepper_columns<kernel>(P.ncols, dyn_col, nsteps);
                if (P.cs_cpb > 0 && (unsigned)P.cs_cpb * 64u <= 1024u) cpb = (unsigned)P.cs_cpb;
                const dim3 g((unsigned)((P.ncols + cpb - 1) / cpb)), b(64u * cpb);
                hipLaunchKernelGGL(kernel, g, b, (unsigned)(cpb * dyn_col), s, P, L, Y, aux, dt, nsteps, bcv);
            }
        });
    }); }); });
}

#define LH_INSTANTIATE_LAYERED_STEPPER(FT)                                                                            \
    template void launch_layered_column_stepper<FT>(const DevParams<FT>&, const LayeredArgs<FT>&, const Planes<FT>&, \
                                                    const Planes<FT>&, FT, int64_t, const FT*, bool, bool, hipStream_t);

} // namespace lh
#endif // LH_LAYERED_STEPPER_TU
