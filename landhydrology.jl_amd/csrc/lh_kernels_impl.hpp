// lh_kernels_impl.hpp -- gfx950 (MI355X, CDNA4) kernels of the batched soil-column
// tendency path.  No MFMA: this is a bandwidth/VALU-bound vertical stencil.
//
// Data layout: every variable is a plane [nlev][stride] with the
// column index fastest, so a wavefront reads 64*CPL consecutive columns of one
// level in one fully coalesced instruction (CPL = 1 for Float64, 2 for Float32:
// 8 B per lane either way).  One lane owns CPL whole columns
// and marches bottom -> top, carrying K, -psi (T, kappa, rho_e_l K) of the previous
// cell and the previous face flux in registers: each face flux is computed once
// and differenced, which keeps the discrete mass/energy conservation the
// reference's equilibrium tests rely on (coupled.jl:117, richards_equation.jl:94).
#pragma once
#include "lh_closures.hpp"
#include "lh_column_ops.hpp"
#include "lh_launch.hpp"
#include "lh_dispatch.hpp"
#include "lh_atmos.hpp"
#include <type_traits>

namespace lh {

// the coupled tendency launches (MODE 0 and 4) without conductivity factors keep their column constants in
// VGPRs, and the Float32 step-bound launch with them too
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int MODE>
constexpr bool f32_coupled_vgpr_constants() {
    if (MODEL != MODEL_COUPLED || PERCOL || !M::is_production || !(MODE == 0 || MODE == 4)) return false;
    // (Float32 with the step bound, measured on C3, fused-dt launch: VGPR constants at 5 waves 0.215 ms; SGPR
    // constants at 8 waves with 12 B of scratch 0.224, at 7 waves 0.222)
    if (sizeof(FT) == 4 && MODE == 4) return true;
    // Float64: without conductivity factors only.  (Round 2 pinned the factors kernels too, +2.5 % at 127
    // VGPRs + 12 B of scratch; with the round-3 closures the pinned tendency kernel needs 154 VGPRs --
    // 3 waves, 0.61 ms on f3c64 -- or spills 76 B at 4 waves, 0.67 ms; unpinned it fits 119 VGPRs at 4
    // waves without scratch and takes 0.58 ms, v_readlane reloads of spilled uniforms and all.)
    return !FACTORS;
}

template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, bool NOICE>
constexpr bool heat_vgpr_constants() {
    return sizeof(FT) == 8 && MODEL != MODEL_RICHARDS && M::is_production && !NOICE;
}

// Minimum waves per SIMD the register allocator must leave room for in the column kernel: the kernel hides
// HBM latency by occupancy.  The plain production kernels are held to 64 VGPRs (8 waves/SIMD); the per-column /
// conductivity-factor variants and the libm debug policy keep what they need (a bound there only produces
// scratch spills).  One line per class of instantiation, the first match wins.
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int PF, int MODE, bool NOICE = false>
constexpr int rhs_waves_per_simd() {
    constexpr bool F64 = sizeof(FT) == 8, RICHARDS = MODEL == MODEL_RICHARDS;
    // the libm debug policy keeps what it needs
    if (!M::is_production) return 1;
    // Float64 heat / coupled tendency with conductivity factors: 127 VGPRs (4 waves/SIMD, 512-thread workgroups)
    // with the uniform constants left to the SGPR file and its spills beats 156 VGPRs with the constants
    // VGPR-resident at 3 waves (f3c64 tendency 0.530 vs 0.554 ms; round 3: pinned, the kernel needs 154, see
    // f32_coupled_vgpr_constants).  The tendency only: the step-bound launch would spill to scratch under that
    // bound and keeps the other arrangement, the fused stages are left unconstrained (the next line).
    if (FACTORS && F64 && !RICHARDS && !PERCOL && MODE == 0) return 4;
    // every other kernel with conductivity factors is left unconstrained.  (Richards: 66 VGPRs = 6 waves;
    // bounded to 64 for 8 waves it spills SGPRs to lanes and 12 B to scratch, 0.324 vs 0.307 ms on f3v64)
    if (FACTORS) return 1;
    // per-column Richards without ice, tendency + step bound (measured on C5): 6 waves (72 VGPRs) 0.511 ms, 8 waves
    // (64 VGPRs + 20 B of scratch) 0.537 ms
    if (RICHARDS && NOICE && PERCOL && MODE == 4) return 6;
    // Float64 Richards without ice fits 64 VGPRs (8 waves) in every mode, but asked for only 6 waves (<= 80 VGPRs,
    // 512-thread workgroups, 3 per CU) the max-ILP scheduler uses the room: tendency -1 %, with the step bound -2 %,
    // C5 -1.6 %, the Dirichlet ensemble C1 -4 %, fused stages equal (round 3, same-process A/B)
    if (RICHARDS && NOICE && F64) return 6;
    // Float32 Richards without ice, per-column parameters (62 VGPRs) or not: no ice ring, fits 64 VGPRs in every
    // mode (its fused stages lose 5 % at 6)
    if (RICHARDS && NOICE) return 8;
    // every other kernel with per-column parameters is left unconstrained
    if (PERCOL) return 1;
    // Richards with ice: a deeper ring costs registers
    if (RICHARDS && PF > 1) return 7;
    if (RICHARDS) return 8;
    // coupled tendency with its column constants in VGPRs (f32_coupled_vgpr_constants): Float64 unconstrained ...
    if (MODEL == MODEL_COUPLED && (MODE == 0 || MODE == 4) && F64) return 1;
    // ... Float32 with the step bound needs ~90 VGPRs (86 unconstrained): held to 72 it spills 18 values per
    // level to scratch and runs 0.34 instead of 0.2x ms on 1e6 x 64; 5 waves, see f32_coupled_vgpr_constants
    if (MODEL == MODEL_COUPLED && MODE == 4) return 5;
    // ... Float32 plain tendency: 72 rather than 64 VGPRs remove every spill (see rhs_kernel)
    if (MODEL == MODEL_COUPLED && MODE == 0) return 7;
    // the other Float32 heat / coupled kernels (heat-only in every mode, the coupled fused stages)
    if (!F64) return 8;
    // ... and the Float64 ones keep what they need
    return 1;
}

// Threads per workgroup of the column kernel.  The Float64 production math stages 48 KiB of
// log2/exp2 tables per workgroup (lh_fastmath.hpp), so a CU holds 3 such workgroups at most:
// kernels that fit 64 VGPRs run 1024-thread workgroups (2 per CU = 8 waves/SIMD), the others
// 512-thread ones (3 per CU = 6 waves/SIMD).  Everything else (Float32: hardware log/exp, the
// libm debug policy) keeps 256.
template <typename M, int WAVES>
constexpr int rhs_max_threads() {
    return M::uses_tables ? (WAVES >= 8 ? 1024 : 512) : 256;
}
// the waves-per-SIMD the compiler is asked to leave room for, given that workgroup size
template <typename M, int WAVES>
constexpr int rhs_min_waves() {
    if (!M::uses_tables) return WAVES;
    return WAVES >= 8 ? 8 : (WAVES >= 6 ? 6 : (WAVES >= 4 ? 4 : (WAVES >= 2 ? 2 : 1)));
}

// ----------------------------------------------------------------- helpers

// Row access through a buffer descriptor: a uniform row pointer (SGPRs) plus a
// 32-bit lane byte offset -- no 64-bit vector address arithmetic, and loads or
// stores past the end of the row are dropped by the hardware range check.
// (hipcc otherwise turns `row + lane` into per-lane 64-bit induction variables.)
template <typename FT, int N, bool NT>
__device__ __forceinline__ void bload(const FT* row, unsigned row_bytes, unsigned lane_byte, FT (&out)[N]) {
    static_assert(sizeof(FT) * N == 8, "one 8-byte access per lane");
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<FT*>(row), 0, row_bytes, 0x00020000);
    u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, lane_byte, 0, NT ? 2 : 0);
    __builtin_memcpy(out, &v, 8);
}
template <typename FT, int N, bool NT>
__device__ __forceinline__ void bstore(FT* row, unsigned row_bytes, unsigned lane_byte, const FT (&in)[N]) {
    static_assert(sizeof(FT) * N == 8, "one 8-byte access per lane");
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, row_bytes, 0x00020000);
    u32x2 v;
    __builtin_memcpy(&v, in, 8);
    __builtin_amdgcn_raw_buffer_store_b64(v, rs, lane_byte, 0, NT ? 2 : 0);
}

// launch shape of the column kernel: columns per lane, levels kept in flight
// ahead of the one being computed, nontemporal global access
// SEG: level-segmented launch for small ensembles (see rhs_kernel)
template <int CPL_, int PF_, bool NT_, bool SEG_>
struct KCfg {
    static constexpr int CPL = CPL_, PF = PF_;
    static constexpr bool NT = NT_, SEG = SEG_;
};

// Orders one wave's LDS traffic around a hand-off between its lanes: the LDS operations of a wave
// execute in order, so no instruction is needed -- the wave barrier pins the compiler's schedule and
// the two wavefront-scope fences (no code on gfx950) keep it from moving a load of another lane's
// word above the store that produced it.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename FT>
__device__ __forceinline__ bool finite(FT x) {
    return x - x == FT(0);
}

// ------------------------------------------------------------- rhs kernel
//
// rhs!(dY, Y, Ya, t): right_hand_side.jl:118-186 (RICHARDS), :192-263 (HEAT),
// :269-369 (COUPLED).  Stencils: InterpolateC2F = mean,
// GradientC2F = difference/dz, DivergenceF2C = flux difference/dz with the two
// boundary faces replaced by the boundary fluxes (SetValue).
//
// MODE 0: write the tendency dY (its theta_i plane is not touched: d theta_i = 0, see below).
// MODE 4: MODE 0 plus the local stable-step bound of the same state (the rule of
//         stable_dt_kernel, from the K, dpsi/dvl, kappa, rho_c_s this pass has in
//         registers anyway, accumulated in Float32: a Courant-type bound needs seven
//         digits, and the maximum of non-negative floats is an integer maximum of their
//         bits): one division and one integer atomicMin per wave into P.dt_out.
// MODE 1..3: fused SSPRK33 stage s (OrdinaryDiffEq SSPRK33, Shu-Osher form):
//   1: U1 = Y + dt f(Y)              (in = Y,  out = U1)
//   2: U1 = (3 Y + U1 + dt f(U1))/4  (in = U1, base = Y, out = U1)
//   3: Y  = (Y + 2 U1 + 2 dt f(U1))/3 (in = U1, base = Y, out = Y)
// MODE 5: stage 2 of a step whose first stage was NOT stored: in = k1 = f(Y) (a tendency, e.g. the
//         one lh_rhs_stable_dt left with the step bound), base = Y.  U1 = Y + dt k1 is formed in
//         registers with MODE 1's expression and used exactly like MODE 2's stored U1:
//         out = (3 Y + U1 + dt f(U1))/4.  An adaptive step is then MODE 4 + MODE 5 + MODE 3: three
//         evaluations of f instead of four, bitwise the four-launch sequence.
// In the fused stages theta_i is read from BASE (= Y) and never written: its
// tendency is identically zero (right_hand_side.jl:182, :359), so every stage
// value of theta_i equals Y's.
//
// CFG::SEG (small ensembles): a column no longer belongs to one lane.  With fewer
// columns than the chip has lanes the launch is bound by the LATENCY of one lane's
// bottom-to-top march (35 us for 64 Float64 levels, whatever the column count up to
// ~1e5), so blockIdx.y splits every column into segments of P.seg_len levels.  A lane
// computes the closures of its own cells plus the one cell below and the one above its
// segment (the face fluxes at the segment ends are evaluated by both neighbours from
// the same inputs in the same order: bitwise equal, conservation is untouched) and
// emits only its own cells.  Results are bitwise those of the unsegmented launch.
//
// Addressing: a uniform row pointer per plane (SGPRs, advanced by `stride` per
// level) plus one 32-bit lane offset, so the loop carries no vector address
// arithmetic.  The level coordinate z_i comes from LDS (staged once per block):
// as a global load it would sit in the vector-memory queue behind the next
// level's prefetch and force a full vmcnt(0) drain every level.
// NOICE: the theta_i plane the launch would read is known to be all zeros (the zero bits of
// lh_state): it is not read, ti is the literal 0 and the ice branches are compiled out -- the
// same numbers the general kernel produces for ti == 0.
// d theta_i = 0 (right_hand_side.jl:182, :359) is never stored by any mode: the host side keeps
// the theta_i plane of a tendency state zero (cleared once, tracked by the state's zero bits).
// VGF (Float64 production math): every column of the context has m = 1 - 1/n >= LH_VG_FAST_MIN_M, so the
// water closures put the exponents of their 2^(.) in place by integer addition (water_closures_log); the
// host decides (DevParams::vg_fast_all), clay-like ensembles run the VGF = false instantiation.
//
// Which variants exist.  The launchers instantiate the combinations these predicates allow and no other;
// rhs_kernel, the two column steppers and the implicit kernels (lh_implicit.hpp) share the first two.
// NOICE: MathLibm is the parity-debugging policy and always reads theta_i, and the impedance factor is a
// function of theta_i, so a launch with conductivity factors reads the plane whatever its zero bit says.
template <typename M>
constexpr bool noice_exists(bool factors) { return M::is_production && !factors; }
// VGF = false: the integer-exponent form it switches off lives in the table-driven 2^(.) of the water
// closures, which only the Float64 production math of a water model has.
template <typename M, int MODEL>
constexpr bool robust_vg_exists() { return M::uses_tables && MODEL != MODEL_HEAT; }
// ... and clay-like ensembles are rare: they get the production launch shape with plain access, nothing else.
template <typename CFG>
constexpr bool robust_shape_exists() { return !CFG::NT && !CFG::SEG; }
// MODE: MathLibm checks the tendency itself (mode 0); the fused stages and the step bound have no such build.
template <typename M, int MODE>
constexpr bool rhs_mode_exists() { return M::is_production || MODE == 0; }
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename CFG, typename M, int MODE, bool NOICE = false, bool VGF = true>
__global__ void __launch_bounds__((rhs_max_threads<M, rhs_waves_per_simd<FT, MODEL, FACTORS, PERCOL, M, CFG::PF, MODE, NOICE>()>()),
                                  (rhs_min_waves<M, rhs_waves_per_simd<FT, MODEL, FACTORS, PERCOL, M, CFG::PF, MODE, NOICE>()>()))
rhs_kernel(const DevParams<FT> P0, const Planes<FT> IN, const Planes<FT> AUX, const Planes<FT> BASE,
           const Planes<FT> OUT, const FT dt_value, const FT* __restrict__ dt_device) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    constexpr bool TEND_MODE = (MODE == 0 || MODE == 4); // (the fused stages: measured slower with it)
    // The Float64 heat kernels with conductivity factors or ice run at 3 waves/SIMD whatever they
    // do (130 VGPRs) and need more uniform constants than there are SGPRs: the compiler spills the
    // excess to VGPR lanes and reloads them with v_readlane in front of every use (20 VALU
    // instructions per cell).  The constants of the heat closures held in VGPRs instead remove that.
    DevParams<FT> P = P0;
    if constexpr (heat_vgpr_constants<FT, MODEL, FACTORS, PERCOL, M, NOICE>() && TEND_MODE && (!FACTORS || PERCOL || MODE == 4)) {
        auto vr = [](FT& x) { asm volatile("" : "+v"(x)); };
        vr(P.rho_c_ds); vr(P.rhocp_l); vr(P.rhocp_i); vr(P.T_ref); vr(P.kappa_sat_unfrozen);
        vr(P.l2_kappa_sat_unfrozen); vr(P.l2_kappa_sat_frozen); vr(P.kersten_exp_unfrozen);
        vr(P.kersten_exp_frozen); vr(P.neg_b_log2e_sc);
        if (MODE != 4) { // (the step-bound bookkeeping of MODE 4 needs the registers: 175 VGPRs = 2 waves/SIMD otherwise)
            vr(P.rho_i); vr(P.LH_f0); vr(P.inv_dz); vr(P.half_inv_dz);
            if (FACTORS) { vr(P.gamma); vr(P.T_ref_visc); vr(P.Omega); }
        }
    }
    // The Float64 tendency with conductivity factors stays at 4 waves per SIMD (128 registers) with the
    // uniforms in the SGPR file and its spills (see rhs_waves_per_simd) -- but the three constants every
    // cell's T and rho_e_l K use fit beside them: 52 -> fewer v_readlane per two cells, f3c64 0.560 ->
    // 0.546 ms (same-process A/B; five -- rhocp_i, rho_i too -- or eight -- LH_f0, gamma, Omega too -- pinned: no
    // further gain).  MODE 0 only: the fused stages carry more state, the same pinning costs them a wave, 0.64 -> 0.81 ms.
    if constexpr (heat_vgpr_constants<FT, MODEL, FACTORS, PERCOL, M, NOICE>() && MODE == 0 && FACTORS && !PERCOL) {
        auto vr = [](FT& x) { asm volatile("" : "+v"(x)); };
        vr(P.rho_c_ds); vr(P.rhocp_l); vr(P.T_ref);
    }
    constexpr int CPL = CFG::CPL, PF = CFG::PF;
    constexpr bool NT = CFG::NT;
    constexpr bool TEND = (MODE == 0 || MODE == 4); // writes a tendency (not a stage state)
    constexpr bool WANT_DT = (MODE == 4);
    // the step size either comes by value or is read from device memory, where a
    // preceding stable-dt reduction / RCCL min all-reduce left it (no host sync)
    const FT dt = (!TEND && dt_device) ? *dt_device : dt_value; // MODE 4: dt_value = courant
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int n = P.nlev;
    // MODE 4: one LDS word per thread for the wave-level maximum of the face diffusivities; lanes
    // past the last column leave the neutral 0 there
    float* s_red = reinterpret_cast<float*>(s_dyn);
    if (WANT_DT) s_red[threadIdx.x] = 0.0f;
    __shared__ unsigned s_waves_done; // MODE 4: waves of this workgroup that have left their maximum in s_red
    if (WANT_DT && threadIdx.x == 0) s_waves_done = 0u;
    // level-uniform prescribed fields of Ya (DevParams::aux_prof), staged behind the reduction
    // words: T for the Richards viscosity factor, vartheta_l and theta_i for the heat-only model
    constexpr bool MAY_PROF = (MODEL == MODEL_HEAT) || (MODEL == MODEL_RICHARDS && FACTORS);
    FT* s_pf = reinterpret_cast<FT*>(s_dyn + (WANT_DT ? ((size_t(blockDim.x) * sizeof(float) + 15) & ~size_t(15)) : 0));
    const FT* pf_T = (MAY_PROF && MODEL == MODEL_RICHARDS) ? P.aux_prof[3] : nullptr;
    const FT* pf_vl = (MAY_PROF && MODEL == MODEL_HEAT) ? P.aux_prof[0] : nullptr;
    const FT* pf_ti = (MAY_PROF && MODEL == MODEL_HEAT) ? P.aux_prof[1] : nullptr;
    if constexpr (MAY_PROF) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            if (pf_T) s_pf[i] = pf_T[i];
            if (pf_vl) s_pf[i] = pf_vl[i];
            if (pf_ti) s_pf[n + i] = pf_ti[i];
        }
    }
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    if (!M::uses_tables) __syncthreads();

    // xcd_block's lines (through the call its blocks land in front of the staging loop and one scalar branch flips)
    unsigned blk = blockIdx.x;
    if (P.xcd_remap) {
        const unsigned per = gridDim.x >> 3;
        if (blk < (per << 3)) blk = (blk & 7u) * per + (blk >> 3);
    }
    const int64_t col0 = (int64_t(blk) * blockDim.x + threadIdx.x) * CPL;
    if (col0 >= P.ncols) return;
    const int64_t stride = P.stride;
    // cells this lane emits: [i_lo, i_hi); cells whose closures it evaluates: [i_first, i_end)
    constexpr bool SEG = CFG::SEG;
    const int i_lo = SEG ? int(blockIdx.y) * P.seg_len : 0;
    const int i_hi = SEG ? (i_lo + P.seg_len < n ? i_lo + P.seg_len : n) : n;
    const int i_first = (SEG && i_lo > 0) ? i_lo - 1 : 0;
    const int i_end = (SEG && i_hi < n) ? i_hi + 1 : n;
    // 32-bit BYTE offset of this lane inside a plane row (lh_create bounds a row to < 4 GiB)
    const unsigned lane_byte = (unsigned)col0 * (unsigned)sizeof(FT);
    const unsigned row_bytes = (unsigned)(stride * (int64_t)sizeof(FT));
    // (one 8-byte access per lane: CPL = 1 Float64, 2 Float32)
    auto rload = [&](const FT* row, FT (&out)[CPL]) { bload<FT, CPL, NT>(row, row_bytes, lane_byte, out); };
    auto rstore = [&](FT* row, const FT (&in)[CPL]) { bstore<FT, CPL, NT>(row, row_bytes, lane_byte, in); };

    // uniform row pointers (level 0); HEAT reads the prescribed water fields from
    // Ya (right_hand_side.jl:200-201); fused stages read theta_i from BASE
    const int64_t in0 = SEG ? stride * i_first : 0, out0 = SEG ? stride * i_lo : 0;
    constexpr bool FROM_K1 = (MODE == 5); // the stage state is Y + dt k1, formed on the fly
    const FT* r_vl = (MODEL == MODEL_HEAT ? AUX.v[0] : (FROM_K1 ? BASE.v[0] : IN.v[0])) + in0;
    const FT* r_ti = NOICE ? nullptr : (MODEL == MODEL_HEAT ? AUX.v[1] : (TEND ? IN.v[1] : BASE.v[1])) + in0;
    const FT* r_re = HEAT ? (FROM_K1 ? BASE.v[2] : IN.v[2]) + in0 : nullptr;
    const FT* r_k1v = (FROM_K1 && WATER) ? IN.v[0] + in0 : nullptr; // k1 = f(Y)
    const FT* r_k1e = (FROM_K1 && HEAT) ? IN.v[2] + in0 : nullptr;
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && FACTORS && P.viscosity_kind;
    const FT* r_Ta = need_Taux ? AUX.v[3] + in0 : nullptr;
    const FT* b_vl = ((MODE == 2 || MODE == 3) && WATER) ? BASE.v[0] + out0 : nullptr;
    const FT* b_re = ((MODE == 2 || MODE == 3) && HEAT) ? BASE.v[2] + out0 : nullptr;
    FT* o_vl = WATER ? OUT.v[0] + out0 : nullptr;
    FT* o_re = HEAT ? OUT.v[2] + out0 : nullptr;

    ColC<FT> c[CPL];
    int64_t colj[CPL]; // column index clamped into [0, ncols): pad lanes reuse the last column
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        colj[j] = col0 + j < P.ncols ? col0 + j : P.ncols - 1;
        c[j] = make_colc<FT, M>(P, colj[j], PERCOL);
        if (WATER && !NOICE) finish_colc<FT, M>(mm, c[j]);
        // (psi's exponent is an fma of two column constants: one of them has to sit in a VGPR anyway --
        // pinned here, it is not re-materialised from its SGPR pair in front of every use)
        if constexpr (M::uses_tables && WATER && !PERCOL && !HEAT) asm volatile("" : "+v"(c[j].e_log2_alpha));
    }
    // Float32 coupled tendency: with every uniform constant in SGPRs the kernel spills 45 of them
    // to VGPR lanes (28 v_readlane per two cells).  Thirteen column constants held in VGPRs
    // instead (and 72 rather than 64 VGPRs: 7 waves/SIMD) remove every spill: +1..2.5 %.
    if constexpr (f32_coupled_vgpr_constants<FT, MODEL, FACTORS, PERCOL, M, MODE>()) {
        auto vr = [](FT& x) { asm volatile("" : "+v"(x)); };
        ColC<FT>& q = c[0];
        vr(q.nu); vr(q.theta_lim); vr(q.theta_r); vr(q.inv_por); vr(q.e_inv_m); vr(q.e_m); vr(q.e_one);
        vr(q.e_inv_n); vr(q.e_log2_alpha); vr(q.Ksat); vr(q.inv_S_s); vr(q.inv_nu); vr(q.k_dry);
        if (!NOICE) vr(q.l2_por);
#pragma unroll
        for (int j = 1; j < CPL; ++j) c[j] = c[0];
    }

    constexpr bool vgf = VGF && M::uses_tables; // integer-exponent 2^(.) (a host decision)
    // fluxes in tendency units, K without Ksat (flux_scales)
    const FT cgT = P.cg2;
    FT cgw[CPL], Ksc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) flux_scales<FT, M>(P, c[j], Ksc[j], cgw[j]);

    FT vl[CPL], ti[CPL], re[CPL], Ta[CPL];         // current cell inputs
    FT vl_n[PF][CPL], ti_n[PF][CPL], re_n[PF][CPL], Ta_n[PF][CPL]; // PF levels in flight
    FT kv_n[PF][CPL], ke_n[PF][CPL];               // MODE 5: k1 of those levels
    FT vl_p[CPL], re_p[CPL];                       // previous cell inputs (fused stages)
    FT yv[CPL], ye[CPL], yv_p[CPL], ye_p[CPL];     // MODE 5: Y of the current / previous cell (the stage's base)
    FT K_p[CPL], psi_p[CPL], T_p[CPL], kap_p[CPL], E_p[CPL];
    FT Fw_lo[CPL], Fe_lo[CPL];
    FT nf_acc = FT(0); // += 0 * tendency: becomes NaN once any tendency is non-finite
    // MODE 4: stable-step bookkeeping, in Float32 whatever FT is (see slope32): n m d psi / d vl
    // and 1 / rho_c_s of the previous cell, and the lane's maxima of TWICE the water (x n m) and
    // heat face diffusivities (the column constant n m and the exact factor 1/2 of the mean
    // coefficients are divided out once per column / wave at the end)
    float dpsi_p[CPL], ircs_p[CPL], DmaxW[CPL], DmaxT[CPL];
    float DmaxWb[CPL]; // the Dirichlet-face terms, formed with TRUE conductivities (DmaxW: relative to Ksc)

#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        K_p[j] = psi_p[j] = T_p[j] = kap_p[j] = E_p[j] = Fw_lo[j] = Fe_lo[j] = FT(0);
        vl_p[j] = re_p[j] = FT(0);
        yv[j] = ye[j] = yv_p[j] = ye_p[j] = FT(0);
        vl[j] = ti[j] = re[j] = FT(0);
        Ta[j] = FT(288); // PrescribedTemperatureModel default (models.jl:53)
        dpsi_p[j] = DmaxW[j] = DmaxWb[j] = DmaxT[j] = ircs_p[j] = 0.0f;
    }
    // loads the level the row pointers currently address into ring slot `slot`,
    // then moves the pointers one level up
    int lev_f = i_first; // the level fetch() addresses
    auto fetch = [&](int slot) {
        if (MAY_PROF && pf_vl) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) vl_n[slot][j] = s_pf[lev_f];
        } else rload(r_vl, vl_n[slot]);
        if (!NOICE) {
            if (MAY_PROF && pf_ti) {
#pragma unroll
                for (int j = 0; j < CPL; ++j) ti_n[slot][j] = s_pf[n + lev_f];
            } else rload(r_ti, ti_n[slot]);
        }
        if (HEAT) rload(r_re, re_n[slot]);
        if (need_Taux) {
            if (MAY_PROF && pf_T) {
#pragma unroll
                for (int j = 0; j < CPL; ++j) Ta_n[slot][j] = s_pf[lev_f];
            } else rload(r_Ta, Ta_n[slot]);
        }
        ++lev_f;
        if (FROM_K1 && WATER) { rload(r_k1v, kv_n[slot]); r_k1v += stride; }
        if (FROM_K1 && HEAT) { rload(r_k1e, ke_n[slot]); r_k1e += stride; }
        r_vl += stride;
        if (!NOICE) r_ti += stride;
        if (HEAT) r_re += stride;
        if (need_Taux) r_Ta += stride;
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl_n[k][j] = ti_n[k][j] = re_n[k][j] = kv_n[k][j] = ke_n[k][j] = FT(0);
            Ta_n[k][j] = FT(288);
        }
        if (i_first + k < i_end) fetch(k);
    }

    // emit the result of the cell the OUT/BASE row pointers address
    auto emit = [&](const FT (&Fw_hi)[CPL], const FT (&Fe_hi)[CPL], const FT (&u_vl)[CPL],
                    const FT (&u_re)[CPL], const FT (&y_vl)[CPL], const FT (&y_re)[CPL]) {
        FT dvl[CPL], dre[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            dvl[j] = WATER ? Fw_lo[j] - Fw_hi[j] : FT(0); // -(F_hi - F_lo), fluxes in tendency units
            dre[j] = HEAT ? Fe_lo[j] - Fe_hi[j] : FT(0);
            if (CPL == 1 || col0 + j < P.ncols) {
                if (WATER) nf_acc = fma_ft(dvl[j], FT(0), nf_acc);
                if (HEAT) nf_acc = fma_ft(dre[j], FT(0), nf_acc);
            }
        }
        if (TEND) {
            if (WATER) rstore(o_vl, dvl); // (d theta_i = 0: the plane is kept zero by the host side)
            if (HEAT) rstore(o_re, dre);
        } else {
            auto stage = [&](const FT* brow, FT* orow, const FT (&u)[CPL], const FT (&k)[CPL], const FT (&yb)[CPL]) {
                constexpr int STAGE = MODE == 1 ? 0 : (MODE == 3 ? 2 : 1); // (MODE 2 and 5 are stage 1)
                FT b[CPL] = {}, r[CPL]; // (b = 0: MODE 1 passes it on, stage 0 ignores it)
                if (MODE == 2 || MODE == 3) rload(brow, b);
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    if (FROM_K1) b[j] = yb[j]; // (the base was read with the state: no second load)
                    r[j] = ssprk33_stage_value<FT>(STAGE, b[j], u[j], k[j], dt);
                }
                rstore(orow, r);
            };
            if (WATER) stage(b_vl, o_vl, u_vl, dvl, y_vl);
            if (HEAT) stage(b_re, o_re, u_re, dre, y_re);
        }
        if (WATER) {
            o_vl += stride;
            if (MODE == 2 || MODE == 3) b_vl += stride;
        }
        if (HEAT) {
            o_re += stride;
            if (MODE == 2 || MODE == 3) b_re += stride;
        }
    };

    for (int i0 = i_first; i0 < i_end; i0 += PF) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int i = i0 + k;
        if (PF > 1 && i >= i_end) break;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            vl[j] = vl_n[k][j];
            ti[j] = NOICE ? FT(0) : ti_n[k][j];
            re[j] = re_n[k][j];
            Ta[j] = Ta_n[k][j];
            if (FROM_K1) { // U1 = Y + dt k1, MODE 1's expression
                yv[j] = vl[j];
                ye[j] = re[j];
                if (WATER) vl[j] = yv[j] + dt * kv_n[k][j];
                if (HEAT) re[j] = ye[j] + dt * ke_n[k][j];
            }
        }
        // keep PF levels in flight ahead of the one computed.  (Refilling the slot only AFTER the cell's
        // closures, so that the load lands in the registers they free and the ring needs no moves,
        // was measured: -1 instruction per cell but the prefetch distance shrinks by a cell -- C2 +2 %,
        // the HBM-bound Float32 C3 +5 % slower; with 4 levels in flight -1 % at twice the code.)
        if (i + PF < i_end) fetch(k);
        FT K[CPL], psi[CPL], T[CPL], kap[CPL], E[CPL]; // (psi[], psi_p[] hold -psi: see head_difference)
        float dpsi[CPL], ircs[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            // cell_closures' lines, kept in this kernel's own text: through the call the step-bound terms of the MODE 4
            // instantiations come out in other registers, and rhs_kernel's device code is held fixed
            FT rcs = FT(1);
            T[j] = Ta[j];
            kap[j] = FT(0);
            K[j] = psi[j] = E[j] = FT(0);
            dpsi[j] = ircs[j] = 0.0f;
            if (HEAT) {
                T[j] = temperature_closure<FT, M, NOICE>(mm, P, c[j], vl[j], ti[j], re[j], rcs);
                kap[j] = kappa_closure<FT, M, NOICE>(mm, P, c[j], vl[j], ti[j]);
                if (WANT_DT) ircs[j] = float(mm.rcp(rcs)); // (the reciprocal temperature_closure formed)
            }
            if (WATER) {
                water_closures<FT, M, FACTORS, true, WANT_DT, NOICE, M::is_production, HEAT, true>(mm, P, c[j], vl[j], ti[j], T[j], K[j],
                                                                                                   psi[j], &dpsi[j], vgf);
                if (HEAT) E[j] = (P.rhocp_l * (T[j] - P.T_ref)) * K[j]; // rho_e_int_l * K (:364)
            }
            if (WANT_DT && i > i_first) { // the rule of stable_dt_kernel per interior face (x 2)
                if (WATER) DmaxW[j] = max_nonneg(DmaxW[j], float(K_p[j] + K[j]) * max_nonneg(dpsi_p[j], dpsi[j]));
                if (HEAT) DmaxT[j] = max_nonneg(DmaxT[j], float(kap_p[j] + kap[j]) * max_nonneg(ircs_p[j], ircs[j]));
            }
        }
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                FT K_f = FT(0), kap_f = FT(0);
                const FT K_c = K[j] * Ksc[j]; // the true conductivity of the boundary cell
                boundary_fluxes<FT, M, MODEL, FACTORS, NOICE>(mm, P, c[j], FACE_BOTTOM, colj[j], vl[j], ti[j],
                                                              T[j], K_c, -psi[j], Fe_lo[j], Fw_lo[j], &K_f, &kap_f, vgf);
                Fe_lo[j] = Fe_lo[j] * P.inv_dz;
                Fw_lo[j] = Fw_lo[j] * P.inv_dz;
                if (WANT_DT) { // the bottom cell's own coefficients; Dirichlet faces: half a cell away, face-state coefficients
                    DmaxW[j] = max_nonneg(DmaxW[j], 2.0f * float(K[j]) * dpsi[j]);
                    DmaxWb[j] = max_nonneg(DmaxWb[j], 4.0f * float(fmax_ft(K_f, K_f > FT(0) ? K_c : FT(0))) * dpsi[j]);
                    if (HEAT) {
                        DmaxT[j] = max_nonneg(DmaxT[j], 2.0f * float(kap[j]) * ircs[j]);
                        DmaxT[j] = max_nonneg(DmaxT[j], 4.0f * float(fmax_ft(kap_f, kap_f > FT(0) ? kap[j] : FT(0))) * ircs[j]);
                    }
                }
            }
        } else if (!SEG || i > i_first) { // (the cell below a segment only primes the *_p values)
            FT Fw[CPL], Fe[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j)
                interior_face<FT, WATER, HEAT>(K_p[j], psi_p[j], T_p[j], kap_p[j], E_p[j], K[j], psi[j], T[j], kap[j], E[j],
                                               P.dz, cgw[j], cgT, Fw[j], Fe[j]);
            if (!SEG || i > i_lo) emit(Fw, Fe, vl_p, re_p, yv_p, ye_p); // cell i-1 belongs to this segment
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
            if (FROM_K1) {
                yv_p[j] = yv[j];
                ye_p[j] = ye[j];
            }
            K_p[j] = K[j];
            psi_p[j] = psi[j];
            T_p[j] = T[j];
            kap_p[j] = kap[j];
            E_p[j] = E[j];
            if (WANT_DT) {
                dpsi_p[j] = dpsi[j];
                ircs_p[j] = ircs[j];
            }
        }
      }
    }
    if (!SEG || i_hi == n) { // the top face of the column
        FT Fw[CPL], Fe[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            FT K_f = FT(0), kap_f = FT(0);
            const FT K_c = K_p[j] * Ksc[j]; // the true conductivity of the boundary cell
            boundary_fluxes<FT, M, MODEL, FACTORS, NOICE>(mm, P, c[j], FACE_TOP, colj[j], vl[j], ti[j], T_p[j],
                                                          K_c, -psi_p[j], Fe[j], Fw[j], &K_f, &kap_f, vgf);
            Fe[j] = Fe[j] * P.inv_dz;
            Fw[j] = Fw[j] * P.inv_dz;
            if (WANT_DT) { // the top cell's own coefficients, and the Dirichlet face's
                DmaxW[j] = max_nonneg(DmaxW[j], 2.0f * float(K_p[j]) * dpsi_p[j]);
                DmaxWb[j] = max_nonneg(DmaxWb[j], 4.0f * float(fmax_ft(K_f, K_f > FT(0) ? K_c : FT(0))) * dpsi_p[j]);
                if (HEAT) {
                    DmaxT[j] = max_nonneg(DmaxT[j], 2.0f * float(kap_p[j]) * ircs_p[j]);
                    DmaxT[j] = max_nonneg(DmaxT[j], 4.0f * float(fmax_ft(kap_f, kap_f > FT(0) ? kap_p[j] : FT(0))) * ircs_p[j]);
                }
            }
        }
        emit(Fw, Fe, vl_p, re_p, yv_p, ye_p);
    }
    if (nf_acc != nf_acc) atomicOr(P.status, 1u);
    if (WANT_DT) { // dt = courant dz^2 / (max D over the wave's columns), one atomicMin per wave
        float dmax = 0.0f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) { // (a column whose maximum is NaN is dropped: it is flagged through P.status)
            const float Dj = max_nonneg(max_nonneg(DmaxW[j] * float(Ksc[j]), DmaxWb[j]) * float(FT(1) / (c[j].n * c[j].m)), DmaxT[j]);
            if ((CPL == 1 || col0 + j < P.ncols) && Dj == Dj) dmax = max_nonneg(dmax, Dj);
        }
        // Wave maximum by a binary tree through LDS (one division per workgroup: bound_publish).
        // Lanes past the last column returned early -- a cross-lane shuffle could read their dead
        // registers; their LDS words hold the neutral 0 from the prologue.  The lanes still here
        // are a prefix of the wave (col0 grows with the lane), so lane l < off always has its
        // partner's word to read.  One wave = one 64-word segment; the LDS operations of a wave
        // execute in order, so the wave barriers only pin the compiler's ordering.
        float* seg = s_red + (threadIdx.x & ~63u);
        const unsigned l = threadIdx.x & 63u;
        seg[l] = dmax;
#pragma unroll
        for (unsigned off = 32; off > 0; off >>= 1) {
            wave_sync();
            if (l < off) {
                dmax = max_nonneg(dmax, seg[l + off]);
                seg[l] = dmax;
            }
        }
        // One candidate per WORKGROUP: the last of its waves to get here (an LDS counter; no barrier, nobody waits)
        // folds the others' maxima in -- seg[0] of every wave, written before that wave's count, in order.
        if (l == 0) {
            const int64_t first_lane = int64_t(blk) * blockDim.x;             // lanes (of CPL columns) before this workgroup
            const int64_t lanes_left = (P.ncols + CPL - 1) / CPL - first_lane;  // > 0: the grid covers the columns
            const unsigned nwaves = blockDim.x >> 6;
            const unsigned nw = lanes_left >= int64_t(blockDim.x) ? nwaves : unsigned((lanes_left + 63) >> 6); // waves not gone at the top
            if (atomicAdd(&s_waves_done, 1u) == nw - 1u) {
                for (unsigned w = 0; w < nwaves; ++w) dmax = max_nonneg(dmax, s_red[w << 6]);
                if (dmax > 0.0f) bound_publish<FT>(P, dt, dmax); // (MODE 4: dt carries the Courant factor)
            }
        }
    }
}

// --------------------------------------------- persistent column stepper
//
// Ensembles of a few columns (the reference's own shape is ONE column): even
// level-segmented, a fused SSPRK33 step is three dependent launches of ~6 us each.
// Here one workgroup owns one column and one thread one CELL, the state lives in
// registers, and the whole loop over steps and stages runs inside one launch: per
// stage every thread evaluates the closures of its cell, publishes K, -psi (T, kappa,
// rho_e_l K) in LDS, and forms the flux of the face below and the face above it from
// its neighbours' values -- each interior face is evaluated by both adjacent threads
// with the expression of rhs_kernel (lower cell first), so the step is bitwise the
// fused-stage one and conservation is untouched.  Two barriers per stage.
// bcv: NULL or [nsteps][3][2][2] FT boundary values (step, stage, face, component).
// This thread-per-cell form serves columns of MORE than 128 levels; up to 128 levels a column is one
// wavefront with one or two adjacent cells per lane and no workgroup barrier at all
// (column_stepper_wave_kernel below).
// exchange arrays per column (StepperLds) / plane tiles of the initial fetch: the two share the dynamic LDS
constexpr int CS_FACE_WORDS = 8; // column_stepper_wave_kernel: 2 faces x (K, psi, kappa) of a Dirichlet face state, padded
// one-wave columns also publish the flux of the face BELOW each cell (water and/or heat), so that the
// face above is read, not evaluated a second time
template <int MODEL> constexpr int cs_flux_arrays() {
    return MODEL == MODEL_COUPLED ? 2 : 1;
}
static inline int cs_fetch_tiles(int model, bool noice, bool need_Taux) {
    if (model == MODEL_RICHARDS) return 1 + (noice ? 0 : 1) + (need_Taux ? 2 : 0); // T sits in tile 3
    return 3; // vl, ti, rhoe (HEAT reads the first two from Ya)
}

template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, bool NOICE = false, bool VGF = true>
__global__ void __launch_bounds__(1024)
column_stepper_kernel(const DevParams<FT> P0, const Planes<FT> Y, const Planes<FT> AUX, const FT dt_value,
                      const FT* __restrict__ dt_device, const int64_t nsteps, const FT* __restrict__ bcv) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 2];
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int n = P0.nlev;
    // a workgroup holds blockDim.x / tpc columns of tpc = roundup(n, 64) threads each (they
    // share the staged math tables; the barriers couple them, which costs nothing)
    const int tpc = (n + 63) & ~63;
    const int slot = int(threadIdx.x) / tpc;
    const int cpb = int(blockDim.x) / tpc;
    const FT dt = dt_device ? *dt_device : dt_value;
    constexpr int NARR = cs_exchange_arrays<MODEL>();
    const StepperLds<FT, MODEL> ex(reinterpret_cast<FT*>(s_dyn) + size_t(slot) * NARR * n, n); // this column's
    const M mm(stage_math_tables<M>(P0.math_tab, s_tab));
    if (!M::uses_tables) __syncthreads();
    DevParams<FT> P = P0; // boundary values change per stage
    const int i = int(threadIdx.x) - slot * tpc;
    const unsigned blk = xcd_block(P.xcd_remap);
    const int64_t col_raw = int64_t(blk) * cpb + slot;
    const bool cell = i < n && col_raw < P.ncols;
    const int ic = i < n ? i : n - 1;
    const int64_t col = col_raw < P.ncols ? col_raw : P.ncols - 1; // spare slots shadow the last column
    ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    if (WATER && !NOICE) finish_colc<FT, M>(mm, c);
    constexpr bool vgf = VGF && M::uses_tables; // (as rhs_kernel)
    const FT cgT = P.cg2;
    FT Ksc, cgw;
    flux_scales<FT, M>(P, c, Ksc, cgw);
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && FACTORS && P.viscosity_kind;
    // Planes are column-fastest, threads here are level-fastest: go through LDS tiles so that
    // global memory sees the cpb adjacent columns of a level as one contiguous piece.  All
    // planes are requested before the one barrier (a block is short-lived when nsteps is
    // small: serialised round trips to HBM would dominate it).
    FT* tiles = reinterpret_cast<FT*>(s_dyn); // tiles [cpb][n] in the exchange arrays' space (tile k <= 3)
    const int64_t col_first = int64_t(blk) * cpb;
    const int tile_n = n * cpb;
    auto request = [&](const FT* plane, int k) {
        for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
            const int lev = e / cpb, cs = e - lev * cpb;
            if (col_first + cs < P.ncols) tiles[k * tile_n + cs * n + lev] = plane[int64_t(lev) * P.stride + col_first + cs];
        }
    };
    auto fetched = [&](int k) -> FT { return (col_raw < P.ncols) ? tiles[k * tile_n + slot * n + ic] : FT(0); };
    // HEAT reads the prescribed water fields from Ya (right_hand_side.jl:200-201); level-uniform
    // prescribed fields (DevParams::aux_prof) come from their [nlev] arrays, not from planes
    const FT* pf_vl = MODEL == MODEL_HEAT ? P.aux_prof[0] : nullptr;
    const FT* pf_ti = MODEL == MODEL_HEAT ? P.aux_prof[1] : nullptr;
    const FT* pf_T = need_Taux ? P.aux_prof[3] : nullptr;
    if (!pf_vl) request(MODEL == MODEL_HEAT ? AUX.v[0] : Y.v[0], 0);
    if (!NOICE && !pf_ti) request(MODEL == MODEL_HEAT ? AUX.v[1] : Y.v[1], 1);
    if (HEAT) request(Y.v[2], 2);
    if (need_Taux && !pf_T) request(AUX.v[3], 3);
    __syncthreads();
    FT y_vl = pf_vl ? pf_vl[ic] : fetched(0);
    const FT ti = NOICE ? FT(0) : (pf_ti ? pf_ti[ic] : fetched(1)); // NOICE: the theta_i plane is known to be all zeros
    FT y_re = HEAT ? fetched(2) : FT(0);
    const FT Ta = need_Taux ? (pf_T ? pf_T[ic] : fetched(3)) : FT(288);
    __syncthreads();
    FT nf_acc = FT(0);
    for (int64_t s = 0; s < nsteps; ++s) {
        FT u_vl = y_vl, u_re = y_re; // the stage state
#pragma unroll 1
        for (int stage = 0; stage < 3; ++stage) {
            if (bcv) set_stage_boundary_values(P, bcv + (s * 3 + stage) * 4);
            FT T, kap, K, psi, E; // psi: -psi
            float dpsi, ircs;     // (the step bound's: not formed here)
            cell_closures<FT, M, MODEL, FACTORS, NOICE, false>(mm, P, c, u_vl, ti, u_re, Ta, vgf, T, kap, K, psi, E, dpsi, ircs);
            if (i < n) {
                if (WATER) { ex.K[i] = K; ex.h[i] = psi; }
                if (HEAT) { ex.T[i] = T; ex.kap[i] = kap; }
                if (HEAT && WATER) ex.E[i] = E;
            }
            __syncthreads();
            FT Fw_lo = FT(0), Fe_lo = FT(0), Fw_hi = FT(0), Fe_hi = FT(0);
            // boundary faces: the bottom thread and the top thread go through boundary_fluxes
            // TOGETHER (one divergent pass, not two, when both faces need closures)
            FT Fw_b = FT(0), Fe_b = FT(0);
            const bool at_bottom = (i == 0), at_top = (i == n - 1);
            if (i < n && (at_bottom || at_top)) {
                boundary_fluxes<FT, M, MODEL, FACTORS, NOICE>(mm, P, c, at_bottom ? FACE_BOTTOM : FACE_TOP, col, u_vl, ti,
                                                              T, K * Ksc, -psi, Fe_b, Fw_b, nullptr, nullptr, vgf);
                Fe_b = Fe_b * P.inv_dz;
                Fw_b = Fw_b * P.inv_dz;
            }
            if (i < n) {
                if (at_bottom) {
                    Fw_lo = Fw_b;
                    Fe_lo = Fe_b;
                } else {
                    interior_face<FT, WATER, HEAT>(ex.K[i - 1], ex.h[i - 1], ex.T[i - 1], ex.kap[i - 1], ex.E[i - 1], K, psi, T, kap, E,
                                                   P.dz, cgw, cgT, Fw_lo, Fe_lo);
                }
                if (at_top) {
                    if (at_bottom) { // a one-cell column: the same thread owns both faces
                        boundary_fluxes<FT, M, MODEL, FACTORS, NOICE>(mm, P, c, FACE_TOP, col, u_vl, ti, T, K * Ksc, -psi, Fe_hi, Fw_hi, nullptr, nullptr, vgf);
                        Fe_hi = Fe_hi * P.inv_dz;
                        Fw_hi = Fw_hi * P.inv_dz;
                    } else {
                        Fw_hi = Fw_b;
                        Fe_hi = Fe_b;
                    }
                } else {
                    interior_face<FT, WATER, HEAT>(K, psi, T, kap, E, ex.K[i + 1], ex.h[i + 1], ex.T[i + 1], ex.kap[i + 1], ex.E[i + 1],
                                                   P.dz, cgw, cgT, Fw_hi, Fe_hi);
                }
            }
            const FT dvl = WATER ? Fw_lo - Fw_hi : FT(0);
            const FT dre = HEAT ? Fe_lo - Fe_hi : FT(0);
            if (cell) {
                if (WATER) nf_acc = fma_ft(dvl, FT(0), nf_acc);
                if (HEAT) nf_acc = fma_ft(dre, FT(0), nf_acc);
            }
            if (WATER) u_vl = ssprk33_stage_value<FT>(stage, y_vl, u_vl, dvl, dt);
            if (HEAT) u_re = ssprk33_stage_value<FT>(stage, y_re, u_re, dre, dt);
            __syncthreads(); // neighbours have read this stage's LDS values
        }
        y_vl = u_vl;
        y_re = u_re;
    }
    __syncthreads(); // the tiles overlay other columns' exchange arrays
    if (i < n) {
        if (WATER) tiles[slot * n + i] = y_vl;
        if (HEAT) tiles[tile_n + slot * n + i] = y_re;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < tile_n; e += blockDim.x) {
        const int lev = e / cpb, cs = e - lev * cpb;
        if (col_first + cs < P.ncols) {
            const int64_t g = int64_t(lev) * P.stride + col_first + cs;
            if (WATER) Y.v[0][g] = tiles[cs * n + lev];
            if (HEAT) Y.v[2][g] = tiles[tile_n + cs * n + lev];
        }
    }
    if (cell && nf_acc != nf_acc) atomicOr(P.status, 1u);
}

// ----------------------------------- persistent column stepper, one wave per column
//
// column_stepper_kernel's one-wave form for columns of up to 64 CW levels: lane l of the column's
// wave owns the CW ADJACENT cells CW l .. CW l + CW - 1, so the faces between them are evaluated in
// the lane, and only the lane's top cell travels through LDS (to lane l + 1) and the flux of the face
// below its bottom cell back (to lane l - 1): every interior face is evaluated ONCE, with
// rhs_kernel's expression (lower cell first), no workgroup barrier anywhere in the time loop (LDS
// operations of one wave execute in order) -- bitwise the fused stages.  CW = 1: columns of <= 64
// levels; CW = 2: the 128-level configurations, which the thread-per-cell form runs with two waves
// per column, two workgroup barriers per stage and every interior face evaluated twice.
// waves per SIMD the compiler is asked to leave room for (wave_stepper_columns picks the workgroup size
// from the register count it ends up with): the Float64 Richards instantiations sit within a register
// or two of the 80-register step (6 waves), so they are held to it
// A value every lane of the wave holds identically (the per-column constants of the one column a wave of
// the wave stepper owns), moved to the scalar register file word by word: the vector registers it
// occupied are free again, and it is used as a uniform operand from then on.
template <typename T>
__device__ __forceinline__ T wave_uniform(const T& x) {
    static_assert(sizeof(T) % 4 == 0, "32-bit words");
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &x, sizeof(T));
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / 4; ++k) w[k] = __builtin_amdgcn_readfirstlane(w[k]);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
}

template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int CW, bool NOICE>
constexpr int cs_wave_min_waves() {
    if (!M::uses_tables || MODEL != MODEL_RICHARDS) return 4; // (1024 threads = 4 waves per SIMD)
    // (per-column parameters are scalar registers here, wave_uniform: the same budgets hold)
    if (CW == 1) return 6; // (the ice-free kernel needs 61 of its own accord; held to 64 it runs 4 % slower)
    return (NOICE && !FACTORS) ? 6 : 4;
}
// BOUND: the call also leaves the stable-step bound of the state it ENDS on in P.dt_out (which the launcher
// has set to +inf), by rhs_kernel MODE 4's rule and with its expressions: one more closure pass over the
// final state, the wave's integer maxima of the face terms, one division and one atomicMin per column.
// dt_device then carries the step and dt_value the Courant factor (as in MODE 4).  The maxima are exact and
// x -> fl(c / x) is monotone, so the word ends up with the bits a MODE 4 launch on the same state leaves.
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M, int CW, bool NOICE = false, bool VGF = true, bool BOUND = false>
__global__ void __launch_bounds__(1024, (cs_wave_min_waves<FT, MODEL, FACTORS, PERCOL, M, CW, NOICE>()))
column_stepper_wave_kernel(const DevParams<FT> P0, const Planes<FT> Y, const Planes<FT> AUX, const FT dt_value,
                           const FT* __restrict__ dt_device, const int64_t nsteps, const FT* __restrict__ bcv) {
    // (the body is shared with series_column_stepper_wave_kernel, lh_series_stepper.hpp; the two differ in these)
#define LH_CSW_FACE_VALUES_FIXED(face) !bcv
#define LH_CSW_STAGE_BOUNDARY_VALUES \
    if (bcv) set_stage_boundary_values(P, bcv + (s * 3 + stage) * 4)
#include "lh_column_stepper_wave_body.inc"
#undef LH_CSW_FACE_VALUES_FIXED
#undef LH_CSW_STAGE_BOUNDARY_VALUES
}

// --------------------------------------------------------- diagnostics
// K, psi, kappa, T of every cell (the pointwise stage only).
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M>
__global__ void __launch_bounds__(256)
diag_kernel(const DevParams<FT> P, const Planes<FT> IN, const Planes<FT> AUX, const Planes<FT> OUT) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    const FT* p_vl = (MODEL == MODEL_HEAT ? AUX.v[0] : IN.v[0]) + col;
    const FT* p_ti = (MODEL == MODEL_HEAT ? AUX.v[1] : IN.v[1]) + col;
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && FACTORS && P.viscosity_kind;
    ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    if (WATER) finish_colc<FT, M>(mm, c);
    const bool vgf = M::uses_tables && P.vg_fast_all != 0; // (kernel-argument constant: a scalar branch)
    for (int i = 0; i < P.nlev; ++i) {
        const int64_t o = int64_t(i) * P.stride;
        FT vl = p_vl[o], ti = p_ti[o];
        FT T = need_Taux ? AUX.v[3][o + col] : FT(288), kap = FT(0), K = FT(0), psi = FT(0);
        if (HEAT) {
            FT rcs;
            T = temperature_closure<FT, M>(mm, P, c, vl, ti, IN.v[2][o + col], rcs);
            kap = kappa_closure<FT, M>(mm, P, c, vl, ti);
        }
        if (WATER) water_closures<FT, M, FACTORS>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
        OUT.v[0][o + col] = K;
        OUT.v[1][o + col] = psi;
        OUT.v[2][o + col] = kap;
        OUT.v[3][o + col] = T;
    }
}

// ------------------------------------------------------ boundary fluxes
// boundary_fluxes(X, bc, face, model, cs, t) (boundary_conditions.jl:470-489; the prescribed
// atmosphere :516-533 arrives as per-column flux values) for ONE face of every column: the pair
// (f_rhoe_int, f_vartheta_l) the tendency launch puts into its SetValue divergence, from the same
// device functions, the same closure instantiation (FACTORS, math policy, K without Ksat times Ksat)
// and therefore the same bits.  A component without a boundary condition (NoBC) gives NaN.
template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename M>
__global__ void __launch_bounds__(256)
boundary_flux_kernel(const DevParams<FT> P, const Planes<FT> IN, const Planes<FT> AUX, const int face, FT* out_e, FT* out_w) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col >= P.ncols) return;
    // interior_values (:174-190): the cell next to the face
    const int64_t o = int64_t(face == FACE_BOTTOM ? 0 : P.nlev - 1) * P.stride + col;
    ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
    if (WATER) finish_colc<FT, M>(mm, c);
    const bool vgf = M::uses_tables && P.vg_fast_all != 0;
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && FACTORS && P.viscosity_kind;
    const FT vl = (MODEL == MODEL_HEAT ? AUX.v[0] : IN.v[0])[o];
    const FT ti = (MODEL == MODEL_HEAT ? AUX.v[1] : IN.v[1])[o];
    FT T = need_Taux ? AUX.v[3][o] : FT(288), K = FT(0), psi = FT(0), rcs = FT(1);
    if (HEAT) T = temperature_closure<FT, M>(mm, P, c, vl, ti, IN.v[2][o], rcs);
    constexpr bool RELK = M::is_production;
    if (WATER) {
        water_closures<FT, M, FACTORS, true, false, false, RELK>(mm, P, c, vl, ti, T, K, psi, nullptr, vgf);
        if (RELK) K = K * c.Ksat; // (as rhs_kernel hands the boundary cell's conductivity over)
    }
    FT fe, fw;
    boundary_fluxes<FT, M, MODEL, FACTORS, false>(mm, P, c, face, col, vl, ti, T, K, psi, fe, fw, nullptr, nullptr, vgf);
    if (P.bc_kind[face][COMP_ENERGY] == BC_NONE) fe = FT(NAN);
    if (P.bc_kind[face][COMP_HYDROLOGY] == BC_NONE) fw = FT(NAN);
    out_e[col] = fe;
    out_w[col] = fw;
}

// ---------------------------------------------------------- stable dt
// min over cells of courant*dz^2/max(K dpsi/dvl, kappa/rho_c_s) (build-defined;
// the reference steps with a fixed user dt, simulation.jl:34-70).  Positive IEEE
// values order like their bit patterns, so the global min is an integer atomicMin.

template <typename FT, int MODEL, bool PERCOL, typename M>
__global__ void __launch_bounds__(256)
stable_dt_kernel(const DevParams<FT> P, const Planes<FT> IN, const Planes<FT> AUX, const FT courant,
                 typename Bits<FT>::type* out_bits) {
    constexpr bool WATER = (MODEL != MODEL_HEAT);
    constexpr bool HEAT = (MODEL != MODEL_RICHARDS);
    using U = typename Bits<FT>::type;
    __shared__ double s_tab[M::uses_tables ? MATH_TAB_DOUBLES : 1];
    const M mm(stage_math_tables<M>(P.math_tab, s_tab));
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    FT best = FT(INFINITY);
    if (col < P.ncols) {
        const FT* p_vl = (MODEL == MODEL_HEAT ? AUX.v[0] : IN.v[0]) + col;
        const FT* p_ti = (MODEL == MODEL_HEAT ? AUX.v[1] : IN.v[1]) + col;
        ColC<FT> c = make_colc<FT, M>(P, col, PERCOL);
        if (WATER) finish_colc<FT, M>(mm, c);
        const FT cdz2 = courant * P.dz * P.dz;
        const int n = P.nlev;
        FT K_p = FT(0), dpsi_p = FT(0), kap_p = FT(0), rcs_p = FT(1);
        for (int i = 0; i < n; ++i) {
            const int64_t o = int64_t(i) * P.stride;
            FT vl = p_vl[o], ti = p_ti[o];
            FT K = FT(0), dpsi = FT(0), kap = FT(0), rcs = FT(1);
            FT Tc = FT(288);
            if (MODEL == MODEL_RICHARDS && P.viscosity_kind) Tc = AUX.v[3][o + col];
            if (HEAT) Tc = temperature_closure<FT, M>(mm, P, c, vl, ti, IN.v[2][o + col], rcs);
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
            if (HEAT) kap = kappa_closure<FT, M>(mm, P, c, vl, ti);
            FT D = FT(0);
            if (i == 0 || i == n - 1) { // boundary cells: their own coefficients
                D = K * dpsi;
                if (HEAT && kap / rcs > D) D = kap / rcs;
                // Dirichlet faces sit half a cell away and use the face state's coefficients
                for (int face = 0; face < 2; ++face) {
                    if ((face == FACE_BOTTOM) != (i == 0) && n > 1) continue;
                    const int kh = P.bc_kind[face][COMP_HYDROLOGY], ke = P.bc_kind[face][COMP_ENERGY];
                    FT vh = P.bc_value[face][COMP_HYDROLOGY];
                    if (P.bc_pc[face][COMP_HYDROLOGY]) vh = P.bc_pc[face][COMP_HYDROLOGY][col];
                    const FT vl_f = (WATER && kh == BC_DIRICHLET) ? vh : vl;
                    FT ve = P.bc_value[face][COMP_ENERGY];
                    if (P.bc_pc[face][COMP_ENERGY]) ve = P.bc_pc[face][COMP_ENERGY][col];
                    const FT T_f = (HEAT && ke == BC_DIRICHLET) ? ve : Tc; // as boundary_fluxes
                    if (WATER && kh == BC_DIRICHLET) {
                        FT K_f, psi_f;
                        water_closures<FT, M, true, false>(mm, P, c, vl_f, ti, T_f, K_f, psi_f);
                        FT Db = FT(2) * (K_f > K ? K_f : K) * dpsi;
                        if (Db > D) D = Db;
                    }
                    if (HEAT && ke == BC_DIRICHLET) {
                        FT kf = kappa_closure<FT, M>(mm, P, c, vl_f, ti);
                        FT Db = FT(2) * (kf > kap ? kf : kap) / rcs;
                        if (Db > D) D = Db;
                    }
                }
            }
            if (i > 0) { // interior face: arithmetic-mean coefficients as in the stencil
                FT Dw = (K_p + K) * FT(0.5) * (dpsi_p > dpsi ? dpsi_p : dpsi);
                FT DT = HEAT ? (kap_p + kap) * FT(0.5) / (rcs_p < rcs ? rcs_p : rcs) : FT(0);
                if (Dw > D) D = Dw;
                if (DT > D) D = DT;
            }
            if (D > FT(0)) {
                FT dtc = cdz2 / D;
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
        FT other = __shfl_down(best, off, 64);
        if (other < best) best = other;
    }
    if ((threadIdx.x & 63) == 0 && best < FT(INFINITY)) {
        U b;
        __builtin_memcpy(&b, &best, sizeof(FT));
        if (b < __atomic_load_n(out_bits, __ATOMIC_RELAXED)) atomicMin(out_bits, b); // (as rhs_kernel MODE 4: a read first)
    }
}

// ------------------------------------------------ layout conversion kernels
// host/user layout a[col*cs + lev*ls]  <->  plane [lev][stride] (column-fastest)
template <typename FT, bool TO_PLANE>
__global__ void __launch_bounds__(256)
strided_copy_kernel(FT* plane, int64_t stride, FT* user, int64_t ls, int64_t cs, int64_t ncols,
                    int nlev) {
    // 64x64 tile through LDS so both sides stay coalesced for the level-fastest
    // case (ls == 1); correct for any strides.
    __shared__ FT tile[64][65];
    const int64_t c0 = int64_t(blockIdx.x) * 64;
    const int l0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6; // 64 x 4
    if (TO_PLANE) {
        for (int r = ty; r < 64; r += 4) { // r = column within tile, tx = level
            int64_t c = c0 + r;
            int l = l0 + tx;
            if (c < ncols && l < nlev) tile[r][tx] = user[c * cs + int64_t(l) * ls];
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) { // r = level within tile, tx = column
            int64_t c = c0 + tx;
            int l = l0 + r;
            if (c < ncols && l < nlev) plane[int64_t(l) * stride + c] = tile[tx][r];
        }
    } else {
        for (int r = ty; r < 64; r += 4) {
            int64_t c = c0 + tx;
            int l = l0 + r;
            if (c < ncols && l < nlev) tile[tx][r] = plane[int64_t(l) * stride + c];
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) {
            int64_t c = c0 + r;
            int l = l0 + tx;
            if (c < ncols && l < nlev) user[c * cs + int64_t(l) * ls] = tile[r][tx];
        }
    }
}

// ------------------------------------------------------- streaming probe
// The access pattern of rhs_kernel with the arithmetic taken out: one lane per CPL columns
// marches bottom -> top, reads one row of each of NR planes per level (PF levels in flight),
// and stores their sum into each of NW planes -- same buffer-descriptor row access, same
// nontemporal policy, same workgroup -> column-block map.  Its rate is the ceiling the column
// launch can reach on THIS set of planes (lh_stream_probe).
template <typename FT, int CPL, int PF, bool NT>
__global__ void __launch_bounds__(256, 8)
stream_probe_kernel(const int64_t ncols, const int64_t stride, const int nlev, const int xcd_remap,
                    const Planes<FT> IN, const int nr, const Planes<FT> OUT, const int nw) {
    static_assert(sizeof(FT) * CPL == 8, "one 8-byte access per lane");
    const unsigned blk = xcd_block(xcd_remap);
    const int64_t col0 = (int64_t(blk) * blockDim.x + threadIdx.x) * CPL;
    if (col0 >= ncols) return;
    const unsigned lane_byte = (unsigned)col0 * (unsigned)sizeof(FT);
    const unsigned row_bytes = (unsigned)(stride * (int64_t)sizeof(FT));
    const FT* r[4];
    FT* w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = IN.v[k];
        w[k] = OUT.v[k];
    }
    FT ring[PF][4][CPL];
#pragma unroll
    for (int q = 0; q < PF; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < CPL; ++j) ring[q][k][j] = FT(0);
    auto fetch = [&](int slot) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nr) {
                bload<FT, CPL, NT>(r[k], row_bytes, lane_byte, ring[slot][k]);
                r[k] += stride;
            }
    };
#pragma unroll
    for (int q = 0; q < PF; ++q)
        if (q < nlev) fetch(q);
    for (int i0 = 0; i0 < nlev; i0 += PF) {
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const int i = i0 + q;
            if (PF > 1 && i >= nlev) break;
            FT x[CPL];
#pragma unroll
            for (int j = 0; j < CPL; ++j) x[j] = (ring[q][0][j] + ring[q][1][j]) + (ring[q][2][j] + ring[q][3][j]);
            if (i + PF < nlev) fetch(q);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nw) {
                    bstore<FT, CPL, NT>(w[k], row_bytes, lane_byte, x);
                    w[k] += stride;
                }
        }
    }
}

template <typename FT>
__global__ void __launch_bounds__(256) fill_kernel(FT* p, int64_t n, FT v) {
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (; i < n; i += step) p[i] = v;
}

template <typename FT>
__global__ void __launch_bounds__(256) broadcast_profile_kernel(FT* plane, const FT* __restrict__ prof, int64_t ncols, int64_t stride) {
    const int64_t col = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (col < ncols) plane[int64_t(blockIdx.y) * stride + col] = prof[blockIdx.y];
}

template <typename FT>
__global__ void __launch_bounds__(256) convert_kernel(FT* dst, const double* src, int64_t n) {
    int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = FT(src[i]);
}

// one thread: dt = min(dt, dt_max) (dt_max <= 0: no cap), elapsed += dt.  A bound that is not a
// positive finite number (no positive diffusivity anywhere and no cap: +inf; a NaN) would turn the
// state into NaNs: the step is then taken with dt = 0 (the state stays) and bit 2 of the status is set.
template <typename FT>
__device__ __forceinline__ FT dt_from_bound(FT d, FT dt_max, uint32_t* status) {
    if (dt_max > FT(0) && !(d <= dt_max)) d = dt_max;
    if (!(d > FT(0)) || d - d != FT(0)) {
        d = FT(0);
        atomicOr(status, 4u);
    }
    return d;
}
template <typename FT>
__global__ void dt_prepare_kernel(FT* dt, FT dt_max, FT* elapsed, uint32_t* status) {
    const FT d = dt_from_bound(*dt, dt_max, status);
    *dt = d;
    if (elapsed) *elapsed += d;
}
// lh_step_ssprk33_adaptive_hold, one thread between two chunks of `hold` steps.  *bound: the
// (rank-reduced) stable-step bound of the current state.  check: a chunk has just ended on that state
// with the step still in *dt -- a bound below that step, or one that is not a positive finite number,
// sets bit 5 of the status (the held step exceeded the stable step of the state it produced).
// hold > 0: *dt = the next chunk's step (dt_prepare_kernel's rule), elapsed += dt, `hold` times.
template <typename FT>
__global__ void dt_hold_prepare_kernel(FT* dt, const FT* bound, FT dt_max, FT* elapsed, int hold, int check, uint32_t* status) {
    const FT b = *bound;
    if (check && (!(b > FT(0)) || b - b != FT(0) || b < *dt)) atomicOr(status, 32u);
    if (hold <= 0) return;
    const FT d = dt_from_bound(b, dt_max, status);
    *dt = d;
    if (elapsed) {
        FT e = *elapsed;
        for (int k = 0; k < hold; ++k) e += d;
        *elapsed = e;
    }
}

template <typename FT>
__global__ void init_bits_kernel(typename Bits<FT>::type* p) {
    FT inf = FT(INFINITY);
    __builtin_memcpy(p, &inf, sizeof(FT));
}

// ------------------------------------------------------------- launchers
// Every launcher normalises its run-time flags, turns them into constants with with_bool / with_int
// (lh_dispatch.hpp) and instantiates exactly the combinations the *_exists predicates beside the
// kernels allow.

static inline dim3 grid_for(int64_t work, int block) {
    return dim3((unsigned)((work + block - 1) / block));
}

using model_list = int_list<MODEL_RICHARDS, MODEL_HEAT, MODEL_COUPLED>; // (with_int: any other value is the coupled model)

template <typename FT, int MODEL, bool FACTORS, bool PERCOL, typename CFG, typename M, bool NOICE, bool VGF>
static void launch_rhs_mode(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                            const Planes<FT>& base, const Planes<FT>& out, FT dt, const FT* dt_dev,
                            int mode, int block_req, hipStream_t s) {
    // (mode 4 last: the list's default)
    with_int(int_list<0, 1, 2, 3, 5, 4>{}, M::is_production ? mode : 0, [&](auto md) {
        constexpr int MODE = decltype(md)::value;
        if constexpr (rhs_mode_exists<M, MODE>()) {
            constexpr auto kernel = rhs_kernel<FT, MODEL, FACTORS, PERCOL, CFG, M, MODE, NOICE, VGF>;
            // workgroup size: the kernel's own (see rhs_max_threads) unless LH_TUNE block= asks for less
            constexpr int kmax = rhs_max_threads<M, rhs_waves_per_simd<FT, MODEL, FACTORS, PERCOL, M, CFG::PF, MODE, NOICE>()>();
            const int block = (block_req > 0 && block_req <= kmax) ? block_req : kmax;
            const int64_t lanes = (P.ncols + CFG::CPL - 1) / CFG::CPL;
            dim3 g = grid_for(lanes, block), b(block);
            if (CFG::SEG) g.y = (unsigned)((P.nlev + P.seg_len - 1) / P.seg_len);
            // dynamic LDS: one word per thread for the mode-4 reduction
            // (+ two level arrays for level-uniform prescribed fields of Ya where the kernel can take them)
            constexpr bool MAY_PROF = (MODEL == MODEL_HEAT) || (MODEL == MODEL_RICHARDS && FACTORS);
            const unsigned dyn = (unsigned)((MODE == 4 ? (((size_t)block * sizeof(float) + 15) & ~(size_t)15) : 0) +
                                            (MAY_PROF ? 2 * (size_t)P.nlev * sizeof(FT) : 0));
            if (MODE == 4) // tendency + stable-step bound; the minimum starts at +inf
                hipLaunchKernelGGL((init_bits_kernel<FT>), dim3(1), dim3(1), 0, s, reinterpret_cast<typename Bits<FT>::type*>(P.dt_out));
            hipLaunchKernelGGL(kernel, g, b, dyn, s, P, in, aux, base, out, dt, dt_dev);
        }
    });
}

template <typename FT, int MODEL, typename M>
static void launch_rhs_model(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                             const Planes<FT>& base, const Planes<FT>& out, FT dt, const FT* dt_dev,
                             int mode, bool factors, bool percol, bool noice, const Tune& tune, hipStream_t s) {
    using CFG = typename DefaultCfg<FT>::type;
    const int block = tune.block; // 0: the kernel's own workgroup size
    const bool ni = noice && noice_exists<M>(factors);
    // Nontemporal access when the launch streams more than the 256 MiB Infinity
    // Cache can hold (measured +4 % on 1e6 x 64 columns); plain access for small
    // ensembles whose planes stay cache-resident between launches.
    const int nplanes = (MODEL == MODEL_COUPLED) ? 6 : (MODEL == MODEL_RICHARDS ? 4 : 4);
    const double touched = double(P.nlev) * double(P.stride) * sizeof(FT) * nplanes;
    const bool nt = tune.nt >= 0 ? tune.nt != 0 : touched > 192.0 * 1024 * 1024;
    // level-segmented (small ensembles: cache-resident)
    const bool seg = M::is_production && P.seg_len > 0 && P.seg_len < P.nlev;
    // clay-like ensembles (some column with m < LH_VG_FAST_MIN_M): the log-domain closures, one launch
    // shape (plain access, unsegmented) -- the Float64 water kernels only
    const bool robust = robust_vg_exists<M, MODEL>() && P.vg_fast_all == 0;
    enum { PLAIN, NONTEMPORAL, SEGMENTED };
    const int shape = robust ? PLAIN : seg ? SEGMENTED : nt ? NONTEMPORAL : PLAIN;
    with_bool(factors, [&](auto f) { with_bool(percol, [&](auto pc) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        with_int(int_list<NONTEMPORAL, SEGMENTED, PLAIN>{}, shape, [&](auto sh) {
            constexpr bool F = decltype(f)::value, PC = decltype(pc)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            constexpr int SH = decltype(sh)::value;
            using C = KCfg<CFG::CPL, CFG::PF, SH == NONTEMPORAL, SH == SEGMENTED>;
            // (the rules of the normalisation above once more: ni, robust and shape never take the other
            // values at run time, the guard only keeps those combinations un-instantiated)
            if constexpr ((!NI || noice_exists<M>(F)) && (VG || (robust_vg_exists<M, MODEL>() && robust_shape_exists<C>())))
                launch_rhs_mode<FT, MODEL, F, PC, C, M, NI, VG>(P, in, aux, base, out, dt, dt_dev, mode, block, s);
        });
    }); }); }); });
}

// All rhs_kernel variants of one model.  Each (FT, MODEL) pair is instantiated in its own
// translation unit (lh_kernels_<ft>_<model>.hip) so the build runs eight compilers side by side.
template <typename FT, int MODEL>
void launch_rhs_for_model(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                          const Planes<FT>& base, const Planes<FT>& out, FT dt, const FT* dt_dev,
                          int mode, bool factors, bool percol, bool noice, int math, const Tune& tune,
                          hipStream_t s) {
    // MathLibm is a parity-debugging policy for the tendency itself (mode 0);
    // the fused SSPRK33 stages and mode 4 always run the production math.
    with_math<FT>(math == MATH_LIBM && mode == 0, [&](auto m) {
        launch_rhs_model<FT, MODEL, typename decltype(m)::type>(P, in, aux, base, out, dt, dt_dev, mode, factors, percol, noice, tune, s);
    });
}

// Columns (= waves) per workgroup of column_stepper_wave_kernel.  Whole multiples of 4, so the four
// SIMDs of a CU carry the same number of waves (measured on 1e6 x 64 Float64 columns, ms per step:
// 8 columns 0.60, 9..11 0.72..0.85, 12 0.56, 13 0.85, 14 0.79, 16 0.71), and among 4 / 8 / 12 the
// count that keeps most waves resident under the instantiation's register count and the LDS of a
// CU (48 KiB of math tables per Float64 workgroup + the exchange arrays of its columns): 12 for
// Float64 Richards without ice (63 / 77 VGPRs, 6 waves per SIMD), 8 for the per-column-parameter
// and ice kernels (94+ VGPRs: a second 768-thread workgroup would not fit), 4 for Float32 (8 for
// short calls).  Small ensembles take 4 to spread over the CUs.
template <auto Kernel>
unsigned wave_stepper_columns(int64_t ncols, size_t dyn_col, int64_t nsteps) {
    static const hipFuncAttributes attr = [] {
        hipFuncAttributes a{};
        if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(Kernel)) != hipSuccess) a.numRegs = 0;
        return a;
    }();
    if (ncols < 4096 || attr.numRegs <= 0) return 4u;
    const unsigned regs = (unsigned(attr.numRegs) + 7u) & ~7u;
    const unsigned waves_cu = 4u * (512u / regs < 8u ? 512u / regs : 8u);
    unsigned best = 4u, best_resident = 0u;
    for (unsigned c = 4u; c <= 12u; c += 4u) {
        const size_t lds = attr.sharedSizeBytes + c * dyn_col;
        const unsigned by_lds = unsigned((size_t(160) << 10) / (lds ? lds : 1));
        const unsigned by_regs = waves_cu / c;
        const unsigned resident = c * (by_lds < by_regs ? by_lds : by_regs);
        // equal residency (Float32: no tables): 4 columns step fastest, 8 halve the row pieces of the
        // tile I/O -- T(n) = 1.26 + 0.422 n against 0.89 + 0.439 n ms on C3 (tools/stepper_call_cost.py):
        // the wider workgroup wins calls of up to 20 steps
        if (resident > best_resident || (resident == best_resident && c == 8u && nsteps <= 20)) best = c, best_resident = resident;
    }
    return best;
}

template <typename FT, int MODEL>
void launch_column_stepper_for_model(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux,
                                     FT dt, const FT* dt_dev, int64_t nsteps, const FT* bcv, bool factors,
                                     bool percol, bool noice, bool bound, hipStream_t s) {
    // One wave per column with 1 or 2 adjacent cells per lane (column_stepper_wave_kernel) for columns
    // of up to 128 levels; one thread per cell with workgroup barriers beyond that.
    const int cw = (P.nlev + 63) / 64;
    const bool wave = cw <= 2;
    const unsigned tpc = wave ? 64u : (unsigned)((P.nlev + 63) / 64 * 64);
    // columns per workgroup of the thread-per-cell kernel: 256 threads, 512 for large Float64
    // ensembles (the Float64 math tables take 48 KiB of LDS per workgroup whatever its size);
    // the wave kernel picks its own from the instantiation's registers (wave_stepper_columns)
    unsigned cpb = 256u / tpc ? 256u / tpc : 1u;
    if (sizeof(FT) == 8 && P.ncols >= 4096) cpb = 512u / tpc ? 512u / tpc : 1u;
    const bool need_Taux = (MODEL == MODEL_RICHARDS) && factors && P.viscosity_kind;
    const int tiles = cs_fetch_tiles(MODEL, noice && !factors, need_Taux);
    // dynamic LDS: the plane tiles of the initial fetch and the exchange arrays share it
    const int narr = cs_exchange_arrays<MODEL>() + (wave ? cs_flux_arrays<MODEL>() : 0);
    const size_t ex_words = wave ? (size_t)narr * 64 + CS_FACE_WORDS : (size_t)narr * (size_t)P.nlev;
    const size_t tile_words = (size_t)tiles * (size_t)P.nlev;
    const size_t dyn_col = (ex_words > tile_words ? ex_words : tile_words) * sizeof(FT);
    using M = MathFast<FT>;
    const bool ni = noice && noice_exists<M>(factors);
    const bool robust = robust_vg_exists<M, MODEL>() && P.vg_fast_all == 0; // (as launch_rhs_model)
    with_bool(factors, [&](auto f) { with_bool(percol, [&](auto pc) { with_bool(ni, [&](auto i) { with_bool(!robust, [&](auto vg) {
        // cells per lane of the wave kernel; 0: the thread-per-cell kernel
        // (bound: the wave kernel only -- the caller asks for it for columns of up to 128 levels, with the
        // step in device memory, the Courant factor in `dt` and P.dt_out addressing the word for the bound)
        with_int(int_list<1, 2, 0>{}, wave ? cw : 0, [&](auto w) { with_bool(bound && wave, [&](auto bd) {
            constexpr bool F = decltype(f)::value, PC = decltype(pc)::value, NI = decltype(i)::value, VG = decltype(vg)::value;
            constexpr int CW = decltype(w)::value;
            constexpr bool B = decltype(bd)::value;
            // (ni and robust are normalised with the same rules: the guard only keeps what cannot occur un-instantiated)
            if constexpr ((!NI || noice_exists<M>(F)) && (VG || robust_vg_exists<M, MODEL>()) && (!B || CW > 0)) {
                constexpr auto kernel = [] {
                    if constexpr (CW > 0) return column_stepper_wave_kernel<FT, MODEL, F, PC, M, CW, NI, VG, B>;
                    else return column_stepper_kernel<FT, MODEL, F, PC, M, NI, VG>;
                }();
                if constexpr (CW > 0) cpb = wave_stepper_columns<kernel>(P.ncols, dyn_col, nsteps);
                if (P.cs_cpb > 0 && (unsigned)P.cs_cpb * tpc <= 1024u) cpb = (unsigned)P.cs_cpb;
                const dim3 g((unsigned)((P.ncols + cpb - 1) / cpb)), b(tpc * cpb);
                const unsigned dyn = (unsigned)(cpb * dyn_col);
                if (B) // the minimum starts at +inf (as launch_rhs_mode does for MODE 4)
                    hipLaunchKernelGGL((init_bits_kernel<FT>), dim3(1), dim3(1), 0, s, reinterpret_cast<typename Bits<FT>::type*>(P.dt_out));
                hipLaunchKernelGGL(kernel, g, b, dyn, s, P, Y, aux, dt, dt_dev, nsteps, bcv);
            }
        }); });
    }); }); }); });
}

#define LH_CS_MODEL_ARGS(FT) \
    const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&, FT, const FT*, int64_t, const FT*, bool, bool, bool, bool, hipStream_t
#define LH_RHS_MODEL_ARGS(FT)                                                                        \
    const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&, const Planes<FT>&, const Planes<FT>&, \
        FT, const FT*, int, bool, bool, bool, int, const Tune&, hipStream_t
#ifndef LH_TU_MODEL // the common translation unit only dispatches
extern template void launch_rhs_for_model<double, MODEL_RICHARDS>(LH_RHS_MODEL_ARGS(double));
extern template void launch_rhs_for_model<double, MODEL_HEAT>(LH_RHS_MODEL_ARGS(double));
extern template void launch_rhs_for_model<double, MODEL_COUPLED>(LH_RHS_MODEL_ARGS(double));
extern template void launch_rhs_for_model<float, MODEL_RICHARDS>(LH_RHS_MODEL_ARGS(float));
extern template void launch_rhs_for_model<float, MODEL_HEAT>(LH_RHS_MODEL_ARGS(float));
extern template void launch_rhs_for_model<float, MODEL_COUPLED>(LH_RHS_MODEL_ARGS(float));
extern template void launch_column_stepper_for_model<double, MODEL_RICHARDS>(LH_CS_MODEL_ARGS(double));
extern template void launch_column_stepper_for_model<double, MODEL_HEAT>(LH_CS_MODEL_ARGS(double));
extern template void launch_column_stepper_for_model<double, MODEL_COUPLED>(LH_CS_MODEL_ARGS(double));
extern template void launch_column_stepper_for_model<float, MODEL_RICHARDS>(LH_CS_MODEL_ARGS(float));
extern template void launch_column_stepper_for_model<float, MODEL_HEAT>(LH_CS_MODEL_ARGS(float));
extern template void launch_column_stepper_for_model<float, MODEL_COUPLED>(LH_CS_MODEL_ARGS(float));
#endif
#define LH_INSTANTIATE_MODEL(FT, MODEL)                                    \
    template void launch_rhs_for_model<FT, MODEL>(LH_RHS_MODEL_ARGS(FT)); \
    template void launch_column_stepper_for_model<FT, MODEL>(LH_CS_MODEL_ARGS(FT));

template <typename FT>
void launch_rhs(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                const Planes<FT>& base, const Planes<FT>& out, FT dt, const FT* dt_dev, int mode,
                bool factors, bool percol, bool noice, int math, const Tune& tune, hipStream_t s) {
    with_int(model_list{}, P.model, [&](auto m) {
        launch_rhs_for_model<FT, decltype(m)::value>(P, in, aux, base, out, dt, dt_dev, mode, factors, percol, noice, math, tune, s);
    });
}

template <typename FT>
void launch_column_stepper(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux, FT dt,
                           const FT* dt_dev, int64_t nsteps, const FT* bcv, bool factors, bool percol,
                           bool noice, bool bound, hipStream_t s) {
    with_int(model_list{}, P.model, [&](auto m) {
        launch_column_stepper_for_model<FT, decltype(m)::value>(P, Y, aux, dt, dt_dev, nsteps, bcv, factors, percol, noice, bound, s);
    });
}

template <typename FT>
void launch_diag(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                 const Planes<FT>& out, bool percol, int math, hipStream_t s) {
    dim3 g = grid_for(P.ncols, 256), b(256);
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_int(model_list{}, P.model, [&](auto md) { with_bool(percol, [&](auto pc) {
        hipLaunchKernelGGL((diag_kernel<FT, decltype(md)::value, true, decltype(pc)::value, typename decltype(m)::type>), g, b, 0, s, P, in, aux, out);
    }); }); });
}

template <typename FT>
void launch_boundary_fluxes(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux, int face, FT* out_e,
                            FT* out_w, bool factors, bool percol, int math, hipStream_t s) {
    dim3 g = grid_for(P.ncols, 256), b(256);
    with_math<FT>(math == MATH_LIBM, [&](auto m) { with_int(model_list{}, P.model, [&](auto md) {
        with_bool(factors, [&](auto f) { with_bool(percol, [&](auto pc) {
            hipLaunchKernelGGL((boundary_flux_kernel<FT, decltype(md)::value, decltype(f)::value, decltype(pc)::value, typename decltype(m)::type>),
                               g, b, 0, s, P, in, aux, face, out_e, out_w);
        }); });
    }); });
}

template <typename FT>
void launch_stable_dt(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                      FT courant, void* out_ft, bool percol, hipStream_t s) {
    using U = typename Bits<FT>::type;
    U* out = reinterpret_cast<U*>(out_ft);
    hipLaunchKernelGGL((init_bits_kernel<FT>), dim3(1), dim3(1), 0, s, out);
    dim3 g = grid_for(P.ncols, 256), b(256);
    with_int(model_list{}, P.model, [&](auto md) { with_bool(percol, [&](auto pc) {
        hipLaunchKernelGGL((stable_dt_kernel<FT, decltype(md)::value, decltype(pc)::value, MathFast<FT>>), g, b, 0, s, P, in, aux, courant, out);
    }); });
}

template <typename FT>
void launch_strided_copy(FT* plane, int64_t stride, FT* user, int64_t ls, int64_t cs,
                         int64_t ncols, int nlev, bool to_plane, hipStream_t s) {
    dim3 g((unsigned)((ncols + 63) / 64), (unsigned)((nlev + 63) / 64)), b(256);
    with_bool(to_plane, [&](auto tp) {
        hipLaunchKernelGGL((strided_copy_kernel<FT, decltype(tp)::value>), g, b, 0, s, plane, stride, user, ls, cs, ncols, nlev);
    });
}

template <typename FT>
void launch_stream_probe(int64_t ncols, int64_t stride, int nlev, int xcd_remap, const Planes<FT>& in, int nr,
                         const Planes<FT>& out, int nw, bool nt, hipStream_t s) {
    using CFG = typename DefaultCfg<FT>::type;
    constexpr int CPL = CFG::CPL, PF = CFG::PF;
    const int64_t lanes = (ncols + CPL - 1) / CPL;
    dim3 g = grid_for(lanes, 256), b(256);
    with_bool(nt, [&](auto n) {
        hipLaunchKernelGGL((stream_probe_kernel<FT, CPL, PF, decltype(n)::value>), g, b, 0, s, ncols, stride, nlev, xcd_remap, in, nr, out, nw);
    });
}

template <typename FT>
void launch_dt_prepare(FT* dt, FT dt_max, FT* elapsed, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL((dt_prepare_kernel<FT>), dim3(1), dim3(1), 0, s, dt, dt_max, elapsed, status);
}

template <typename FT>
void launch_dt_hold_prepare(FT* dt, const FT* bound, FT dt_max, FT* elapsed, int hold, bool check, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL((dt_hold_prepare_kernel<FT>), dim3(1), dim3(1), 0, s, dt, bound, dt_max, elapsed, hold, check ? 1 : 0, status);
}

template <typename FT>
void launch_fill(FT* p, int64_t n, FT v, hipStream_t s) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((fill_kernel<FT>), dim3((unsigned)blocks), dim3(256), 0, s, p, n, v);
}

template <typename FT>
void launch_broadcast_profile(FT* plane, const FT* prof, int64_t ncols, int64_t stride, int nlev, hipStream_t s) {
    dim3 g((unsigned)((ncols + 255) / 256), (unsigned)nlev);
    hipLaunchKernelGGL((broadcast_profile_kernel<FT>), g, dim3(256), 0, s, plane, prof, ncols, stride);
}

template <typename FT>
void launch_convert(FT* dst, const double* src, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL((convert_kernel<FT>), grid_for(n, 256), dim3(256), 0, s, dst, src, n);
}

// explicit instantiation for one working type per translation unit
#define LH_INSTANTIATE(FT)                                                                            \
    template void launch_rhs<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&,          \
                                 const Planes<FT>&, const Planes<FT>&, FT, const FT*, int, bool, bool, \
                                 bool, int, const Tune&, hipStream_t);                                                      \
    template void launch_column_stepper<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&, \
                                            FT, const FT*, int64_t, const FT*, bool, bool, bool, bool, hipStream_t); \
    template void launch_diag<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&,         \
                                  const Planes<FT>&, bool, int, hipStream_t);                         \
    template void launch_stable_dt<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&,    \
                                       FT, void*, bool, hipStream_t);                                 \
    template void launch_boundary_fluxes<FT>(const DevParams<FT>&, const Planes<FT>&, const Planes<FT>&, int, FT*, FT*, \
                                             bool, bool, int, hipStream_t);                           \
    template void launch_strided_copy<FT>(FT*, int64_t, FT*, int64_t, int64_t, int64_t, int, bool,    \
                                          hipStream_t);                                               \
    template void launch_stream_probe<FT>(int64_t, int64_t, int, int, const Planes<FT>&, int,         \
                                          const Planes<FT>&, int, bool, hipStream_t);                 \
    template void launch_atmos_flux<FT>(const DevParams<FT>&, const AtmosParams<FT>&, int64_t, bool,  \
                                        bool, const FT*, const FT*, const FT*, FT*, FT*, hipStream_t); \
    template void launch_fill<FT>(FT*, int64_t, FT, hipStream_t);                                     \
    template void launch_broadcast_profile<FT>(FT*, const FT*, int64_t, int64_t, int, hipStream_t);   \
    template void launch_dt_prepare<FT>(FT*, FT, FT*, uint32_t*, hipStream_t);                                   \
    template void launch_dt_hold_prepare<FT>(FT*, const FT*, FT, FT*, int, bool, uint32_t*, hipStream_t);        \
    template void launch_convert<FT>(FT*, const double*, int64_t, hipStream_t);

} // namespace lh
