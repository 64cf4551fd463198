// lh_api.hip -- the C ABI of liblandhydro_hip.so (include/landhydro.h).
// Host logic only: parameter rounding, validation, state management, launches.
// There is no CPU fallback: without a HIP device lh_create fails loudly.
#include "../../include/landhydro.h"
#include "lh_launch.hpp"
#include "lh_layered.hpp"
#include "lh_layered_implicit.hpp"
#include "lh_factors_implicit.hpp"
#include "lh_coupled_factors_implicit.hpp"
#include "lh_layered_heat.hpp"
#include "lh_layered_heat_implicit.hpp"
#include "lh_layered_heat_trbdf2.hpp"
#include "lh_layered_coupled_implicit.hpp"
#include "lh_layered_coupled_trbdf2.hpp"
#include "lh_layered_stepper.hpp"
#include "lh_series.hpp"
#include "lh_series_heat.hpp"
#include "lh_series_layered_coupled.hpp"
#include "lh_series_stepper.hpp"
#include "lh_dense.hpp"
#include "lh_dense_heat.hpp"
#include "lh_dense_layered_coupled.hpp"
#include "lh_fastmath.hpp"
#include "lh_closures.hpp"

#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

using namespace lh;

// default address stagger between consecutively allocated planes (bytes)

namespace {

thread_local std::string g_create_error;

struct HostParams {
    lh_earth_params earth{};
    bool earth_set = false;
    lh_soil_params soil{};
    lh_vg_params vg{};
    int32_t viscosity_kind = LH_FACTOR_NONE, impedance_kind = LH_FACTOR_NONE;
    double gamma = 2.64e-2, T_ref_visc = 288.0, Omega = 7.0; // SoilWaterParameterizations.jl:49-64
    int32_t bc_kind[2][2] = {{0, 0}, {0, 0}};
    double bc_value[2][2] = {{0, 0}, {0, 0}};
    int32_t consistent_bottom_sign = 0;
    bool atmos_on = false;
    lh_atmos_forcing atmos{};
};

} // namespace

struct lh_state {
    lh_ctx* ctx;
    uint32_t mask;
    // Planes the library KNOWS to be all (+)zeros: set by creation (memset), a zero fill and by
    // launches that store zeros; cleared by anything else that may write (upload, fill, copy of
    // a non-zero plane, a launch writing the plane, handing out the device pointer).  A launch
    // neither reads a theta_i plane known to be zero (rhs_kernel NOICE) nor re-stores the
    // identically zero d theta_i into a plane that already holds zeros (no kernel stores it).
    uint32_t zero_mask;
    // Planes whose device pointer was handed out (lh_state_device_ptr) and not released
    // (lh_state_release_ptr): the caller may write through the pointer at any time, so the library
    // assumes NOTHING about their contents -- the zero bit is never set for them (a zero fill, a copy
    // of a zero plane or the d theta_i = 0 clear of lh_rhs still write the zeros, every time).
    uint32_t exposed_mask;
    // LEVEL-UNIFORM variables (lh_upload_profile): profile[var] holds FT[nlev] on the device and IS the
    // variable; stale_mask marks planes that have not received those values (the column kernels read a
    // prescribed profile of Ya from LDS and never need them; everything else materialises first)
    uint32_t profile_mask, stale_mask;
    void* profile[LH_NVARS];
    void* plane[LH_NVARS]; // what kernels address (a slot of a context arena)
};

// Planes are carved from a few large device allocations (8 plane slots each)
// instead of one hipMalloc per plane: states that are streamed together then sit
// next to each other in one contiguous range, and state creation costs no
// allocator round trip.
struct PlaneArena {
    char* base = nullptr;
    size_t slot_bytes = 0;
    int nslots = 0;
    std::vector<char> used;
};

// A boundary-value time series (lh_bc_series_create): the knot times on both sides, and per (face, component)
// a table of doubles on the device -- [nknots][stride] (per-column, column-fastest) or [nknots] (uniform)
struct lh_bc_series {
    lh_ctx* ctx = nullptr;
    std::vector<double> times;
    double* d_times = nullptr;
    double* d_val[2][2] = {};
    bool percol[2][2] = {};
};

struct lh_ctx {
    lh_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t stride = 0; // plane row length (elements), multiple of 64
    size_t esize = 8;
    HostParams hp;
    void* d_zc = nullptr;              // FT[nlev]
    void* d_pc[LH_PC_COUNT] = {};      // FT[ncols] or null
    double pc_lo[LH_PC_COUNT] = {}, pc_hi[LH_PC_COUNT] = {}; // range of each per-column array (NaN if it holds a NaN)
    void* d_bc_pc[2][2] = {};          // FT[ncols] or null
    uint32_t* d_status = nullptr;
    void* d_dt = nullptr;              // FT scratch for lh_stable_dt
    void* d_atm_pc[3] = {};            // per-column u_atm / theta_atm / q_atm (FT[ncols]) or null
    void* d_atm_flux[2] = {};          // the top-face fluxes of the prescribed atmosphere: heat, water (FT[ncols])
    double* d_math_tab = nullptr;      // log2/exp2 tables of MathFast<double>
    char* h_ring = nullptr;            // pinned staging ring of lh_upload_profile (asynchronous small uploads)
    size_t ring_bytes = 0, ring_pos = 0;
    lh_state* scratch_u1 = nullptr;    // SSPRK33 stage state
    lh_state* scratch_u2 = nullptr;    // second stage state (level-segmented launches cannot update U1 in place)
    lh_state* scratch_k1 = nullptr;    // f(Y) of lh_step_ssprk33_adaptive
    void* d_imp = nullptr;             // lh_step_implicit_euler: three FT planes [nlev][stride] (v_n, c', d')
    void* d_imp_stats = nullptr;       // ... and its statistics: int32 max iterations, uint64 unconverged, uint64 iterations
    void* d_tr = nullptr;              // lh_integrate_trbdf2: six FT planes [nlev][stride] (Y_n, f_n, Y_gamma, w, c', d')
    void* d_tr_stats = nullptr;        // ... and its LH_TRBDF2_NSTATS uint64 counters
    void* d_heat = nullptr;            // lh_step_heat_implicit, lh_step_layered_heat_implicit: eight FT planes [nlev][stride] (three of the factorisation, kc, z; kappa sums, alpha, beta)
    void* d_cpl = nullptr;             // lh_step_coupled_implicit, lh_step_layered_coupled_implicit: three FT planes [nlev][stride] (the water stage's w, c', d'; the energy solve reuses c', d')
    void* d_cpl_tr = nullptr;          // ... and four more for LH_COUPLED_TRBDF2 (the water's Y_n and f_n, the energy's f_n and w2)
    // layered soils (lh_layered.hpp): the classes as given, their ColC<FT> table on the device, and the class
    // plane [nlev][stride] bytes; a context is "layered" while it holds a map
    std::vector<lh_soil_class> soil_classes;
    void* d_cls_table = nullptr;
    uint8_t* d_cls_map = nullptr;
    int cls_map_max = 0;               // the largest class index of the map in place
    // ... and their thermal supplement (lh_layered_heat.hpp): one entry per class, or none; its ThermC<FT> table
    std::vector<lh_soil_class_thermal> soil_thermal;
    void* d_cls_therm = nullptr;
    bool cls_any_om = false;           // some class has 1 - nu_om != 1 in the working type
    void* d_series_stage = nullptr;    // lh_step_ssprk33_series on the fused stages: FT[3][2][2][stride], the sampled values of one step
    void* d_series_dt = nullptr;       // lh_integrate_series: FT[ncols] step proposals carried across sub-intervals where the caller passes none
    std::vector<lh_bc_series*> series; // the series alive (lh_bc_series_create .. lh_bc_series_destroy)
    void* d_cpl_ad = nullptr;          // lh_integrate_coupled_trbdf2, lh_integrate_layered_coupled_trbdf2: ten FT planes [nlev][stride] (d_tr's six for the water; the energy's Y_n, f_n, Y_gamma, w2)
    void* d_heat_ad = nullptr;         // lh_integrate_heat_trbdf2, lh_integrate_layered_heat_trbdf2: twelve FT planes [nlev][stride] (rho_c_s, alpha, kappa sums, k; the attempt's factorisation; Y_n, f_n, Y_gamma, w2, r')
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int math = MATH_FAST;
    Tune tune;
    unsigned plane_counter = 0;
    std::vector<PlaneArena> arenas;
    std::vector<double> zc_host;
    std::string err;
    std::vector<lh_state*> states;
    // the one collective of the path: min all-reduce of the stable-step bound
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_nranks = 1;
};

namespace {

// roctx range around one call of the path (rhs, stage, step, allreduce): what a rocprofv3
// --marker-trace of a multi-GPU run is read by; a few tens of nanoseconds without a tool attached
struct Range {
    explicit Range(const char* name) { roctxRangePushA(name); }
    ~Range() { roctxRangePop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

int fail(lh_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

// LH_OK, or the error of a HIP call: lh_last_error names the call as the source writes it
int hip_status(lh_ctx* ctx, hipError_t e, const char* call) {
    if (e == hipSuccess) return LH_OK;
    return fail(ctx, e == hipErrorOutOfMemory ? LH_ENOMEM : LH_ENODEVICE, "%s failed: %s", call, hipGetErrorString(e));
}
#define LH_HIP(ctx, call)                                      \
    do {                                                       \
        if (int rc_ = hip_status(ctx, (call), #call)) return rc_; \
    } while (0)

// f(FT(0)) for the context's working type: how every entry point picks its <double> or <float> instantiation
template <typename F>
inline auto with_ft(const lh_ctx* c, F&& f) {
    return c->cfg.dtype == LH_F64 ? f(double(0)) : f(float(0));
}

// a transient device allocation, released on every way out of its scope
struct DeviceBuffer {
    void* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() {
        if (p) (void)hipFree(p);
    }
};

// n boundary values (doubles) rounded to the working type and uploaded into `buf`
int upload_boundary_values(lh_ctx* c, const double* bcv, size_t n, DeviceBuffer& buf) {
    std::vector<char> tmp(n * c->esize);
    for (size_t k = 0; k < n; ++k) {
        if (c->cfg.dtype == LH_F64) reinterpret_cast<double*>(tmp.data())[k] = bcv[k];
        else reinterpret_cast<float*>(tmp.data())[k] = float(bcv[k]);
    }
    if (int rc = hip_status(c, hipMalloc(&buf.p, n * c->esize), "hipMalloc(&d_bcv, nv * c->esize)")) return rc;
    hipError_t e = hipMemcpyAsync(buf.p, tmp.data(), n * c->esize, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // tmp is pageable host memory
    if (e != hipSuccess) return fail(c, LH_ENODEVICE, "boundary-value upload failed: %s", hipGetErrorString(e));
    return LH_OK;
}

// The launch error of a call that may have handed `buf` to its kernel: the launch reads it, so wait
// before the buffer is released
hipError_t launch_error(lh_ctx* c, const DeviceBuffer& buf) {
    hipError_t e = hipGetLastError();
    if (buf.p) {
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = e2;
    }
    return e;
}

// In-place min all-reduce of one FT value over the attached communicator, enqueued on the
// context's stream behind whatever produced the value (no host round trip).
int allreduce_min(lh_ctx* c, void* value_device_ft) {
    if (!c->comm) return LH_OK;
    Range r_("lh:allreduce_min");
    const ncclResult_t r = ncclAllReduce(value_device_ft, value_device_ft, 1,
                                         c->cfg.dtype == LH_F64 ? ncclDouble : ncclFloat, ncclMin, c->comm, c->stream);
    if (r != ncclSuccess) return fail(c, LH_ENODEVICE, "ncclAllReduce(min) failed: %s", ncclGetErrorString(r));
    return LH_OK;
}

// Uniform mesh of domain.jl:58-69: faces are the correctly rounded
// zmin + k L / n (Julia ranges step in twice precision), centres are face
// midpoints in FT, bottom first (coupled.jl:198).
template <typename FT>
void make_grid(double zmin, double zmax, int n, std::vector<FT>& zc) {
    zc.resize(n);
    FT lo = FT(zmin), hi = FT(zmax), prev = lo;
    for (int k = 1; k <= n; ++k) {
        long double x = (long double)lo + ((long double)hi - (long double)lo) * k / n;
        FT f = (k == n) ? hi : FT(x);
        zc[k - 1] = (prev + f) / FT(2);
        prev = f;
    }
}

template <typename FT> FT host_pow(FT x, FT y);
template <> double host_pow<double>(double x, double y) { return std::pow(x, y); }
template <> float host_pow<float>(float x, float y) { return powf(x, y); }

// Build the kernel argument, rounding to FT where the Julia constructors do.
// Levels per segment of the level-segmented launch (rhs_kernel, CFG::SEG), 0 = one lane
// marches the whole column.  Below ~2.6e5 lanes the launch time is the latency of one
// lane's march, so the column is cut into as many segments as it takes to fill the chip,
// each at least 4 levels long (every segment evaluates two extra cells).
int segment_length(const lh_ctx* c) {
    const int nlev = c->cfg.nlev;
    if (c->tune.seg < 0) return 0;
    if (c->tune.seg > 0) return c->tune.seg < nlev ? c->tune.seg : 0;
    const int64_t lanes = c->cfg.dtype == LH_F64 ? c->cfg.ncols : (c->cfg.ncols + 1) / 2;
    const int64_t target = 262144; // 256 CUs x 4 SIMDs x 64 lanes x 4 waves
    if (lanes * 2 > target || nlev < 16) return 0;
    int64_t nseg = (target + lanes - 1) / lanes;
    if (nseg > nlev / 4) nseg = nlev / 4;
    if (nseg < 2) return 0;
    const int len = int((nlev + nseg - 1) / nseg);
    return len < nlev ? len : 0;
}

bool closure_integer_exponent(const lh_ctx* c);

template <typename FT>
DevParams<FT> make_params(const lh_ctx* c) {
    const HostParams& h = c->hp;
    DevParams<FT> P;
    memset(&P, 0, sizeof P);
    P.ncols = c->cfg.ncols;
    P.stride = c->stride;
    P.nlev = c->cfg.nlev;
    P.model = c->cfg.model;
    P.dz = (FT(c->cfg.zmax) - FT(c->cfg.zmin)) / FT(c->cfg.nlev);
    P.inv_dz = FT(1) / P.dz;
    P.half_inv_dz = FT(0.5) * P.inv_dz;
    P.cg2 = P.half_inv_dz * P.inv_dz;
    P.half_dz = P.dz / FT(2);
    P.zc = static_cast<const FT*>(c->d_zc);
    P.vg_n = FT(h.vg.n);
    P.vg_alpha = FT(h.vg.alpha);
    P.vg_theta_r = FT(h.vg.theta_r);
    P.vg_Ksat = FT(h.vg.Ksat);
    P.nu = FT(h.soil.nu);
    P.S_s = FT(h.soil.S_s);
    P.rho_c_ds = FT(h.soil.rho_c_ds);
    P.kappa_solid = FT(h.soil.kappa_solid);
    P.rho_p = FT(h.soil.rho_p);
    P.kappa_sat_unfrozen = FT(h.soil.kappa_sat_unfrozen);
    P.kappa_sat_frozen = FT(h.soil.kappa_sat_frozen);
    P.kappa_dry_parameter = FT(h.soil.kappa_dry_parameter);
    P.nu_ss_om = FT(h.soil.nu_ss_om);
    P.b = FT(h.soil.b);
    const FT om = FT(h.soil.nu_ss_om), q = FT(h.soil.nu_ss_quartz), g = FT(h.soil.nu_ss_gravel),
             a = FT(h.soil.a);
    P.kersten_exp_unfrozen = (FT(1) + om - a * q - g) / FT(2); // SoilHeatParameterizations.jl:165
    P.kersten_exp_frozen = FT(1) + om;                         // :171
    P.one_minus_om = FT(1) - om;                               // :169
    P.neg_b_log2e_sc = FT(-double(P.b) * 1.4426950408889634 * (sizeof(FT) == 8 ? double(EXP_TAB_N) : 1.0));
    P.l2_kappa_sat_unfrozen = FT(std::log2(double(P.kappa_sat_unfrozen)));
    P.l2_kappa_sat_frozen = FT(std::log2(double(P.kappa_sat_frozen)));
    // FT(cp_l(param_set) * _rho_l): Float64 product of the constant and the
    // already rounded density (SoilHeatParameterizations.jl:71-75)
    P.rho_i = FT(h.earth.rho_ice);
    const FT rho_l = FT(h.earth.rho_liq);
    P.rhocp_i = FT(h.earth.cp_i * double(P.rho_i));
    P.rhocp_l = FT(h.earth.cp_l * double(rho_l));
    P.T_ref = FT(h.earth.T_0);
    P.LH_f0 = FT(h.earth.LH_f0);
    P.k_air = FT(h.earth.K_therm);
    P.viscosity_kind = h.viscosity_kind;
    P.impedance_kind = h.impedance_kind;
    P.gamma = FT(h.gamma);
    P.T_ref_visc = FT(h.T_ref_visc);
    P.Omega = FT(h.Omega);
    // uniform column constants, host libm
    ColC<FT>& u = P.uc;
    u.nu = P.nu;
    u.S_s = P.S_s;
    u.theta_r = P.vg_theta_r;
    u.theta_lim = u.theta_r + Limits<FT>::eps();
    u.n = P.vg_n;
    u.inv_n = FT(1) / u.n;
    u.m = FT(1) - FT(1) / u.n;
    u.inv_m = FT(1) / u.m;
    u.alpha_pnn = host_pow<FT>(P.vg_alpha, -u.n);
    u.Ksat = P.vg_Ksat;
    u.cgw = P.cg2 * u.Ksat;
    u.inv_por = FT(1) / (u.nu - u.theta_r);
    u.inv_S_s = FT(1) / u.S_s;
    u.inv_nu = FT(1) / u.nu;
    u.log2_alpha = FT(std::log2(double(P.vg_alpha)));
    set_fast_vg(u, P.vg_alpha);
    u.l2_por = FT(0); // filled on the device by finish_colc (the device math policy's own log2)
    {   // exponent multipliers in the exp2 unit of the production math (lh_fastmath.hpp)
        const FT sc = sizeof(FT) == 8 ? FT(MathFast<double>::EXP2_SCALE) : FT(1);
        u.e_one = sc;
        u.e_inv_m = sc * u.inv_m;
        u.e_m = sc * u.m;
        u.e_inv_n = u.inv_n;
        u.e_log2_alpha = sc * u.log2_alpha;
    }
    if (!(u.nu > u.theta_r)) u.Ksat = u.cgw = u.inv_S_s = u.log2_alpha = u.e_log2_alpha = u.alpha_pnn = FT(NAN);
    {
        FT rho_b = (FT(1) - u.nu) * P.rho_p;
        FT num = (P.kappa_dry_parameter * P.kappa_solid - P.k_air) * rho_b + P.k_air * P.rho_p;
        FT den = P.rho_p - (FT(1) - P.kappa_dry_parameter) * rho_b;
        u.k_dry = num / den;
    }
    for (int i = 0; i < LH_PC_COUNT; ++i) P.pc[i] = static_cast<const FT*>(c->d_pc[i]);
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k) {
            P.bc_kind[f][k] = h.bc_kind[f][k];
            P.bc_value[f][k] = FT(h.bc_value[f][k]);
            P.bc_pc[f][k] = static_cast<const FT*>(c->d_bc_pc[f][k]);
        }
    if (h.atmos_on) // the top face is the prescribed atmosphere: a (per-column) flux once evaluated
        P.bc_kind[LH_FACE_TOP][LH_COMP_ENERGY] = P.bc_kind[LH_FACE_TOP][LH_COMP_HYDROLOGY] = LH_BC_FLUX;
    P.consistent_bottom_sign = h.consistent_bottom_sign;
    P.status = c->d_status;
    P.math_tab = c->d_math_tab;
    P.dt_out = nullptr;
    P.xcd_remap = 0;
    P.seg_len = segment_length(c);
    P.cs_cpb = c->tune.cpb;
    P.vg_fast_all = closure_integer_exponent(c) ? 1 : 0;
    return P;
}

template <typename FT>
AtmosParams<FT> make_atmos_params(const lh_ctx* c) {
    const lh_atmos_forcing& a = c->hp.atmos;
    AtmosParams<FT> A;
    memset(&A, 0, sizeof A);
    A.u_atm = FT(a.u_atm);
    A.theta_atm = FT(a.theta_atm);
    A.z_atm = FT(a.z_atm);
    A.theta_scale = FT(a.theta_scale);
    A.rho_a_sfc = FT(a.rho_a_sfc);
    A.q_atm = FT(a.q_atm);
    A.z_0m = FT(a.z_0m);
    A.z_0s = FT(a.z_0s);
    A.R_v = FT(a.R_v);
    A.R_d = FT(a.R_d);
    A.grav = FT(a.grav);
    A.cp_d = FT(a.cp_d);
    A.cp_v = FT(a.cp_v);
    A.T_triple = FT(a.T_triple);
    A.press_triple = FT(a.press_triple);
    A.von_karman = FT(a.von_karman);
    A.cp_l = FT(c->hp.earth.cp_l);
    A.T_0 = FT(c->hp.earth.T_0);
    A.rho_liq = FT(c->hp.earth.rho_liq);
    A.cp_v_d = a.cp_v;
    A.LH_v0_d = a.LH_v0;
    A.pc_u = static_cast<const FT*>(c->d_atm_pc[0]);
    A.pc_theta = static_cast<const FT*>(c->d_atm_pc[1]);
    A.pc_q = static_cast<const FT*>(c->d_atm_pc[2]);
    return A;
}

// "block=128,nt=1,seg=16": launch overrides (lh_launch.hpp, Tune); a key it does not scan for is ignored
void parse_tune(Tune& tu, const char* t) {
    tu = Tune();
    int v;
    const char* q;
    if ((q = strstr(t, "cpb=")) && sscanf(q + 4, "%d", &v) == 1 && v >= 0 && v <= 16) tu.cpb = v;
    if ((q = strstr(t, "persist=")) && sscanf(q + 8, "%d", &v) == 1 && v >= 0 && v <= 2) tu.persist = v;
    if ((q = strstr(t, "graph=")) && sscanf(q + 6, "%d", &v) == 1 && (v == 0 || v == 1)) tu.graph = v;
    if ((q = strstr(t, "seg=")) && sscanf(q + 4, "%d", &v) == 1 && v >= -1 && v <= 4096) tu.seg = v;
    if ((q = strstr(t, "place_mem=")) && sscanf(q + 10, "%d", &v) == 1 && v >= 1 && v <= 90) tu.place_mem = v;
    if ((q = strstr(t, "zero=")) && sscanf(q + 5, "%d", &v) == 1 && (v == 0 || v == 1)) tu.zero = v;
    if ((q = strstr(t, "xcd=")) && sscanf(q + 4, "%d", &v) == 1 && (v == 0 || v == 1)) tu.xcd = v;
    if ((q = strstr(t, "vgfast=")) && sscanf(q + 7, "%d", &v) == 1 && (v == 0 || v == 1)) tu.vgfast = v;
    if ((q = strstr(t, "trk=")) && sscanf(q + 4, "%d", &v) == 1 && v >= 1 && v <= 10000) tu.trk = v;
    if ((q = strstr(t, "trn=")) && sscanf(q + 4, "%d", &v) == 1 && v >= 1 && v <= 100) tu.trn = v;
    if ((q = strstr(t, "block=")) && sscanf(q + 6, "%d", &v) == 1 && v >= 64 && v <= 1024 && v % 64 == 0) tu.block = v;
    if ((q = strstr(t, "nt=")) && sscanf(q + 3, "%d", &v) == 1) tu.nt = v;
    if ((q = strstr(t, "arena=")) && sscanf(q + 6, "%d", &v) == 1 && v >= 1 && v <= 64) tu.arena = v;
    if ((q = strstr(t, "rowpad=")) && sscanf(q + 7, "%d", &v) == 1 && v >= 0 && v % 2 == 0) tu.rowpad = v;
    for (q = strstr(t, "pad="); q; q = strstr(q + 4, "pad=")) // not the tail of "rowpad="
        if ((q == t || q[-1] == ',' || q[-1] == ' ') && sscanf(q + 4, "%d", &v) == 1 && v >= 0 && v % 256 == 0) tu.pad = v;
}

// Whether EVERY column may take the integer-exponent 2^(.) in its water closures (ColC::vg_fast): decided
// on the host from the scalar parameters and the ranges of the per-column arrays, conservatively (an
// interval test; every comparison is false for a NaN), because the choice selects the kernel
// instantiation (rhs_kernel VGF).
bool vg_fast_all(const lh_ctx* c) {
    const HostParams& h = c->hp;
    auto lo = [&](int id, double scalar) { return c->d_pc[id] ? c->pc_lo[id] : scalar; };
    auto hi = [&](int id, double scalar) { return c->d_pc[id] ? c->pc_hi[id] : scalar; };
    const double n_lo = lo(LH_PC_VG_N, h.vg.n), n_hi = hi(LH_PC_VG_N, h.vg.n);
    const double a_lo = lo(LH_PC_VG_ALPHA, h.vg.alpha), a_hi = hi(LH_PC_VG_ALPHA, h.vg.alpha);
    const double t_lo = lo(LH_PC_VG_THETA_R, h.vg.theta_r), t_hi = hi(LH_PC_VG_THETA_R, h.vg.theta_r);
    const double nu_lo = lo(LH_PC_NU, h.soil.nu), nu_hi = hi(LH_PC_NU, h.soil.nu);
    const double m_lo = 1.0 - 1.0 / n_lo; // (Float32 rounding of the parameters moves m by 1e-7: the margin below covers it)
    return n_lo > 1.0 && n_hi < 1e30 && m_lo >= LH_VG_FAST_MIN_M * 1.001 && a_lo > 1.01e-20 && a_hi < 0.99e20 &&
           nu_lo - t_hi >= 1.01e-5 && nu_hi - t_lo <= 1.0;
}

bool any_percol(const lh_ctx* c) {
    for (int i = 0; i < LH_PC_COUNT; ++i)
        if (c->d_pc[i]) return true;
    return false;
}

// ---- layered soils: a class map is in place (lh_set_soil_class_map)
bool layered(const lh_ctx* c) { return c->d_cls_map != nullptr; }

// what a layered context cannot be combined with, checked by every entry point that takes the layered kernels
int layered_check(lh_ctx* c, const char* who) {
    if (!layered(c)) return LH_OK;
    if (c->cfg.model != LH_MODEL_RICHARDS && c->soil_thermal.empty()) // (lh_set_soil_class_map refuses it already)
        return fail(c, LH_EMODEL, "%s: soil classes are for LH_MODEL_RICHARDS only (the heat closures read nu)", who);
    if (c->hp.atmos_on && c->cfg.model != LH_MODEL_RICHARDS) // (a Richards context: validate_model's refusal, as before)
        return fail(c, LH_EMODEL, "%s: soil classes (a class map is set) cannot be combined with a prescribed-atmosphere top (lh_set_atmos_forcing)", who);
    if (any_percol(c))
        return fail(c, LH_EMODEL, "%s: soil classes (a class map is set) cannot be combined with per-column parameter arrays (lh_set_percol_param)", who);
    if (c->math == MATH_LIBM)
        return fail(c, LH_EMODEL, "%s: soil classes (a class map is set) have no LH_MATH_LIBM kernels", who);
    return LH_OK;
}
// ... and the entry points that have no layered kernels.  `twin`: the layered call that takes the refused one's place on
// a Richards context (the adaptive SSPRK33 calls); without one the message is what it was
int layered_unsupported(lh_ctx* c, const char* who, const char* twin = nullptr) {
    if (!layered(c)) return LH_OK;
    if (c->cfg.model != LH_MODEL_RICHARDS) // (the layered implicit integrators step Richards contexts only)
        return fail(c, LH_EMODEL, "%s is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, "
                                  "lh_step_ssprk33, lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are", who);
    return fail(c, LH_EMODEL, "%s is not available with soil classes (a class map is set): lh_rhs, lh_ssprk33_stage, lh_step_ssprk33, "
                              "lh_stable_dt, lh_diagnostics and lh_boundary_fluxes are, and lh_step_layered_implicit_euler and "
                              "lh_integrate_layered_trbdf2 step implicitly%s%s", who, twin ? "; a layered Richards context calls " : "",
                twin ? twin : "");
}
// vg_fast_all over the classes: whether EVERY class may take the integer-exponent 2^(.) (the same interval test)
bool classes_vg_fast(const lh_ctx* c) {
    for (const lh_soil_class& k : c->soil_classes) {
        const double m = 1.0 - 1.0 / k.n;
        if (!(k.n > 1.0 && k.n < 1e30 && m >= LH_VG_FAST_MIN_M * 1.001 && k.alpha > 1.01e-20 && k.alpha < 0.99e20 &&
              k.nu - k.theta_r >= 1.01e-5 && k.nu - k.theta_r <= 1.0))
            return false;
    }
    return true;
}
// DevParams::vg_fast_all of the next water launch, for make_params, layered_params and lh_closure_form alike:
// the tuning key first, then the interval test over the classes while a class map is set, over the columns otherwise
bool closure_integer_exponent(const lh_ctx* c) {
    return c->tune.vgfast != 0 && (layered(c) ? classes_vg_fast(c) : vg_fast_all(c));
}
// the coupled and the heat-only model with a map take the kernels of lh_layered_heat.hpp
bool layered_heat(const lh_ctx* c) { return layered(c) && c->cfg.model != LH_MODEL_RICHARDS; }
template <typename FT>
LayeredHeatArgs<FT> layered_heat_args(const lh_ctx* c) {
    LayeredHeatArgs<FT> L;
    L.cls = c->d_cls_map;
    L.table = static_cast<const ColC<FT>*>(c->d_cls_table);
    L.therm = static_cast<const ThermC<FT>*>(c->d_cls_therm);
    L.ncls = int32_t(c->soil_classes.size());
    L.any_om = c->cls_any_om ? 1 : 0;
    return L;
}
template <typename FT>
LayeredArgs<FT> layered_args(const lh_ctx* c) {
    LayeredArgs<FT> L;
    L.cls = c->d_cls_map;
    L.table = static_cast<const ColC<FT>*>(c->d_cls_table);
    L.ncls = int32_t(c->soil_classes.size());
    L.pad_ = 0;
    return L;
}
// the launch argument of a layered launch: unsegmented, no profile in LDS, the closure form decided over the classes
template <typename FT>
void layered_params(const lh_ctx* c, DevParams<FT>& P) {
    P.seg_len = 0;
    for (int i = 0; i < 4; ++i) P.aux_prof[i] = nullptr;
    P.vg_fast_all = closure_integer_exponent(c) ? 1 : 0;
}

bool model_water(int m) { return m != LH_MODEL_HEAT; }
bool model_heat(int m) { return m != LH_MODEL_RICHARDS; }

uint32_t prognostic_mask(int model) {
    switch (model) {
        case LH_MODEL_RICHARDS: return LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_THETA_I);
        case LH_MODEL_HEAT: return LH_MASK(LH_VAR_RHOE_INT);
        default: return LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_THETA_I) | LH_MASK(LH_VAR_RHOE_INT);
    }
}

uint32_t aux_mask(const lh_ctx* c) {
    if (c->cfg.model == LH_MODEL_HEAT) return LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_THETA_I);
    if (c->cfg.model == LH_MODEL_RICHARDS && c->hp.viscosity_kind != LH_FACTOR_NONE)
        return LH_MASK(LH_VAR_T);
    return 0;
}

// The combinations for which the reference has a method; anything else raises
// there (MethodError / SetValue(nothing)) and is LH_EMODEL here.
int validate_model(lh_ctx* c) {
    const HostParams& h = c->hp;
    const int m = c->cfg.model;
    if (h.atmos_on && m != LH_MODEL_COUPLED) // compute_turbulent_surface_fluxes has one method (:553-560)
        return fail(c, LH_EMODEL, "PrescribedAtmosForcing needs SoilEnergyModel + SoilHydrologyModel (no method for this model)");
    for (int f = 0; f < 2; ++f) {
        if (f == LH_FACE_TOP && h.atmos_on) continue; // the whole top face is the prescribed atmosphere
        const int ke = h.bc_kind[f][LH_COMP_ENERGY], kh = h.bc_kind[f][LH_COMP_HYDROLOGY];
        const char* fn = f == LH_FACE_TOP ? "top" : "bottom";
        if (ke == LH_BC_FREE_DRAINAGE)
            return fail(c, LH_EMODEL, "FreeDrainage is a hydrology boundary condition (%s energy)", fn);
        if (model_heat(m)) {
            if (ke == LH_BC_NONE)
                return fail(c, LH_EMODEL, "SoilEnergyModel needs an energy boundary condition at the %s face (got NoBC)", fn);
        } else if (ke == LH_BC_DIRICHLET) {
            return fail(c, LH_EMODEL, "Dirichlet energy BC has no method for PrescribedTemperatureModel (%s)", fn);
        }
        if (model_water(m)) {
            if (kh == LH_BC_NONE)
                return fail(c, LH_EMODEL, "SoilHydrologyModel needs a hydrology boundary condition at the %s face (got NoBC)", fn);
        } else if (kh == LH_BC_DIRICHLET || kh == LH_BC_FREE_DRAINAGE) {
            return fail(c, LH_EMODEL, "hydrology BC of this kind has no method for PrescribedHydrologyModel (%s)", fn);
        }
    }
    if (model_heat(m) && !h.earth_set)
        return fail(c, LH_EINVAL, "earth parameters (lh_set_earth_params) are required by the energy model");
    return LH_OK;
}

int check_state(lh_ctx* c, const lh_state* s, uint32_t need, const char* what) {
    if (need == 0) return LH_OK;
    if (!s) return fail(c, LH_ESTATE, "%s state is NULL but the model reads it", what);
    if (s->ctx != c) return fail(c, LH_EINVAL, "%s state belongs to another context", what);
    if ((s->mask & need) != need)
        return fail(c, LH_ESTATE, "%s state lacks a required variable (has mask 0x%x, needs 0x%x)", what, s->mask, need);
    return LH_OK;
}

template <typename FT>
Planes<FT> planes_of(const lh_state* s) {
    Planes<FT> p;
    for (int i = 0; i < LH_NVARS; ++i) p.v[i] = s ? static_cast<FT*>(s->plane[i]) : nullptr;
    return p;
}

// the zero bit of a plane the library has just filled with zeros (never for an exposed plane)
void mark_zero(lh_state* s, int var) {
    if (!(s->exposed_mask & (1u << var))) s->zero_mask |= 1u << var;
}
// a plane is about to be (or may have been) overwritten with arbitrary values
void mark_written(lh_state* s, uint32_t vars) {
    s->zero_mask &= ~vars;
    s->profile_mask &= ~vars;
    s->stale_mask &= ~vars;
}

// Give the planes of `vars` the values of their level-uniform profiles (one broadcast launch per
// stale plane); the profile stays valid.  Every consumer that addresses planes calls this first.
int materialize(lh_ctx* c, const lh_state* cs, uint32_t vars) {
    lh_state* s = const_cast<lh_state*>(cs);
    if (!s) return LH_OK;
    const uint32_t todo = s->stale_mask & s->profile_mask & vars;
    for (int i = 0; i < LH_NVARS && todo; ++i)
        if (todo >> i & 1u) {
            with_ft(c, [&](auto ft) {
                using FT = decltype(ft);
                launch_broadcast_profile<FT>(static_cast<FT*>(s->plane[i]), static_cast<const FT*>(s->profile[i]),
                                             c->cfg.ncols, c->stride, c->cfg.nlev, c->stream);
            });
            LH_HIP(c, hipGetLastError());
        }
    s->stale_mask &= ~todo;
    return LH_OK;
}

// the variables of Ya a column launch takes from a level-uniform profile instead of a plane
uint32_t aux_profile_vars(const lh_ctx* c, const lh_state* aux) {
    if (!aux) return 0;
    uint32_t m = 0;
    if (c->cfg.model == LH_MODEL_HEAT) m = LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_THETA_I);
    else if (c->cfg.model == LH_MODEL_RICHARDS) m = LH_MASK(LH_VAR_T);
    return m & aux->profile_mask;
}
template <typename FT>
void set_aux_profiles(const lh_ctx* c, const lh_state* aux, DevParams<FT>& P) {
    const uint32_t m = aux_profile_vars(c, aux);
    for (int i = 0; i < LH_NVARS; ++i) P.aux_prof[i] = (m >> i & 1u) ? static_cast<const FT*>(aux->profile[i]) : nullptr;
}

template <typename FT>
int do_rhs(lh_ctx* c, const lh_state* in, const lh_state* aux, const lh_state* base, lh_state* out,
           double dt, int mode, const double* bc_override, const void* dt_device = nullptr,
           void* dt_out = nullptr, bool unsegmented = false, const void* const (*bc_arrays)[2] = nullptr) {
    static const char* const range_names[6] = {"lh:rhs", "lh:stage1", "lh:stage2", "lh:stage3", "lh:rhs_stable_dt", "lh:stage2_from_k1"};
    Range r_(range_names[mode >= 0 && mode < 6 ? mode : 0]);
    DevParams<FT> P = make_params<FT>(c);
    if (unsegmented) P.seg_len = 0; // an in-place stage must not be level-segmented
    P.dt_out = dt_out;
    {   // level-uniform variables: Ya's prescribed profiles go to the kernel as they are, the rest become planes
        int rc;
        if ((rc = materialize(c, in, ~0u)) || (rc = materialize(c, base, ~0u)) || (rc = materialize(c, out, ~0u)) ||
            (rc = materialize(c, aux, layered(c) ? ~0u : ~aux_profile_vars(c, aux))))
            return rc;
        if (!layered(c)) set_aux_profiles<FT>(c, aux, P);
    }
    P.xcd_remap = c->tune.xcd;
    if (bc_override)
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 2; ++k) P.bc_value[f][k] = FT(bc_override[f * 2 + k]);
    if (bc_arrays) // per-column values of this launch alone (lh_step_ssprk33_series): FT[ncols], or NULL where lh_set_bc's stay
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 2; ++k)
                if (bc_arrays[f][k]) P.bc_pc[f][k] = static_cast<const FT*>(bc_arrays[f][k]);
    const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
    const bool tend = mode == 0 || mode == 4;
    const uint32_t ti_bit = LH_MASK(LH_VAR_THETA_I);
    if (c->hp.atmos_on) {
        // boundary_fluxes(X, bc::PrescribedAtmosForcing, :top, ...) (:516-533): the surface fluxes of
        // the state this evaluation reads, from its top cells, into the per-column flux arrays the
        // column kernel takes as VerticalFlux values at the top face
        const size_t top = size_t(c->cfg.nlev - 1) * size_t(c->stride);
        const lh_state* ti_state = tend ? in : base; // fused stages keep theta_i in the base state
        const FT* vl_top = static_cast<const FT*>(in->plane[LH_VAR_VARTHETA_L]) + top;
        const FT* ti_top = static_cast<const FT*>(ti_state->plane[LH_VAR_THETA_I]) + top;
        const FT* re_top = static_cast<const FT*>(in->plane[LH_VAR_RHOE_INT]) + top;
        launch_atmos_flux<FT>(P, make_atmos_params<FT>(c), c->cfg.ncols, true, any_percol(c), vl_top, ti_top, re_top,
                              static_cast<FT*>(c->d_atm_flux[0]), static_cast<FT*>(c->d_atm_flux[1]), c->stream);
        P.bc_kind[LH_FACE_TOP][LH_COMP_ENERGY] = P.bc_kind[LH_FACE_TOP][LH_COMP_HYDROLOGY] = LH_BC_FLUX;
        P.bc_pc[LH_FACE_TOP][LH_COMP_ENERGY] = static_cast<const FT*>(c->d_atm_flux[0]);
        P.bc_pc[LH_FACE_TOP][LH_COMP_HYDROLOGY] = static_cast<const FT*>(c->d_atm_flux[1]);
    }
    // the state theta_i is read from: Ya (HEAT), Y (tendency), the step's base state (fused stages)
    const lh_state* ti_src = c->cfg.model == LH_MODEL_HEAT ? aux : (tend ? in : base);
    const bool noice = c->tune.zero != 0 && ti_src && (ti_src->zero_mask & ti_bit);
    const bool water = model_water(c->cfg.model);
    // d theta_i = 0 (right_hand_side.jl:182, :359): no kernel stores it -- the tendency state's
    // theta_i plane is cleared here unless it is known to hold zeros already (normally once per
    // state; LH_TUNE zero=0 clears it at every launch, the traffic of a kernel that stores it)
    if (tend && water && (c->tune.zero == 0 || !(out->zero_mask & ti_bit))) {
        const size_t bytes = size_t(c->cfg.nlev) * size_t(c->stride) * c->esize;
        LH_HIP(c, hipMemsetAsync(out->plane[LH_VAR_THETA_I], 0, bytes, c->stream));
        mark_written(out, ti_bit);
        mark_zero(out, LH_VAR_THETA_I);
    }
    if (layered(c)) { // (the entry points let modes 0..3 with the step by value through, nothing else)
        layered_params<FT>(c, P);
        if (layered_heat(c))
            launch_layered_heat_rhs<FT>(P, layered_heat_args<FT>(c), planes_of<FT>(in), planes_of<FT>(aux), planes_of<FT>(base),
                                        planes_of<FT>(out), FT(dt), mode, c->cfg.model, factors, noice, c->stream);
        else
            launch_layered_rhs<FT>(P, layered_args<FT>(c), planes_of<FT>(in), planes_of<FT>(aux), planes_of<FT>(base),
                                   planes_of<FT>(out), FT(dt), mode, factors, noice, c->stream);
    } else
        launch_rhs<FT>(P, planes_of<FT>(in), planes_of<FT>(aux), planes_of<FT>(base), planes_of<FT>(out),
                       FT(dt), static_cast<const FT*>(dt_device), mode, factors, any_percol(c), noice, c->math, c->tune, c->stream);
    LH_HIP(c, hipGetLastError());
    // what the launch wrote: vartheta_l / rhoe_int values
    if (water) mark_written(out, LH_MASK(LH_VAR_VARTHETA_L));
    if (model_heat(c->cfg.model)) mark_written(out, LH_MASK(LH_VAR_RHOE_INT));
    return LH_OK;
}

constexpr int ARENA_SLOTS = 8;

void* plane_alloc(lh_ctx* c, size_t bytes) {
    // (no stagger by default: no consistent gain measured, profiles/round1_tune_plane_stagger.txt -- placement noise is +-5 %)
    const size_t pad = c->tune.pad >= 0 ? size_t(c->tune.pad) : 0;
    // slot pitch: plane size rounded to 2 MiB, plus the stagger (LH_TUNE pad=, a multiple of 256 B)
    const size_t slot = (((bytes + (size_t(2) << 20) - 1) >> 21) << 21) + pad;
    for (auto& a : c->arenas)
        if (a.slot_bytes == slot)
            for (int k = 0; k < a.nslots; ++k)
                if (!a.used[k]) {
                    a.used[k] = 1;
                    return a.base + size_t(k) * slot;
                }
    PlaneArena a;
    a.slot_bytes = slot;
    a.nslots = c->tune.arena > 0 ? c->tune.arena : ARENA_SLOTS;
    // small ensembles: one slot per arena would waste nothing, but keep it uniform
    if (hipMalloc(reinterpret_cast<void**>(&a.base), slot * size_t(a.nslots)) != hipSuccess) {
        (void)hipGetLastError();
        a.nslots = 1; // memory is tight: fall back to a single-plane arena
        if (hipMalloc(reinterpret_cast<void**>(&a.base), slot) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    a.used.assign(a.nslots, 0);
    a.used[0] = 1;
    c->arenas.push_back(a);
    return c->arenas.back().base;
}

void plane_free(lh_ctx* c, void* p) {
    for (size_t i = 0; i < c->arenas.size(); ++i) {
        PlaneArena& a = c->arenas[i];
        char* q = static_cast<char*>(p);
        if (q >= a.base && q < a.base + a.slot_bytes * size_t(a.nslots)) {
            a.used[(q - a.base) / a.slot_bytes] = 0;
            bool any = false;
            for (char u : a.used) any = any || u;
            if (!any) { // release an arena once its last plane is gone
                (void)hipFree(a.base);
                c->arenas.erase(c->arenas.begin() + i);
            }
            return;
        }
    }
}

int state_alloc(lh_ctx* c, uint32_t mask, lh_state** out) {
    lh_state* s = new (std::nothrow) lh_state();
    if (!s) return fail(c, LH_ENOMEM, "out of host memory");
    s->ctx = c;
    s->mask = mask;
    s->zero_mask = mask; // every plane is cleared below
    s->exposed_mask = s->profile_mask = s->stale_mask = 0;
    for (int i = 0; i < LH_NVARS; ++i) s->profile[i] = nullptr;
    const size_t bytes = size_t(c->cfg.nlev) * size_t(c->stride) * c->esize;
    for (int i = 0; i < LH_NVARS; ++i) s->plane[i] = nullptr;
    for (int i = 0; i < LH_NVARS; ++i) {
        if (mask & (1u << i)) {
            s->plane[i] = plane_alloc(c, bytes);
            if (!s->plane[i]) {
                for (int j = 0; j < i; ++j)
                    if (s->plane[j]) plane_free(c, s->plane[j]);
                delete s;
                return fail(c, LH_ENOMEM, "device allocation of a %zu-byte plane failed", bytes);
            }
            hipError_t e = hipMemsetAsync(s->plane[i], 0, bytes, c->stream);
            if (e != hipSuccess) {
                for (int j = 0; j <= i; ++j)
                    if (s->plane[j]) plane_free(c, s->plane[j]);
                delete s;
                return fail(c, LH_ENODEVICE, "hipMemsetAsync failed: %s", hipGetErrorString(e));
            }
        }
    }
    c->states.push_back(s);
    *out = s;
    return LH_OK;
}

void state_free(lh_ctx* c, lh_state* s) {
    for (int i = 0; i < LH_NVARS; ++i) {
        if (s->plane[i]) plane_free(c, s->plane[i]);
        if (s->profile[i]) (void)hipFree(s->profile[i]);
    }
    for (size_t i = 0; i < c->states.size(); ++i)
        if (c->states[i] == s) {
            c->states.erase(c->states.begin() + i);
            break;
        }
    delete s;
}

// The persistent column stepper keeps the state in registers over all steps of a call: 0.56 ms per
// step on 1e6 x 64 Float64 columns against 0.82 ms for three fused-stage launches, and 2-3 us per
// step for a single column.  Getting the level-fastest registers from and to the column-fastest
// planes costs about one step per call at that size, so large ensembles take it from 3 steps per call
// on; small ones (<= 2^20 threads) always.  Not for columns with more levels than a workgroup has threads.
// LH_TUNE=persist=0: never (fused-stage launches), persist=2: always.
// A Dirichlet face needs the closures of the face state.  rhs_kernel evaluates them for 64 columns
// at once; in the stepper the one lane next to the face does, with its whole wave waiting: a second
// closure pass per stage.  The wave stepper (<= 128 levels) evaluates them ONCE per call when the
// boundary values are constant over the call and nothing else the face state reads moves (the rule
// of face_state_is_static, lh_closures.hpp, restated here); otherwise large ensembles with a
// Dirichlet face stay with the fused-stage launches.
static bool dirichlet_faces_are_hoisted(const lh_ctx* c, bool bcv) {
    const bool water = c->cfg.model != LH_MODEL_HEAT, heat = c->cfg.model != LH_MODEL_RICHARDS;
    bool any = false, all_static = true;
    for (int f = 0; f < 2; ++f) {
        const int kh = c->hp.bc_kind[f][LH_COMP_HYDROLOGY], ke = c->hp.bc_kind[f][LH_COMP_ENERGY];
        const bool needs_w = water && kh == LH_BC_DIRICHLET, needs_k = heat && ke == LH_BC_DIRICHLET;
        any = any || needs_w || needs_k;
        if (needs_w && c->hp.viscosity_kind != LH_FACTOR_NONE && heat && ke != LH_BC_DIRICHLET) all_static = false;
        if (needs_k && water && kh != LH_BC_DIRICHLET) all_static = false;
    }
    if (!any) return true;
    // (measured, 1e6 columns, ms per step, stepper vs fused stages: Richards with a viscosity factor
    // 0.80 vs 1.05; the coupled model with both conductivity factors and ice, where the closures and not
    // the planes' traffic bound either engine, 0.749 vs 0.753 in Float32 and 2.03 vs 1.97 in Float64)
    const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
    if (c->cfg.model == LH_MODEL_COUPLED && factors && c->cfg.dtype == LH_F64) return false;
    return all_static && !bcv && c->cfg.nlev <= 128;
}

bool use_column_stepper(const lh_ctx* c, int64_t nsteps, bool bcv = false) {
    if (c->tune.persist == 0 || c->cfg.nlev > 1024) return false;
    if (c->hp.atmos_on) return false; // the surface fluxes are re-evaluated before every stage launch
    if (c->tune.persist == 2) return true;
    const int64_t threads = c->cfg.ncols * int64_t((c->cfg.nlev + 63) / 64 * 64);
    if (threads <= (int64_t(1) << 20)) return true;
    if (!dirichlet_faces_are_hoisted(c, bcv)) return false;
    return nsteps >= 3;
}

// bound_out (the wave stepper, <= 128 levels, with dt_device): one FT word that receives the stable-step
// bound of the state the call ends on, `dt` then being the Courant factor (lh_step_ssprk33_adaptive_hold)
int run_column_stepper(lh_ctx* c, lh_state* Y, const lh_state* Ya, double dt, const void* dt_device,
                       int64_t nsteps, const double* bcv, void* bound_out = nullptr) {
    if (nsteps <= 0) return LH_OK;
    Range r_("lh:column_stepper");
    DeviceBuffer d_bcv; // [nsteps][3][2][2] doubles -> FT on the device
    if (bcv) {
        const int rc = upload_boundary_values(c, bcv, size_t(nsteps) * 12, d_bcv);
        if (rc) return rc;
    }
    const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
    const lh_state* ti_src = c->cfg.model == LH_MODEL_HEAT ? Ya : Y;
    const bool noice = c->tune.zero != 0 && !factors && ti_src && (ti_src->zero_mask & LH_MASK(LH_VAR_THETA_I));
    {
        int rc;
        if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~aux_profile_vars(c, Ya)))) return rc;
    }
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        set_aux_profiles<FT>(c, Ya, P);
        P.dt_out = bound_out;
        launch_column_stepper<FT>(P, planes_of<FT>(Y), planes_of<FT>(Ya), FT(dt), static_cast<const FT*>(dt_device),
                                  nsteps, static_cast<const FT*>(d_bcv.p), factors, any_percol(c), noice, bound_out != nullptr, c->stream);
    });
    mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_RHOE_INT));
    const hipError_t e = launch_error(c, d_bcv);
    if (e != hipSuccess) return fail(c, LH_ENODEVICE, "column stepper launch failed: %s", hipGetErrorString(e));
    return LH_OK;
}

// The layered twin (layered_column_stepper_wave_kernel): a Richards context with a class map
// takes the stepper only when the tuning says persist=2 ("always"), for columns one wave can hold.  With the
// default tuning it keeps the fused stages; the layered coupled and heat-only kernels have no stepper.
bool use_layered_column_stepper(const lh_ctx* c) {
    return layered(c) && c->cfg.model == LH_MODEL_RICHARDS && c->tune.persist == 2 && c->cfg.nlev <= 128 && !c->hp.atmos_on;
}

// run_column_stepper for a layered Richards context: the class plane and table beside the state.  dt_device (with
// bound_out): the step is read from that FT word, `dt` is the Courant factor and bound_out, an FT
// word, receives the stable-step bound of the state the call ends on; zero steps are then legal (the bound of Y,
// no plane written).
int run_layered_column_stepper(lh_ctx* c, lh_state* Y, const lh_state* Ya, double dt, int64_t nsteps, const double* bcv,
                               const void* dt_device = nullptr, void* bound_out = nullptr) {
    if (nsteps <= 0 && !bound_out) return LH_OK;
    Range r_("lh:layered_column_stepper");
    DeviceBuffer d_bcv; // [nsteps][3][2][2] doubles -> FT on the device
    if (bcv && nsteps > 0) {
        const int rc = upload_boundary_values(c, bcv, size_t(nsteps) * 12, d_bcv);
        if (rc) return rc;
    }
    const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
    // (as do_rhs decides it for a fused stage, whose theta_i is the base state's: the launcher drops it with factors)
    const bool noice = c->tune.zero != 0 && (Y->zero_mask & LH_MASK(LH_VAR_THETA_I));
    {
        int rc;
        if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    }
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        layered_params<FT>(c, P);
        if (bound_out) {
            P.dt_out = bound_out;
            launch_fill<FT>(static_cast<FT*>(bound_out), 1, FT(INFINITY), c->stream); // the minimum starts at +inf
            launch_layered_column_stepper_bound<FT>(P, layered_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), FT(dt),
                                                    static_cast<const FT*>(dt_device), nsteps, static_cast<const FT*>(d_bcv.p),
                                                    factors, noice, c->stream);
        } else {
            launch_layered_column_stepper<FT>(P, layered_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), FT(dt), nsteps,
                                              static_cast<const FT*>(d_bcv.p), factors, noice, c->stream);
        }
    });
    if (nsteps > 0) mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L));
    const hipError_t e = launch_error(c, d_bcv);
    if (e != hipSuccess) return fail(c, LH_ENODEVICE, "layered column stepper launch failed: %s", hipGetErrorString(e));
    return LH_OK;
}

// A level-segmented stage reads cells its neighbour segments write: it needs a target
// other than its input, i.e. a second stage state.
int second_stage_state(lh_ctx* c, lh_state** U2) {
    if (segment_length(c) <= 0) return LH_OK; // in place
    if (!c->scratch_u2) {
        const uint32_t pm = prognostic_mask(c->cfg.model);
        int rc = state_alloc(c, pm & ~LH_MASK(LH_VAR_THETA_I), &c->scratch_u2);
        if (rc) return rc;
    }
    *U2 = c->scratch_u2;
    return LH_OK;
}

// ---- what the stepping entry points share on the host

// The opening of every stepping call, after its own argument checks: the model, the two states, the device
int stepping_preamble(lh_ctx* c, const lh_state* Y, const lh_state* Ya) {
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = check_state(c, Y, prognostic_mask(c->cfg.model), "Y"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    (void)hipSetDevice(c->device);
    return LH_OK;
}

// The stage states of the fused SSPRK33 launches, allocated on first use.  The stage state carries no
// theta_i plane: the fused stages read theta_i from Y.  U2 (may be NULL: not wanted, not allocated) is U1
// itself unless the launch is level-segmented.
int stage_states(lh_ctx* c, lh_state** U1, lh_state** U2) {
    int rc;
    if (!c->scratch_u1 && (rc = state_alloc(c, prognostic_mask(c->cfg.model) & ~LH_MASK(LH_VAR_THETA_I), &c->scratch_u1)))
        return rc;
    *U1 = c->scratch_u1;
    if (!U2) return LH_OK;
    *U2 = *U1;
    return second_stage_state(c, U2);
}

// Per-column boundary values of the three stages of one step: device FT arrays [ncols], or NULL where lh_set_bc's stay
struct StageBoundaryArrays {
    const void* p[3][2][2];
};

// One SSPRK33 step as three fused-stage launches.  The step is `dt`, or the device word `dt_device` when
// there is one; bc3: [3 stages][2][2] boundary values, or NULL; arrays: per-column ones, or NULL.
int fused_ssprk33_step(lh_ctx* c, lh_state* Y, const lh_state* Ya, lh_state* U1, lh_state* U2, double dt,
                       const void* dt_device, const double* bc3, const StageBoundaryArrays* arrays = nullptr) {
    for (int stage = 0; stage < 3; ++stage) {
        const double* ov = bc3 ? bc3 + stage * 4 : nullptr;
        // stage 1: U1 = Y + dt f(Y); 2: U2 = (3Y + U1 + dt f(U1))/4; 3: Y = (Y + 2U2 + 2dt f(U2))/3
        const lh_state* in = stage == 0 ? Y : (stage == 1 ? U1 : U2);
        lh_state* out = stage == 2 ? Y : (stage == 1 ? U2 : U1);
        int rc = with_ft(c, [&](auto ft) {
            return do_rhs<decltype(ft)>(c, in, Ya, Y, out, dt, stage + 1, ov, dt_device, nullptr, false, arrays ? arrays->p[stage] : nullptr);
        });
        if (rc) return rc;
    }
    return LH_OK;
}

// Small ensembles with constant boundary values: the launches themselves are the cost of a step (a few
// microseconds of device work each), so a block of steps is captured once into a hipGraph and replayed.
// Returns the steps replayed; anything that goes wrong with the capture leaves the rest to plain launches
// (*rc: a launch refused while capturing, or a replay that failed part of the way).
template <typename STEP>
int64_t replay_step_graph(lh_ctx* c, int64_t nsteps, STEP one_step, int* rc) {
    constexpr int GRAPH_STEPS = 16;
    int64_t done = 0;
    *rc = LH_OK;
    if (c->tune.graph == 0 || segment_length(c) <= 0 || nsteps < 4 * GRAPH_STEPS) return 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        for (int k = 0; k < GRAPH_STEPS && !*rc; ++k) *rc = one_step(nullptr);
        ok = hipStreamEndCapture(c->stream, &graph) == hipSuccess && graph && !*rc;
        if (*rc) { // a launch was refused while capturing: nothing has run yet
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            return 0;
        }
    }
    if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (ok)
        for (; done + GRAPH_STEPS <= nsteps; done += GRAPH_STEPS)
            if (hipGraphLaunch(exec, c->stream) != hipSuccess) {
                ok = false;
                break;
            }
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {
        const hipError_t e = hipGetLastError();
        if (done > 0 && done < nsteps && e != hipSuccess)
            *rc = fail(c, LH_ENODEVICE, "hipGraphLaunch failed after %lld steps: %s", (long long)done, hipGetErrorString(e));
    }
    return done;
}

// Names the successive `pl`-element planes of a scratch block, in the block's order
template <typename FT>
void carve_planes(void* block, size_t pl, std::initializer_list<FT**> names) {
    FT* p = static_cast<FT*>(block);
    for (FT** name : names) {
        *name = p;
        p += pl;
    }
}

// ---- how the implicit entry points fill what their launch arguments share

// the water planes of Y, which every Newton launch iterates on
template <typename FT, typename ARGS>
void point_at_water(const lh_state* Y, ARGS& A) {
    A.y = static_cast<FT*>(Y->plane[LH_VAR_VARTHETA_L]);
    A.ti = static_cast<const FT*>(Y->plane[LH_VAR_THETA_I]); // (read only by the kernels that do not know it zero)
}
// the three Newton counters of ImplicitArgs / CoupledImplicitArgs, pointed into the context's ImplicitStats block
template <typename ARGS>
void point_at_newton_stats(const lh_ctx* c, ARGS& A) {
    ImplicitStats* const st = static_cast<ImplicitStats*>(c->d_imp_stats); // (device memory: addresses only)
    A.max_iters = &st->max_iters;
    A.unconverged = &st->unconverged;
    A.total_iters = &st->total_iters;
}

// lh_integrate_trbdf2's defaults (LH_TUNE trk= / trn= override the Newton pair)
#define LH_TRBDF2_ABSTOL_DEFAULT 1e-6
#define LH_TRBDF2_RELTOL_DEFAULT 1e-3
#define LH_TRBDF2_NEWTON_KAPPA 0.01 // stage Newton test: max |delta| / (atol + rtol |Y|) <= this ...
#define LH_TRBDF2_NEWTON_MAX 10     // ... within this many iterations, else the step is rejected

// what Trbdf2Args and CoupledTrbdf2Args share besides the planes: the interval, the water's tolerances, the boundary
// table, the stage Newton test and the statistics block
template <typename FT, typename ARGS>
void fill_trbdf2_args(const lh_ctx* c, ARGS& A, double t0, double t1, double dt, double abstol, double reltol,
                      void* dt_cols_device_ft, const double* bcv) {
    A.dt_cols = static_cast<FT*>(dt_cols_device_ft);
    A.t0 = t0;
    A.t1 = t1;
    A.dt = dt;
    A.abstol = abstol;
    A.reltol = reltol;
    A.has_bcv = bcv != nullptr;
    for (int k = 0; k < 8; ++k) A.bcv[k] = bcv ? bcv[k] : 0.0;
    A.kappa = FT(c->tune.trk > 0 ? 1e-4 * c->tune.trk : LH_TRBDF2_NEWTON_KAPPA);
    A.newton_max = c->tune.trn > 0 ? c->tune.trn : LH_TRBDF2_NEWTON_MAX;
    A.stats = static_cast<unsigned long long*>(c->d_tr_stats);
}

int upload_percol(lh_ctx* c, void** slot, const double* host) {
    if (*slot) {
        LH_HIP(c, hipStreamSynchronize(c->stream));
        (void)hipFree(*slot);
        *slot = nullptr;
    }
    if (!host) return LH_OK;
    const int64_t n = c->cfg.ncols;
    double* tmp = nullptr;
    LH_HIP(c, hipMalloc(&tmp, size_t(n) * sizeof(double)));
    hipError_t e = hipMalloc(slot, size_t(n) * c->esize);
    if (e != hipSuccess) {
        (void)hipFree(tmp);
        return fail(c, LH_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    LH_HIP(c, hipMemcpyAsync(tmp, host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    with_ft(c, [&](auto ft) { launch_convert<decltype(ft)>(static_cast<decltype(ft)*>(*slot), tmp, n, c->stream); });
    LH_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(tmp);
    return LH_OK;
}

} // namespace

// Placement tuning.  On MI355X the speed of the column kernel depends on WHERE
// the planes it streams together sit relative to each other in HBM: the same
// launch on the same data runs at one of a few discrete rates (e.g. 0.339 /
// 0.378 / 0.393 ms on the 1e6 x 64 Float64 Richards case) depending on which
// arena slots hold the written state, reproducibly for a given set of slots and
// with no usable rule in the virtual addresses (profiles/round1_placement_notes.txt).
// So the library measures: it times the real launch with the written state in
// up to `max_candidates` different slot sets and keeps the fastest.
namespace {

// keep_contents: every candidate receives a copy of the target's planes (an INPUT
// of the launch is being moved); otherwise candidates start zeroed (an output).
// plane_mask: which planes of the target move (the others stay where they are).
template <typename RUN>
int tune_state_planes(lh_ctx* c, lh_state* target, uint32_t plane_mask, int max_candidates,
                      bool keep_contents, RUN&& run, float* ms_before, float* ms_after,
                      float goal_ms = 0.0f) {
    struct Cand {
        void* plane[LH_NVARS];
        float ms;
    };
    const size_t bytes = size_t(c->cfg.nlev) * size_t(c->stride) * c->esize;
    int nplanes = 0;
    for (int i = 0; i < LH_NVARS; ++i) nplanes += (target->plane[i] != nullptr) && (plane_mask >> i & 1u);
    if (!nplanes) return LH_OK;
    int K = max_candidates > 0 ? max_candidates : 6;
    if (K > 64) K = 64;
    // every candidate stays allocated until the choice is made: keep well inside free memory
    size_t free_b = 0, total_b = 0;
    LH_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const size_t per_cand = (bytes + (size_t(4) << 20)) * size_t(nplanes);
    const size_t arena_b = (bytes + (size_t(4) << 20)) * ARENA_SLOTS;
    // transient memory of the search: at most LH_TUNE place_mem=PCT percent of the free device
    // memory (default 25)
    const size_t budget = free_b / 100 * size_t(c->tune.place_mem > 0 ? c->tune.place_mem : 25);
    while (K > 1 && size_t(K - 1) * per_cand + 2 * arena_b > budget) --K;

    // the trial launches must not leave their own mark in the status word
    uint32_t status_saved = 0;
    LH_HIP(c, hipMemcpyAsync(&status_saved, c->d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    LH_HIP(c, hipStreamSynchronize(c->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    LH_HIP(c, hipEventCreate(&e0));
    {
        const hipError_t ee = hipEventCreate(&e1);
        if (ee != hipSuccess) {
            (void)hipEventDestroy(e0);
            return fail(c, LH_ENODEVICE, "hipEventCreate failed: %s", hipGetErrorString(ee));
        }
    }
    int rc = LH_OK;
    auto timed = [&](float& ms) -> int {
        constexpr int REPS = 5;
        for (int r = 0; r < 2 && !rc; ++r) rc = run();
        if (rc) return rc;
        if (hipEventRecord(e0, c->stream) != hipSuccess) return LH_ENODEVICE;
        for (int r = 0; r < REPS && !rc; ++r) rc = run();
        if (rc) return rc;
        if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
            hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
            return LH_ENODEVICE;
        ms /= REPS;
        return LH_OK;
    };
    std::vector<Cand> cands;
    Cand cur;
    for (int i = 0; i < LH_NVARS; ++i) cur.plane[i] = target->plane[i];
    cur.ms = 0;
    cands.push_back(cur);
    for (int r = 0; r < 20 && !rc; ++r) rc = run(); // clocks up before anything is compared
    for (int k = 1; k < K && !rc; ++k) {
        Cand nc;
        bool ok = true;
        for (int i = 0; i < LH_NVARS; ++i) {
            nc.plane[i] = nullptr;
            if (!(plane_mask >> i & 1u)) {
                nc.plane[i] = cur.plane[i]; // shared with every candidate, never freed here
                continue;
            }
            if (ok && target->plane[i]) {
                nc.plane[i] = plane_alloc(c, bytes);
                if (!nc.plane[i]) ok = false;
                else if ((keep_contents ? hipMemcpyAsync(nc.plane[i], cands[0].plane[i], bytes,
                                                         hipMemcpyDeviceToDevice, c->stream)
                                        : hipMemsetAsync(nc.plane[i], 0, bytes, c->stream)) != hipSuccess)
                    ok = false;
            }
        }
        if (!ok) { // out of memory: work with the candidates there are
            (void)hipGetLastError();
            for (int i = 0; i < LH_NVARS; ++i)
                if (nc.plane[i] && (plane_mask >> i & 1u)) plane_free(c, nc.plane[i]);
            break;
        }
        nc.ms = 0;
        cands.push_back(nc);
        if (goal_ms > 0) { // a long search stops as soon as a candidate reaches the goal
            for (int i = 0; i < LH_NVARS; ++i) target->plane[i] = nc.plane[i];
            float ms = 0;
            if ((rc = timed(ms))) break;
            if (ms <= goal_ms) break;
        }
    }
    // two interleaved passes, the minimum counts
    for (int pass = 0; pass < 2 && !rc; ++pass)
        for (auto& cd : cands) {
            for (int i = 0; i < LH_NVARS; ++i) target->plane[i] = cd.plane[i];
            float ms = 0;
            if ((rc = timed(ms))) break;
            cd.ms = (pass == 0 || ms < cd.ms) ? ms : cd.ms;
        }
    size_t best = 0;
    if (!rc)
        for (size_t k = 1; k < cands.size(); ++k)
            if (cands[k].ms < cands[best].ms * 0.985f) best = k; // move only for a real gain
    (void)hipStreamSynchronize(c->stream);
    for (size_t k = 0; k < cands.size(); ++k) {
        if (k == best) continue;
        for (int i = 0; i < LH_NVARS; ++i)
            if (cands[k].plane[i] && (plane_mask >> i & 1u)) plane_free(c, cands[k].plane[i]);
    }
    for (int i = 0; i < LH_NVARS; ++i) target->plane[i] = cands[best].plane[i];
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipMemcpyAsync(c->d_status, &status_saved, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    (void)hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (ms_before) *ms_before = cands[0].ms;
    if (ms_after) *ms_after = cands[best].ms;
    return LH_OK;
}

} // namespace

namespace {

template <typename FT>
int boundary_fluxes_impl(lh_ctx* c, const lh_state* Y, const lh_state* Ya, int32_t face, double* f_energy, double* f_water) {
    const int64_t n = c->cfg.ncols;
    FT* d_out = nullptr;
    LH_HIP(c, hipMalloc(reinterpret_cast<void**>(&d_out), size_t(n) * 2 * sizeof(FT)));
    DevParams<FT> P = make_params<FT>(c);
    if (c->hp.atmos_on && face == LH_FACE_TOP) {
        // boundary_fluxes(X, bc::PrescribedAtmosForcing, :top, ...) (:516-533), as do_rhs prepares it
        const size_t top = size_t(c->cfg.nlev - 1) * size_t(c->stride);
        launch_atmos_flux<FT>(P, make_atmos_params<FT>(c), n, true, any_percol(c),
                              static_cast<const FT*>(Y->plane[LH_VAR_VARTHETA_L]) + top,
                              static_cast<const FT*>(Y->plane[LH_VAR_THETA_I]) + top,
                              static_cast<const FT*>(Y->plane[LH_VAR_RHOE_INT]) + top,
                              static_cast<FT*>(c->d_atm_flux[0]), static_cast<FT*>(c->d_atm_flux[1]), c->stream);
        P.bc_kind[LH_FACE_TOP][LH_COMP_ENERGY] = P.bc_kind[LH_FACE_TOP][LH_COMP_HYDROLOGY] = LH_BC_FLUX;
        P.bc_pc[LH_FACE_TOP][LH_COMP_ENERGY] = static_cast<const FT*>(c->d_atm_flux[0]);
        P.bc_pc[LH_FACE_TOP][LH_COMP_HYDROLOGY] = static_cast<const FT*>(c->d_atm_flux[1]);
    }
    const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
    if (layered(c)) {
        layered_params<FT>(c, P);
        if (layered_heat(c))
            launch_layered_heat_boundary_fluxes<FT>(P, layered_heat_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), face, d_out,
                                                    d_out + n, c->cfg.model, factors, c->stream);
        else
            launch_layered_boundary_fluxes<FT>(P, layered_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), face, d_out, d_out + n,
                                               factors, c->stream);
    } else
        launch_boundary_fluxes<FT>(P, planes_of<FT>(Y), planes_of<FT>(Ya), face, d_out, d_out + n, factors, any_percol(c),
                                   c->math, c->stream);
    hipError_t e = hipGetLastError();
    std::vector<FT> h(size_t(n) * 2);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(FT), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(d_out);
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(c, LH_ENODEVICE, "lh_boundary_fluxes failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    for (int64_t i = 0; i < n; ++i) {
        if (f_energy) f_energy[i] = double(h[size_t(i)]);
        if (f_water) f_water[i] = double(h[size_t(n + i)]);
    }
    return LH_OK;
}

} // namespace

// ---- layered soils: what the three entry points share
namespace {

// the class map goes with its classes
int drop_class_map(lh_ctx* c) {
    if (!c->d_cls_map) return LH_OK;
    LH_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_cls_map);
    c->d_cls_map = nullptr;
    c->cls_map_max = 0;
    return LH_OK;
}

// The ColC<FT> of one class, by the arithmetic make_params applies to the scalar parameters: a context whose
// six scalars are the class's gets exactly this entry as its DevParams::uc
// With the class's thermal supplement `t` the eight fields it holds replace the context's too: k_dry then comes from
// the class's own nu, rho_p, kappa_solid, and the returned block holds the class's thermal constants.
template <typename FT>
DevParams<FT> class_params(lh_ctx* c, const lh_soil_class& k, const lh_soil_class_thermal* t) {
    const HostParams saved = c->hp;
    c->hp.vg.n = k.n;
    c->hp.vg.alpha = k.alpha;
    c->hp.vg.theta_r = k.theta_r;
    c->hp.vg.Ksat = k.Ksat;
    c->hp.soil.nu = k.nu;
    c->hp.soil.S_s = k.S_s;
    if (t) {
        c->hp.soil.rho_c_ds = t->rho_c_ds;
        c->hp.soil.kappa_solid = t->kappa_solid;
        c->hp.soil.rho_p = t->rho_p;
        c->hp.soil.kappa_sat_unfrozen = t->kappa_sat_unfrozen;
        c->hp.soil.kappa_sat_frozen = t->kappa_sat_frozen;
        c->hp.soil.nu_ss_gravel = t->nu_ss_gravel;
        c->hp.soil.nu_ss_om = t->nu_ss_om;
        c->hp.soil.nu_ss_quartz = t->nu_ss_quartz;
    }
    const DevParams<FT> P = make_params<FT>(c);
    c->hp = saved;
    return P;
}
template <typename FT>
ColC<FT> class_colc(lh_ctx* c, const lh_soil_class& k) { return class_params<FT>(c, k, nullptr).uc; }

// the class table (and, with a supplement, the thermal table) of the classes and supplement given, to the device
int upload_class_tables(lh_ctx* c, int nclasses, const lh_soil_class* classes, const lh_soil_class_thermal* thermal) {
    static_assert(LH_MAX_SOIL_CLASSES == LH_LAYERED_MAX_CLASSES, "the header's limit is the kernels' table size");
    if (!c->d_cls_table)
        LH_HIP(c, hipMalloc(&c->d_cls_table, size_t(LH_MAX_SOIL_CLASSES) * sizeof(ColC<double>)));
    if (thermal && !c->d_cls_therm)
        LH_HIP(c, hipMalloc(&c->d_cls_therm, size_t(LH_MAX_SOIL_CLASSES) * sizeof(ThermC<double>)));
    std::vector<char> tab(size_t(nclasses) * sizeof(ColC<double>)), th(size_t(nclasses) * sizeof(ThermC<double>));
    size_t bytes = 0, th_bytes = 0;
    bool any_om = false;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        for (int k = 0; k < nclasses; ++k) {
            const DevParams<FT> P = class_params<FT>(c, classes[k], thermal ? thermal + k : nullptr);
            memcpy(tab.data() + size_t(k) * sizeof P.uc, &P.uc, sizeof P.uc);
            ThermC<FT> t;
            t.rho_c_ds = P.rho_c_ds;
            t.kappa_sat_unfrozen = P.kappa_sat_unfrozen;
            t.kappa_sat_frozen = P.kappa_sat_frozen;
            t.l2_kappa_sat_unfrozen = P.l2_kappa_sat_unfrozen;
            t.l2_kappa_sat_frozen = P.l2_kappa_sat_frozen;
            t.kersten_exp_unfrozen = P.kersten_exp_unfrozen;
            t.kersten_exp_frozen = P.kersten_exp_frozen;
            t.one_minus_om = P.one_minus_om;
            memcpy(th.data() + size_t(k) * sizeof t, &t, sizeof t);
            any_om = any_om || (thermal && P.one_minus_om != FT(1));
        }
        bytes = size_t(nclasses) * sizeof(ColC<FT>);
        th_bytes = size_t(nclasses) * sizeof(ThermC<FT>);
    });
    LH_HIP(c, hipStreamSynchronize(c->stream)); // launches in flight read the tables in place
    LH_HIP(c, hipMemcpy(c->d_cls_table, tab.data(), bytes, hipMemcpyHostToDevice));
    if (thermal) LH_HIP(c, hipMemcpy(c->d_cls_therm, th.data(), th_bytes, hipMemcpyHostToDevice));
    c->cls_any_om = any_om;
    return LH_OK;
}

// The tables hold what make_params forms from the classes AND the context's scalars (a, kappa_dry_parameter, the
// air's conductivity: the Kersten exponent and k_dry), so a setter of those scalars forms them again
int refresh_class_tables(lh_ctx* c) {
    if (c->soil_classes.empty()) return LH_OK;
    (void)hipSetDevice(c->device);
    return upload_class_tables(c, int(c->soil_classes.size()), c->soil_classes.data(),
                               c->soil_thermal.empty() ? nullptr : c->soil_thermal.data());
}

} // namespace

// ============================================================== C ABI

extern "C" {

int lh_version(void) { return LH_VERSION_MAJOR * 100 + LH_VERSION_MINOR; }

const char* lh_last_error(const lh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int lh_create(lh_ctx** out, const lh_config* cfg) {
    if (!out || !cfg) return fail(nullptr, LH_EINVAL, "lh_create: NULL argument");
    *out = nullptr;
    if (cfg->ncols < 1 || cfg->nlev < 1) return fail(nullptr, LH_EINVAL, "lh_create: ncols and nlev must be >= 1");
    if (cfg->ncols > (int64_t(1) << 28)) return fail(nullptr, LH_EINVAL, "lh_create: more than 2^28 columns per context is not supported (a plane row must stay below 4 GiB); partition the ensemble");
    if (cfg->nlev > 4096) return fail(nullptr, LH_EINVAL, "lh_create: nlev > 4096 is not supported (level coordinates are staged in LDS)");
    if (!(cfg->zmin < cfg->zmax)) return fail(nullptr, LH_EINVAL, "lh_create: zlim[1] < zlim[2] required (domain.jl:30)");
    if (cfg->dtype != LH_F32 && cfg->dtype != LH_F64) return fail(nullptr, LH_EINVAL, "lh_create: dtype must be LH_F32 or LH_F64");
    if (cfg->model < LH_MODEL_RICHARDS || cfg->model > LH_MODEL_COUPLED) return fail(nullptr, LH_EINVAL, "lh_create: unknown model");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, LH_ENODEVICE, "lh_create: no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    int dev = cfg->device;
    if (dev < 0) {
        e = hipGetDevice(&dev);
        if (e != hipSuccess) return fail(nullptr, LH_ENODEVICE, "hipGetDevice failed: %s", hipGetErrorString(e));
    }
    if (dev >= ndev) return fail(nullptr, LH_EINVAL, "lh_create: device %d out of range (%d devices)", dev, ndev);
    e = hipSetDevice(dev);
    if (e != hipSuccess) return fail(nullptr, LH_ENODEVICE, "hipSetDevice(%d) failed: %s", dev, hipGetErrorString(e));

    lh_ctx* c = new (std::nothrow) lh_ctx();
    if (!c) return fail(nullptr, LH_ENOMEM, "out of host memory");
    c->cfg = *cfg;
    c->device = dev;
    c->esize = cfg->dtype == LH_F64 ? 8 : 4;
    // Plane row length: whole 512-B units, and an ODD number of them.  The column
    // kernel has every level of a plane in flight at once (waves drift apart), so
    // a level stride with a large power-of-two factor piles those streams onto
    // the same HBM channels/banks: 2^20 columns ran at 59.5 % of peak with the
    // natural 8-MiB stride and at 65-66 % with one extra unit (profiles/
    // round1_placement_notes.txt).
    {
        const int64_t unit = 512 / int64_t(c->esize); // elements per 512 B
        int64_t units = (cfg->ncols + unit - 1) / unit;
        if (units % 2 == 0) ++units;
        c->stride = units * unit;
    }
    // reference defaults: loam vanGenuchten, default SoilParams
    c->hp.vg = lh_vg_params{1.56, 3.6, 0.0, 2.9e-7};
    c->hp.soil = lh_soil_params{0.43, 1e-3, 0.0, 0.0, 0.41, 2700.0, 3.97, 2700.0, 1.72, 3.13, 0.24, 18.1, 0.053};
    if (const char* m = getenv("LH_MATH"))
        if (!strcmp(m, "libm")) c->math = MATH_LIBM;
    if (const char* t = getenv("LH_TUNE")) parse_tune(c->tune, t);
    if (c->tune.rowpad >= 0) c->stride += c->tune.rowpad; // explicit row padding (elements)

#define CREATE_HIP(call)                                                                           \
    do {                                                                                           \
        hipError_t e2_ = (call);                                                                   \
        if (e2_ != hipSuccess) {                                                                   \
            int rc_ = fail(nullptr, e2_ == hipErrorOutOfMemory ? LH_ENOMEM : LH_ENODEVICE,         \
                           "lh_create: %s failed: %s", #call, hipGetErrorString(e2_));             \
            lh_destroy(c);                                                                         \
            return rc_;                                                                            \
        }                                                                                          \
    } while (0)

    if (cfg->stream) {
        c->stream = static_cast<hipStream_t>(cfg->stream);
    } else {
        CREATE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    CREATE_HIP(hipEventCreate(&c->ev0));
    CREATE_HIP(hipEventCreate(&c->ev1));
    CREATE_HIP(hipMalloc(&c->d_zc, size_t(cfg->nlev) * c->esize));
    CREATE_HIP(hipMalloc(&c->d_status, sizeof(uint32_t)));
    CREATE_HIP(hipMemsetAsync(c->d_status, 0, sizeof(uint32_t), c->stream));
    CREATE_HIP(hipMalloc(&c->d_dt, 8));
    {
        // tables of lh_fastmath.hpp, built in long double and rounded once
        std::vector<double> tab(MATH_TAB_DOUBLES);
        for (int i = 0; i < LOG_TAB_N; ++i) {
            long double cc = 0.5L * (1.0L + (i + 0.5L) / LOG_TAB_N);
            if (i == 0) cc = 0.5L;               // log2(1) == 0 exactly, and
            if (i == LOG_TAB_N - 1) cc = 1.0L;   // nothing lost next to 1
            tab[2 * i] = double(1.0L / cc);
            tab[2 * i + 1] = double(log2l(cc));
        }
        for (int j = 0; j < EXP_TAB_N; ++j) {
            // 2^(j/2048), stored with (j << 9) subtracted from its high word: the kernels put the
            // binary exponent in place by ONE integer addition of (k << 9), k = 2048 e + j
            // (MathFast<double>::exp2_scaled_ins); the low word is the value's own
            const double v = double(exp2l((long double)j / EXP_TAB_N));
            uint64_t bits;
            memcpy(&bits, &v, 8);
            bits -= uint64_t(uint32_t(j) << 9) << 32;
            memcpy(&tab[2 * LOG_TAB_N + j], &bits, 8);
        }
        CREATE_HIP(hipMalloc(&c->d_math_tab, tab.size() * sizeof(double)));
        CREATE_HIP(hipMemcpy(c->d_math_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    c->zc_host.resize(cfg->nlev);
    if (cfg->dtype == LH_F64) {
        std::vector<double> z;
        make_grid<double>(cfg->zmin, cfg->zmax, cfg->nlev, z);
        for (int i = 0; i < cfg->nlev; ++i) c->zc_host[i] = z[i];
        CREATE_HIP(hipMemcpy(c->d_zc, z.data(), z.size() * 8, hipMemcpyHostToDevice));
    } else {
        std::vector<float> z;
        make_grid<float>(cfg->zmin, cfg->zmax, cfg->nlev, z);
        for (int i = 0; i < cfg->nlev; ++i) c->zc_host[i] = z[i];
        CREATE_HIP(hipMemcpy(c->d_zc, z.data(), z.size() * 4, hipMemcpyHostToDevice));
    }
#undef CREATE_HIP
    *out = c;
    return LH_OK;
}

int lh_destroy(lh_ctx* c) {
    if (!c) return LH_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) {
        (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
    }
    while (!c->states.empty()) state_free(c, c->states.back());
    while (!c->series.empty()) (void)lh_bc_series_destroy(c, c->series.back());
    if (c->d_series_dt) (void)hipFree(c->d_series_dt);
    if (c->d_series_stage) (void)hipFree(c->d_series_stage);
    for (auto& a : c->arenas) (void)hipFree(a.base); // none should be left
    c->arenas.clear();
    for (int i = 0; i < LH_PC_COUNT; ++i)
        if (c->d_pc[i]) (void)hipFree(c->d_pc[i]);
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k)
            if (c->d_bc_pc[f][k]) (void)hipFree(c->d_bc_pc[f][k]);
    if (c->d_zc) (void)hipFree(c->d_zc);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_dt) (void)hipFree(c->d_dt);
    if (c->d_imp) (void)hipFree(c->d_imp);
    if (c->d_imp_stats) (void)hipFree(c->d_imp_stats);
    if (c->d_tr) (void)hipFree(c->d_tr);
    if (c->d_tr_stats) (void)hipFree(c->d_tr_stats);
    if (c->d_heat) (void)hipFree(c->d_heat);
    if (c->d_cpl) (void)hipFree(c->d_cpl);
    if (c->d_cpl_tr) (void)hipFree(c->d_cpl_tr);
    if (c->d_cpl_ad) (void)hipFree(c->d_cpl_ad);
    if (c->d_heat_ad) (void)hipFree(c->d_heat_ad);
    if (c->d_cls_table) (void)hipFree(c->d_cls_table);
    if (c->d_cls_map) (void)hipFree(c->d_cls_map);
    if (c->d_cls_therm) (void)hipFree(c->d_cls_therm);
    for (int k = 0; k < 3; ++k)
        if (c->d_atm_pc[k]) (void)hipFree(c->d_atm_pc[k]);
    for (int k = 0; k < 2; ++k)
        if (c->d_atm_flux[k]) (void)hipFree(c->d_atm_flux[k]);
    if (c->d_math_tab) (void)hipFree(c->d_math_tab);
    if (c->h_ring) (void)hipHostFree(c->h_ring);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return LH_OK;
}

int lh_set_earth_params(lh_ctx* c, const lh_earth_params* p) {
    if (!c || !p) return fail(c, LH_EINVAL, "lh_set_earth_params: NULL argument");
    c->hp.earth = *p;
    c->hp.earth_set = true;
    return refresh_class_tables(c);
}

int lh_set_soil_params(lh_ctx* c, const lh_soil_params* p) {
    if (!c || !p) return fail(c, LH_EINVAL, "lh_set_soil_params: NULL argument");
    c->hp.soil = *p;
    return refresh_class_tables(c);
}

int lh_set_vg_params(lh_ctx* c, const lh_vg_params* p) {
    if (!c || !p) return fail(c, LH_EINVAL, "lh_set_vg_params: NULL argument");
    c->hp.vg = *p;
    return LH_OK;
}

int lh_set_percol_param(lh_ctx* c, int32_t id, const double* host) {
    if (!c) return LH_EINVAL;
    if (id < 0 || id >= LH_PC_COUNT) return fail(c, LH_EINVAL, "lh_set_percol_param: unknown parameter id %d", id);
    (void)hipSetDevice(c->device);
    if (host) { // the array's range decides which closure form the ensemble may take (vg_fast_all)
        double lo = host[0], hi = host[0];
        bool nan = false;
        for (int64_t k = 0; k < c->cfg.ncols; ++k) {
            const double v = host[k];
            nan = nan || v != v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        c->pc_lo[id] = nan ? NAN : lo;
        c->pc_hi[id] = nan ? NAN : hi;
    }
    return upload_percol(c, &c->d_pc[id], host);
}

// ---- layered soils (build extension; kernels in lh_layered.hpp)

int lh_set_soil_classes(lh_ctx* c, int32_t nclasses, const lh_soil_class* classes) {
    if (!c) return LH_EINVAL;
    if (nclasses < 0 || nclasses > LH_MAX_SOIL_CLASSES)
        return fail(c, LH_EINVAL, "lh_set_soil_classes: nclasses must be 0 .. %d, got %d", int(LH_MAX_SOIL_CLASSES), int(nclasses));
    (void)hipSetDevice(c->device);
    // (the call drops the thermal supplement, which a map on a coupled or heat-only context cannot be without)
    if (layered_heat(c))
        return fail(c, LH_EMODEL, "lh_set_soil_classes: class map in place needs thermal properties (remove the map first: "
                                  "lh_set_soil_class_map(NULL), then lh_set_soil_classes and lh_set_soil_class_thermal)");
    if (nclasses == 0) { // the classes, their supplement and the map go
        if (int rc = drop_class_map(c)) return rc;
        c->soil_classes.clear();
        c->soil_thermal.clear();
        c->cls_any_om = false;
        return LH_OK;
    }
    // (what lh_set_vg_params / lh_set_soil_params refuse is a NULL argument; parameter values are not judged
    // here either: nu <= theta_r poisons the class's cells like a column's, make_params)
    if (!classes) return fail(c, LH_EINVAL, "lh_set_soil_classes: NULL argument (class 0 of %d)", int(nclasses));
    if (c->d_cls_map && c->cls_map_max >= nclasses)
        return fail(c, LH_EINVAL, "lh_set_soil_classes: the class map in place uses class %d, %d classes given", c->cls_map_max, int(nclasses));
    if (int rc = upload_class_tables(c, nclasses, classes, nullptr)) return rc;
    c->soil_classes.assign(classes, classes + nclasses);
    c->soil_thermal.clear();
    return LH_OK;
}

int lh_set_soil_class_thermal(lh_ctx* c, int32_t nclasses, const lh_soil_class_thermal* classes) {
    if (!c) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    const int have = int(c->soil_classes.size());
    if (nclasses == 0) { // the supplement goes: the class table is the one lh_set_soil_classes built
        if (layered_heat(c))
            return fail(c, LH_EMODEL, "lh_set_soil_class_thermal: the class map in place needs the thermal properties of the soil "
                                      "classes (remove the map first: lh_set_soil_class_map(NULL))");
        if (c->soil_thermal.empty()) return LH_OK;
        if (int rc = upload_class_tables(c, have, c->soil_classes.data(), nullptr)) return rc;
        c->soil_thermal.clear();
        return LH_OK;
    }
    if (nclasses != have)
        return fail(c, LH_EINVAL, "lh_set_soil_class_thermal: %d thermal classes given, %d soil classes are set (lh_set_soil_classes)",
                    int(nclasses), have);
    if (!classes) return fail(c, LH_EINVAL, "lh_set_soil_class_thermal: NULL argument (class 0 of %d)", int(nclasses));
    // (values are not judged, as in lh_set_soil_params)
    if (int rc = upload_class_tables(c, have, c->soil_classes.data(), classes)) return rc;
    c->soil_thermal.assign(classes, classes + nclasses);
    return LH_OK;
}

int lh_soil_class_thermal_info(const lh_ctx* c, int32_t* has_thermal) {
    if (!c) return LH_EINVAL;
    if (has_thermal) *has_thermal = c->soil_thermal.empty() ? 0 : 1;
    return LH_OK;
}

int lh_set_soil_class_map(lh_ctx* c, const uint8_t* host_map, int64_t lev_stride, int64_t col_stride) {
    if (!c) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    if (!host_map) return drop_class_map(c);
    if (c->soil_classes.empty()) return fail(c, LH_EMODEL, "lh_set_soil_class_map: no soil classes are set (lh_set_soil_classes)");
    if (c->cfg.model != LH_MODEL_RICHARDS && c->soil_thermal.empty())
        return fail(c, LH_EMODEL, "lh_set_soil_class_map: soil classes are for LH_MODEL_RICHARDS only (the heat closures read nu) "
                                  "unless they carry their thermal properties (lh_set_soil_class_thermal)");
    const int64_t ncols = c->cfg.ncols;
    const int nlev = c->cfg.nlev, ncls = int(c->soil_classes.size());
    std::vector<uint8_t> plane(size_t(nlev) * size_t(c->stride), uint8_t(0)); // pad columns: class 0
    int top = 0;
    for (int64_t col = 0; col < ncols; ++col)
        for (int lev = 0; lev < nlev; ++lev) {
            const uint8_t k = host_map[col * col_stride + int64_t(lev) * lev_stride];
            if (k >= ncls)
                return fail(c, LH_EINVAL, "lh_set_soil_class_map: class %d at (column %lld, level %d), %d classes are set", int(k),
                            (long long)col, lev, ncls);
            top = k > top ? k : top;
            plane[size_t(lev) * size_t(c->stride) + size_t(col)] = k;
        }
    if (!c->d_cls_map) LH_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->d_cls_map), plane.size()));
    LH_HIP(c, hipStreamSynchronize(c->stream)); // launches in flight read the map in place
    LH_HIP(c, hipMemcpy(c->d_cls_map, plane.data(), plane.size(), hipMemcpyHostToDevice));
    c->cls_map_max = top;
    return LH_OK;
}

int lh_soil_class_info(const lh_ctx* c, int32_t* nclasses, int32_t* has_map) {
    if (!c) return LH_EINVAL;
    if (nclasses) *nclasses = int32_t(c->soil_classes.size());
    if (has_map) *has_map = c->d_cls_map ? 1 : 0;
    return LH_OK;
}

int lh_set_conductivity_factors(lh_ctx* c, int32_t vk, double gamma, double T_ref, int32_t ik, double Omega) {
    if (!c) return LH_EINVAL;
    if ((vk != LH_FACTOR_NONE && vk != LH_FACTOR_ON) || (ik != LH_FACTOR_NONE && ik != LH_FACTOR_ON))
        return fail(c, LH_EINVAL, "lh_set_conductivity_factors: kind must be LH_FACTOR_NONE or LH_FACTOR_ON");
    c->hp.viscosity_kind = vk;
    c->hp.impedance_kind = ik;
    c->hp.gamma = gamma;
    c->hp.T_ref_visc = T_ref;
    c->hp.Omega = Omega;
    return LH_OK;
}

int lh_set_bc(lh_ctx* c, int32_t face, int32_t comp, int32_t kind, double value, const double* percol) {
    if (!c) return LH_EINVAL;
    if (face != LH_FACE_BOTTOM && face != LH_FACE_TOP)
        return fail(c, LH_EINVAL, "Expected :top or :bottom"); // boundary_conditions.jl:188
    if (comp != LH_COMP_ENERGY && comp != LH_COMP_HYDROLOGY) return fail(c, LH_EINVAL, "lh_set_bc: unknown component %d", comp);
    if (kind < LH_BC_NONE || kind > LH_BC_FREE_DRAINAGE) return fail(c, LH_EINVAL, "lh_set_bc: unknown kind %d", kind);
    c->hp.bc_kind[face][comp] = kind;
    c->hp.bc_value[face][comp] = value;
    (void)hipSetDevice(c->device);
    return upload_percol(c, &c->d_bc_pc[face][comp], percol);
}

int lh_set_atmos_forcing(lh_ctx* c, const lh_atmos_forcing* f, const double* percol) {
    if (!c) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    if (!f) { // back to the component boundary conditions of lh_set_bc
        c->hp.atmos_on = false;
        for (int k = 0; k < 3; ++k) {
            int rc = upload_percol(c, &c->d_atm_pc[k], nullptr);
            if (rc) return rc;
        }
        return LH_OK;
    }
    if (c->cfg.model != LH_MODEL_COUPLED)
        return fail(c, LH_EMODEL, "PrescribedAtmosForcing needs SoilEnergyModel + SoilHydrologyModel (no method for this model)");
    if (!(f->z_atm > 0) || !(f->z_0m > 0) || !(f->z_0s > 0) || !(f->rho_a_sfc > 0) || !(f->theta_scale > 0) ||
        !(f->R_v > 0) || !(f->von_karman > 0) || !(f->T_triple > 0))
        return fail(c, LH_EINVAL, "lh_set_atmos_forcing: z_atm, z_0m, z_0s, rho_a_sfc, theta_scale, R_v, von_karman, T_triple must be > 0");
    for (int k = 0; k < 2; ++k)
        if (!c->d_atm_flux[k]) LH_HIP(c, hipMalloc(&c->d_atm_flux[k], size_t(c->cfg.ncols) * c->esize));
    for (int k = 0; k < 3; ++k) {
        int rc = upload_percol(c, &c->d_atm_pc[k], percol ? percol + size_t(k) * size_t(c->cfg.ncols) : nullptr);
        if (rc) return rc;
    }
    c->hp.atmos = *f;
    c->hp.atmos_on = true;
    return LH_OK;
}

int lh_atmos_surface_fluxes(lh_ctx* c, int64_t n, const double* vl, const double* ti, const double* T,
                            double* heat, double* water) {
    if (!c || !vl || !ti || !T || !heat || !water) return fail(c, LH_EINVAL, "lh_atmos_surface_fluxes: NULL argument");
    if (n < 0) return fail(c, LH_EINVAL, "lh_atmos_surface_fluxes: n < 0");
    if (!c->hp.atmos_on) return fail(c, LH_EMODEL, "no PrescribedAtmosForcing is set on this model (lh_set_atmos_forcing)");
    int rc = validate_model(c);
    if (rc) return rc;
    if (n == 0) return LH_OK;
    (void)hipSetDevice(c->device);
    const size_t es = c->esize;
    double* d_in = nullptr;   // 3 n doubles in, converted to FT; 2 n FT out
    char* d_ft = nullptr;
    LH_HIP(c, hipMalloc(&d_in, size_t(n) * 3 * sizeof(double)));
    hipError_t e = hipMalloc(&d_ft, size_t(n) * 5 * es);
    if (e != hipSuccess) {
        (void)hipFree(d_in);
        return fail(c, LH_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    auto cleanup = [&]() {
        (void)hipFree(d_in);
        (void)hipFree(d_ft);
    };
    const double* src[3] = {vl, ti, T};
    for (int k = 0; k < 3 && e == hipSuccess; ++k)
        e = hipMemcpyAsync(d_in + size_t(k) * n, src[k], size_t(n) * sizeof(double), hipMemcpyHostToDevice, c->stream);
    std::vector<char> out(size_t(n) * 2 * es);
    if (e == hipSuccess) {
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            FT* f = reinterpret_cast<FT*>(d_ft);
            launch_convert<FT>(f, d_in, 3 * n, c->stream);
            launch_atmos_flux<FT>(make_params<FT>(c), make_atmos_params<FT>(c), n, false, false, f, f + n, f + 2 * n,
                                  f + 3 * n, f + 4 * n, c->stream);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_ft + size_t(n) * 3 * es, size_t(n) * 2 * es, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    cleanup();
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(c, LH_ENODEVICE, "lh_atmos_surface_fluxes failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    with_ft(c, [&](auto ft) {
        const auto* o = reinterpret_cast<const decltype(ft)*>(out.data());
        for (int64_t i = 0; i < n; ++i) heat[i] = o[i], water[i] = o[n + i];
    });
    return LH_OK;
}

int lh_set_bottom_sign_consistent(lh_ctx* c, int32_t flag) {
    if (!c) return LH_EINVAL;
    c->hp.consistent_bottom_sign = flag ? 1 : 0;
    return LH_OK;
}

int lh_set_tuning(lh_ctx* c, const char* spec) {
    if (!c || !spec) return LH_EINVAL;
    const int arena = c->tune.arena, pad = c->tune.pad, rowpad = c->tune.rowpad; // fixed at lh_create
    parse_tune(c->tune, spec);
    c->tune.arena = arena;
    c->tune.pad = pad;
    c->tune.rowpad = rowpad;
    return LH_OK;
}

int lh_set_math_mode(lh_ctx* c, int32_t mode) {
    if (!c) return LH_EINVAL;
    if (mode != LH_MATH_FAST && mode != LH_MATH_LIBM) return fail(c, LH_EINVAL, "lh_set_math_mode: unknown mode %d", mode);
    c->math = mode == LH_MATH_LIBM ? MATH_LIBM : MATH_FAST;
    return LH_OK;
}

int lh_state_create(lh_ctx* c, uint32_t mask, lh_state** out) {
    if (!c || !out) return fail(c, LH_EINVAL, "lh_state_create: NULL argument");
    if (mask == 0) mask = prognostic_mask(c->cfg.model);
    if (mask >= (1u << LH_NVARS)) return fail(c, LH_EINVAL, "lh_state_create: bad variable mask 0x%x", mask);
    (void)hipSetDevice(c->device);
    return state_alloc(c, mask, out);
}

int lh_state_destroy(lh_ctx* c, lh_state* s) {
    if (!c || !s) return LH_OK;
    if (s->ctx != c) return fail(c, LH_EINVAL, "lh_state_destroy: state belongs to another context");
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->scratch_u1 == s) c->scratch_u1 = nullptr;
    if (c->scratch_u2 == s) c->scratch_u2 = nullptr;
    if (c->scratch_k1 == s) c->scratch_k1 = nullptr;
    state_free(c, s);
    return LH_OK;
}

static int transfer(lh_ctx* c, lh_state* s, int32_t var, void* host, int64_t ls, int64_t cs, bool upload) {
    if (!c || !s || !host) return fail(c, LH_EINVAL, "lh_upload/lh_download: NULL argument");
    if (s->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if (var < 0 || var >= LH_NVARS || !(s->mask & (1u << var))) return fail(c, LH_ESTATE, "state has no variable %d", var);
    if (ls < 1 || cs < 1) return fail(c, LH_EINVAL, "strides must be >= 1");
    (void)hipSetDevice(c->device);
    if (upload) mark_written(s, 1u << var);
    else {
        int rc = materialize(c, s, 1u << var);
        if (rc) return rc;
    }
    const int64_t ncols = c->cfg.ncols;
    const int nlev = c->cfg.nlev;
    const size_t es = c->esize;
    char* plane = static_cast<char*>(s->plane[var]);
    if (cs == 1 && ls >= ncols) { // already column-fastest: one 2-D copy
        if (upload)
            LH_HIP(c, hipMemcpy2DAsync(plane, size_t(c->stride) * es, host, size_t(ls) * es, size_t(ncols) * es, nlev, hipMemcpyHostToDevice, c->stream));
        else
            LH_HIP(c, hipMemcpy2DAsync(host, size_t(ls) * es, plane, size_t(c->stride) * es, size_t(ncols) * es, nlev, hipMemcpyDeviceToHost, c->stream));
        LH_HIP(c, hipStreamSynchronize(c->stream));
        return LH_OK;
    }
    const int64_t span = (ncols - 1) * cs + int64_t(nlev - 1) * ls + 1;
    void* tmp = nullptr;
    LH_HIP(c, hipMalloc(&tmp, size_t(span) * es));
    hipError_t e = hipSuccess;
    if (upload) e = hipMemcpyAsync(tmp, host, size_t(span) * es, hipMemcpyHostToDevice, c->stream);
    else if (span != ncols * int64_t(nlev)) // gaps in the user layout keep their contents
        e = hipMemcpyAsync(tmp, host, size_t(span) * es, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            launch_strided_copy<FT>(reinterpret_cast<FT*>(plane), c->stride, static_cast<FT*>(tmp), ls, cs, ncols, nlev, upload, c->stream);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess && !upload) e = hipMemcpyAsync(host, tmp, size_t(span) * es, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(c, LH_ENODEVICE, "transfer failed: %s", hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(c, LH_ENODEVICE, "transfer failed: %s", hipGetErrorString(e2));
    return LH_OK;
}

int lh_upload(lh_ctx* c, lh_state* s, int32_t var, const void* host, int64_t ls, int64_t cs) {
    return transfer(c, s, var, const_cast<void*>(host), ls, cs, true);
}

int lh_download(lh_ctx* c, const lh_state* s, int32_t var, void* host, int64_t ls, int64_t cs) {
    return transfer(c, const_cast<lh_state*>(s), var, host, ls, cs, false);
}

int lh_download_level(lh_ctx* c, const lh_state* s, int32_t var, int32_t level, void* host) {
    if (!c || !s || !host) return fail(c, LH_EINVAL, "lh_download_level: NULL argument");
    if (s->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if (var < 0 || var >= LH_NVARS || !(s->mask & (1u << var))) return fail(c, LH_ESTATE, "state has no variable %d", var);
    if (level < 0 || level >= c->cfg.nlev) return fail(c, LH_EINVAL, "lh_download_level: level %d outside [0, %d)", level, c->cfg.nlev);
    (void)hipSetDevice(c->device);
    {
        int rc = materialize(c, s, 1u << var);
        if (rc) return rc;
    }
    // a level of a plane is one contiguous row of ncols elements
    const char* row = static_cast<const char*>(s->plane[var]) + size_t(level) * size_t(c->stride) * c->esize;
    LH_HIP(c, hipMemcpyAsync(host, row, size_t(c->cfg.ncols) * c->esize, hipMemcpyDeviceToHost, c->stream));
    LH_HIP(c, hipStreamSynchronize(c->stream));
    return LH_OK;
}

int lh_state_fill(lh_ctx* c, lh_state* s, int32_t var, double value) {
    if (!c || !s) return fail(c, LH_EINVAL, "lh_state_fill: NULL argument");
    if (s->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if (var < 0 || var >= LH_NVARS || !(s->mask & (1u << var))) return fail(c, LH_ESTATE, "state has no variable %d", var);
    (void)hipSetDevice(c->device);
    const int64_t n = int64_t(c->cfg.nlev) * c->stride;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        launch_fill<FT>(static_cast<FT*>(s->plane[var]), n, FT(value), c->stream);
    });
    LH_HIP(c, hipGetLastError());
    mark_written(s, 1u << var);
    if (value == 0.0 && !std::signbit(value)) mark_zero(s, var);
    return LH_OK;
}

int lh_state_copy(lh_ctx* c, lh_state* dst, const lh_state* src) {
    if (!c || !dst || !src) return fail(c, LH_EINVAL, "lh_state_copy: NULL argument");
    if (dst->ctx != c || src->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if ((dst->mask & src->mask) != src->mask) return fail(c, LH_ESTATE, "lh_state_copy: destination lacks planes of the source");
    (void)hipSetDevice(c->device);
    const size_t bytes = size_t(c->cfg.nlev) * size_t(c->stride) * c->esize;
    int rc = materialize(c, src, ~0u); // (the copy carries planes, not profiles)
    if (rc) return rc;
    for (int i = 0; i < LH_NVARS; ++i)
        if (src->mask & (1u << i)) {
            LH_HIP(c, hipMemcpyAsync(dst->plane[i], src->plane[i], bytes, hipMemcpyDeviceToDevice, c->stream));
            mark_written(dst, 1u << i);
            if (src->zero_mask & (1u << i)) mark_zero(dst, i);
        }
    return LH_OK;
}

int lh_state_device_ptr(lh_ctx* c, const lh_state* s, int32_t var, void** dptr, int64_t* ls, int64_t* cs) {
    if (!c || !s || !dptr) return fail(c, LH_EINVAL, "lh_state_device_ptr: NULL argument");
    if (var < 0 || var >= LH_NVARS || !(s->mask & (1u << var))) return fail(c, LH_ESTATE, "state has no variable %d", var);
    (void)hipSetDevice(c->device);
    {
        int rc = materialize(c, s, 1u << var);
        if (rc) return rc;
    }
    *dptr = s->plane[var];
    // the caller may write through the pointer, now or later: nothing is assumed about this plane
    // until lh_state_release_ptr
    mark_written(const_cast<lh_state*>(s), 1u << var);
    const_cast<lh_state*>(s)->exposed_mask |= 1u << var;
    if (ls) *ls = c->stride;
    if (cs) *cs = 1;
    return LH_OK;
}

int lh_state_release_ptr(lh_ctx* c, lh_state* s, int32_t var) {
    if (!c || !s) return fail(c, LH_EINVAL, "lh_state_release_ptr: NULL argument");
    if (s->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if (var < -1 || var >= LH_NVARS) return fail(c, LH_EINVAL, "lh_state_release_ptr: bad variable %d", var);
    s->exposed_mask &= var < 0 ? 0u : ~(1u << var);
    return LH_OK;
}

int lh_upload_profile(lh_ctx* c, lh_state* s, int32_t var, const void* host) {
    if (!c || !s || !host) return fail(c, LH_EINVAL, "lh_upload_profile: NULL argument");
    if (s->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if (var < 0 || var >= LH_NVARS || !(s->mask & (1u << var))) return fail(c, LH_ESTATE, "state has no variable %d", var);
    (void)hipSetDevice(c->device);
    const int nlev = c->cfg.nlev;
    const size_t bytes = size_t(nlev) * c->esize;
    {   // an all-(+0) profile is a zero fill: the plane is then KNOWN to be zero (no ice: not even read)
        bool allzero = true;
        const unsigned char* b = static_cast<const unsigned char*>(host);
        for (size_t k = 0; k < bytes && allzero; ++k) allzero = b[k] == 0;
        if (allzero) return lh_state_fill(c, s, var, 0.0);
    }
    if (!s->profile[var]) LH_HIP(c, hipMalloc(&s->profile[var], bytes));
    // through a pinned staging ring, so that the copy is asynchronous and the call returns at once
    // (a time-dependent prescribed profile is refreshed at every stage: three uploads per step)
    if (!c->h_ring) {
        c->ring_bytes = size_t(1) << 18;
        if (c->ring_bytes < 4 * bytes) c->ring_bytes = 4 * bytes;
        LH_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_ring), c->ring_bytes, hipHostMallocDefault));
        c->ring_pos = 0;
    }
    const size_t need = (bytes + 255) & ~size_t(255);
    if (c->ring_pos + need > c->ring_bytes) { // wrap: every earlier copy out of the ring must have completed
        LH_HIP(c, hipStreamSynchronize(c->stream));
        c->ring_pos = 0;
    }
    memcpy(c->h_ring + c->ring_pos, host, bytes);
    LH_HIP(c, hipMemcpyAsync(s->profile[var], c->h_ring + c->ring_pos, bytes, hipMemcpyHostToDevice, c->stream));
    c->ring_pos += need;
    mark_written(s, 1u << var);
    s->profile_mask |= 1u << var;
    s->stale_mask |= 1u << var;
    return LH_OK;
}

int lh_coordinates(const lh_ctx* c, double* zc) {
    if (!c || !zc) return LH_EINVAL;
    memcpy(zc, c->zc_host.data(), c->zc_host.size() * sizeof(double));
    return LH_OK;
}

int lh_rhs(lh_ctx* c, double t, const lh_state* Y, const lh_state* Ya, lh_state* dY) {
    (void)t; // boundary/aux closures of t are evaluated by the host shim
    if (!c) return LH_EINVAL;
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = layered_check(c, "lh_rhs"))) return rc;
    const uint32_t pm = prognostic_mask(c->cfg.model);
    if ((rc = check_state(c, Y, pm, "Y"))) return rc;
    if ((rc = check_state(c, dY, pm, "dY"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    (void)hipSetDevice(c->device);
    return with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, nullptr, dY, 0.0, 0, nullptr); });
}

int lh_rhs_stable_dt(lh_ctx* c, double t, const lh_state* Y, const lh_state* Ya, lh_state* dY,
                     double courant, void* dt_device_ft) {
    (void)t;
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "lh_rhs_stable_dt: NULL argument");
    if (!(courant > 0)) return fail(c, LH_EINVAL, "lh_rhs_stable_dt: courant must be > 0");
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = layered_unsupported(c, "lh_rhs_stable_dt", "lh_layered_step_bound_device"))) return rc;
    const uint32_t pm = prognostic_mask(c->cfg.model);
    if ((rc = check_state(c, Y, pm, "Y"))) return rc;
    if ((rc = check_state(c, dY, pm, "dY"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    (void)hipSetDevice(c->device);
    rc = with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, nullptr, dY, courant, 4, nullptr, nullptr, dt_device_ft); });
    if (rc) return rc;
    return allreduce_min(c, dt_device_ft); // the global minimum when a communicator is attached
}

int lh_boundary_fluxes(lh_ctx* c, const lh_state* Y, const lh_state* Ya, double t, int32_t face, double* f_energy,
                       double* f_water) {
    (void)t; // boundary values of time t are set by the host shim (lh_set_bc) before the call, as for lh_rhs
    if (!c) return LH_EINVAL;
    if (face != LH_FACE_BOTTOM && face != LH_FACE_TOP) return fail(c, LH_EINVAL, "Expected :top or :bottom"); // boundary_conditions.jl:188
    if (!f_energy && !f_water) return fail(c, LH_EINVAL, "lh_boundary_fluxes: both outputs are NULL");
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = layered_check(c, "lh_boundary_fluxes"))) return rc;
    if ((rc = check_state(c, Y, prognostic_mask(c->cfg.model), "Y"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    (void)hipSetDevice(c->device);
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    Range r_("lh:boundary_fluxes");
    return with_ft(c, [&](auto ft) { return boundary_fluxes_impl<decltype(ft)>(c, Y, Ya, face, f_energy, f_water); });
}

int lh_diagnostics(lh_ctx* c, const lh_state* Y, const lh_state* Ya, lh_state* out) {
    if (!c) return LH_EINVAL;
    int rc;
    if (model_heat(c->cfg.model) && !c->hp.earth_set)
        return fail(c, LH_EINVAL, "earth parameters (lh_set_earth_params) are required by the energy model");
    if ((rc = check_state(c, Y, prognostic_mask(c->cfg.model), "Y"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    if ((rc = check_state(c, out, 0xFu, "diagnostic"))) return rc;
    if ((rc = layered_check(c, "lh_diagnostics"))) return rc;
    (void)hipSetDevice(c->device);
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (layered(c)) {
            layered_params<FT>(c, P);
            if (layered_heat(c))
                launch_layered_heat_diag<FT>(P, layered_heat_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), planes_of<FT>(out),
                                             c->cfg.model, c->stream);
            else
                launch_layered_diag<FT>(P, layered_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), planes_of<FT>(out), c->stream);
        } else
            launch_diag<FT>(P, planes_of<FT>(Y), planes_of<FT>(Ya), planes_of<FT>(out), any_percol(c), c->math, c->stream);
    });
    LH_HIP(c, hipGetLastError());
    mark_written(out, ~0u);
    return LH_OK;
}

int lh_step_engine(const lh_ctx* c, int64_t nsteps, int32_t per_stage_boundary_values) {
    if (!c || nsteps < 0) return LH_EINVAL;
    if (layered(c)) return use_layered_column_stepper(c) ? LH_ENGINE_COLUMN_STEPPER : LH_ENGINE_FUSED_STAGES;
    return use_column_stepper(c, nsteps, per_stage_boundary_values != 0) ? LH_ENGINE_COLUMN_STEPPER : LH_ENGINE_FUSED_STAGES;
}

int lh_closure_form(const lh_ctx* c) {
    if (!c) return LH_EINVAL;
    // (robust_vg_exists: only the Float64 production math of a model with water has two forms)
    if (c->cfg.dtype != LH_F64 || c->cfg.model == LH_MODEL_HEAT || c->math == MATH_LIBM) return LH_CLOSURE_NOT_APPLICABLE;
    return closure_integer_exponent(c) ? LH_CLOSURE_INTEGER_EXPONENT : LH_CLOSURE_LDEXP;
}

int lh_step_ssprk33(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                    const double* bcv) {
    (void)t;
    if (!c) return LH_EINVAL;
    if (nsteps < 0 || !(dt > 0)) return fail(c, LH_EINVAL, "lh_step_ssprk33: need nsteps >= 0 and dt > 0");
    Range r_("lh:step_ssprk33");
    int rc = stepping_preamble(c, Y, Ya);
    if (rc) return rc;
    if (layered(c)) {
        if ((rc = layered_check(c, "lh_step_ssprk33"))) return rc;
        // persist=2: all nsteps in one launch of the layered column stepper; otherwise
        // three unsegmented fused-stage launches per step, the stage state updated in place
        if (use_layered_column_stepper(c)) return run_layered_column_stepper(c, Y, Ya, dt, nsteps, bcv);
        lh_state* U1;
        if ((rc = stage_states(c, &U1, nullptr))) return rc;
        for (int64_t s = 0; s < nsteps; ++s)
            if ((rc = fused_ssprk33_step(c, Y, Ya, U1, U1, dt, nullptr, bcv ? bcv + s * 12 : nullptr))) return rc;
        return LH_OK;
    }
    // Default: all nsteps in ONE launch of the persistent column stepper (state in registers,
    // no plane traffic between stages or steps; column_stepper_kernel)
    if (use_column_stepper(c, nsteps, bcv != nullptr)) return run_column_stepper(c, Y, Ya, dt, nullptr, nsteps, bcv);
    lh_state *U1, *U2;
    if ((rc = stage_states(c, &U1, &U2))) return rc;
    auto one_step = [&](const double* bc3) { return fused_ssprk33_step(c, Y, Ya, U1, U2, dt, nullptr, bc3); };
    const int64_t done = bcv ? 0 : replay_step_graph(c, nsteps, one_step, &rc);
    if (rc) return rc;
    for (int64_t s = done; s < nsteps; ++s)
        if ((rc = one_step(bcv ? bcv + s * 12 : nullptr))) return rc;
    return LH_OK;
}

int lh_ssprk33_stage(lh_ctx* c, int32_t stage, lh_state* Y, lh_state* U, const lh_state* Ya, double dt,
                     const double* bc_values) {
    if (!c) return LH_EINVAL;
    if (stage < 1 || stage > 3) return fail(c, LH_EINVAL, "lh_ssprk33_stage: stage must be 1, 2 or 3");
    if (!(dt > 0)) return fail(c, LH_EINVAL, "lh_ssprk33_stage: need dt > 0");
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = layered_check(c, "lh_ssprk33_stage"))) return rc;
    const uint32_t pm = prognostic_mask(c->cfg.model);
    if ((rc = check_state(c, Y, pm, "Y"))) return rc;
    if ((rc = check_state(c, U, pm & ~LH_MASK(LH_VAR_THETA_I), "U"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    if (U == Y) return fail(c, LH_EINVAL, "lh_ssprk33_stage: U must not be Y");
    (void)hipSetDevice(c->device);
    // stage 1: U = Y + dt f(Y); 2: U = (3Y + U + dt f(U))/4; 3: Y = (Y + 2U + 2dt f(U))/3
    const lh_state* in = stage == 1 ? Y : U;
    lh_state* out = stage == 3 ? Y : U;
    return with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, in, Ya, Y, out, dt, stage, bc_values, nullptr, nullptr, true); });
}

int lh_step_ssprk33_device_dt(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t,
                              const void* dt_device_ft, const double* bcv) {
    (void)t;
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "lh_step_ssprk33_device_dt: NULL argument");
    int rc = stepping_preamble(c, Y, Ya);
    if (rc) return rc;
    if ((rc = layered_unsupported(c, "lh_step_ssprk33_device_dt", "lh_step_layered_ssprk33_device_dt"))) return rc;
    if (use_column_stepper(c, 1, bcv != nullptr)) return run_column_stepper(c, Y, Ya, 0.0, dt_device_ft, 1, bcv);
    lh_state *U1, *U2;
    if ((rc = stage_states(c, &U1, &U2))) return rc;
    return fused_ssprk33_step(c, Y, Ya, U1, U2, 0.0, dt_device_ft, bcv);
}

int lh_step_ssprk33_adaptive(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double courant, double dt_max,
                             int64_t nsteps, void* dt_device_ft, void* elapsed_device_ft) {
    (void)t;
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "lh_step_ssprk33_adaptive: NULL argument");
    if (nsteps < 0 || !(courant > 0)) return fail(c, LH_EINVAL, "lh_step_ssprk33_adaptive: need nsteps >= 0 and courant > 0");
    Range r_("lh:step_ssprk33_adaptive");
    int rc = stepping_preamble(c, Y, Ya);
    if (rc) return rc;
    if ((rc = layered_unsupported(c, "lh_step_ssprk33_adaptive", "lh_step_layered_ssprk33_adaptive_hold"))) return rc;
    if (!c->scratch_k1 && (rc = state_alloc(c, prognostic_mask(c->cfg.model), &c->scratch_k1))) return rc;
    lh_state* K1 = c->scratch_k1;
    // With a prescribed atmosphere the surface fluxes of a stage come from the stage state's top
    // cells, which MODE 5 never stores: that model takes the four-launch sequence.
    const bool three = !c->hp.atmos_on;
    lh_state *U1, *U2 = nullptr; // (the three-launch sequence has no second stage state)
    if ((rc = stage_states(c, &U1, three ? nullptr : &U2))) return rc;
    for (int64_t s = 0; s < nsteps; ++s) {
        // f(Y) and the step bound of Y in one launch; the global minimum with a communicator
        rc = with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, nullptr, K1, courant, 4, nullptr, nullptr, dt_device_ft); });
        if (rc) return rc;
        if ((rc = allreduce_min(c, dt_device_ft))) return rc;
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            launch_dt_prepare<FT>(static_cast<FT*>(dt_device_ft), FT(dt_max), static_cast<FT*>(elapsed_device_ft), c->d_status, c->stream);
        });
        if (three) {
            // stage 2 from (Y, k1): U1 = Y + dt k1 formed in registers; then stage 3
            rc = with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, K1, Ya, Y, U1, 0.0, 5, nullptr, dt_device_ft); });
            if (rc) return rc;
            rc = with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, U1, Ya, Y, Y, 0.0, 3, nullptr, dt_device_ft); });
            if (rc) return rc;
        } else if ((rc = fused_ssprk33_step(c, Y, Ya, U1, U2, 0.0, dt_device_ft, nullptr))) {
            return rc;
        }
    }
    LH_HIP(c, hipGetLastError());
    return LH_OK;
}

// The longest chunk (2^20 steps): the one-thread kernel between two chunks advances `elapsed` by `hold`
// successive additions, and one stepper launch runs `hold` steps -- both stay well inside a second.
static constexpr int32_t ADAPTIVE_HOLD_MAX = 1 << 20;

// One stepper launch per chunk: the stepper serves a call of `hold` steps and the column fits its wave form
static bool adaptive_hold_in_stepper(const lh_ctx* c, int32_t hold) {
    return use_column_stepper(c, hold, false) && c->cfg.nlev <= 128;
}

int lh_adaptive_hold_engine(const lh_ctx* c, int32_t hold) {
    if (!c || hold < 1 || hold > ADAPTIVE_HOLD_MAX) return LH_EINVAL;
    return adaptive_hold_in_stepper(c, hold) ? LH_ENGINE_COLUMN_STEPPER : LH_ENGINE_FUSED_STAGES;
}

int lh_step_ssprk33_adaptive_hold(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double courant, double dt_max,
                                  int64_t nchunks, int32_t hold, void* dt_device_ft, void* elapsed_device_ft) {
    (void)t;
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "lh_step_ssprk33_adaptive_hold: NULL argument");
    if (nchunks < 0 || hold < 1 || hold > ADAPTIVE_HOLD_MAX || !(courant > 0))
        return fail(c, LH_EINVAL, "lh_step_ssprk33_adaptive_hold: need nchunks >= 0, 1 <= hold <= %d and courant > 0", int(ADAPTIVE_HOLD_MAX));
    Range r_("lh:step_ssprk33_adaptive_hold");
    int rc = stepping_preamble(c, Y, Ya);
    if (rc) return rc;
    if ((rc = layered_unsupported(c, "lh_step_ssprk33_adaptive_hold", "lh_step_layered_ssprk33_adaptive_hold"))) return rc;
    if (nchunks == 0) return LH_OK;
    if (!c->scratch_k1 && (rc = state_alloc(c, prognostic_mask(c->cfg.model), &c->scratch_k1))) return rc;
    lh_state* K1 = c->scratch_k1; // the tendency the bound's launch writes with it: not used
    void* bound = c->d_dt;        // the bound of the current Y; dt_device_ft keeps the step of the chunk
    // f(Y) and the step bound of Y in one launch (rhs_kernel MODE 4)
    auto bound_of_Y = [&]() {
        return with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, nullptr, K1, courant, 4, nullptr, nullptr, bound); });
    };
    // the global minimum with a communicator; then the overrun check of the chunk that ended, the next dt, elapsed
    auto prepare = [&](int steps, bool check) -> int {
        if (int r = allreduce_min(c, bound)) return r;
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            launch_dt_hold_prepare<FT>(static_cast<FT*>(dt_device_ft), static_cast<const FT*>(bound), FT(dt_max),
                                       static_cast<FT*>(elapsed_device_ft), steps, check, c->d_status, c->stream);
        });
        return LH_OK;
    };
    if (adaptive_hold_in_stepper(c, hold)) {
        // the first bound from the tendency launch; every chunk's stepper launch leaves the next
        if ((rc = bound_of_Y())) return rc;
        for (int64_t k = 0; k < nchunks; ++k) {
            if ((rc = prepare(hold, k > 0))) return rc;
            if ((rc = run_column_stepper(c, Y, Ya, courant, dt_device_ft, hold, nullptr, bound))) return rc;
        }
    } else {
        lh_state *U1, *U2;
        if ((rc = stage_states(c, &U1, &U2))) return rc;
        for (int64_t k = 0; k < nchunks; ++k) {
            if ((rc = bound_of_Y()) || (rc = prepare(hold, k > 0))) return rc;
            for (int32_t s = 0; s < hold; ++s)
                if ((rc = fused_ssprk33_step(c, Y, Ya, U1, U2, 0.0, dt_device_ft, nullptr))) return rc;
        }
        if ((rc = bound_of_Y())) return rc; // the bound of the state the last chunk ended on
    }
    if ((rc = prepare(0, true))) return rc;
    LH_HIP(c, hipGetLastError());
    return LH_OK;
}

// ---- what the implicit entry points share on the host

static const char* const RICHARDS_MODELS = "Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)";
static const char* const COUPLED_MODELS = "coupled models only (SoilEnergyModel + SoilHydrologyModel)";

// The Newton calls (all but lh_step_heat_implicit) refuse the same configurations and states, in this order.  `who`:
// the entry point, for lh_last_error; `model`, `models`: the one model it steps and the words for it; `scalar`: NULL
// for a call that steps contexts without a class map, else (a layered call, which needs the map) the call that does
static int implicit_refusals(lh_ctx* c, const char* who, const lh_state* Y, const lh_state* Ya, int model, const char* models,
                             const char* scalar = nullptr) {
    if (c->cfg.model != model)
        return scalar && layered(c)
                   ? fail(c, LH_EMODEL, "%s is not available with soil classes (a class map is set) on this model: it steps %s", who, models)
                   : fail(c, LH_EMODEL, "%s: %s", who, models);
    if (scalar) {
        if (!layered(c))
            return fail(c, LH_EMODEL, "%s: the context has no class map (lh_set_soil_class_map); %s steps a model without soil classes",
                        who, scalar);
        if (int rc = layered_check(c, who)) return rc;
    } else if (int rc = layered_unsupported(c, who))
        return rc;
    if (c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE)
        return fail(c, LH_EMODEL, "%s: conductivity factors other than NoEffect are not supported", who);
    // (validate_model refuses a prescribed atmosphere on any model but the coupled one already; kept so
    // that this path stays closed to it should that change)
    if (c->hp.atmos_on) return fail(c, LH_EMODEL, "%s: a prescribed-atmosphere top is not supported", who);
    return stepping_preamble(c, Y, Ya);
}

// The two calls for a Richards context WITH conductivity factors refuse, in this order: any other
// model, a class map, a context whose factors are both NoEffect (`plain` serves it, as the layered calls send a context
// without a map to the scalar call), a prescribed atmosphere, and what stepping_preamble refuses
static int factors_implicit_refusals(lh_ctx* c, const char* who, const char* plain, const lh_state* Y, const lh_state* Ya) {
    if (c->cfg.model != LH_MODEL_RICHARDS) return fail(c, LH_EMODEL, "%s: %s", who, RICHARDS_MODELS);
    if (int rc = layered_unsupported(c, who)) return rc;
    if (c->hp.viscosity_kind == LH_FACTOR_NONE && c->hp.impedance_kind == LH_FACTOR_NONE)
        return fail(c, LH_EMODEL, "%s: the context has no conductivity factor other than NoEffect (lh_set_conductivity_factors); "
                                  "%s steps a model without conductivity factors", who, plain);
    if (c->hp.atmos_on) return fail(c, LH_EMODEL, "%s: a prescribed-atmosphere top is not supported", who);
    return stepping_preamble(c, Y, Ya);
}

// The call for a coupled context WITH the impedance factor refuses, in this order: any other model,
// a class map, a viscosity factor (the water would read the unknown T), a context without the impedance factor (`plain`
// serves it), a prescribed atmosphere, and what stepping_preamble refuses
static int coupled_factors_implicit_refusals(lh_ctx* c, const char* who, const char* plain, const lh_state* Y, const lh_state* Ya) {
    if (c->cfg.model != LH_MODEL_COUPLED) return fail(c, LH_EMODEL, "%s: %s", who, COUPLED_MODELS);
    if (int rc = layered_unsupported(c, who)) return rc;
    if (c->hp.viscosity_kind != LH_FACTOR_NONE)
        return fail(c, LH_EMODEL, "%s: a viscosity factor other than NoEffect is not supported: the water then reads the unknown T "
                                  "and the stage is no longer block triangular", who);
    if (c->hp.impedance_kind == LH_FACTOR_NONE)
        return fail(c, LH_EMODEL, "%s: the context has no impedance factor (lh_set_conductivity_factors); "
                                  "%s steps a model without conductivity factors", who, plain);
    if (c->hp.atmos_on) return fail(c, LH_EMODEL, "%s: a prescribed-atmosphere top is not supported", who);
    return stepping_preamble(c, Y, Ya);
}

// ---- adaptive SSPRK33 for layered Richards soils: the BOUND flavour of the layered column
// stepper is their one engine, so they do not consult `persist` -- that key chooses where there are two engines

// What the three calls refuse, in this order.  `scalar`: the call that serves a context without a class map
static int layered_adaptive_refusals(lh_ctx* c, const char* who, const char* scalar, const lh_state* Y, const lh_state* Ya) {
    if (c->cfg.model != LH_MODEL_RICHARDS)
        return layered(c) ? fail(c, LH_EMODEL, "%s is not available with soil classes (a class map is set) on this model: it steps %s",
                                 who, RICHARDS_MODELS)
                          : fail(c, LH_EMODEL, "%s: %s", who, RICHARDS_MODELS);
    if (!layered(c))
        return fail(c, LH_EMODEL, "%s: the context has no class map (lh_set_soil_class_map); %s serves a model without soil classes",
                    who, scalar);
    if (int rc = layered_check(c, who)) return rc;
    if (c->cfg.nlev > 128)
        return fail(c, LH_EMODEL, "%s: columns of more than 128 levels are not supported (this context has %d): one wave holds a column",
                    who, int(c->cfg.nlev));
    if (c->hp.atmos_on) return fail(c, LH_EMODEL, "%s: a prescribed-atmosphere top is not supported", who);
    return stepping_preamble(c, Y, Ya);
}

int lh_layered_step_bound_device(lh_ctx* c, const lh_state* Y, const lh_state* Ya, double courant, void* dt_device_ft) {
    static const char* const who = "lh_layered_step_bound_device";
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "%s: NULL argument", who);
    if (!(courant > 0)) return fail(c, LH_EINVAL, "%s: need courant > 0", who);
    if (int rc = layered_adaptive_refusals(c, who, "lh_rhs_stable_dt", Y, Ya)) return rc;
    // a zero-step launch: the prologue and the bound epilogue, no plane of Y written (so the const is kept in effect);
    // the step word it reads and does not use is the context's own
    if (int rc = run_layered_column_stepper(c, const_cast<lh_state*>(Y), Ya, courant, 0, nullptr, c->d_dt, dt_device_ft)) return rc;
    return allreduce_min(c, dt_device_ft); // the global minimum when a communicator is attached
}

int lh_step_layered_ssprk33_device_dt(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, const void* dt_device_ft,
                                      int64_t nsteps, const double* bcv) {
    (void)t;
    static const char* const who = "lh_step_layered_ssprk33_device_dt";
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "%s: NULL argument", who);
    if (nsteps < 0) return fail(c, LH_EINVAL, "%s: need nsteps >= 0", who);
    if (int rc = layered_adaptive_refusals(c, who, "lh_step_ssprk33_device_dt", Y, Ya)) return rc;
    if (nsteps == 0) return LH_OK;
    // the BOUND flavour is the one kernel that reads its step from device memory: the bound it leaves (under a
    // Courant factor of 1) goes to the context's own word and is discarded
    return run_layered_column_stepper(c, Y, Ya, 1.0, nsteps, bcv, dt_device_ft, c->d_dt);
}

int lh_step_layered_ssprk33_adaptive_hold(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double courant, double dt_max,
                                          int64_t nchunks, int32_t hold, void* dt_device_ft, void* elapsed_device_ft) {
    (void)t;
    static const char* const who = "lh_step_layered_ssprk33_adaptive_hold";
    if (!c || !dt_device_ft) return fail(c, LH_EINVAL, "%s: NULL argument", who); // (elapsed may be NULL, as in the scalar call)
    if (nchunks < 0 || hold < 1 || hold > ADAPTIVE_HOLD_MAX || !(courant > 0))
        return fail(c, LH_EINVAL, "%s: need nchunks >= 0, 1 <= hold <= %d and courant > 0", who, int(ADAPTIVE_HOLD_MAX));
    Range r_("lh:step_layered_ssprk33_adaptive_hold");
    if (int rc = layered_adaptive_refusals(c, who, "lh_step_ssprk33_adaptive_hold", Y, Ya)) return rc;
    if (nchunks == 0) return LH_OK;
    int rc;
    void* bound = c->d_dt; // the bound of the current Y; dt_device_ft keeps the step of the chunk
    // (lh_step_ssprk33_adaptive_hold's: the global minimum, the overrun check of the chunk that ended, the next dt, elapsed)
    auto prepare = [&](int steps, bool check) -> int {
        if (int r = allreduce_min(c, bound)) return r;
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            launch_dt_hold_prepare<FT>(static_cast<FT*>(dt_device_ft), static_cast<const FT*>(bound), FT(dt_max),
                                       static_cast<FT*>(elapsed_device_ft), steps, check, c->d_status, c->stream);
        });
        return LH_OK;
    };
    // the first bound from a zero-step launch; every chunk's launch of `hold` steps leaves the next
    if ((rc = run_layered_column_stepper(c, Y, Ya, courant, 0, nullptr, dt_device_ft, bound))) return rc;
    for (int64_t k = 0; k < nchunks; ++k) {
        if ((rc = prepare(hold, k > 0))) return rc;
        if ((rc = run_layered_column_stepper(c, Y, Ya, courant, hold, nullptr, dt_device_ft, bound))) return rc;
    }
    if ((rc = prepare(0, true))) return rc;
    LH_HIP(c, hipGetLastError());
    return LH_OK;
}

// The helpers below take the buffer's name and size as the entry points write them (`name`, `size`), so that a
// failure reads in lh_last_error as the call on that buffer: "hipMalloc(&c->d_tr, 6 * plane) failed: ..."
static int named_status(lh_ctx* c, hipError_t e, const char* fmt, const char* name, const char* size) {
    char call[160];
    snprintf(call, sizeof call, fmt, name, size);
    return hip_status(c, e, call);
}
// A statistics block describes one call from its first line on, also when the call is refused: zeroed
// here if it exists ...
static int zero_stats(lh_ctx* c, void* d_stats, size_t bytes, const char* name, const char* size) {
    if (!d_stats) return LH_OK;
    return named_status(c, hipMemsetAsync(d_stats, 0, bytes, c->stream), "hipMemsetAsync(%s, 0, %s, c->stream)", name, size);
}
// ... and allocated (zeroed) on the first call that gets as far as needing it, like the scratch planes
static int ensure_scratch(lh_ctx* c, void** slot, size_t bytes, const char* name, const char* size, bool zeroed = false) {
    if (*slot) return LH_OK;
    if (int rc = named_status(c, hipMalloc(slot, bytes), "hipMalloc(&%s, %s)", name, size)) return rc;
    return zeroed ? zero_stats(c, *slot, bytes, name, size) : LH_OK;
}
// ... and read back: zeros before the first call
static int read_stats(lh_ctx* c, const void* d_stats, void* host, size_t bytes, const char* name) {
    memset(host, 0, bytes);
    if (!d_stats) return LH_OK;
    (void)hipSetDevice(c->device);
    if (int rc = named_status(c, hipMemcpyAsync(host, d_stats, bytes, hipMemcpyDeviceToHost, c->stream),
                              "hipMemcpyAsync(host, %s, %s, hipMemcpyDeviceToHost, c->stream)", name, "bytes"))
        return rc;
    LH_HIP(c, hipStreamSynchronize(c->stream));
    return LH_OK;
}
// theta_i known zero (the state's zero bits): the kernels that do not read the plane
static bool implicit_noice(const lh_ctx* c, const lh_state* Y) {
    return c->tune.zero != 0 && (Y->zero_mask & LH_MASK(LH_VAR_THETA_I));
}

// lh_step_implicit_euler's Newton test where the caller passes none (tol <= 0, max_iter <= 0): also
// lh_step_coupled_implicit's, and the fixed mode of the TR-BDF2 calls
static void newton_defaults(const lh_ctx* c, double& tol, int32_t& max_iter) {
    if (!(tol > 0)) tol = c->cfg.dtype == LH_F64 ? 1e-10 : 1e-5;
    if (max_iter <= 0) max_iter = 50;
}
// the argument checks of lh_step_heat_implicit and lh_step_coupled_implicit (`allowed`: the call's TR-BDF2 flag)
static int fixed_step_argument_refusals(lh_ctx* c, const char* who, int64_t nsteps, double dt, uint32_t flags, uint32_t allowed) {
    if (nsteps < 0 || !std::isfinite(dt) || !(dt > 0)) return fail(c, LH_EINVAL, "%s: need nsteps >= 0 and a finite dt > 0", who);
    if (flags & ~allowed) return fail(c, LH_EINVAL, "%s: unknown flags 0x%x", who, flags);
    return LH_OK;
}
// ... and the coefficient of their stage solves: dt (backward Euler) or (2 - sqrt 2)/2 dt (both TR-BDF2 stages)
static double stage_coefficient(bool trbdf2, double dt) { return trbdf2 ? 0.5 * (2.0 - 1.4142135623730951) * dt : dt; }
// The last line of every implicit call: the fixed-step ones hand it launch_error(c, d_bcv), the adaptive ones (which
// upload no table) hipGetLastError(); `launch` names the launch in lh_last_error
static int launch_status(lh_ctx* c, hipError_t e, const char* launch) {
    return e == hipSuccess ? LH_OK : fail(c, LH_ENODEVICE, "%s launch failed: %s", launch, hipGetErrorString(e));
}

// The two Richards calls exist three times, for contexts without and with a class map (lh_implicit.hpp,
// lh_layered_implicit.hpp) and for contexts with conductivity factors (lh_factors_implicit.hpp;
// DESIGN section 4.32), on the same scratch and statistics blocks.  One body each; what a
// layered entry point words or does differently is its flavour: besides the names below, implicit_refusals' list for
// a context that must hold a map, layered_params, and the launcher that takes layered_args.  The factors flavour has
// its own refusals (factors_implicit_refusals), hands the kernels Ya's prescribed T (factors_temperature) and takes
// lh_factors_implicit.hpp's launchers.
struct RichardsFlavour {
    const char* who;    // the entry point, for lh_last_error
    const char* scalar; // a layered call: the call for a context without a class map; NULL for that call itself
    const char* range;  // the roctx range
    const char* launch; // the launch, in the words of its failure message
    const char* plain = nullptr; // a factors call: the call for a context whose factors are both NoEffect
    bool layered() const { return scalar != nullptr; }
    bool factors() const { return plain != nullptr; }
};
static int richards_refusals(lh_ctx* c, const RichardsFlavour& fl, const lh_state* Y, const lh_state* Ya) {
    if (fl.factors()) return factors_implicit_refusals(c, fl.who, fl.plain, Y, Ya);
    return implicit_refusals(c, fl.who, Y, Ya, LH_MODEL_RICHARDS, RICHARDS_MODELS, fl.scalar);
}
// The prescribed T a factors launch reads: Ya's planes made current but for a T that comes as a level-uniform profile
// (which goes to the kernel as it is, set_aux_profiles); nothing where no viscosity factor reads a temperature
static int factors_temperature(lh_ctx* c, const lh_state* Ya) {
    if (c->hp.viscosity_kind == LH_FACTOR_NONE) return LH_OK;
    return materialize(c, Ya, ~aux_profile_vars(c, Ya));
}
// ... and its plane: NULL where a profile stands for it (set_aux_profiles hands that over) or nothing reads it
static const void* factors_temperature_plane(const lh_ctx* c, const lh_state* Ya) {
    if (c->hp.viscosity_kind == LH_FACTOR_NONE || (aux_profile_vars(c, Ya) & LH_MASK(LH_VAR_T))) return nullptr;
    return Ya->plane[LH_VAR_T];
}

static int richards_implicit_euler(lh_ctx* c, const RichardsFlavour& fl, lh_state* Y, const lh_state* Ya, double dt,
                                   int64_t nsteps, const double* bcv, double tol, int32_t max_iter) {
    if (!c) return LH_EINVAL;
    int rc = zero_stats(c, c->d_imp_stats, sizeof(ImplicitStats), "c->d_imp_stats", "24");
    if (rc) return rc;
    if (nsteps < 0 || !(dt > 0)) return fail(c, LH_EINVAL, "%s: need nsteps >= 0 and dt > 0", fl.who);
    Range r_(fl.range);
    if ((rc = richards_refusals(c, fl, Y, Ya))) return rc;
    newton_defaults(c, tol, max_iter);
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_imp, 3 * pl * c->esize, "c->d_imp", "3 * plane"))) return rc;
    if ((rc = ensure_scratch(c, &c->d_imp_stats, sizeof(ImplicitStats), "c->d_imp_stats", "24", true))) return rc;
    if (nsteps == 0) return LH_OK;
    if ((rc = materialize(c, Y, ~0u))) return rc;
    if (fl.factors() && (rc = factors_temperature(c, Ya))) return rc;
    DeviceBuffer d_bcv; // [nsteps][2][2] doubles -> FT on the device
    if (bcv && (rc = upload_boundary_values(c, bcv, size_t(nsteps) * 4, d_bcv))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        ImplicitArgs<FT> A;
        point_at_water<FT>(Y, A);
        carve_planes<FT>(c->d_imp, pl, {&A.yn, &A.cp, &A.dp});
        A.bcv = static_cast<const FT*>(d_bcv.p);
        A.dt = FT(dt);
        A.tol = FT(tol);
        A.max_iter = max_iter;
        A.nsteps = nsteps;
        point_at_newton_stats(c, A);
        if (fl.factors()) {
            set_aux_profiles<FT>(c, Ya, P);
            launch_factors_implicit_euler<FT>(P, A, static_cast<const FT*>(factors_temperature_plane(c, Ya)), any_percol(c), c->math,
                                              c->stream);
        } else if (fl.layered()) launch_layered_implicit_euler<FT>(P, layered_args<FT>(c), A, implicit_noice(c, Y), c->stream);
        else launch_implicit_euler<FT>(P, A, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
    });
    mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L));
    return launch_status(c, launch_error(c, d_bcv), fl.launch);
}

int lh_step_implicit_euler(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                           const double* bcv, double tol, int32_t max_iter) {
    (void)t; // boundary values of t_{n+1} come through bcv or lh_set_bc, as for lh_step_ssprk33
    static const RichardsFlavour fl = {"lh_step_implicit_euler", nullptr, "lh:step_implicit_euler", "implicit Euler"};
    return richards_implicit_euler(c, fl, Y, Ya, dt, nsteps, bcv, tol, max_iter);
}

int lh_step_layered_implicit_euler(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                                   const double* bcv, double tol, int32_t max_iter) {
    (void)t; // as for lh_step_implicit_euler
    static const RichardsFlavour fl = {"lh_step_layered_implicit_euler", "lh_step_implicit_euler",
                                       "lh:step_layered_implicit_euler", "layered implicit Euler"};
    return richards_implicit_euler(c, fl, Y, Ya, dt, nsteps, bcv, tol, max_iter);
}

int lh_step_factors_implicit_euler(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                                   const double* bcv, double tol, int32_t max_iter) {
    (void)t; // as for lh_step_implicit_euler
    static const RichardsFlavour fl = {"lh_step_factors_implicit_euler", nullptr, "lh:step_factors_implicit_euler",
                                       "factors implicit Euler", "lh_step_implicit_euler"};
    return richards_implicit_euler(c, fl, Y, Ya, dt, nsteps, bcv, tol, max_iter);
}

int lh_implicit_iterations(lh_ctx* c, int64_t* iterations) {
    if (!c || !iterations) return fail(c, LH_EINVAL, "lh_implicit_iterations: NULL argument");
    ImplicitStats st;
    const int rc = read_stats(c, c->d_imp_stats, &st, sizeof st, "c->d_imp_stats");
    *iterations = int64_t(st.total_iters);
    return rc;
}

int lh_implicit_stats(lh_ctx* c, int32_t* max_iters, int64_t* unconverged) {
    if (!c || !max_iters || !unconverged) return fail(c, LH_EINVAL, "lh_implicit_stats: NULL argument");
    ImplicitStats st;
    const int rc = read_stats(c, c->d_imp_stats, &st, sizeof st, "c->d_imp_stats");
    *max_iters = st.max_iters;
    *unconverged = int64_t(st.unconverged);
    return rc;
}

static const size_t TRBDF2_STATS_BYTES = LH_TRBDF2_NSTATS * sizeof(uint64_t);

// The argument checks of the three adaptive calls, in this order.  `tols`: every tolerance the call takes; `allowed`:
// the flags it knows (lh_integrate_coupled_trbdf2: none, its fixed steps are lh_step_coupled_implicit's LH_COUPLED_TRBDF2)
static int trbdf2_argument_refusals(lh_ctx* c, const char* who, double t0, double t1, double dt, std::initializer_list<double> tols,
                                    uint32_t flags, uint32_t allowed, const double* bcv) {
    if (!std::isfinite(t0) || !std::isfinite(t1) || !(t1 >= t0)) return fail(c, LH_EINVAL, "%s: need finite t0 <= t1", who);
    if (!std::isfinite(dt) || !(dt > 0)) return fail(c, LH_EINVAL, "%s: need a finite dt > 0", who);
    for (const double tol : tols)
        if (!std::isfinite(tol) || tol < 0) return fail(c, LH_EINVAL, "%s: tolerances must be finite and >= 0", who);
    if (flags & ~allowed) return fail(c, LH_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (bcv)
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(bcv[k])) return fail(c, LH_EINVAL, "%s: non-finite boundary value", who);
    return LH_OK;
}
// each tolerance that is 0 takes its own default (OrdinaryDiffEq's)
static void trbdf2_tolerance_defaults(double& abstol, double& reltol) {
    if (!(abstol > 0)) abstol = LH_TRBDF2_ABSTOL_DEFAULT;
    if (!(reltol > 0)) reltol = LH_TRBDF2_RELTOL_DEFAULT;
}

static int richards_trbdf2(lh_ctx* c, const RichardsFlavour& fl, lh_state* Y, const lh_state* Ya, double t0, double t1,
                           double dt, double abstol, double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    if (!c) return LH_EINVAL;
    int rc = zero_stats(c, c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat");
    if (rc) return rc;
    if ((rc = trbdf2_argument_refusals(c, fl.who, t0, t1, dt, {abstol, reltol}, flags, LH_TRBDF2_FIXED, bcv))) return rc;
    Range r_(fl.range);
    if ((rc = richards_refusals(c, fl, Y, Ya))) return rc;
    trbdf2_tolerance_defaults(abstol, reltol);
    double tol = 0; // (fixed mode: lh_step_implicit_euler's defaults)
    int32_t max_iter = 0;
    newton_defaults(c, tol, max_iter);
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_tr, 6 * pl * c->esize, "c->d_tr", "6 * plane"))) return rc;
    if ((rc = ensure_scratch(c, &c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat", true))) return rc;
    if (t1 == t0) return LH_OK;
    if ((rc = materialize(c, Y, ~0u))) return rc;
    if (fl.factors() && (rc = factors_temperature(c, Ya))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        Trbdf2Args<FT> A;
        point_at_water<FT>(Y, A);
        carve_planes<FT>(c->d_tr, pl, {&A.yn, &A.fn, &A.yg, &A.w, &A.cp, &A.dp});
        fill_trbdf2_args<FT>(c, A, t0, t1, dt, abstol, reltol, dt_cols_device_ft, bcv);
        A.fixed = (flags & LH_TRBDF2_FIXED) != 0;
        A.tol = FT(tol);
        A.max_iter = max_iter;
        if (fl.factors()) {
            set_aux_profiles<FT>(c, Ya, P);
            launch_factors_trbdf2<FT>(P, A, static_cast<const FT*>(factors_temperature_plane(c, Ya)), any_percol(c), c->math, c->stream);
        } else if (fl.layered()) launch_layered_trbdf2<FT>(P, layered_args<FT>(c), A, implicit_noice(c, Y), c->stream);
        else launch_trbdf2<FT>(P, A, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
    });
    mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L));
    return launch_status(c, hipGetLastError(), fl.launch);
}

int lh_integrate_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt, double abstol,
                        double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const RichardsFlavour fl = {"lh_integrate_trbdf2", nullptr, "lh:integrate_trbdf2", "TR-BDF2"};
    return richards_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, reltol, flags, dt_cols_device_ft, bcv);
}

int lh_integrate_layered_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt, double abstol,
                                double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const RichardsFlavour fl = {"lh_integrate_layered_trbdf2", "lh_integrate_trbdf2", "lh:integrate_layered_trbdf2",
                                       "layered TR-BDF2"};
    return richards_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, reltol, flags, dt_cols_device_ft, bcv);
}

int lh_integrate_factors_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt, double abstol,
                                double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const RichardsFlavour fl = {"lh_integrate_factors_trbdf2", nullptr, "lh:integrate_factors_trbdf2", "factors TR-BDF2",
                                       "lh_integrate_trbdf2"};
    return richards_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, reltol, flags, dt_cols_device_ft, bcv);
}

int lh_trbdf2_stats(lh_ctx* c, int64_t* stats) {
    if (!c || !stats) return fail(c, LH_EINVAL, "lh_trbdf2_stats: NULL argument");
    uint64_t u[LH_TRBDF2_NSTATS];
    const int rc = read_stats(c, c->d_tr_stats, u, sizeof u, "c->d_tr_stats");
    for (int k = 0; k < LH_TRBDF2_NSTATS; ++k) stats[k] = int64_t(u[k]);
    return rc;
}

// The heat-only call exists twice, for contexts without and with a class map (lh_heat_implicit.hpp,
// lh_layered_heat_implicit.hpp), on the same scratch planes and table of boundary values.  One
// body; what the layered entry point words or does differently is its flavour (RichardsFlavour's fields): the refusal
// of a context WITHOUT a map and layered_check where the scalar call refuses a map, layered_params, and the launcher
// that takes layered_heat_args.
using HeatFlavour = RichardsFlavour;

static int heat_implicit_steps(lh_ctx* c, const HeatFlavour& fl, lh_state* Y, const lh_state* Ya, double dt, int64_t nsteps,
                               uint32_t flags, const double* bcv) {
    if (!c) return LH_EINVAL;
    const char* const who = fl.who;
    int rc = fixed_step_argument_refusals(c, who, nsteps, dt, flags, LH_HEAT_TRBDF2);
    if (rc) return rc;
    Range r_(fl.range);
    // (its own order, not implicit_refusals': the model, the states, then the class map)
    if (c->cfg.model != LH_MODEL_HEAT) return fail(c, LH_EMODEL, "%s: heat-only models (SoilEnergyModel + PrescribedHydrologyModel)", who);
    if ((rc = stepping_preamble(c, Y, Ya))) return rc;
    if (!fl.layered()) {
        if ((rc = layered_unsupported(c, who))) return rc;
    } else {
        if (!layered(c))
            return fail(c, LH_EMODEL, "%s: the context has no class map (lh_set_soil_class_map); %s steps a model without soil classes",
                        who, fl.scalar);
        if ((rc = layered_check(c, who))) return rc;
    }
    if (nsteps == 0) return LH_OK;
    const bool trbdf2 = (flags & LH_HEAT_TRBDF2) != 0;
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_heat, 8 * pl * c->esize, "c->d_heat", "8 * plane"))) return rc;
    // (level-uniform variables of Ya become planes: the prologue reads each cell once)
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    DeviceBuffer d_bcv; // [nsteps + 1][2][2] doubles -> FT on the device
    if (bcv && (rc = upload_boundary_values(c, bcv, size_t(nsteps + 1) * 4, d_bcv))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        HeatImplicitArgs<FT> A;
        A.y = static_cast<FT*>(Y->plane[LH_VAR_RHOE_INT]);
        A.vl = static_cast<const FT*>(Ya->plane[LH_VAR_VARTHETA_L]);
        A.ti = static_cast<const FT*>(Ya->plane[LH_VAR_THETA_I]);
        carve_planes<FT>(c->d_heat, pl, {&A.a, &A.iden, &A.cp, &A.kc, &A.z, &A.ks, &A.al, &A.be});
        A.bcv = static_cast<const FT*>(d_bcv.p);
        A.coef = FT(stage_coefficient(trbdf2, dt));
        A.nsteps = nsteps;
        if (fl.layered()) launch_layered_heat_implicit<FT>(P, layered_heat_args<FT>(c), A, trbdf2, c->stream);
        else launch_heat_implicit<FT>(P, A, any_percol(c), trbdf2, c->math, c->stream);
    });
    mark_written(Y, LH_MASK(LH_VAR_RHOE_INT));
    return launch_status(c, launch_error(c, d_bcv), fl.launch);
}

int lh_step_heat_implicit(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                          uint32_t flags, const double* bcv) {
    (void)t; // boundary values come through bcv or lh_set_bc, as for lh_step_implicit_euler
    static const HeatFlavour fl = {"lh_step_heat_implicit", nullptr, "lh:step_heat_implicit", "heat implicit"};
    return heat_implicit_steps(c, fl, Y, Ya, dt, nsteps, flags, bcv);
}

int lh_step_layered_heat_implicit(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                                  uint32_t flags, const double* bcv) {
    (void)t; // as for lh_step_heat_implicit
    static const HeatFlavour fl = {"lh_step_layered_heat_implicit", "lh_step_heat_implicit", "lh:step_layered_heat_implicit",
                                   "layered heat implicit"};
    return heat_implicit_steps(c, fl, Y, Ya, dt, nsteps, flags, bcv);
}

// The coupled call exists three times, for contexts without and with a class map (lh_coupled_implicit.hpp,
// lh_layered_coupled_implicit.hpp) and for contexts with the impedance factor
// (lh_coupled_factors_implicit.hpp), on the same scratch planes, statistics block and table of
// boundary values.  One body; what the layered entry point words or does differently is its flavour (a RichardsFlavour:
// the fields are the same): implicit_refusals' list for a context that must hold a map, layered_params, and the launcher
// that takes layered_heat_args.  The factors flavour has its own refusals (coupled_factors_implicit_refusals) and its
// own launcher, which has no NOICE variant.
static int coupled_implicit_steps(lh_ctx* c, const RichardsFlavour& fl, lh_state* Y, const lh_state* Ya, double dt,
                                  int64_t nsteps, uint32_t flags, const double* bcv, double tol, int32_t max_iter) {
    if (!c) return LH_EINVAL;
    const char* const who = fl.who;
    int rc = zero_stats(c, c->d_imp_stats, sizeof(ImplicitStats), "c->d_imp_stats", "24");
    if (rc) return rc;
    if ((rc = fixed_step_argument_refusals(c, who, nsteps, dt, flags, LH_COUPLED_TRBDF2))) return rc;
    Range r_(fl.range);
    // (with a viscosity factor the water reads T: the Jacobian is no longer block triangular)
    if ((rc = fl.factors() ? coupled_factors_implicit_refusals(c, who, fl.plain, Y, Ya)
                           : implicit_refusals(c, who, Y, Ya, LH_MODEL_COUPLED, COUPLED_MODELS, fl.scalar)))
        return rc;
    newton_defaults(c, tol, max_iter);
    const bool trbdf2 = (flags & LH_COUPLED_TRBDF2) != 0;
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_imp_stats, sizeof(ImplicitStats), "c->d_imp_stats", "24", true))) return rc;
    if (nsteps == 0) return LH_OK;
    if ((rc = ensure_scratch(c, &c->d_cpl, 3 * pl * c->esize, "c->d_cpl", "3 * plane"))) return rc;
    if (trbdf2 && (rc = ensure_scratch(c, &c->d_cpl_tr, 4 * pl * c->esize, "c->d_cpl_tr", "4 * plane"))) return rc;
    if ((rc = materialize(c, Y, ~0u))) return rc;
    DeviceBuffer d_bcv; // [nsteps + 1][2][2] doubles -> FT on the device
    if (bcv && (rc = upload_boundary_values(c, bcv, size_t(nsteps + 1) * 4, d_bcv))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        CoupledImplicitArgs<FT> A;
        point_at_water<FT>(Y, A);
        A.e = static_cast<FT*>(Y->plane[LH_VAR_RHOE_INT]);
        carve_planes<FT>(c->d_cpl, pl, {&A.w, &A.cp, &A.dp});
        A.yn = A.fn = A.fe = A.we = nullptr;
        if (trbdf2) carve_planes<FT>(c->d_cpl_tr, pl, {&A.yn, &A.fn, &A.fe, &A.we});
        A.bcv = static_cast<const FT*>(d_bcv.p);
        A.coef = FT(stage_coefficient(trbdf2, dt));
        A.tol = FT(tol);
        A.max_iter = max_iter;
        A.nsteps = nsteps;
        point_at_newton_stats(c, A);
        if (fl.factors())
            launch_coupled_factors_implicit<FT>(P, A, any_percol(c), trbdf2, c->math, c->stream);
        else if (fl.layered())
            launch_layered_coupled_implicit<FT>(P, layered_heat_args<FT>(c), A, implicit_noice(c, Y), trbdf2, c->stream);
        else
            launch_coupled_implicit<FT>(P, A, any_percol(c), implicit_noice(c, Y), trbdf2, c->math, c->stream);
    });
    mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_RHOE_INT));
    return launch_status(c, launch_error(c, d_bcv), fl.launch);
}

int lh_step_coupled_implicit(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                             uint32_t flags, const double* bcv, double tol, int32_t max_iter) {
    (void)t; // boundary values come through bcv or lh_set_bc, as for lh_step_heat_implicit
    static const RichardsFlavour fl = {"lh_step_coupled_implicit", nullptr, "lh:step_coupled_implicit", "coupled implicit"};
    return coupled_implicit_steps(c, fl, Y, Ya, dt, nsteps, flags, bcv, tol, max_iter);
}

int lh_step_layered_coupled_implicit(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                                     uint32_t flags, const double* bcv, double tol, int32_t max_iter) {
    (void)t; // as for lh_step_coupled_implicit
    static const RichardsFlavour fl = {"lh_step_layered_coupled_implicit", "lh_step_coupled_implicit",
                                      "lh:step_layered_coupled_implicit", "layered coupled implicit"};
    return coupled_implicit_steps(c, fl, Y, Ya, dt, nsteps, flags, bcv, tol, max_iter);
}

int lh_step_coupled_factors_implicit(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t, double dt, int64_t nsteps,
                                     uint32_t flags, const double* bcv, double tol, int32_t max_iter) {
    (void)t; // as for lh_step_coupled_implicit
    static const RichardsFlavour fl = {"lh_step_coupled_factors_implicit", nullptr, "lh:step_coupled_factors_implicit",
                                       "coupled factors implicit", "lh_step_coupled_implicit"};
    return coupled_implicit_steps(c, fl, Y, Ya, dt, nsteps, flags, bcv, tol, max_iter);
}

// ---- what the boundary-value-series entry points share (lh_series.hpp; DESIGN sections 4.21 and 4.28)

static bool series_of(const lh_ctx* c, const lh_bc_series* s) {
    for (const lh_bc_series* k : c->series)
        if (k == s) return true;
    return false;
}

static int series_handle_refusals(lh_ctx* c, const char* who, const lh_bc_series* sr) {
    if (!sr) return fail(c, LH_EINVAL, "%s: the series is NULL", who);
    if (!series_of(c, sr)) return fail(c, LH_EINVAL, "%s: not a series of this context", who);
    return LH_OK;
}

static int series_span_refusal(lh_ctx* c, const char* who, const lh_bc_series* sr, double t0, double t1) {
    if (t0 < sr->times.front() || t1 > sr->times.back())
        return fail(c, LH_EINVAL, "%s: [t0, t1] = [%g, %g] leaves the series' knots [%g, %g] (no extrapolation)", who, t0, t1,
                    sr->times.front(), sr->times.back());
    return LH_OK;
}

// A series on a component the model does not have, or on a (face, component) whose kind reads no value.  A heat-only
// model has no hydrology boundary condition whose kind could be asked: its hydrology series are refused last, as such
static int series_kind_refusals(lh_ctx* c, const char* who, const lh_bc_series* sr) {
    const int model = c->cfg.model;
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k) {
            if (!sr->d_val[f][k]) continue;
            const char* fn = f == LH_FACE_TOP ? "top" : "bottom";
            if (k == LH_COMP_ENERGY && model == LH_MODEL_RICHARDS)
                return fail(c, LH_EMODEL, "%s: the series has %s energy values, and a Richards model has no energy component", who, fn);
            if (k == LH_COMP_HYDROLOGY && model == LH_MODEL_HEAT) continue;
            const int kind = c->hp.bc_kind[f][k];
            if (kind != LH_BC_FLUX && kind != LH_BC_DIRICHLET)
                return fail(c, LH_EMODEL, "%s: the series has %s %s values, and the boundary condition there (lh_set_bc) reads no value",
                            who, fn, k == LH_COMP_ENERGY ? "energy" : "hydrology");
        }
    if (model == LH_MODEL_HEAT)
        for (int f = 0; f < 2; ++f)
            if (sr->d_val[f][LH_COMP_HYDROLOGY])
                return fail(c, LH_EMODEL, "%s: the series has %s hydrology values, and a heat-only model has no hydrology component", who,
                            f == LH_FACE_TOP ? "top" : "bottom");
    return LH_OK;
}

// Where the caller passes no step proposals they are carried all the same: in a zeroed buffer of the library's own
static int series_proposals(lh_ctx* c, void** dt_cols_device_ft) {
    if (*dt_cols_device_ft) return LH_OK;
    const size_t bytes = size_t(c->cfg.ncols) * c->esize;
    if (int rc = ensure_scratch(c, &c->d_series_dt, bytes, "c->d_series_dt", "ncols")) return rc;
    if (int rc = zero_stats(c, c->d_series_dt, bytes, "c->d_series_dt", "ncols")) return rc;
    *dt_cols_device_ft = c->d_series_dt;
    return LH_OK;
}

// The table's launch argument for [t0, t1]
static SeriesArgs series_args(const lh_ctx* c, const lh_bc_series* sr, double t0, double t1) {
    SeriesArgs S;
    S.times = sr->d_times;
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k) {
            S.val[f][k] = sr->d_val[f][k];
            S.knot_stride[f][k] = sr->percol[f][k] ? c->stride : 1;
            S.col_varies[f][k] = sr->percol[f][k] ? 1 : 0;
        }
    // the first knot after t0 and the first one at or after t1: the knots in between are the interior breakpoints
    const int nk = int(sr->times.size());
    int k_first = 1, k_end = 1;
    while (k_first < nk - 1 && !(sr->times[size_t(k_first)] > t0)) ++k_first;
    while (k_end < nk - 1 && !(sr->times[size_t(k_end)] >= t1)) ++k_end;
    S.k0 = k_first - 1;
    S.nsub = k_end - k_first + 1;
    return S;
}

// lh_set_bc's values at both ends of every sub-interval: what the chain's bcv holds where there is no series
static void series_own_values(const lh_ctx* c, double bcv[8]) {
    for (int k = 0; k < 8; ++k) bcv[k] = c->hp.bc_value[(k >> 1) & 1][k & 1];
}

// ---- the output of the dense calls (lh_dense.hpp; DESIGN sections 4.29 and 4.30): what lh_integrate_dense,
// lh_integrate_heat_dense and lh_integrate_layered_coupled_dense add to the series call they wrap

#define LH_DENSE_MAX_SAVES 65536
struct DenseCall {
    int32_t nsave;
    const double* times;       // host, [nsave]
    lh_state* const* snapshots; // host, [nsave]
};

static bool state_of(const lh_ctx* c, const lh_state* s) {
    for (const lh_state* k : c->states)
        if (k == s) return true;
    return false;
}

// Its checks, behind those of the call it wraps; `vars`: the planes the call writes
static int dense_refusals(lh_ctx* c, const char* who, const DenseCall& dc, const lh_state* Y, const lh_state* Ya, double t0,
                          double t1, uint32_t vars) {
    if (dc.nsave < 0 || dc.nsave > LH_DENSE_MAX_SAVES)
        return fail(c, LH_EINVAL, "%s: nsave = %d is outside [0, %d]", who, int(dc.nsave), LH_DENSE_MAX_SAVES);
    if (dc.nsave > 0 && (!dc.times || !dc.snapshots))
        return fail(c, LH_EINVAL, "%s: nsave = %d with a NULL %s array", who, int(dc.nsave), dc.times ? "snapshots" : "save_times");
    for (int k = 0; k < dc.nsave; ++k) {
        const double s = dc.times[k];
        if (!std::isfinite(s)) return fail(c, LH_EINVAL, "%s: save time %d is not finite", who, k);
        if (k > 0 && !(s > dc.times[k - 1]))
            return fail(c, LH_EINVAL, "%s: save time %d = %g is not above save time %d = %g (strictly increasing)", who, k, s, k - 1,
                        dc.times[k - 1]);
        if (s < t0 || s > t1) return fail(c, LH_EINVAL, "%s: save time %d = %g is outside [t0, t1] = [%g, %g]", who, k, s, t0, t1);
    }
    for (int k = 0; k < dc.nsave; ++k) {
        const lh_state* const sn = dc.snapshots[k];
        if (!sn) return fail(c, LH_EINVAL, "%s: snapshot %d is NULL", who, k);
        if (!state_of(c, sn)) return fail(c, LH_EINVAL, "%s: snapshot %d is not a state of this context", who, k);
        if (sn == Y || sn == Ya) return fail(c, LH_EINVAL, "%s: snapshot %d is %s", who, k, sn == Y ? "Y" : "Ya");
        for (int j = 0; j < k; ++j)
            if (dc.snapshots[j] == sn) return fail(c, LH_EINVAL, "%s: snapshot %d is snapshot %d again", who, k, j);
        if ((sn->mask & vars) != vars)
            return fail(c, LH_EINVAL, "%s: snapshot %d lacks a plane the call writes (has mask 0x%x, needs 0x%x)", who, k, sn->mask, vars);
    }
    return LH_OK;
}

// `bytes` of host memory into a transient device buffer
static int upload_bytes(lh_ctx* c, const void* host, size_t bytes, DeviceBuffer& buf, const char* what) {
    if (int rc = named_status(c, hipMalloc(&buf.p, bytes), "hipMalloc(&%s, %s)", what, "nsave")) return rc;
    hipError_t e = hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (pageable host memory)
    return e == hipSuccess ? LH_OK : fail(c, LH_ENODEVICE, "%s upload failed: %s", what, hipGetErrorString(e));
}

// The save times and the snapshots' plane tables ([nsave] pointers per written variable) on the device, for the
// launch's lifetime: the caller keeps the three buffers alive until launch_error(c, d_times) has waited.  `vars`: the
// planes the call writes -- the first of them (vartheta_l, or the heat-only call's rhoe_int) goes to d_first, rhoe_int
// behind vartheta_l to d_e
static int upload_dense_tables(lh_ctx* c, const DenseCall& dc, uint32_t vars, DeviceBuffer& d_times, DeviceBuffer& d_first,
                               DeviceBuffer& d_e) {
    if (dc.nsave == 0) return LH_OK;
    const size_t n = size_t(dc.nsave);
    const bool water = (vars & LH_MASK(LH_VAR_VARTHETA_L)) != 0, energy = (vars & LH_MASK(LH_VAR_RHOE_INT)) != 0;
    std::vector<void*> planes(n);
    if (int rc = upload_bytes(c, dc.times, n * sizeof(double), d_times, "d_save_times")) return rc;
    for (size_t k = 0; k < n; ++k) planes[k] = dc.snapshots[k]->plane[water ? LH_VAR_VARTHETA_L : LH_VAR_RHOE_INT];
    if (int rc = upload_bytes(c, planes.data(), n * sizeof(void*), d_first, "d_snapshot_planes")) return rc;
    if (!(water && energy)) return LH_OK;
    for (size_t k = 0; k < n; ++k) planes[k] = dc.snapshots[k]->plane[LH_VAR_RHOE_INT];
    return upload_bytes(c, planes.data(), n * sizeof(void*), d_e, "d_snapshot_planes");
}

// t1 == t0: nothing to integrate; the one save time there can be is t0, Y as passed
static int dense_at_t0(lh_ctx* c, const DenseCall& dc, lh_state* Y, uint32_t vars) {
    if (dc.nsave == 0) return LH_OK;
    if (int rc = materialize(c, Y, vars)) return rc;
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    for (int i = 0; i < LH_NVARS; ++i)
        if (vars >> i & 1u) {
            LH_HIP(c, hipMemcpyAsync(dc.snapshots[0]->plane[i], Y->plane[i], pl * c->esize, hipMemcpyDeviceToDevice, c->stream));
            mark_written(dc.snapshots[0], 1u << i);
        }
    return LH_OK;
}

// What lh_integrate_heat_series and lh_integrate_layered_coupled_series add to the call they wrap (heat_trbdf2,
// coupled_trbdf2 below): the series as the caller passed it.  Its checks come behind the wrapped call's own
struct SeriesCall {
    const lh_bc_series* sr;
};
static int series_call_refusals(lh_ctx* c, const char* who, const SeriesCall& sc, double t0, double t1) {
    if (int rc = series_handle_refusals(c, who, sc.sr)) return rc;
    if (int rc = series_span_refusal(c, who, sc.sr, t0, t1)) return rc;
    return series_kind_refusals(c, who, sc.sr);
}

// The adaptive coupled call exists twice as well (lh_coupled_trbdf2.hpp, lh_layered_coupled_trbdf2.hpp; DESIGN section
// 4.26), on the same ten scratch planes and statistics block.  One body; the layered flavour is coupled_implicit_steps'.
// `sc`: NULL, or the series of lh_integrate_layered_coupled_series (bcv is NULL then: one launch for the chain of calls).
// `dc`: NULL, or the output of lh_integrate_layered_coupled_dense (a layered flavour; bcv is NULL), whose checks come
// last and whose series may be NULL: one sub-interval, no table, the plain call with bcv = NULL.
static int coupled_trbdf2(lh_ctx* c, const RichardsFlavour& fl, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                          double abstol, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv,
                          const SeriesCall* sc = nullptr, const DenseCall* dc = nullptr) {
    if (!c) return LH_EINVAL;
    const char* const who = fl.who;
    int rc = zero_stats(c, c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat");
    if (rc) return rc;
    if ((rc = trbdf2_argument_refusals(c, who, t0, t1, dt, {abstol, abstol_e, reltol}, flags, 0, bcv))) return rc;
    Range r_(fl.range);
    if ((rc = implicit_refusals(c, who, Y, Ya, LH_MODEL_COUPLED, COUPLED_MODELS, fl.scalar))) return rc;
    if (sc && (rc = series_call_refusals(c, who, *sc, t0, t1))) return rc;
    const uint32_t written = LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_RHOE_INT);
    if (dc && (rc = dense_refusals(c, who, *dc, Y, Ya, t0, t1, written))) return rc;
    trbdf2_tolerance_defaults(abstol, reltol);
    // (the energy's own default is that of 1e-6 K in water)
    if (!(abstol_e > 0)) abstol_e = LH_TRBDF2_ABSTOL_DEFAULT * (c->hp.earth.cp_l * c->hp.earth.rho_liq);
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_cpl_ad, 10 * pl * c->esize, "c->d_cpl_ad", "10 * plane"))) return rc;
    if ((rc = ensure_scratch(c, &c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat", true))) return rc;
    if (t1 == t0) return dc ? dense_at_t0(c, *dc, Y, written) : LH_OK;
    double own[8];
    SeriesArgs S{}; // (no table: one sub-interval)
    S.nsub = 1;
    if (sc) {
        if ((rc = series_proposals(c, &dt_cols_device_ft))) return rc;
        series_own_values(c, own);
        bcv = own;
        S = series_args(c, sc->sr, t0, t1);
    }
    if ((rc = materialize(c, Y, ~0u))) return rc;
    DeviceBuffer d_times, d_snap_y, d_snap_e; // (dc: read by the launch)
    if (dc && (rc = upload_dense_tables(c, *dc, written, d_times, d_snap_y, d_snap_e))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        CoupledTrbdf2Args<FT> A;
        point_at_water<FT>(Y, A);
        A.e = static_cast<FT*>(Y->plane[LH_VAR_RHOE_INT]);
        carve_planes<FT>(c->d_cpl_ad, pl, {&A.yn, &A.fn, &A.yg, &A.w, &A.cp, &A.dp, &A.en, &A.fe, &A.eg, &A.we});
        fill_trbdf2_args<FT>(c, A, t0, t1, dt, abstol, reltol, dt_cols_device_ft, bcv);
        A.abstol_e = abstol_e;
        if (dc) { // (a layered flavour)
            const DenseArgs<FT> D = {static_cast<const double*>(d_times.p), static_cast<FT* const*>(d_snap_y.p),
                                     static_cast<FT* const*>(d_snap_e.p), dc->nsave};
            launch_dense_layered_coupled_trbdf2<FT>(P, layered_heat_args<FT>(c), A, S, D, implicit_noice(c, Y), c->stream);
        } else if (sc) // (a layered flavour: the series of a context without a map is lh_integrate_series')
            launch_series_layered_coupled_trbdf2<FT>(P, layered_heat_args<FT>(c), A, S, implicit_noice(c, Y), c->stream);
        else if (fl.layered()) launch_layered_coupled_trbdf2<FT>(P, layered_heat_args<FT>(c), A, implicit_noice(c, Y), c->stream);
        else launch_coupled_trbdf2<FT>(P, A, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
    });
    mark_written(Y, written);
    for (int k = 0; dc && k < dc->nsave; ++k) mark_written(dc->snapshots[k], written);
    return launch_status(c, launch_error(c, d_times), fl.launch); // (waits only where tables were uploaded: nsave > 0)
}

int lh_integrate_coupled_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt, double abstol,
                                double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const RichardsFlavour fl = {"lh_integrate_coupled_trbdf2", nullptr, "lh:integrate_coupled_trbdf2", "coupled TR-BDF2"};
    return coupled_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, dt_cols_device_ft, bcv);
}

int lh_integrate_layered_coupled_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                                        double abstol, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft,
                                        const double* bcv) {
    static const RichardsFlavour fl = {"lh_integrate_layered_coupled_trbdf2", "lh_integrate_coupled_trbdf2",
                                       "lh:integrate_layered_coupled_trbdf2", "layered coupled TR-BDF2"};
    return coupled_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, dt_cols_device_ft, bcv);
}

// The adaptive heat-only call exists twice as well (lh_heat_trbdf2.hpp, lh_layered_heat_trbdf2.hpp; DESIGN section
// 4.27), on the same twelve scratch planes and lh_integrate_trbdf2's statistics block.  One body: lh_integrate_trbdf2's
// argument checks, then heat_implicit_steps' refusals in its order; the layered flavour is heat_implicit_steps'.
// `sc`: NULL, or the series of lh_integrate_heat_series (bcv is NULL then: one launch for the chain of calls).
// `dc`: NULL, or the output of lh_integrate_heat_dense (bcv is NULL), whose checks come last and whose series may be
// NULL: one sub-interval, no table, the plain call with bcv = NULL.  Only rhoe_int is written, also of a snapshot.
static int heat_trbdf2(lh_ctx* c, const HeatFlavour& fl, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                       double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv,
                       const SeriesCall* sc = nullptr, const DenseCall* dc = nullptr) {
    if (!c) return LH_EINVAL;
    const char* const who = fl.who;
    int rc = zero_stats(c, c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat");
    if (rc) return rc;
    if ((rc = trbdf2_argument_refusals(c, who, t0, t1, dt, {abstol_e, reltol}, flags, 0, bcv))) return rc;
    Range r_(fl.range);
    if (c->cfg.model != LH_MODEL_HEAT) return fail(c, LH_EMODEL, "%s: heat-only models (SoilEnergyModel + PrescribedHydrologyModel)", who);
    if ((rc = stepping_preamble(c, Y, Ya))) return rc;
    if (!fl.layered()) {
        if ((rc = layered_unsupported(c, who))) return rc;
    } else {
        if (!layered(c))
            return fail(c, LH_EMODEL, "%s: the context has no class map (lh_set_soil_class_map); %s steps a model without soil classes",
                        who, fl.scalar);
        if ((rc = layered_check(c, who))) return rc;
    }
    if (sc && (rc = series_call_refusals(c, who, *sc, t0, t1))) return rc;
    const uint32_t written = LH_MASK(LH_VAR_RHOE_INT);
    if (dc && (rc = dense_refusals(c, who, *dc, Y, Ya, t0, t1, written))) return rc;
    if (!(reltol > 0)) reltol = LH_TRBDF2_RELTOL_DEFAULT;
    // (lh_integrate_coupled_trbdf2's default for the energy: that of 1e-6 K in water)
    if (!(abstol_e > 0)) abstol_e = LH_TRBDF2_ABSTOL_DEFAULT * (c->hp.earth.cp_l * c->hp.earth.rho_liq);
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if ((rc = ensure_scratch(c, &c->d_heat_ad, 12 * pl * c->esize, "c->d_heat_ad", "12 * plane"))) return rc;
    if ((rc = ensure_scratch(c, &c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat", true))) return rc;
    if (t1 == t0) return dc ? dense_at_t0(c, *dc, Y, written) : LH_OK;
    double own[8];
    SeriesArgs S{}; // (no table: one sub-interval)
    S.nsub = 1;
    if (sc) {
        if ((rc = series_proposals(c, &dt_cols_device_ft))) return rc;
        series_own_values(c, own);
        bcv = own;
        S = series_args(c, sc->sr, t0, t1);
    }
    // (level-uniform variables of Ya become planes: the prologue reads each cell once)
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    DeviceBuffer d_times, d_snap_e, d_unused; // (dc: read by the launch)
    if (dc && (rc = upload_dense_tables(c, *dc, written, d_times, d_snap_e, d_unused))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (fl.layered()) layered_params<FT>(c, P);
        HeatTrbdf2Args<FT> A;
        A.y = static_cast<FT*>(Y->plane[LH_VAR_RHOE_INT]);
        A.vl = static_cast<const FT*>(Ya->plane[LH_VAR_VARTHETA_L]);
        A.ti = static_cast<const FT*>(Ya->plane[LH_VAR_THETA_I]);
        carve_planes<FT>(c->d_heat_ad, pl, {&A.rc, &A.al, &A.ks, &A.k, &A.a, &A.iden, &A.cp, &A.yn, &A.fn, &A.yg, &A.w, &A.z});
        A.dt_cols = static_cast<FT*>(dt_cols_device_ft);
        A.t0 = t0;
        A.t1 = t1;
        A.dt = dt;
        A.abstol_e = abstol_e;
        A.reltol = reltol;
        A.has_bcv = bcv != nullptr;
        for (int k = 0; k < 8; ++k) A.bcv[k] = bcv ? bcv[k] : 0.0;
        A.stats = static_cast<unsigned long long*>(c->d_tr_stats);
        if (dc) { // (the snapshots' rhoe_int planes in the functor's one table)
            const DenseArgs<FT> D = {static_cast<const double*>(d_times.p), static_cast<FT* const*>(d_snap_e.p), nullptr, dc->nsave};
            if (fl.layered()) launch_dense_layered_heat_trbdf2<FT>(P, layered_heat_args<FT>(c), A, S, D, c->stream);
            else launch_dense_heat_trbdf2<FT>(P, A, S, D, any_percol(c), c->math, c->stream);
        } else if (sc) {
            if (fl.layered()) launch_series_layered_heat_trbdf2<FT>(P, layered_heat_args<FT>(c), A, S, c->stream);
            else launch_series_heat_trbdf2<FT>(P, A, S, any_percol(c), c->math, c->stream);
        } else if (fl.layered()) launch_layered_heat_trbdf2<FT>(P, layered_heat_args<FT>(c), A, c->stream);
        else launch_heat_trbdf2<FT>(P, A, any_percol(c), c->math, c->stream);
    });
    mark_written(Y, written);
    for (int k = 0; dc && k < dc->nsave; ++k) mark_written(dc->snapshots[k], written);
    return launch_status(c, launch_error(c, d_times), fl.launch); // (waits only where tables were uploaded: nsave > 0)
}

int lh_integrate_heat_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt, double abstol_e,
                             double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const HeatFlavour fl = {"lh_integrate_heat_trbdf2", nullptr, "lh:integrate_heat_trbdf2", "heat TR-BDF2"};
    return heat_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, dt_cols_device_ft, bcv);
}

int lh_integrate_layered_heat_trbdf2(lh_ctx* c, lh_state* Y, const lh_state* Ya, double t0, double t1, double dt,
                                     double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, const double* bcv) {
    static const HeatFlavour fl = {"lh_integrate_layered_heat_trbdf2", "lh_integrate_heat_trbdf2", "lh:integrate_layered_heat_trbdf2",
                                   "layered heat TR-BDF2"};
    return heat_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, dt_cols_device_ft, bcv);
}

// ---- boundary-value time series (lh_series.hpp)

int lh_bc_series_create(lh_ctx* c, int32_t nknots, const double* times, lh_bc_series** out) {
    if (!c) return LH_EINVAL;
    if (!times || !out) return fail(c, LH_EINVAL, "lh_bc_series_create: NULL argument");
    *out = nullptr;
    if (nknots < 2) return fail(c, LH_EINVAL, "lh_bc_series_create: need nknots >= 2");
    for (int32_t k = 0; k < nknots; ++k) {
        if (!std::isfinite(times[k])) return fail(c, LH_EINVAL, "lh_bc_series_create: knot %d is not finite", k);
        if (k > 0 && !(times[k] > times[k - 1]))
            return fail(c, LH_EINVAL, "lh_bc_series_create: knot %d is not after knot %d (the times must increase strictly)", k, k - 1);
    }
    (void)hipSetDevice(c->device);
    lh_bc_series* s = new (std::nothrow) lh_bc_series();
    if (!s) return fail(c, LH_ENOMEM, "out of host memory");
    s->ctx = c;
    s->times.assign(times, times + nknots);
    hipError_t e = hipMalloc(&s->d_times, size_t(nknots) * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(s->d_times, times, size_t(nknots) * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s->d_times) (void)hipFree(s->d_times);
        delete s;
        return hip_status(c, e, "lh_bc_series_create: the upload of the knot times");
    }
    c->series.push_back(s);
    *out = s;
    return LH_OK;
}

int lh_bc_series_set(lh_ctx* c, lh_bc_series* s, int32_t face, int32_t comp, const double* values, int64_t knot_stride,
                     int64_t col_stride) {
    if (!c) return LH_EINVAL;
    if (!s || !series_of(c, s)) return fail(c, LH_EINVAL, "lh_bc_series_set: not a series of this context");
    if (face != LH_FACE_BOTTOM && face != LH_FACE_TOP) return fail(c, LH_EINVAL, "lh_bc_series_set: unknown face %d", face);
    if (comp != LH_COMP_ENERGY && comp != LH_COMP_HYDROLOGY) return fail(c, LH_EINVAL, "lh_bc_series_set: unknown component %d", comp);
    (void)hipSetDevice(c->device);
    if (s->d_val[face][comp]) { // (a launch in flight may still read the table)
        LH_HIP(c, hipStreamSynchronize(c->stream));
        (void)hipFree(s->d_val[face][comp]);
        s->d_val[face][comp] = nullptr;
    }
    if (!values) return LH_OK;
    const int64_t nk = int64_t(s->times.size());
    const bool percol = col_stride != 0;
    const int64_t row = percol ? c->stride : 1, n = percol ? c->cfg.ncols : 1;
    std::vector<double> tab(size_t(nk) * size_t(row), 0.0);
    for (int64_t k = 0; k < nk; ++k)
        for (int64_t j = 0; j < n; ++j) tab[size_t(k * row + j)] = values[k * knot_stride + j * col_stride];
    double* d = nullptr;
    LH_HIP(c, hipMalloc(&d, tab.size() * sizeof(double)));
    const hipError_t e = hipMemcpy(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_status(c, e, "lh_bc_series_set: the upload of the table");
    }
    s->d_val[face][comp] = d;
    s->percol[face][comp] = percol;
    return LH_OK;
}

int lh_bc_series_destroy(lh_ctx* c, lh_bc_series* s) {
    if (!c) return LH_EINVAL;
    if (!s) return LH_OK;
    if (!series_of(c, s)) return fail(c, LH_EINVAL, "lh_bc_series_destroy: not a series of this context");
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream); // (a launch in flight may still read the tables)
    for (size_t k = 0; k < c->series.size(); ++k)
        if (c->series[k] == s) {
            c->series.erase(c->series.begin() + long(k));
            break;
        }
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k)
            if (s->d_val[f][k]) (void)hipFree(s->d_val[f][k]);
    if (s->d_times) (void)hipFree(s->d_times);
    delete s;
    return LH_OK;
}

// ---- lh_integrate_series and lh_integrate_dense (lh_series.hpp, lh_dense.hpp; DESIGN sections 4.21 and 4.29)

// One launch for the chain of lh_integrate_trbdf2 / lh_integrate_layered_trbdf2 / lh_integrate_coupled_trbdf2 calls
// over the sub-intervals of [t0, t1] between the knots: the refusals, the defaults, the scratch and the launch
// arguments are those calls' own, in their order; the series adds its checks behind them.  `dc`: NULL, or the output
// of lh_integrate_dense, whose checks come last and whose series may be NULL (one sub-interval, no table: those calls
// with bcv = NULL).
static int integrate_series(lh_ctx* c, const char* who, const char* range, const char* launch, lh_state* Y, const lh_state* Ya,
                            const lh_bc_series* sr, double t0, double t1, double dt, double abstol, double abstol_e, double reltol,
                            uint32_t flags, void* dt_cols_device_ft, const DenseCall* dc) {
    if (!c) return LH_EINVAL;
    int rc = zero_stats(c, c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat");
    if (rc) return rc;
    const bool tabled = sr || !dc;
    if (tabled && (rc = series_handle_refusals(c, who, sr))) return rc;
    if (c->cfg.model == LH_MODEL_HEAT)
        return fail(c, LH_EMODEL, "%s: Richards models, with or without a class map, and coupled models without one only", who);
    const bool coupled = c->cfg.model == LH_MODEL_COUPLED;
    const bool lay = !coupled && layered(c);
    rc = coupled ? trbdf2_argument_refusals(c, who, t0, t1, dt, {abstol, abstol_e, reltol}, flags, 0, nullptr)
                 : trbdf2_argument_refusals(c, who, t0, t1, dt, {abstol, reltol}, flags, LH_TRBDF2_FIXED, nullptr);
    if (rc) return rc;
    if (tabled && (rc = series_span_refusal(c, who, sr, t0, t1))) return rc;
    Range r_(range);
    if ((rc = implicit_refusals(c, who, Y, Ya, coupled ? LH_MODEL_COUPLED : LH_MODEL_RICHARDS, coupled ? COUPLED_MODELS : RICHARDS_MODELS,
                                lay ? "lh_integrate_trbdf2" : nullptr)))
        return rc;
    if (tabled && (rc = series_kind_refusals(c, who, sr))) return rc;
    const uint32_t written = LH_MASK(LH_VAR_VARTHETA_L) | (coupled ? LH_MASK(LH_VAR_RHOE_INT) : 0u);
    if (dc && (rc = dense_refusals(c, who, *dc, Y, Ya, t0, t1, written))) return rc;
    trbdf2_tolerance_defaults(abstol, reltol);
    if (!(abstol_e > 0)) abstol_e = LH_TRBDF2_ABSTOL_DEFAULT * (c->hp.earth.cp_l * c->hp.earth.rho_liq);
    double tol = 0; // (fixed mode: lh_step_implicit_euler's defaults)
    int32_t max_iter = 0;
    newton_defaults(c, tol, max_iter);
    const size_t pl = size_t(c->cfg.nlev) * size_t(c->stride);
    if (coupled) {
        if ((rc = ensure_scratch(c, &c->d_cpl_ad, 10 * pl * c->esize, "c->d_cpl_ad", "10 * plane"))) return rc;
    } else if ((rc = ensure_scratch(c, &c->d_tr, 6 * pl * c->esize, "c->d_tr", "6 * plane")))
        return rc;
    if ((rc = ensure_scratch(c, &c->d_tr_stats, TRBDF2_STATS_BYTES, "c->d_tr_stats", "nstat", true))) return rc;
    if (t1 == t0) return dc ? dense_at_t0(c, *dc, Y, written) : LH_OK;
    if (tabled && (rc = series_proposals(c, &dt_cols_device_ft))) return rc;
    if ((rc = materialize(c, Y, ~0u))) return rc;
    SeriesArgs S{}; // (no table: one sub-interval)
    S.nsub = 1;
    double own[8];
    const double* bcv = nullptr;
    if (tabled) {
        S = series_args(c, sr, t0, t1);
        series_own_values(c, own);
        bcv = own;
    }
    DeviceBuffer d_times, d_snap_y, d_snap_e; // (dc: read by the launch)
    if (dc && (rc = upload_dense_tables(c, *dc, written, d_times, d_snap_y, d_snap_e))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        const DenseArgs<FT> D = {static_cast<const double*>(d_times.p), static_cast<FT* const*>(d_snap_y.p),
                                 static_cast<FT* const*>(d_snap_e.p), dc ? dc->nsave : 0};
        if (coupled) {
            CoupledTrbdf2Args<FT> A;
            point_at_water<FT>(Y, A);
            A.e = static_cast<FT*>(Y->plane[LH_VAR_RHOE_INT]);
            carve_planes<FT>(c->d_cpl_ad, pl, {&A.yn, &A.fn, &A.yg, &A.w, &A.cp, &A.dp, &A.en, &A.fe, &A.eg, &A.we});
            fill_trbdf2_args<FT>(c, A, t0, t1, dt, abstol, reltol, dt_cols_device_ft, bcv);
            A.abstol_e = abstol_e;
            if (dc) launch_dense_coupled_trbdf2<FT>(P, A, S, D, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
            else launch_series_coupled_trbdf2<FT>(P, A, S, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
        } else {
            if (lay) layered_params<FT>(c, P);
            Trbdf2Args<FT> A;
            point_at_water<FT>(Y, A);
            carve_planes<FT>(c->d_tr, pl, {&A.yn, &A.fn, &A.yg, &A.w, &A.cp, &A.dp});
            fill_trbdf2_args<FT>(c, A, t0, t1, dt, abstol, reltol, dt_cols_device_ft, bcv);
            A.fixed = (flags & LH_TRBDF2_FIXED) != 0;
            A.tol = FT(tol);
            A.max_iter = max_iter;
            if (!dc && lay) launch_series_layered_trbdf2<FT>(P, layered_args<FT>(c), A, S, implicit_noice(c, Y), c->stream);
            else if (!dc) launch_series_trbdf2<FT>(P, A, S, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
            else if (lay) launch_dense_layered_trbdf2<FT>(P, layered_args<FT>(c), A, S, D, implicit_noice(c, Y), c->stream);
            else launch_dense_trbdf2<FT>(P, A, S, D, any_percol(c), implicit_noice(c, Y), c->math, c->stream);
        }
    });
    mark_written(Y, written);
    for (int k = 0; dc && k < dc->nsave; ++k) mark_written(dc->snapshots[k], written);
    return launch_status(c, launch_error(c, d_times), launch);
}

int lh_integrate_series(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1, double dt,
                        double abstol, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft) {
    return integrate_series(c, "lh_integrate_series", "lh:integrate_series", "series TR-BDF2", Y, Ya, sr, t0, t1, dt, abstol, abstol_e,
                            reltol, flags, dt_cols_device_ft, nullptr);
}

// ... with output at save times, interpolated in the launch from the accepted steps (lh_dense.hpp)
int lh_integrate_dense(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1, double dt,
                       double abstol, double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, int32_t nsave,
                       const double* save_times, lh_state* const* snapshots) {
    const DenseCall dc = {nsave, save_times, snapshots};
    return integrate_series(c, "lh_integrate_dense", "lh:integrate_dense", "dense TR-BDF2", Y, Ya, sr, t0, t1, dt, abstol, abstol_e,
                            reltol, flags, dt_cols_device_ft, &dc);
}

// One launch for the chain of lh_integrate_heat_trbdf2 or, with a class map, lh_integrate_layered_heat_trbdf2 calls
// (DESIGN section 4.28): heat_trbdf2 in the flavour of the context, under this call's name
int lh_integrate_heat_series(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1, double dt,
                             double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft) {
    if (!c) return LH_EINVAL;
    static const char* const who = "lh_integrate_heat_series";
    static const HeatFlavour scalar = {who, nullptr, "lh:integrate_heat_series", "heat series TR-BDF2"};
    static const HeatFlavour lay = {who, who, "lh:integrate_heat_series", "layered heat series TR-BDF2"};
    const SeriesCall sc = {sr};
    return heat_trbdf2(c, layered(c) ? lay : scalar, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, dt_cols_device_ft, nullptr, &sc);
}

// ... and for the chain of lh_integrate_layered_coupled_trbdf2 calls: a coupled context without a class map is
// lh_integrate_series'
int lh_integrate_layered_coupled_series(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1,
                                        double dt, double abstol, double abstol_e, double reltol, uint32_t flags,
                                        void* dt_cols_device_ft) {
    static const RichardsFlavour fl = {"lh_integrate_layered_coupled_series", "lh_integrate_series",
                                       "lh:integrate_layered_coupled_series", "layered coupled series TR-BDF2"};
    const SeriesCall sc = {sr};
    return coupled_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, dt_cols_device_ft, nullptr, &sc);
}

// lh_integrate_heat_series with output at save times, interpolated in the launch from the accepted steps
// (lh_dense_heat.hpp).  Without a series: lh_integrate_heat_trbdf2 or, with a class map,
// lh_integrate_layered_heat_trbdf2 with bcv = NULL
int lh_integrate_heat_dense(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1, double dt,
                            double abstol_e, double reltol, uint32_t flags, void* dt_cols_device_ft, int32_t nsave,
                            const double* save_times, lh_state* const* snapshots) {
    if (!c) return LH_EINVAL;
    static const char* const who = "lh_integrate_heat_dense";
    static const HeatFlavour scalar = {who, nullptr, "lh:integrate_heat_dense", "heat dense TR-BDF2"};
    static const HeatFlavour lay = {who, who, "lh:integrate_heat_dense", "layered heat dense TR-BDF2"};
    const SeriesCall sc = {sr};
    const DenseCall dc = {nsave, save_times, snapshots};
    return heat_trbdf2(c, layered(c) ? lay : scalar, Y, Ya, t0, t1, dt, abstol_e, reltol, flags, dt_cols_device_ft, nullptr,
                       sr ? &sc : nullptr, &dc);
}

// ... and lh_integrate_layered_coupled_series; without a series lh_integrate_layered_coupled_trbdf2 with bcv = NULL.
// A coupled context without a class map is lh_integrate_dense's
int lh_integrate_layered_coupled_dense(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t0, double t1,
                                       double dt, double abstol, double abstol_e, double reltol, uint32_t flags,
                                       void* dt_cols_device_ft, int32_t nsave, const double* save_times,
                                       lh_state* const* snapshots) {
    static const RichardsFlavour fl = {"lh_integrate_layered_coupled_dense", "lh_integrate_dense",
                                       "lh:integrate_layered_coupled_dense", "layered coupled dense TR-BDF2"};
    const SeriesCall sc = {sr};
    const DenseCall dc = {nsave, save_times, snapshots};
    return coupled_trbdf2(c, fl, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, dt_cols_device_ft, nullptr, sr ? &sc : nullptr,
                          &dc);
}

// ---- lh_step_ssprk33_series (lh_series_stepper.hpp)

// The wave stepper samples the series itself (columns of up to 128 levels, no class map); everything else takes the
// fused stages, one launch of sampled per-column values ahead of each step.  Large ensembles (more than 2^20 threads,
// use_column_stepper's line) take the stepper only under persist=2: a wave reads its two knot values per component
// and stage from rows of ncols doubles, one sector each, where the sampling launch reads the rows coalesced --
// measured on 1e6 x 64 columns at 30 steps per call, ms per step, stepper vs fused: 0.94 vs 0.83 (Float64), 0.66 vs
// 0.38 (Float32); at 4096 columns and below the stepper is 1.6 to 6.9 times faster.
static bool series_in_stepper(const lh_ctx* c, int64_t nsteps) {
    if (layered(c) || c->cfg.nlev > 128 || !use_column_stepper(c, nsteps, /*bcv=*/true)) return false;
    const int64_t threads = c->cfg.ncols * int64_t((c->cfg.nlev + 63) / 64 * 64);
    return c->tune.persist == 2 || threads <= (int64_t(1) << 20);
}

int lh_step_series_engine(const lh_ctx* c, int64_t nsteps) {
    if (!c || nsteps < 0) return LH_EINVAL;
    return series_in_stepper(c, nsteps) ? LH_ENGINE_COLUMN_STEPPER : LH_ENGINE_FUSED_STAGES;
}

int lh_step_ssprk33_series(lh_ctx* c, lh_state* Y, const lh_state* Ya, const lh_bc_series* sr, double t, double dt,
                           int64_t nsteps) {
    const char* who = "lh_step_ssprk33_series";
    if (!c) return LH_EINVAL;
    if (nsteps < 0 || !(dt > 0)) return fail(c, LH_EINVAL, "%s: need nsteps >= 0 and dt > 0", who);
    Range r_("lh:step_ssprk33_series");
    int rc = stepping_preamble(c, Y, Ya);
    if (rc) return rc;
    if (layered(c) && (rc = layered_check(c, who))) return rc;
    if (!std::isfinite(t)) return fail(c, LH_EINVAL, "%s: t is not finite", who);
    if ((rc = series_handle_refusals(c, who, sr))) return rc;
    if ((rc = series_kind_refusals(c, who, sr))) return rc;
    if (nsteps == 0) return LH_OK;
    // the span: t + dt k is monotone in k and the three offsets are 0 <= dt / 2 <= dt, so the first stage time of the
    // first step and the second one of the last step bound all of them
    const double first = series_stage_time(t, dt, 0, 0), last = series_stage_time(t, dt, nsteps - 1, 1);
    if (first < sr->times.front() || !(last <= sr->times.back()))
        return fail(c, LH_EINVAL, "%s: the stage time %.17g leaves the series' knots [%.17g, %.17g] (no extrapolation)", who,
                    first < sr->times.front() ? first : last, sr->times.front(), sr->times.back());
    SeriesStepArgs S{};
    S.times = sr->d_times;
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 2; ++k) {
            S.val[f][k] = sr->d_val[f][k];
            if (sr->percol[f][k]) S.percol |= 1u << (2 * f + k);
        }
    S.nknots = int32_t(sr->times.size());
    S.t = t;
    S.dt = dt;
    if (series_in_stepper(c, nsteps)) { // run_column_stepper's launch with the table in place of bcv
        Range r2_("lh:series_column_stepper");
        const bool factors = c->hp.viscosity_kind != LH_FACTOR_NONE || c->hp.impedance_kind != LH_FACTOR_NONE;
        const lh_state* ti_src = c->cfg.model == LH_MODEL_HEAT ? Ya : Y;
        const bool noice = c->tune.zero != 0 && !factors && ti_src && (ti_src->zero_mask & LH_MASK(LH_VAR_THETA_I));
        if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~aux_profile_vars(c, Ya)))) return rc;
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            DevParams<FT> P = make_params<FT>(c);
            set_aux_profiles<FT>(c, Ya, P);
            launch_series_column_stepper<FT>(P, planes_of<FT>(Y), planes_of<FT>(Ya), FT(dt), nsteps, S, factors, any_percol(c), noice,
                                             c->stream);
        });
        mark_written(Y, LH_MASK(LH_VAR_VARTHETA_L) | LH_MASK(LH_VAR_RHOE_INT));
        return launch_status(c, hipGetLastError(), "series column stepper");
    }
    // the fused stages: the three stages' values of a step as per-column arrays, which the launches take where
    // lh_set_bc's per-column arrays go
    const size_t row = size_t(c->stride) * c->esize;
    if ((rc = ensure_scratch(c, &c->d_series_stage, 12 * row, "c->d_series_stage", "12 * stride"))) return rc;
    StageBoundaryArrays arrays{};
    for (int stage = 0; stage < 3; ++stage)
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 2; ++k)
                if (sr->d_val[f][k]) arrays.p[stage][f][k] = static_cast<const char*>(c->d_series_stage) + size_t((stage * 2 + f) * 2 + k) * row;
    lh_state *U1, *U2;
    if (layered(c)) { // (as lh_step_ssprk33: unsegmented launches, the stage state updated in place)
        if ((rc = stage_states(c, &U1, nullptr))) return rc;
        U2 = U1;
    } else if ((rc = stage_states(c, &U1, &U2)))
        return rc;
    for (int64_t s = 0; s < nsteps; ++s) {
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            launch_series_stage_values<FT>(make_params<FT>(c), S, s, static_cast<FT*>(c->d_series_stage), c->stream);
        });
        if ((rc = launch_status(c, hipGetLastError(), "series stage values"))) return rc;
        if ((rc = fused_ssprk33_step(c, Y, Ya, U1, U2, dt, nullptr, nullptr, &arrays))) return rc;
    }
    return LH_OK;
}

int lh_stable_dt_device(lh_ctx* c, const lh_state* Y, const lh_state* Ya, double courant, void* d_out) {
    if (!c || !d_out) return fail(c, LH_EINVAL, "lh_stable_dt_device: NULL argument");
    int rc;
    if (model_heat(c->cfg.model) && !c->hp.earth_set)
        return fail(c, LH_EINVAL, "earth parameters (lh_set_earth_params) are required by the energy model");
    if ((rc = check_state(c, Y, prognostic_mask(c->cfg.model), "Y"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    if ((rc = layered_check(c, "lh_stable_dt"))) return rc;
    (void)hipSetDevice(c->device);
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u))) return rc;
    with_ft(c, [&](auto ft) {
        using FT = decltype(ft);
        DevParams<FT> P = make_params<FT>(c);
        if (layered(c)) {
            layered_params<FT>(c, P);
            launch_fill<FT>(static_cast<FT*>(d_out), 1, FT(INFINITY), c->stream); // the minimum starts at +inf
            if (layered_heat(c))
                launch_layered_heat_stable_dt<FT>(P, layered_heat_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), FT(courant), d_out,
                                                  c->cfg.model, c->stream);
            else
                launch_layered_stable_dt<FT>(P, layered_args<FT>(c), planes_of<FT>(Y), planes_of<FT>(Ya), FT(courant), d_out, c->stream);
        } else
            launch_stable_dt<FT>(P, planes_of<FT>(Y), planes_of<FT>(Ya), FT(courant), d_out, any_percol(c), c->stream);
    });
    LH_HIP(c, hipGetLastError());
    return allreduce_min(c, d_out); // the global minimum when a communicator is attached
}

int lh_stable_dt(lh_ctx* c, const lh_state* Y, const lh_state* Ya, double courant, double* dt_host) {
    if (!c || !dt_host) return fail(c, LH_EINVAL, "lh_stable_dt: NULL argument");
    int rc = lh_stable_dt_device(c, Y, Ya, courant, c->d_dt);
    if (rc) return rc;
    return with_ft(c, [&](auto ft) {
        decltype(ft) v;
        LH_HIP(c, hipMemcpyAsync(&v, c->d_dt, sizeof v, hipMemcpyDeviceToHost, c->stream));
        LH_HIP(c, hipStreamSynchronize(c->stream));
        *dt_host = v;
        return int(LH_OK);
    });
}

int lh_get_status(lh_ctx* c, uint32_t* flags) {
    if (!c || !flags) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    LH_HIP(c, hipMemcpyAsync(flags, c->d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    LH_HIP(c, hipMemsetAsync(c->d_status, 0, sizeof(uint32_t), c->stream));
    LH_HIP(c, hipStreamSynchronize(c->stream));
    return LH_OK;
}

int lh_synchronize(lh_ctx* c) {
    if (!c) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    LH_HIP(c, hipStreamSynchronize(c->stream));
    return LH_OK;
}

int lh_tune_placement(lh_ctx* c, lh_state* Y, const lh_state* Ya, lh_state* dY, int max_candidates,
                      uint32_t flags, float* ms_before, float* ms_after) {
    if (!c) return LH_EINVAL;
    int rc = validate_model(c);
    if (rc) return rc;
    if ((rc = layered_unsupported(c, "lh_tune_placement"))) return rc;
    const uint32_t pm = prognostic_mask(c->cfg.model);
    if ((rc = check_state(c, Y, pm, "Y"))) return rc;
    if ((rc = check_state(c, Ya, aux_mask(c), "Ya"))) return rc;
    if (dY && (rc = check_state(c, dY, pm, "dY"))) return rc;
    if (dY == Y) return fail(c, LH_EINVAL, "lh_tune_placement: dY must not be Y");
    if (flags & ~uint32_t(LH_PLACE_MOVE_INPUT)) return fail(c, LH_EINVAL, "lh_tune_placement: unknown flag bits");
    (void)hipSetDevice(c->device);
    if ((rc = materialize(c, Y, ~0u)) || (rc = materialize(c, Ya, ~0u)) || (rc = materialize(c, dY, ~0u))) return rc;
    lh_state* written = dY;
    if (!dY && (use_column_stepper(c, 1) || segment_length(c) > 0)) { // no stage state in HBM, or a cache-resident one
        if (ms_before) *ms_before = 0;
        if (ms_after) *ms_after = 0;
        return LH_OK;
    }
    if (!dY) { // the stage state of the fused SSPRK33 stepper
        if (!c->scratch_u1 && (rc = state_alloc(c, pm & ~LH_MASK(LH_VAR_THETA_I), &c->scratch_u1))) return rc;
        written = c->scratch_u1;
    }
    auto run = [&]() -> int {
        if (dY) // the tendency launch of lh_rhs / lh_rhs_stable_dt
            return with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, nullptr, dY, 0.0, 0, nullptr); });
        // stages 1 and 2 with dt = 0 stream the same planes as a step and leave Y untouched
        // (U1 = Y + 0 f(Y); U1 = (3Y + U1 + 0 f(U1))/4)
        lh_state* U1 = c->scratch_u1;
        int r = with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, Y, Ya, Y, U1, 0.0, 1, nullptr); });
        if (r) return r;
        return with_ft(c, [&](auto ft) { return do_rhs<decltype(ft)>(c, U1, Ya, Y, U1, 0.0, 2, nullptr); });
    };
    // The written planes matter most (two write streams in an unlucky relative position cost
    // ~12 %; reads hardly care): first the written state as a whole, then each of its planes
    // on its own against the others, then -- if allowed -- the read state.
    // (a tendency state's theta_i plane is never written -- d theta_i = 0 is kept by the zero bits --
    // so it does not take part)
    float b0 = 0, a0 = 0, b1 = 0, a1 = 0;
    uint32_t wmask = 0;
    for (int i = 0; i < LH_NVARS; ++i)
        if (written->plane[i] && !(dY && i == LH_VAR_THETA_I)) wmask |= 1u << i;
    if ((rc = tune_state_planes(c, written, wmask, max_candidates, false, run, &b0, &a0))) return rc;
    int nwritten = 0;
    for (int i = 0; i < LH_NVARS; ++i) nwritten += (wmask >> i) & 1u;
    for (int i = 0; i < LH_NVARS && nwritten > 1; ++i)
        if (wmask >> i & 1u) {
            if ((rc = tune_state_planes(c, written, 1u << i, max_candidates, false, run, &b1, &a1))) return rc;
            if (a1 < a0) a0 = a1; // b1 re-measures the placement a0 was measured on
        }
    if (flags & LH_PLACE_MOVE_INPUT) {
        if ((rc = tune_state_planes(c, Y, ~0u, max_candidates, true, run, &b1, &a1))) return rc;
        if (a1 < a0) a0 = a1;
    }
    if (ms_before) *ms_before = b0;
    if (ms_after) *ms_after = a0;
    return LH_OK;
}

int lh_block_range(int64_t ncols_global, int32_t rank, int32_t nranks, int64_t* lo, int64_t* hi) {
    if (!lo || !hi || nranks < 1 || rank < 0 || rank >= nranks || ncols_global < nranks) return LH_EINVAL;
    const int64_t q = ncols_global / nranks, r = ncols_global % nranks;
    *lo = rank * q + (rank < r ? rank : r);
    *hi = *lo + q + (rank < r ? 1 : 0);
    return LH_OK;
}

int lh_comm_unique_id(void* id_out) {
    static_assert(sizeof(ncclUniqueId) == LH_COMM_ID_BYTES, "LH_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    if (!id_out) return fail(nullptr, LH_EINVAL, "lh_comm_unique_id: NULL argument");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, LH_ENODEVICE, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    memcpy(id_out, &id, sizeof id);
    return LH_OK;
}

int lh_comm_init(lh_ctx* c, int32_t rank, int32_t nranks, const void* unique_id) {
    if (!c || !unique_id) return fail(c, LH_EINVAL, "lh_comm_init: NULL argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, LH_EINVAL, "lh_comm_init: rank %d outside [0, %d)", rank, nranks);
    if (c->comm) return fail(c, LH_EINVAL, "lh_comm_init: a communicator is already attached (lh_comm_destroy first)");
    (void)hipSetDevice(c->device);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, nranks, id, rank);
    if (r != ncclSuccess) return fail(c, LH_ENODEVICE, "ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, ncclGetErrorString(r));
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_nranks = nranks;
    return LH_OK;
}

int lh_comm_destroy(lh_ctx* c) {
    if (!c) return LH_EINVAL;
    if (!c->comm) return LH_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const ncclResult_t r = ncclCommDestroy(c->comm);
    c->comm = nullptr;
    c->comm_rank = 0;
    c->comm_nranks = 1;
    if (r != ncclSuccess) return fail(c, LH_ENODEVICE, "ncclCommDestroy failed: %s", ncclGetErrorString(r));
    return LH_OK;
}

int lh_comm_info(const lh_ctx* c, int32_t* rank, int32_t* nranks) {
    if (!c) return LH_EINVAL;
    if (rank) *rank = c->comm ? c->comm_rank : 0;
    if (nranks) *nranks = c->comm ? c->comm_nranks : 1;
    return LH_OK;
}

int lh_allreduce_min(lh_ctx* c, void* value_device_ft) {
    if (!c || !value_device_ft) return fail(c, LH_EINVAL, "lh_allreduce_min: NULL argument");
    (void)hipSetDevice(c->device);
    return allreduce_min(c, value_device_ft);
}

int lh_stream_probe(lh_ctx* c, const lh_state* in, uint32_t read_mask, lh_state* out, uint32_t write_mask,
                    int reps, float* ms_per_launch) {
    if (!c || !in || !out || !ms_per_launch) return fail(c, LH_EINVAL, "lh_stream_probe: NULL argument");
    if (in->ctx != c || out->ctx != c) return fail(c, LH_EINVAL, "state belongs to another context");
    if ((in->mask & read_mask) != read_mask || (out->mask & write_mask) != write_mask)
        return fail(c, LH_ESTATE, "lh_stream_probe: a selected plane does not exist");
    if (reps < 1) reps = 20;
    (void)hipSetDevice(c->device);
    {
        int rc;
        if ((rc = materialize(c, in, read_mask)) || (rc = materialize(c, out, write_mask))) return rc;
    }
    // the selected planes, packed to the front
    void *rp[4] = {nullptr, nullptr, nullptr, nullptr}, *wp[4] = {nullptr, nullptr, nullptr, nullptr};
    int nr = 0, nw = 0;
    for (int i = 0; i < LH_NVARS; ++i) {
        if (read_mask >> i & 1u) rp[nr++] = in->plane[i];
        if (write_mask >> i & 1u) wp[nw++] = out->plane[i];
    }
    const double touched = double(c->cfg.nlev) * double(c->stride) * double(c->esize) * (nr + nw);
    const bool nt = c->tune.nt >= 0 ? c->tune.nt != 0 : touched > 192.0 * 1024 * 1024; // as launch_rhs_model
    auto go = [&]() {
        with_ft(c, [&](auto ft) {
            using FT = decltype(ft);
            Planes<FT> pi, po;
            for (int k = 0; k < 4; ++k) pi.v[k] = static_cast<FT*>(rp[k]), po.v[k] = static_cast<FT*>(wp[k]);
            launch_stream_probe<FT>(c->cfg.ncols, c->stride, c->cfg.nlev, c->tune.xcd, pi, nr, po, nw, nt, c->stream);
        });
    };
    mark_written(out, write_mask);
    for (int r = 0; r < 3; ++r) go();
    LH_HIP(c, hipGetLastError());
    LH_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int r = 0; r < reps; ++r) go();
    LH_HIP(c, hipEventRecord(c->ev1, c->stream));
    LH_HIP(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    LH_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *ms_per_launch = ms / float(reps);
    return LH_OK;
}

int lh_timer_start(lh_ctx* c) {
    if (!c) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    LH_HIP(c, hipEventRecord(c->ev0, c->stream));
    return LH_OK;
}

int lh_timer_stop(lh_ctx* c, float* ms) {
    if (!c || !ms) return LH_EINVAL;
    (void)hipSetDevice(c->device);
    LH_HIP(c, hipEventRecord(c->ev1, c->stream));
    LH_HIP(c, hipEventSynchronize(c->ev1));
    LH_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return LH_OK;
}

} // extern "C"
