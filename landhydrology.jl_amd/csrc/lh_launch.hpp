// lh_launch.hpp -- host-callable launchers implemented in lh_kernels.hip.
#pragma once
#include "lh_device.hpp"

namespace lh {

enum { MATH_FAST = 0, MATH_LIBM = 1 };

template <int CPL_, int PF_, bool NT_, bool SEG_ = false> struct KCfg;
// production launch shape per working type (chosen by measurement)
template <typename FT> struct DefaultCfg;
// (Float64: 2 levels in flight ahead of the one computed, -2..3 % against 1, profiles/round1_tune_prefetch.txt)
template <> struct DefaultCfg<double> { using type = KCfg<1, 2, false>; };
template <> struct DefaultCfg<float> { using type = KCfg<2, 1, false>; };

// run-time launch overrides (LH_TUNE environment variable, lh_set_tuning): one field per key parse_tune scans for
struct Tune {
    int block = 0; // threads per workgroup of the column kernel (0: the kernel's own, see rhs_max_threads)
    int nt = -1;   // nontemporal global access (-1: by the bytes the launch streams, see launch_rhs_model)
    int pad = -1; // plane address stagger in bytes (state allocation)
    int arena = 0; // plane slots per device allocation (0 = default)
    int rowpad = -1; // extra elements per plane row (-1 = library default)
    int seg = 0;     // levels per segment of the level-segmented launch (0 = automatic, -1 = never)
    int cpb = 0;     // persistent column stepper: columns per workgroup (0 = default)
    int persist = 1; // persistent column stepper (0: fused-stage launches instead)
    int graph = 1;   // replay blocks of fused SSPRK33 steps of small ensembles as a hipGraph (0: plain launches)
    int xcd = 1;     // XCD-contiguous workgroup map (0: workgroup b = column block b)
    int place_mem = 0;  // lh_tune_placement: transient memory bound, percent of free memory (0 = 25)
    int zero = 1;    // use the states' known-zero plane bits (0: always read theta_i and store d theta_i = 0)
    int vgfast = 1;  // Float64: integer-exponent 2^(.) in the water closures when every column allows it (0: v_ldexp form always)
    // lh_integrate_trbdf2: the stage Newton test kappa in units of 1e-4 and its iteration cap
    int trk = 0, trn = 0;
};

// mode 0: tendency into `out`; 4: tendency + step bound; 1..3, 5: fused SSPRK33 stages (see rhs_kernel)
template <typename FT>
void launch_rhs(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                const Planes<FT>& base, const Planes<FT>& out, FT dt, const FT* dt_dev, int mode,
                bool factors, bool percol, bool noice, int math, const Tune& tune, hipStream_t s);
// nsteps fused SSPRK33 steps of a small ensemble in ONE launch (workgroup = column, thread = cell)
template <typename FT>
void launch_column_stepper(const DevParams<FT>& P, const Planes<FT>& Y, const Planes<FT>& aux, FT dt,
                           const FT* dt_dev, int64_t nsteps, const FT* bcv, bool factors, bool percol,
                           bool noice, bool bound, hipStream_t s);
template <typename FT>
void launch_diag(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                 const Planes<FT>& out, bool percol, int math, hipStream_t s);
// boundary_fluxes of one face for every column (lh_boundary_fluxes): FT[ncols] each
template <typename FT>
void launch_boundary_fluxes(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux, int face, FT* out_e,
                            FT* out_w, bool factors, bool percol, int math, hipStream_t s);
template <typename FT>
void launch_stable_dt(const DevParams<FT>& P, const Planes<FT>& in, const Planes<FT>& aux,
                      FT courant, void* out_ft, bool percol, hipStream_t s);
template <typename FT>
void launch_strided_copy(FT* plane, int64_t stride, FT* user, int64_t ls, int64_t cs,
                         int64_t ncols, int nlev, bool to_plane, hipStream_t s);
// the column launch's access pattern without arithmetic: nr planes of `in` read, nw planes of `out` written
template <typename FT>
void launch_stream_probe(int64_t ncols, int64_t stride, int nlev, int xcd_remap, const Planes<FT>& in, int nr,
                         const Planes<FT>& out, int nw, bool nt, hipStream_t s);
// compute_turbulent_surface_fluxes for n top-cell states (lh_atmos.hpp)
template <typename FT>
void launch_atmos_flux(const DevParams<FT>& P, const AtmosParams<FT>& A, int64_t n, bool from_state, bool percol,
                       const FT* vl, const FT* ti, const FT* third, FT* out_heat, FT* out_water, hipStream_t s);
template <typename FT>
void launch_fill(FT* p, int64_t n, FT v, hipStream_t s);
// plane[lev][col] = prof[lev]: a level-uniform variable made a plane (lh_upload_profile)
template <typename FT>
void launch_broadcast_profile(FT* plane, const FT* prof, int64_t ncols, int64_t stride, int nlev, hipStream_t s);
// one thread: dt = min(dt, dt_max), elapsed += dt (lh_step_ssprk33_adaptive)
template <typename FT>
void launch_dt_prepare(FT* dt, FT dt_max, FT* elapsed, uint32_t* status, hipStream_t s);
// one thread between two chunks of lh_step_ssprk33_adaptive_hold: the overrun check of the chunk that
// ended (check), the next chunk's dt from *bound and elapsed += dt, hold times (hold > 0)
template <typename FT>
void launch_dt_hold_prepare(FT* dt, const FT* bound, FT dt_max, FT* elapsed, int hold, bool check, uint32_t* status, hipStream_t s);
// nsteps backward-Euler steps of a Richards model in one launch (lh_implicit.hpp)
template <typename FT>
void launch_implicit_euler(const DevParams<FT>& P, const ImplicitArgs<FT>& A, bool percol, bool noice, int math,
                           hipStream_t s);
// TR-BDF2 of a Richards model over [t0, t1], per-column step control, in one launch (lh_implicit.hpp)
template <typename FT>
void launch_trbdf2(const DevParams<FT>& P, const Trbdf2Args<FT>& A, bool percol, bool noice, int math, hipStream_t s);
// nsteps backward-Euler or fixed-step TR-BDF2 steps of a heat-only model in one launch (lh_heat_implicit.hpp)
template <typename FT>
void launch_heat_implicit(const DevParams<FT>& P, const HeatImplicitArgs<FT>& A, bool percol, bool trbdf2, int math,
                          hipStream_t s);
// nsteps backward-Euler or fixed-step TR-BDF2 steps of a coupled model in one launch (lh_coupled_implicit.hpp)
template <typename FT>
void launch_coupled_implicit(const DevParams<FT>& P, const CoupledImplicitArgs<FT>& A, bool percol, bool noice,
                             bool trbdf2, int math, hipStream_t s);
// TR-BDF2 of a coupled model over [t0, t1], per-column step control, in one launch (lh_coupled_trbdf2.hpp)
template <typename FT>
void launch_coupled_trbdf2(const DevParams<FT>& P, const CoupledTrbdf2Args<FT>& A, bool percol, bool noice, int math,
                           hipStream_t s);
template <typename FT>
void launch_convert(FT* dst, const double* src, int64_t n, hipStream_t s);

} // namespace lh
