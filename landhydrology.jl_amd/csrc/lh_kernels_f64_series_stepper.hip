// gfx950 kernels of lh_step_ssprk33_series (lh_series_stepper.hpp: the wave stepper under a boundary-value series and
// the per-step stage values of the fused path), double
#define LH_TU_MODEL
#define LH_LAYERED_TU // (what lh_series.hpp's second part includes; no kernel of these headers is instantiated here)
#define LH_LAYERED_IMPLICIT_TU
#define LH_SERIES_TU // (series_value, series_params)
#define LH_SERIES_STEPPER_TU
#include "lh_series_stepper.hpp"
namespace lh {
LH_INSTANTIATE_SERIES_STEPPER(double)
}
