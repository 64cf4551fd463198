// gfx950 layered-soil heat kernels (lh_layered_heat.hpp: per-cell soil classes, coupled and heat-only models), double
#define LH_LAYERED_TU
#define LH_LAYERED_HEAT_TU
#include "lh_layered_heat.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_HEAT(double)
}
