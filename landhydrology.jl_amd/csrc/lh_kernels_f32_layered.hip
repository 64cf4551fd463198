// gfx950 layered-soil kernels (lh_layered.hpp: per-cell soil classes, Richards model), float
#define LH_LAYERED_TU
#include "lh_layered.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED(float)
}
