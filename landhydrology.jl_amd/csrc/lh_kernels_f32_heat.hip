// gfx950 column kernels (rhs_kernel), float, heat model
#define LH_TU_MODEL
#include "lh_kernels_impl.hpp"
#include "lh_heat_implicit.hpp"
namespace lh {
LH_INSTANTIATE_MODEL(float, MODEL_HEAT)
LH_INSTANTIATE_HEAT_IMPLICIT(float)
}
