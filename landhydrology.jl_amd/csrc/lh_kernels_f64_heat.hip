// gfx950 column kernels (rhs_kernel), double, heat model
#define LH_TU_MODEL
#include "lh_kernels_impl.hpp"
#include "lh_heat_implicit.hpp"
namespace lh {
LH_INSTANTIATE_MODEL(double, MODEL_HEAT)
LH_INSTANTIATE_HEAT_IMPLICIT(double)
}
