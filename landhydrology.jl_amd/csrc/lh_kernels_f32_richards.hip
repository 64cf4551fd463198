// gfx950 column kernels (rhs_kernel), float, richards model
#define LH_TU_MODEL
#include "lh_kernels_impl.hpp"
#include "lh_implicit.hpp"
namespace lh {
LH_INSTANTIATE_MODEL(float, MODEL_RICHARDS)
LH_INSTANTIATE_IMPLICIT(float)
}
