// gfx950 column kernels (rhs_kernel), double, richards model
#define LH_TU_MODEL
#include "lh_kernels_impl.hpp"
#include "lh_implicit.hpp"
namespace lh {
LH_INSTANTIATE_MODEL(double, MODEL_RICHARDS)
LH_INSTANTIATE_IMPLICIT(double)
}
