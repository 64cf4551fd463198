// gfx950 implicit steps of the coupled model (coupled_implicit_kernel), double
#define LH_TU_MODEL
#include "lh_coupled_implicit.hpp"
namespace lh {
LH_INSTANTIATE_COUPLED_IMPLICIT(double)
}
