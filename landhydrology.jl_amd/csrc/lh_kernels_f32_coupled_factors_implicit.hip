// gfx950 implicit steps of the coupled model with the IceImpedance factor (coupled_factors_implicit_kernel,
// lh_coupled_factors_implicit.hpp), float
#define LH_TU_MODEL
#define LH_FACTORS_IMPLICIT_TU
#define LH_COUPLED_FACTORS_IMPLICIT_TU
#include "lh_coupled_factors_implicit.hpp"
namespace lh {
LH_INSTANTIATE_COUPLED_FACTORS_IMPLICIT(float)
}
