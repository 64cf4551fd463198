// gfx950 implicit kernels of Richards soils with conductivity factors (lh_factors_implicit.hpp: backward Euler and
// TR-BDF2 with TemperatureDependentViscosity and / or IceImpedance), float
#define LH_FACTORS_IMPLICIT_TU
#include "lh_factors_implicit.hpp"
namespace lh {
LH_INSTANTIATE_FACTORS_IMPLICIT(float)
}
