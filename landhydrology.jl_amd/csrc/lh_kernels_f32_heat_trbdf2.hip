// gfx950 adaptive TR-BDF2 of the heat-only model (heat_trbdf2_kernel, lh_heat_trbdf2.hpp), float
#define LH_TU_MODEL
#define LH_HEAT_TRBDF2_TU
#include "lh_heat_trbdf2.hpp"
namespace lh {
LH_INSTANTIATE_HEAT_TRBDF2(float)
}
