// gfx950 adaptive TR-BDF2 of the coupled model (coupled_trbdf2_kernel), double
#define LH_TU_MODEL
#include "lh_coupled_trbdf2.hpp"
namespace lh {
LH_INSTANTIATE_COUPLED_TRBDF2(double)
}
