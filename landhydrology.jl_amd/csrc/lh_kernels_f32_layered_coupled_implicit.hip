// gfx950 implicit kernels of layered coupled soils (lh_layered_coupled_implicit.hpp: backward Euler and fixed-step
// TR-BDF2 of water and heat with per-cell soil classes and their thermal supplement), float
#define LH_LAYERED_TU          // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_HEAT_TU     // (stage_therm_table and the two closures; no kernel of lh_layered_heat.hpp either)
#define LH_LAYERED_IMPLICIT_TU // (layered_newton_stage, layered_sweep_up, layered_face_states; no kernel of lh_layered_implicit.hpp)
#define LH_LAYERED_COUPLED_IMPLICIT_TU
#include "lh_layered_coupled_implicit.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_COUPLED_IMPLICIT(float)
}
