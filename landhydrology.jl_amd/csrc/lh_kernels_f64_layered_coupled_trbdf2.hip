// gfx950 adaptive TR-BDF2 kernels of layered coupled soils (lh_layered_coupled_trbdf2.hpp: error-controlled steps of
// water and heat with per-cell soil classes and their thermal supplement), double
#define LH_LAYERED_TU                  // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_HEAT_TU             // (stage_therm_table and the two closures; no kernel of lh_layered_heat.hpp either)
#define LH_LAYERED_IMPLICIT_TU         // (layered_newton_stage, layered_sweep_up, layered_face_states; no kernel of lh_layered_implicit.hpp)
#define LH_LAYERED_COUPLED_IMPLICIT_TU // (layered_energy_sweep_up, layered_energy_face; no kernel of lh_layered_coupled_implicit.hpp)
#define LH_LAYERED_COUPLED_TRBDF2_TU
#include "lh_layered_coupled_trbdf2.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_COUPLED_TRBDF2(double)
}
