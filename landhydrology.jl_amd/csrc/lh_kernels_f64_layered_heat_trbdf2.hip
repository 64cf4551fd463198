// gfx950 adaptive TR-BDF2 of layered heat-only soils (layered_heat_trbdf2_kernel, lh_layered_heat_trbdf2.hpp:
// error-controlled steps with per-cell soil classes and their thermal supplement), double
#define LH_LAYERED_TU               // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_HEAT_TU          // (stage_therm_table and the two closures; no kernel of lh_layered_heat.hpp either)
#define LH_LAYERED_HEAT_IMPLICIT_TU // (ThermView; no kernel of lh_layered_heat_implicit.hpp)
#define LH_HEAT_TRBDF2_TU           // (heat_trbdf2_column; no kernel of lh_heat_trbdf2.hpp)
#define LH_LAYERED_HEAT_TRBDF2_TU
#include "lh_layered_heat_trbdf2.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_HEAT_TRBDF2(double)
}
