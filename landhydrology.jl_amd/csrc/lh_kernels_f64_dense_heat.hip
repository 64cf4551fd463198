// gfx950 dense-output kernels of the heat-only model (lh_dense_heat.hpp: lh_integrate_heat_dense over
// heat_trbdf2_column with the scalar and the layered CELLS objects), double
#define LH_TU_MODEL
#define LH_LAYERED_TU               // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_IMPLICIT_TU      // (what lh_series.hpp's own kernel templates name; none of them is instantiated here)
#define LH_LAYERED_HEAT_TU          // (stage_therm_table and the two closures; no kernel of lh_layered_heat.hpp either)
#define LH_LAYERED_HEAT_IMPLICIT_TU // (ThermView; no kernel of lh_layered_heat_implicit.hpp)
#define LH_HEAT_TRBDF2_TU           // (heat_trbdf2_column, HeatCells; no kernel of lh_heat_trbdf2.hpp)
#define LH_LAYERED_HEAT_TRBDF2_TU   // (LayeredHeatCells; no kernel of lh_layered_heat_trbdf2.hpp)
#define LH_SERIES_TU                // (series_sub_interval and its neighbours; no kernel of lh_series.hpp)
#define LH_DENSE_OUTPUT_TU          // (DenseOutput, dense_walk; no kernel of lh_dense.hpp)
#define LH_DENSE_HEAT_TU
#include "lh_dense_heat.hpp"
namespace lh {
LH_INSTANTIATE_DENSE_HEAT(double)
}
