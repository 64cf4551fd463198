// gfx950 dense-output kernels of layered coupled soils (lh_dense_layered_coupled.hpp:
// lh_integrate_layered_coupled_dense over layered_coupled_trbdf2_column), double
#define LH_TU_MODEL
#define LH_LAYERED_TU                  // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_HEAT_TU             // (stage_therm_table and the two closures; no kernel of lh_layered_heat.hpp either)
#define LH_LAYERED_IMPLICIT_TU         // (layered_newton_stage, layered_sweep_up, layered_face_states; no kernel of lh_layered_implicit.hpp)
#define LH_LAYERED_COUPLED_IMPLICIT_TU // (layered_energy_sweep_up, layered_energy_face; no kernel of lh_layered_coupled_implicit.hpp)
#define LH_LAYERED_COUPLED_TRBDF2_TU   // (layered_coupled_trbdf2_column; no kernel of lh_layered_coupled_trbdf2.hpp)
#define LH_SERIES_TU                   // (series_sub_interval and its neighbours; no kernel of lh_series.hpp)
#define LH_DENSE_OUTPUT_TU             // (DenseOutput, dense_walk; no kernel of lh_dense.hpp)
#define LH_DENSE_LAYERED_COUPLED_TU
#include "lh_dense_layered_coupled.hpp"
namespace lh {
LH_INSTANTIATE_DENSE_LAYERED_COUPLED(double)
}
