// gfx950 dense-output kernels (lh_dense.hpp: lh_integrate_dense over the scalar, the layered and the coupled TR-BDF2
// column routines), float
#define LH_TU_MODEL
#define LH_LAYERED_TU // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_IMPLICIT_TU // (layered_trbdf2_column; no kernel of lh_layered_implicit.hpp is instantiated here)
#define LH_SERIES_TU // (series_sub_interval and its neighbours; no kernel of lh_series.hpp)
#define LH_DENSE_TU
#include "lh_dense.hpp"
namespace lh {
LH_INSTANTIATE_DENSE(float)
}
