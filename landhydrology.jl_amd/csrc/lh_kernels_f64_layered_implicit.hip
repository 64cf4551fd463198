// gfx950 implicit kernels of layered soils (lh_layered_implicit.hpp: backward Euler and TR-BDF2 with per-cell
// soil classes), double
#define LH_LAYERED_TU // (stage_class_table; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_IMPLICIT_TU
#include "lh_layered_implicit.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_IMPLICIT(double)
}
