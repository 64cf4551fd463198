// gfx950 persistent column stepper of layered soils (lh_layered_stepper.hpp: one wave per column, per-cell soil
// classes, Richards model), double
#define LH_LAYERED_TU // (stage_class_table, layered_variant_exists; no kernel of lh_layered.hpp is instantiated here)
#define LH_LAYERED_STEPPER_TU
#include "lh_layered_stepper.hpp"
namespace lh {
LH_INSTANTIATE_LAYERED_STEPPER(double)
}
