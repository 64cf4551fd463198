"""NumPy reference for the adaptive TR-BDF2 of a LAYERED heat-only model (lh_integrate_layered_heat_trbdf2, DESIGN
section 4.27): heat_trbdf2_ref's integrator (its attempt, error norm, controller and FT rounding) on
layered_heat_implicit_ref's tendency and bands.  Needs neither the oracle's tendency nor the library.

Test infrastructure (tests/test_layered_heat_trbdf2_reference.py, tests/test_gpu_layered_heat_trbdf2.py)."""
from __future__ import annotations

import case_model as M
import heat_trbdf2_ref as T
import layered_heat_implicit_ref as LI
import layered_heat_ref as LH
import layered_ref as R

attempt, integrate, fixed_trbdf2, error_norm, step_factor = T.attempt, T.integrate, T.fixed_trbdf2, T.error_norm, T.step_factor
true_local_error, fresh_tendency, abstol_e_default = T.true_local_error, T.fresh_tendency, T.abstol_e_default


def sixteen_class_case(dtype, ncols, nlev, ice=False):
    """all 16 classes of layered_ref.texture_classes with their thermal supplement, another class in every cell,
    Dirichlet faces"""
    return LH.make_layered_heat(dtype, ncols, nlev, LI.cell_map(ncols, nlev, 16), model=M.MODEL_HEAT, classes=R.texture_classes(),
                                thermal=LH.thermal_classes(), bc="dirichlet", ice=ice, name="layered_heat_trbdf2")


def problem(lay, bands=None):
    """The Problem of a layered_heat_ref case (its Float64 twin).  bands: affine_parts(lay)[0] where the caller has it."""
    if bands is None:
        bands, _ = LI.affine_parts(lay)
    return T.Problem(lay.case.om, lambda y, smp: LI.tendency(lay, y, smp), bands, lay.case.vl.shape)
