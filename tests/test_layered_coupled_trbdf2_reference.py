"""tests/layered_coupled_trbdf2_ref.py, the NumPy reference of lh_integrate_layered_coupled_trbdf2, on the CPU: against
the scalar reference (tests/coupled_trbdf2_ref.py) on a map whose columns are one class each, the single-attempt
conditions the GPU tests rest on, the integrator against layered_heat_ref.ssprk33, and the block-diagonal error
filter against the full block-triangular one.  Cases A-D of layered_coupled_trbdf2_ref.CASES, Float64; tolerances
abstol 1e-6, abstol_e 1e-6 rho_l c_l, reltol 1e-3 unless stated."""
import numpy as np
import pytest

import coupled_implicit_ref as CR
import coupled_trbdf2_ref as CT
import layered_coupled_implicit_ref as LC
import layered_coupled_trbdf2_ref as LT
import layered_heat_ref as LH
import case_model as M

NAMES = sorted(LT.CASES)
_CASES = {}


def case(name):
    if name not in _CASES:
        lay = LT.make_case(name)
        _CASES[name] = (lay, LC.stable_dt(lay))
    return _CASES[name]


def test_the_default_energy_tolerance_is_the_scalar_reference_s():
    lay, _ = case("A")
    assert LT.abstol_e_default(lay) == CT.abstol_e_default(lay.case.om)
    assert (LT.GAMMA, LT.D, LT.B, LT.HMIN_FRAC) == (CT.GAMMA, CT.D, CT.B, CT.HMIN_FRAC)
    assert LT.device_newton() == CT.device_newton()


def test_column_uniform_map_agrees_with_the_scalar_reference():
    """12 columns x 12 levels, every column one of 3 classes, ice, Dirichlet top / free drainage, Dirichlet energy:
    over 16 stable steps from h0 = the stable step under the device's Newton rule the layered integrator agrees with
    coupled_trbdf2_ref.integrate on the per-class scalar twins (layered_heat_ref.per_class_cases) with the same
    accepted and rejected counts in every column, vartheta_l to 1e-10 -- the Float64 parity bound of
    test_layered_implicit_reference.py's column-uniform check -- and rhoe_int to the same 1e-10 of max |rhoe_int|
    (rhoe_int is of order 1e7 to 1e8 J/m^3, vartheta_l of order 1: the bound is relative to the variable's size)."""
    lay = LC.layered_case(np.float64, 12, 12, kind="columns", hyd=(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), energy="dirichlet", ice=True)
    sd = LC.stable_dt(lay)
    v, e = LC.state64(lay)
    T = 16 * sd
    gv, ge, gi = LT.integrate(lay, v, e, 0.0, T, sd, newton=LT.device_newton())
    assert not gi["failed"].any() and np.max(np.abs(gv - v)) > 1e-6
    for cols, scalar in LH.per_class_cases(lay):
        sv, sti, se = CR.f64(scalar)
        wv, we, wi = CT.integrate(scalar.om, sv, sti, se, 0.0, T, sd, newton=CT.device_newton())
        err_v = float(np.max(np.abs(gv[cols] - wv)))
        err_e = float(np.max(np.abs(ge[cols] - we))) / float(np.max(np.abs(we)))
        print(f"columns {cols}: vl {err_v:.3g}, rhoe (relative) {err_e:.3g}, accepted {gi['accepted'][cols]}, rejected {gi['rejected'][cols]}")
        assert np.array_equal(gi["accepted"][cols], wi["accepted"]) and np.array_equal(gi["rejected"][cols], wi["rejected"])
        assert err_v <= 1e-10 and err_e <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_single_attempt_conditions(name):
    """What the GPU tests' accept / reject assertions rest on, under the device's Newton rule: at 0.25 and 1 stable
    step every column has E <= 0.5 and both water stages converge; at 64 stable steps every column has E >= 1.4 or a
    stage that did not converge.  (4 and 16 stable steps straddle E = 1 and are not used.)"""
    lay, sd = case(name)
    for mult in (0.25, 1.0):
        r, E = LT.first_attempt(lay, mult * sd, newton=LT.device_newton())
        print(f"{name} {mult}x: E {E.min():.3g} .. {E.max():.3g}, Newton iterations {r['iters']}")
        assert np.all(r["conv"]) and np.all(E <= 0.5), (mult, E, r["conv"])
    r, E = LT.first_attempt(lay, 64.0 * sd, newton=LT.device_newton())
    print(f"{name} 64x: E {E.min():.3g} .. {E.max():.3g}, converged {r['conv']}")
    assert np.all((E >= 1.4) | ~r["conv"]), (E, r["conv"])


@pytest.mark.parametrize("name", NAMES)
def test_integrator_against_ssprk33(name):
    """64 stable steps from h0 = the stable step at reltol 1e-3 and 1e-4 under the device's Newton rule: no column
    fails, every column lands on t1, and the error against layered_heat_ref.ssprk33 at a quarter of the stable step
    falls from reltol 1e-3 to 1e-4 in both variables."""
    lay, sd = case(name)
    want = LT.ssprk33_reference(name, lay)
    last = None
    for reltol in (1e-3, 1e-4):
        v1, e1, info = LT.integrated(name, lay, reltol)
        err = (float(np.max(np.abs(v1 - want[0]))), float(np.max(np.abs(e1 - want[1]))))
        print(f"{name} reltol {reltol}: accepted {info['accepted']}, rejected {info['rejected']}, errors {err[0]:.3g} {err[1]:.3g}, "
              f"the state moved by {np.max(np.abs(want[0] - LC.state64(lay)[0])):.3g}")
        assert not info["failed"].any() and np.all(info["t"] == LT.SPAN * sd)
        if last is not None:
            assert err[0] < last[0] and err[1] < last[1], (err, last)
        last = err


def test_the_columns_choose_their_own_steps():
    """In each of the cases A-D at reltol 1e-4 the columns do not all take the same number of attempted steps (the
    counts are printed): the per-column controller is exercised."""
    differ = []
    for name in NAMES:
        lay, _ = case(name)
        _, _, info = LT.integrated(name, lay, 1e-4)
        steps = info["accepted"] + info["rejected"]
        print(f"{name}: attempted steps per column {steps}")
        differ.append(len(set(steps.tolist())) > 1)
    assert all(differ), differ


def test_block_diagonal_filter_against_the_full_one():
    """Case A at 1, 16 and 64 stable steps (round-off Newton): the block-diagonal E the device forms against the E of
    the full block-triangular filter, per column.  Measured gaps max |E / E_full - 1|: 7.9 % at 1x (E 0.068 against
    0.063), 21 % at 16x (column 1; the others at most 7.6 %) and 3.3 % at 64x -- far more than the scalar cases'
    0.27 % (tests/test_coupled_trbdf2_reference.py): across a horizon interface K jumps by more than 100, and with
    it d f_e / d vartheta_l, the block the diagonal filter drops.  The gap is held to what the controller itself
    allows for: the step is h 0.9 E^(-1/3), and its safety factor 0.9 absorbs an E that is low by 0.9^-3 - 1 = 37 %;
    inside that the two filters propose steps within the safety factor of each other."""
    lay, sd = case("A")
    allowed = 0.9 ** -3 - 1.0
    for mult in (1.0, 16.0, 64.0):
        r, E = LT.first_attempt(lay, mult * sd)
        full, Ef = LT.first_attempt(lay, mult * sd, block="full")
        np.testing.assert_array_equal(full["v1"], r["v1"])
        gap = float(np.max(np.abs(E / Ef - 1.0)))
        print(f"A {mult}x: E {E.max():.4g}, full {Ef.max():.4g}, gap {gap:.3g} (per column {np.round(E / Ef - 1.0, 4)})")
        assert gap <= allowed, (mult, E, Ef)
        assert np.max(np.abs(full["ee"] - r["ee"])) > 0
