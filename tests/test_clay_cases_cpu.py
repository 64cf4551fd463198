"""CPU-side guard of the clay-like cases (tests/clay_cases.py): what the REFERENCE alone must satisfy for
the GPU tests of tests/test_gpu_closure_forms.py to mean something.  For van Genuchten n in [1.03, 1.07]
the reference's own closures turn into rounding noise in dry cells, where the tolerance model of
tests/parity_cases.py is wide by design; the cases stay moist (S in [0.5, 1.1]), and this file asserts
that this is enough: no noise-valued cell, finite values, a tolerance that stays below the plain
statistic's 1e-13 of the field scale, and a stepped state that moves far more than the asserted bound.
If a seed fails a condition the seed or the generator's range changes, never the condition."""
import numpy as np
import pytest

import case_model as M
import clay_cases as cc
import parity_cases as pc

O = pc.O


@pytest.mark.parametrize("spec", cc.RHS_CASES + cc.STEP_CASES, ids=lambda s: "-".join(str(x) for x in s))
def test_the_reference_is_well_conditioned_on_the_clay_cases(spec):
    case = cc.clay_case(*spec)
    assert not cc.ill_cells(case).any()
    diag = O.diagnostics(case.om, case.vl, case.ti, case.rhoe, case.T_aux)
    for k, v in diag.items():
        if case.om.model == M.MODEL_RICHARDS and k in ("T", "kappa"):
            continue
        assert np.all(np.isfinite(v)), k
    want = pc.run_oracle_rhs(case)
    for k, v in want.items():
        assert np.all(np.isfinite(v)), k
    # the model cannot be satisfied by an error that is visible at field scale
    tol = pc.tendency_tolerance(case, 4.0)
    scale = np.max(np.abs(want["vl"]))
    assert scale > 0 and tol["vl"].max() < pc.PLAIN_REL[np.dtype(np.float64)] * scale, (tol["vl"].max(), scale)
    # every column is clay-like by the host's rule, or (mixed) the two clay columns are
    n = pc._percol(case, "vg_n", case.om.vg.n)
    assert (1.0 - 1.0 / n.min()) < 0.07 * 1.001


@pytest.mark.parametrize("spec", cc.STEP_CASES, ids=lambda s: "-".join(str(x) for x in s))
def test_the_reference_state_moves_far_more_than_the_asserted_bound(spec):
    case = cc.clay_case(*spec)
    dt = O.stable_dt(case.om, case.vl, case.ti, case.rhoe, cc.STEP_COURANT, case.T_aux)
    assert np.isfinite(dt) and dt > 0
    vl = case.vl.copy()
    rhoe = None if case.rhoe is None else case.rhoe.copy()
    O.ssprk33(case.om, dt, cc.STEP_COUNT, vl=vl, ti=case.ti.copy(), rhoe=rhoe, T_aux=case.T_aux)
    assert np.all(np.isfinite(vl))
    moved = np.max(np.abs(vl - case.vl))
    assert moved >= 100 * cc.STEP_BOUND * np.max(np.abs(vl)), (moved, dt)
    assert not cc.ill_cells(pc.Case("end", case.om, case.dtype, case.ncols, vl=vl, ti=case.ti)).any()


def test_bone_dry_clay_in_the_reference():
    """What the GPU test of the bone-dry columns relies on: the reference's K is exactly 0 in all 18
    columns, psi is finite or -Inf (S^(-1/m) overflowed), and the moist columns around them are
    well conditioned."""
    case, nd = cc.dry_clay_columns(moist=46)
    diag = O.diagnostics(case.om, case.vl, case.ti)
    assert nd == 18 and np.all(diag["K"][:nd] == 0.0)
    psi = diag["psi"][:nd]
    assert np.all(np.isfinite(psi) | np.isneginf(psi)) and np.isneginf(psi).any() and np.isfinite(psi).any()
    assert not cc.ill_cells(case)[nd:].any()
    assert np.all(np.isfinite(diag["K"][nd:])) and np.all(np.isfinite(diag["psi"][nd:]))
    want = pc.run_oracle_rhs(case)
    assert np.all(np.isfinite(want["vl"][nd:]))


@pytest.mark.parametrize("model", cc.MODELS, ids=["richards", "coupled"])
def test_the_numpy_references_converge_on_the_family_cases(model):
    """The implicit families' clay-like runs compare with the NumPy references: those must themselves converge in
    every column (they cycle at the saturation kink on some seeds), on a case without a noise-valued cell."""
    import coupled_implicit_ref as CR
    import implicit_ref as IR
    case = cc.family_case(model)
    assert not cc.ill_cells(case).any()
    dt = cc.FAMILY_STEP * O.stable_dt(case.om, case.vl, case.ti, case.rhoe, 0.5)
    if model == M.MODEL_RICHARDS:
        _, iters = IR.implicit_euler(case.om, case.vl, case.ti, dt, 1)
        assert iters.max() < 120
    else:
        for method in ("euler", "trbdf2"):
            _, _, info = CR.coupled_implicit(case.om, *CR.f64(case), dt, 1, method)
            assert info["unconverged"] == 0 and info["iters"] < 120, (method, info)


def test_the_layered_clay_case_is_moist_in_every_class():
    import layered_implicit_ref as LI
    import layered_ref as R
    lay = cc.layered_clay_case()
    assert {3, 11} <= set(np.unique(lay.class_map).tolist()) and np.all(lay.classes[[3, 11], 0] == cc.MIXED_CLAY_N)
    p = R.cell_params(lay)
    S = (lay.case.vl - p["theta_r"]) / (p["nu"] - p["theta_r"])
    assert S.min() >= 0.5 and S.max() <= 1.1
    m = 1.0 - 1.0 / p["n"]
    with np.errstate(all="ignore"):
        t = np.where(S < 1, S ** (1.0 / m), 1.0)
        inner = np.where(S < 1, 1.0 - (1.0 - t) ** m, 1.0)
    assert np.all(inner >= 64 * np.finfo(np.float64).eps)
    _, iters = LI.implicit_euler(lay, cc.FAMILY_STEP * R.stable_dt(lay), 1)
    assert np.max(iters) < 120
