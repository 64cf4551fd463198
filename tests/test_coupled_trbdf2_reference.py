"""tests/coupled_trbdf2_ref.py, the NumPy reference of lh_integrate_coupled_trbdf2, on the CPU: the quality of the
block-diagonal error estimate against the true local error, against the full block-triangular filter and
against no filter, and the integrator against oracle SSPRK33.  4 columns x 64 levels of the two cases below;
tolerances abstol 1e-6, abstol_e 1e-6 rho_l c_l = 4.181, reltol 1e-3."""
import numpy as np
import pytest

import case_model as M
import coupled_implicit_ref as CR
import coupled_trbdf2_ref as CT

CASES = {"iced": lambda: CR.coupled_case(M.BC_DIRICHLET, M.BC_FREE_DRAINAGE, ncols=4, ice=True),
         "flux": lambda: CR.coupled_case(M.BC_FLUX, M.BC_FLUX, ncols=4)}
MULTS = (0.25, 1.0, 4.0, 16.0, 64.0, 256.0)
_START = {}   # per case: (case, vl, ti, rhoe, f_w, f_e, stable step), computed once, never modified


def start(name):
    if name not in _START:
        case = CASES[name]()
        v, ti, e = CR.f64(case)
        fv, fe = CR.tendencies(case.om, v, ti, e)
        _START[name] = (case, v, ti, e, fv, fe, CR.stable_dt(case))
    return _START[name]


def norms(name, r, v, e, water="ev", energy="ee"):
    """E of the fields `water`, `energy` of an attempt's dict, per column."""
    om = start(name)[0].om
    ev, ee = r[water], r[energy]
    return CT.error_norm(ev, ee, v, r["v1"], e, r["e1"], CT.ABSTOL, CT.abstol_e_default(om), CT.RELTOL)


def test_the_default_energy_tolerance_is_that_of_a_microkelvin_in_water():
    om = start("iced")[0].om
    assert CT.abstol_e_default(om) == 1e-6 * (om.earth.cp_l * om.earth.rho_liq)
    assert abs(CT.abstol_e_default(om) - 4.18) < 0.01


@pytest.mark.parametrize("name", sorted(CASES))
def test_estimate_over_true_local_error(name):
    """E of one step over the same norm of Y_1 - (32 TR-BDF2 sub-steps of h / 32), per column, within [0.9, 1.15]
    at 0.25x and 1x the stable step.  Measured: iced 1.008-1.010 and 1.048-1.061, flux 1.010 and 1.063-1.064
    (E itself: iced 0.0150 and 0.615, flux 0.0122 and 0.468 in the worst column)."""
    case, v, ti, e, fv, fe, sd = start(name)
    for mult in (0.25, 1.0):
        h = mult * sd
        r = CT.attempt(case.om, v, e, fv, fe, ti, 0.0, h)
        vf, ef, info = CR.coupled_implicit(case.om, v, ti, e, h / 32, 32, "trbdf2")
        assert info["unconverged"] == 0 and np.all(r["conv"])
        E = norms(name, r, v, e)
        true = norms(name, dict(r, dv=r["v1"] - vf, de=r["e1"] - ef), v, e, water="dv", energy="de")
        print(f"{name} {mult}x: E {E}, E / true {E / true}")
        assert np.all(E / true >= 0.9) and np.all(E / true <= 1.15), (mult, E / true)


@pytest.mark.parametrize("name", sorted(CASES))
def test_block_diagonal_filter_against_the_full_one_and_none(name):
    """From 0.25x to 256x the stable step the block-diagonal E is within 1 % of the E of the full block-triangular
    filter (measured: the largest gap 0.27 %, iced at 256x, 176.0 against 175.5; below 3e-4 up to 64x), and at
    256x the unfiltered r is at least 10x the filtered estimate (measured: 27x iced, 36x flux)."""
    case, v, ti, e, fv, fe, sd = start(name)
    for mult in MULTS:
        h = mult * sd
        r = CT.attempt(case.om, v, e, fv, fe, ti, 0.0, h)
        full = CT.attempt(case.om, v, e, fv, fe, ti, 0.0, h, block="full")
        np.testing.assert_array_equal(full["v1"], r["v1"])
        E, Ef, Eu = norms(name, r, v, e), norms(name, full, v, e), norms(name, r, v, e, water="rv", energy="re")
        print(f"{name} {mult}x: E {E.max():.4g}, full {Ef.max():.4g}, gap {np.max(np.abs(E / Ef - 1)):.3g}, "
              f"unfiltered / E {np.min(Eu / E):.3g}")
        assert np.all(np.abs(E / Ef - 1.0) <= 0.01), (mult, E, Ef)
        assert np.max(np.abs(full["ee"] - r["ee"])) > 0
        if mult == 256.0:
            assert np.all(Eu >= 10.0 * E), (Eu / E)


# measured with this reference over 64 stable steps from h0 = the stable step, per reltol: (accepted steps of the
# four columns, rejected steps, max |error| in vartheta_l and rhoe_int against oracle SSPRK33 at sd / 8)
MEASURED = {
    "iced": {1e-3: ((14, 10, 10, 10), (0, 0, 0, 0), 2.03e-5, 2.12e4),
             1e-4: ((29, 19, 20, 19), (2, 1, 1, 1), 6.91e-6, 7.10e3),
             1e-5: ((57, 39, 40, 39), (2, 2, 2, 2), 1.66e-6, 1.68e3)},
    "flux": {1e-3: ((10, 10, 10, 10), (0, 0, 0, 0), 9.10e-8, 2.12e4),
             1e-4: ((19, 19, 19, 20), (1, 1, 1, 1), 3.12e-8, 7.10e3),
             1e-5: ((38, 39, 39, 39), (2, 2, 2, 2), 7.66e-9, 1.70e3)},
}
_INTEGRATED = {}


def integrated(name, reltol):
    """(vl, rhoe, info) of the reference integrator over 64 stable steps, and the SSPRK33 solution; shared."""
    key = (name, reltol)
    if key not in _INTEGRATED:
        case, v, ti, e, fv, fe, sd = start(name)
        if name not in _INTEGRATED:
            _INTEGRATED[name] = CR.ssprk33_reference(case, 64.0)
        _INTEGRATED[key] = CT.integrate(case.om, v, ti, e, 0.0, 64 * sd, sd, reltol=reltol) + (_INTEGRATED[name],)
    return _INTEGRATED[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_integrator_against_ssprk33(name):
    """64 stable steps at reltol 1e-3, 1e-4, 1e-5 (MEASURED above: 10-14, 19-29 and 38-57 accepted steps; 0, 1-2 and
    2 rejected; iced errors 2.03e-5 / 2.12e4, 6.91e-6 / 7.10e3, 1.66e-6 / 1.68e3 in vartheta_l / rhoe_int).  No
    column fails, every column lands on t1, the error falls with reltol; the step counts stay within 15 % (and
    one step) of the measured ones, the rejected steps within one, the errors within 25 %."""
    sd = start(name)[6]
    last = None
    for reltol in (1e-3, 1e-4, 1e-5):
        v1, e1, info, want = integrated(name, reltol)
        acc, rej, err_v, err_e = MEASURED[name][reltol]
        got_v, got_e = float(np.max(np.abs(v1 - want[0]))), float(np.max(np.abs(e1 - want[1])))
        print(f"{name} reltol {reltol}: accepted {info['accepted']}, rejected {info['rejected']}, errors {got_v:.3g} {got_e:.3g}")
        assert not info["failed"].any() and np.all(info["t"] == 64 * sd)
        assert np.all(np.abs(info["accepted"] - np.array(acc)) <= 0.15 * np.array(acc) + 1), info["accepted"]
        assert np.all(np.abs(info["rejected"] - np.array(rej)) <= 1), info["rejected"]
        assert err_v / 1.25 <= got_v <= 1.25 * err_v and err_e / 1.25 <= got_e <= 1.25 * err_e, (got_v, got_e)
        if last is not None:
            assert got_v < last[0] and got_e < last[1]
        last = (got_v, got_e)


def test_the_device_newton_rule_changes_little():
    """The water stages stopped by the device's rule (kappa 0.01 on abstol + reltol |vartheta_l|, at most 10
    iterations) instead of iterated to round-off: the same accepted and rejected counts at reltol 1e-3 on the
    iced case, and a state within reltol of the round-off one in the controller's own scale."""
    case, v, ti, e, fv, fe, sd = start("iced")
    v0, e0, i0, _ = integrated("iced", 1e-3)
    v1, e1, i1 = CT.integrate(case.om, v, ti, e, 0.0, 64 * sd, sd, newton=CT.device_newton())
    np.testing.assert_array_equal(i1["accepted"], i0["accepted"])
    np.testing.assert_array_equal(i1["rejected"], i0["rejected"])
    ae = CT.abstol_e_default(case.om)
    q = CT.error_norm(v1 - v0, e1 - e0, v0, v1, e0, e1, CT.ABSTOL, ae, CT.RELTOL)
    print("device Newton rule against round-off, in tolerance units:", q)
    assert np.all(q <= 1.0), q


def test_a_tolerance_that_cannot_be_met_fails_the_column_and_keeps_its_state():
    """Every stage output rounded to Float32 and all three tolerances 1e-14: h falls to the floor, every column
    fails with nothing accepted and keeps its initial state."""
    case, v, ti, e, fv, fe, sd = start("flux")
    v1, e1, info = CT.integrate(case.om, v, ti, e, 0.0, 10 * sd, sd, abstol=1e-14, abstol_e=1e-14, reltol=1e-14,
                                round_to=np.float32)
    assert info["failed"].all() and not info["accepted"].any() and np.all(info["t"] == 0.0)
    np.testing.assert_array_equal(v1, v)
    np.testing.assert_array_equal(e1, e)
