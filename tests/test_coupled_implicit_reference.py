"""tests/coupled_implicit_ref.py, the NumPy reference of lh_step_coupled_implicit, on the CPU: the two properties
of the oracle's coupled tendency that make a stage block triangular, the reference's own full coupled
residuals and the order of both methods against oracle SSPRK33."""
import numpy as np
import pytest

import case_model as M
import coupled_implicit_ref as CR
import parity_cases as pc

CASES = [(k, ice) for k in CR.KINDS for ice in (False, True)]


def _c3():
    case = pc.make_case("c3_coupled_f64", ncols=8)
    return case, (M.BC_FLUX, M.BC_FLUX), False


def _cases():
    for kinds, ice in CASES:
        yield CR.coupled_case(*kinds, ncols=8, nlev=48 if ice else 64, ice=ice), kinds, ice
    yield _c3()


def test_the_water_tendency_does_not_read_the_energy():
    """d vartheta_l / dt with rhoe_int replaced by 1.37 rhoe_int + 5e5 (and by 0) is bitwise the same."""
    for case, kinds, ice in _cases():
        vl, ti, re = CR.f64(case)
        fw = CR.tendencies(case.om, vl, ti, re)[0]
        np.testing.assert_array_equal(CR.tendencies(case.om, vl, ti, 1.37 * re + 5e5)[0], fw)
        np.testing.assert_array_equal(CR.water_tendency(case.om, vl, ti), fw)
        assert np.max(np.abs(fw)) > 0


def test_the_energy_tendency_is_affine_in_the_energy():
    """|f(e + 2d) - 2 f(e + d) + f(e)| / max |f| <= 1e-10 at fixed vartheta_l, theta_i (measured: 9e-15 with
    ice, 2.5e-12 on c3_coupled_f64)."""
    worst = 0.0
    for case, kinds, ice in _cases():
        vl, ti, re = CR.f64(case)
        c = np.arange(case.ncols)[:, None]
        d = 0.05 * np.abs(re) * (0.5 + pc.uhash(c, np.arange(case.om.nlev)[None, :] + 3, 1000))
        f = lambda e: CR.energy_tendency(case.om, vl, ti, e)
        f0, f1, f2 = f(re), f(re + d), f(re + 2 * d)
        sd = np.max(np.abs(f2 - 2 * f1 + f0)) / np.max(np.abs(f0))
        worst = max(worst, float(sd))
        assert sd <= 1e-10, (kinds, ice, float(sd))
        assert np.max(np.abs(f1 - f0)) > 0   # (and it does read it)
    print("largest relative second difference", worst)


@pytest.mark.parametrize("kinds", CR.KINDS)
def test_the_stage_solves_the_full_coupled_residual(kinds):
    """One backward-Euler step at 10x and 100x the stable step: Y1 - Yn - dt f(Y1) through the oracle's full
    coupled tendency, water <= 1e-12, energy <= 1e-10 relative to max |rhoe_int| (measured: 6e-15, 5e-12);
    Newton converges (measured: 5-6 iterations)."""
    case = CR.coupled_case(*kinds, ncols=8, ice=True)
    vl, ti, re = CR.f64(case)
    sd = CR.stable_dt(case)
    for mult in (10.0, 100.0):
        v1, e1, info = CR.coupled_implicit(case.om, vl, ti, re, mult * sd, 1)
        rw, r_e = CR.residual(case.om, vl, re, ti, v1, e1, mult * sd)
        rw, r_e = float(np.max(np.abs(rw))), float(np.max(np.abs(r_e)) / np.max(np.abs(re)))
        print(kinds, mult, "iterations", info["iters"], "water", rw, "energy (relative)", r_e)
        assert info["unconverged"] == 0 and info["iters"] <= 20
        assert rw <= 1e-12 and r_e <= 1e-10, (mult, rw, r_e)
        assert np.max(np.abs(v1 - vl)) > 0 and np.max(np.abs(e1 - re)) > 0
    # the device's stopping rule costs at most a few tol: the two references agree that closely
    vt, et, it = CR.coupled_implicit(case.om, vl, ti, re, 10 * sd, 1, tol=1e-10)
    v1, e1, _ = CR.coupled_implicit(case.om, vl, ti, re, 10 * sd, 1)
    assert it["unconverged"] == 0 and np.max(np.abs(vt - v1)) <= 1e-9


@pytest.mark.parametrize("method", ["euler", "trbdf2"])
def test_order(method):
    """Global error ratios per halving of h over T = 16 stable steps, h = T/4 -> T/8 -> T/16, against oracle
    SSPRK33 at sd / 8: backward Euler in [1.8, 2.2], TR-BDF2 in [3.7, 4.5] (measured: 1.93-2.03, 4.00-4.22),
    in both variables."""
    solve = lambda case, dt, n: CR.coupled_implicit(case.om, *CR.f64(case), dt, n, method)[:2]
    ratios, errs = CR.order_ratios(method, solve)
    print(method, errs, ratios)
    lo, hi = CR.ORDER_BANDS[method]
    assert all(lo <= r <= hi for rs in ratios.values() for r in rs), (errs, ratios)


def test_boundary_value_table():
    """A constant table equals no table; a ramped one differs, and backward Euler reads sample k + 1."""
    case = CR.coupled_case(M.BC_DIRICHLET, M.BC_DIRICHLET, ncols=4, nlev=16, ice=True)
    vl, ti, re = CR.f64(case)
    dt, n = 20 * CR.stable_dt(case), 2
    const = np.zeros((n + 1, 2, 2))
    for (f, c), (kind, v) in case.om.bc.items():
        const[:, f, c] = v
    for method in ("euler", "trbdf2"):
        a = CR.coupled_implicit(case.om, vl, ti, re, dt, n, method)
        b = CR.coupled_implicit(case.om, vl, ti, re, dt, n, method, bcv=const)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    ramp = const.copy()
    ramp[:, M.FACE_TOP, M.COMP_ENERGY] += np.arange(n + 1)
    ramp[:, M.FACE_TOP, M.COMP_HYDROLOGY] += 0.01 * np.arange(n + 1)
    r = CR.coupled_implicit(case.om, vl, ti, re, dt, n, "euler", bcv=ramp)
    om1 = CR.with_bc(case.om, ramp[1])
    s1 = CR.coupled_implicit(om1, vl, ti, re, dt, 1, "euler")
    s2 = CR.coupled_implicit(CR.with_bc(case.om, ramp[2]), s1[0], ti, s1[1], dt, 1, "euler")
    np.testing.assert_array_equal(r[0], s2[0])
    np.testing.assert_array_equal(r[1], s2[1])
    assert np.max(np.abs(r[1] - CR.coupled_implicit(case.om, vl, ti, re, dt, n, "euler")[1])) > 0
