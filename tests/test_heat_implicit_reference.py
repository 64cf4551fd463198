"""tests/heat_implicit_ref.py, the NumPy reference of lh_step_heat_implicit, on the CPU: the affinity of the
oracle's heat tendency that everything rests on, the analytic problem of the reference
(heat_test_interface.jl) and the order of both methods."""
import dataclasses

import numpy as np
import pytest

import case_model as M
import heat_implicit_ref as H
import parity_cases as pc

CASES = {
    "flux_flux": dict(bottom=M.BC_FLUX, top=M.BC_FLUX),
    "dirichlet_dirichlet": dict(bottom=M.BC_DIRICHLET, top=M.BC_DIRICHLET),
    "dirichlet_flux_ice": dict(bottom=M.BC_DIRICHLET, top=M.BC_FLUX, ice=True),
    "flux_dirichlet_percol_ice": dict(bottom=M.BC_FLUX, top=M.BC_DIRICHLET, ice=True, percol_bc=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("nlev", [1, 3, 60])
def test_the_heat_tendency_is_affine(name, nlev):
    """f(a x + (1 - a) y) = a f(x) + (1 - a) f(y) to the round-off of the three evaluations: each one is
    allowed its own tendency_tolerance with Cw = 4 (Float64's constant in assert_tendencies_close)."""
    case = H.heat_case(8, nlev, **CASES[name])
    vl, ti, x = H.f64(case)
    c = np.arange(8)[:, None]
    y = x * (0.7 + 0.6 * pc.uhash(c, np.arange(nlev)[None, :] + 3, 1000))   # another state, +-30 %
    f = lambda r: H.tendency(case.om, vl, ti, r)
    tol = lambda r: pc.tendency_tolerance(dataclasses.replace(case, rhoe=np.ascontiguousarray(r)), 4.0)["rhoe"]
    for a in (0.25, -0.5, 1.75):
        z = a * x + (1 - a) * y
        err = np.abs(f(z) - (a * f(x) + (1 - a) * f(y)))
        allowed = tol(z) + abs(a) * tol(x) + abs(1 - a) * tol(y)
        assert np.all(err <= allowed), (a, float(np.max(err / allowed)))
    if nlev > 1:   # (one cell between two flux faces: the tendency does not read the state)
        assert np.max(np.abs(f(x) - f(y))) > 0


def test_noBC_energy_faces_have_no_method():
    """A NoBC energy face on SoilEnergyModel is refused by the oracle (as by the reference, which has no
    method for it, and by validate_model in the library): there is no NoBC heat tendency to be affine."""
    case = H.heat_case(2, 3, bottom=M.BC_NONE, top=M.BC_FLUX)
    with pytest.raises(ValueError):
        H.tendency(case.om, *H.f64(case))


def test_bands_reproduce_the_tendency():
    """A Y + f(0) is the oracle's tendency (the matrix the solves use)."""
    case = H.heat_case(5, 60, ice=True)
    vl, ti, y = H.f64(case)
    (lo, di, up), f0 = H.affine_parts(case.om, vl, ti)
    Ay = di * y
    Ay[:, 1:] += lo[:, 1:] * y[:, :-1]
    Ay[:, :-1] += up[:, :-1] * y[:, 1:]
    want = H.tendency(case.om, vl, ti, y)
    tol = pc.tendency_tolerance(case, 4.0)["rhoe"]
    assert np.all(np.abs(Ay + f0 - want) <= 2 * tol)
    # a column-diagonally-dominant M-matrix: no pivoting
    assert np.all(di < 0) and np.all(lo >= 0) and np.all(up >= 0)
    col_sum = di.copy()
    col_sum[:, :-1] += lo[:, 1:]
    col_sum[:, 1:] += up[:, :-1]
    assert np.all(col_sum <= 1e-12 * np.abs(di))


def test_analytic_problem_trbdf2():
    """heat_test_interface.jl with 400 TR-BDF2 steps of 5e-3 s instead of 20 000 SSPRK33 steps: the
    reference's criterion MSE < 1e-6 (measured 1.7e-7)."""
    case = H.analytic_case()
    vl, ti, re = H.f64(case)
    y = H.heat_implicit(case.om, vl, ti, re, 5e-3, 400, "trbdf2", H.analytic_bcv(5e-3, 400))
    mse = H.analytic_mse(case, y, 2.0)
    print("TR-BDF2 dt = 5e-3: MSE", mse)
    assert mse < 1e-6
    # backward Euler is first order: 2000 steps of 1e-3 s miss it (3.1e-6)
    y = H.heat_implicit(case.om, vl, ti, re, 1e-3, 2000, "euler", H.analytic_bcv(1e-3, 2000))
    assert 1e-6 < H.analytic_mse(case, y, 2.0) < 1e-5


def test_analytic_problem_backward_euler():
    """Backward Euler at the reference's own dt = 1e-4 s, on the shortened span [1.8 s, 2 s] (2000 steps)
    from the discrete periodic state: the initial condition is the TR-BDF2 solution at 1.8 s (360 steps of
    5e-3 s from the reference's T = 0 start, past the transient).  MSE < 1e-6 at 2 s."""
    case = H.analytic_case()
    vl, ti, re = H.f64(case)
    y = H.heat_implicit(case.om, vl, ti, re, 5e-3, 360, "trbdf2", H.analytic_bcv(5e-3, 360))
    y = H.heat_implicit(case.om, vl, ti, y, 1e-4, 2000, "euler", H.analytic_bcv(1e-4, 2000, t0=1.8))
    mse = H.analytic_mse(case, y, 2.0)
    print("backward Euler dt = 1e-4 over [1.8, 2]: MSE", mse)
    assert mse < 1e-6


@pytest.mark.parametrize("method,lo,hi", [("euler", 1.8, 2.2), ("trbdf2", 3.6, 4.4)])
def test_order(method, lo, hi):
    """Error ratio per halving of dt on a smooth case with constant Dirichlet values.  Measured:
    backward Euler 1.90, 1.94, 1.97; TR-BDF2 4.08, 4.04, 4.02."""
    errs = H.order_errors(method, lambda c, dt, n: H.heat_implicit(c.om, *H.f64(c), dt, n, method))
    r = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
    print(method, errs, r)
    assert all(lo <= x <= hi for x in r), (errs, r)
