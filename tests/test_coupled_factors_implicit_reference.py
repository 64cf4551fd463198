"""tests/coupled_factors_implicit_ref.py on the CPU: with the IceImpedance factor on (and no viscosity factor) the
oracle's coupled tendency keeps the two properties that make a stage block triangular, the reference Newton converges
on every case the GPU test runs, both methods keep their order, and an energy stage formed with the NoEffect K is far
outside the GPU parity assertion's allowance."""
import numpy as np
import pytest

import case_model as M
import coupled_factors_implicit_ref as CF
import parity_cases as pc

CR = CF.CR


def _cases():
    """67 columns of 1, 2, 3 and 16 levels, the five boundary pairs, ice up to 0.04 and up to 0.15."""
    for kinds in CR.KINDS:
        for nlev in CF.NLEVS:
            for most in (CF.ICE_GENERAL, CF.ICE_LARGE):
                yield CF.factors_case(*kinds, nlev=nlev, most_ice=most), kinds, nlev, most


def test_the_cases_have_the_factor_on_and_it_matters():
    """The impedance changes f_w by tens of per cent and f_e by 1e-5 to 1e-2 of its size: small in the energy, which is
    why the mutant below is measured against the parity allowance and not against f_e."""
    case = CF.factors_case(*CR.KINDS[1])
    assert (case.om.cf.impedance_kind, case.om.cf.viscosity_kind) == (1, 0)
    vl, ti, re = CR.f64(case)
    fw, fe = CR.tendencies(case.om, vl, ti, re)
    gw, ge = CR.tendencies(CF.without_factors(case.om), vl, ti, re)
    icy = np.any(ti > 0, axis=1)
    rw = np.max(np.abs(fw - gw)[icy]) / np.max(np.abs(gw)[icy])
    r_e = np.max(np.abs(fe - ge)[icy]) / np.max(np.abs(ge)[icy])
    print("the factor changes f_w by", rw, "and f_e by", r_e, "of their largest entry")
    assert rw > 0.1 and 1e-6 < r_e < 0.1
    np.testing.assert_array_equal(fw[~icy], gw[~icy])   # (no ice: the factor is exactly 1)
    np.testing.assert_array_equal(fe[~icy], ge[~icy])


def test_the_water_tendency_does_not_read_the_energy():
    """d vartheta_l / dt with rhoe_int replaced by 1.37 rhoe_int + 5e5 (and by 0) is bitwise the same."""
    for case, kinds, nlev, most in _cases():
        vl, ti, re = CR.f64(case)
        fw = CR.tendencies(case.om, vl, ti, re)[0]
        np.testing.assert_array_equal(CR.tendencies(case.om, vl, ti, 1.37 * re + 5e5)[0], fw)
        np.testing.assert_array_equal(CR.water_tendency(case.om, vl, ti), fw)
        if not (nlev == 1 and kinds == CR.KINDS[0]):   # (one cell between two equal fluxes is at rest)
            assert np.max(np.abs(fw)) > 0


def test_the_energy_tendency_is_affine_in_the_energy():
    """|f(e + 2d) - 2 f(e + d) + f(e)| / max |f| <= 1e-10 at fixed vartheta_l, theta_i: DESIGN section 4.16's bound
    (measured: 1.4e-14)."""
    worst = 0.0
    for case, kinds, nlev, most in _cases():
        vl, ti, re = CR.f64(case)
        c = np.arange(case.ncols)[:, None]
        d = 0.05 * np.abs(re) * (0.5 + pc.uhash(c, np.arange(nlev)[None, :] + 3, 1000))
        f = lambda e: CR.energy_tendency(case.om, vl, ti, e)
        f0, f1, f2 = f(re), f(re + d), f(re + 2 * d)
        sd = np.max(np.abs(f2 - 2 * f1 + f0)) / np.max(np.abs(f0))
        worst = max(worst, float(sd))
        assert sd <= 1e-10, (kinds, nlev, most, float(sd))
        assert np.max(np.abs(f1 - f0)) > 0   # (and it does read it)
    print("largest relative second difference", worst)


@pytest.mark.parametrize("which", CF.RESIDUAL_CASES)
def test_newton_converges_and_the_stage_solves_the_full_residual(which):
    """The residual cases of the GPU test, one backward-Euler step at 10x and 100x the stable step: Newton converges in
    every column (measured: 5 to 7 iterations to round-off, 15 to 18 with per-column parameters), and Y1 - Yn - dt f(Y1) through the oracle's full coupled tendency is
    <= 1e-12 for the water and <= 1e-10 of max |rhoe_int| for the energy (tests/test_coupled_implicit_reference.py's
    bounds; measured 1.9e-13 and 3.0e-13)."""
    label, kinds, case = CF.residual_case(which, np.float64)
    vl, ti, re = CR.f64(case)
    sd = CR.stable_dt(case)
    for mult in (10.0, 100.0):
        v1, e1, info = CR.coupled_implicit(case.om, vl, ti, re, mult * sd, 1)
        rw, r_e = CR.residual(case.om, vl, re, ti, v1, e1, mult * sd)
        rw, r_e = float(np.max(np.abs(rw))), float(np.max(np.abs(r_e)) / np.max(np.abs(re)))
        print(which, mult, "iterations", info["iters"], "water", rw, "energy (relative)", r_e)
        assert info["unconverged"] == 0 and info["iters"] <= 20
        assert rw <= 1e-12 and r_e <= 1e-10, (mult, rw, r_e)
        assert np.max(np.abs(v1 - vl)) > 0 and np.max(np.abs(e1 - re)) > 0


@pytest.mark.parametrize("dtype", CF.DTYPES)
@pytest.mark.parametrize("name", sorted(CF.PARITY))
def test_newton_converges_on_the_parity_cases_and_the_mutant_is_far_outside(name, dtype):
    """Every parity case of the GPU test, both methods and types: the reference Newton converges in every column, and the
    MUTANT energy tendency -- K without the factor wherever the energy is formed -- ends at least 10x the GPU assertion's
    allowance 4 d + 64 eps ||rhoe_int|| away in rhoe_int while its vartheta_l is bitwise the reference's.  Measured:
    5.7e9 to 2.8e10 times the allowance in Float64, 10.6 to 52 times in Float32.

    One level is the exception, by construction and not by measurement: K enters the energy through the advected energy
    of INTERIOR faces only (a boundary face's energy flux is the prescribed flux or the conduction to the Dirichlet T),
    and a column of one cell has none -- there the mutant is the right answer, bit for bit, which is asserted."""
    case, dt = CF.parity_case(name, dtype)
    vl, ti, re = CR.f64(case)
    for method in CF.METHODS:
        for nsteps in CF.PARITY[name]["nsteps"]:
            (vr, er, info), d, scale = CF.parity_reference(name, dtype, nsteps, method)
            assert info["unconverged"] == 0 and info["iters"] <= 20, info
            vm, em, _ = CF.noeffect_energy_mutant(case.om, vl, ti, re, dt, nsteps, method)
            np.testing.assert_array_equal(vm, vr)
            away = float(np.max(np.abs(em - er)))
            allowance = CF.parity_bound(case, d, scale)
            print(f"mutant {name} {np.dtype(dtype).name} {method} nsteps={nsteps}: {away:.3g} = {away / allowance:.3g} x the allowance")
            if case.om.nlev == 1:
                np.testing.assert_array_equal(em, er)
            else:
                assert away >= 10 * allowance, (method, nsteps, away, allowance)


@pytest.mark.parametrize("nlev", [16, 64])
@pytest.mark.parametrize("method", CF.METHODS)
def test_order(method, nlev):
    """CR.order_ratios on 4 columns of 16 and of 64 levels with the factor on: inside CR.ORDER_BANDS in both variables
    (measured: backward Euler 1.96-2.03, TR-BDF2 4.01-4.20)."""
    solve = lambda case, dt, n: CR.coupled_implicit(case.om, *CR.f64(case), dt, n, method)[:2]
    ratios, errs = CR.order_ratios(method, solve, CF.order_case(nlev))
    print(method, nlev, errs, ratios)
    lo, hi = CR.ORDER_BANDS[method]
    assert all(lo <= r <= hi for rs in ratios.values() for r in rs), (errs, ratios)
