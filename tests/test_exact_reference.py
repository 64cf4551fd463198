"""The exact (mpmath) reference of tests/exact_ref.py and its fixtures under tests/golden/exact/, on the CPU:

  - every fixture file is what regenerating it gives, bit for bit, and 400 bits round to the same Float64 as the
    200 the fixtures were made with;
  - the third statement of the closed forms meets the known answers tests/test_oracle_pins.py pins the oracle
    with (K1 ... K7);
  - the fixtures hold what they are for (cells the rest of the suite masks, every table interval and entry);
  - the ORACLE is inside every bound of exact_ref on every fixture with NO cell masked -- a bound the reference's
    own arithmetic does not meet would be a wrong form, not a tight constant.  Its use of each bound is printed
    as an `EXACT-USE oracle` line (-s); profiles/exact_reference_use.txt keeps them.

The one exception is stated where it is made: where the REFERENCE's S^(-1/m) overflows (the `overflow`
fixtures exist for exactly those cells) the oracle returns psi = -Inf and Inf - Inf = NaN tendencies; the exact
value is finite, and it is the device, not the oracle, that tests/test_gpu_exact.py holds to it."""
import math
import os
import sys

import numpy as np
import pytest

mpmath = pytest.importorskip("mpmath")

import case_model as M  # noqa: E402
import exact_ref as X  # noqa: E402
import parity_cases as pc  # noqa: E402

NAMES = X.fixture_names()
_cache = {}


def generated(name):
    if name not in _cache:
        fx = X.build_fixture(name, generate=True)
        _cache[name] = (fx, X.fixture_arrays(fx))
    return _cache[name]


def exact_of(name):
    fx, arrays = generated(name)
    return fx, X.with_plain_bounds(fx, arrays)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_regenerates_bit_for_bit(name):
    fx, arrays = generated(name)
    assert os.path.getsize(fx.path) <= 64 * 1024
    with np.load(fx.path) as z:
        assert sorted(z.files) == sorted(arrays)
        for k in z.files:
            assert same_bits(z[k], arrays[k]), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_400_bits_round_to_the_same_float64(name):
    """the outputs AND the bounds, every cell of every fixture"""
    fx, arrays = generated(name)
    again = X.fixture_arrays(fx, prec=400)
    for k, v in again.items():
        assert same_bits(arrays[k], v), (name, k)


def test_fixtures_are_read_without_mpmath(monkeypatch):
    """what the GPU tests do: the case and the exact values from the file alone"""
    monkeypatch.setitem(sys.modules, "mpmath", None)
    for name in NAMES:
        fx = X.build_fixture(name)
        ex = X.load_exact(fx)
        assert ex["K" if "K" in ex else "T"].shape == (fx.case.ncols, fx.case.om.nlev)
        assert same_bits(np.asarray(fx.case.vl), np.asarray(generated(name)[0].case.vl)), name


# ------------------------------------------------------------------ what the fixtures hold

def _ill(fx):
    """the fuzz test's own criterion for a cell it masks: 1 - (1 - S^(1/m))^m < 64 eps"""
    case = fx.case
    with np.errstate(all="ignore"):
        nn = pc._percol(case, "vg_n", case.om.vg.n)[:, None]
        mm = 1.0 - 1.0 / nn
        nu = pc._percol(case, "nu", case.om.soil.nu)[:, None]
        th = pc._percol(case, "vg_theta_r", case.om.vg.theta_r)[:, None]
        S = (np.maximum(case.vl.astype(np.float64), th + np.finfo(case.dtype).eps) - th) / (nu - th)
        t = np.where(S < 1, S ** (1.0 / mm), 1.0)
        return np.where(S < 1, 1.0 - (1.0 - t) ** mm, 1.0) < 64 * np.finfo(case.dtype).eps


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("fuzz")])
def test_fuzz_fixtures_hold_the_cells_the_fuzz_test_masks(name):
    fx, ex = generated(name)
    ill = _ill(fx)
    assert ill.sum() >= 10, "no bone-dry cell in the fixture"
    assert np.all(np.isfinite(ex["K"])) and np.all(ex["K"][ill] > 0), "the exact K of a bone-dry cell is positive"
    assert np.all(np.isfinite(ex["dvl"][ill.any(axis=1)])), "the tendencies of their columns are in the fixture"
    for k in X.fields_of(fx.case.om.model):
        assert not np.isnan(ex[k]).any(), (name, k)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_overflow_fixtures_hold_finite_psi_where_the_reference_overflows(tag):
    fx, ex = generated(f"overflow_{tag}")
    with np.errstate(all="ignore"):
        opsi = pc.O.diagnostics(fx.case.om, fx.case.vl, fx.case.ti)["psi"]
    lost = np.isneginf(opsi) & np.isfinite(ex["psi"])
    assert lost.sum() >= 20, "cells where the reference overflows and the exact psi is a finite number"
    big = 1e200 if tag == "f64" else 1e30
    assert (np.abs(ex["psi"][lost]) > big).sum() >= 5
    assert np.isfinite(ex["dvl"][lost]).sum() >= 10, "with tendencies"
    if tag == "f64":
        assert (np.isfinite(ex["psi"]) & (np.abs(ex["psi"]) > 2.8e299)).sum() >= 5, "finite values beyond 2.8e299"
        assert np.isneginf(ex["psi"]).sum() >= 20, "and cells beyond the Float64 range"
    ordinary = np.arange(fx.case.ncols) % 4 == 3
    assert np.all(np.isfinite(opsi[ordinary])) and np.all(np.isfinite(ex["dvl"][ordinary]))


def test_sweeps_visit_every_table_interval_and_entry():
    seen = np.zeros(2048, int)
    for p in range(X.SWEEP_PARTS["log2"]):
        S = 2.0 * generated(f"sweep_log2_{p:02d}_f64")[0].case.vl
        m, _ = np.frexp(S)
        j = np.floor((m - 0.5) * 4096).astype(int)
        lo, hi = 0.5 + j / 4096.0, 0.5 + (j + 1) / 4096.0
        assert np.all((m == lo + 2.0 ** -53) | (m == hi - 2.0 ** -53)), "one ulp inside an end of the interval"
        np.add.at(seen, j.ravel(), 1)
    assert np.all(seen >= 2)
    entry, below, above = np.zeros(2048, int), np.zeros(2048, int), np.zeros(2048, int)
    with mpmath.workprec(200):
        for p in range(X.SWEEP_PARTS["exp2"]):
            for s in (2.0 * generated(f"sweep_exp2_{p:02d}_f64")[0].case.vl).ravel():
                u = mpmath.log(mpmath.mpf(float(s)), 2) * 4096          # log2(S) / m x 2048, m = 1/2
                k = int(mpmath.floor(u))                                 # the tie is k + 1/2
                d = float(u - k - mpmath.mpf(1) / 2)
                assert abs(d) < 2e-12
                (below if d < 0 else above)[k % 2048] += 1
                entry[(k if d < 0 else k + 1) % 2048] += 1
    assert np.all(below >= 1) and np.all(above >= 1) and np.all(entry >= 1)


def test_edge_clamp_and_mixed_fixtures_hold_their_cells():
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        fx, ex = generated(f"edge_{tag}")
        icy = fx.case.ti != 0
        S = np.where(icy, 4.0, 2.0) * fx.case.vl.astype(np.float64)
        for v in X._edge_values(dt):
            assert np.any((S == v) & icy) and np.any((S == v) & ~icy), v
        fx, ex = generated(f"clamp_{tag}")
        FT = np.dtype(dt).type
        thr = fx.case.om.percol["vg_theta_r"].astype(dt)[:, None]
        lim = (thr + FT(np.finfo(dt).eps)).astype(dt)
        for special in (FT(thr - FT(1e-3)).astype(dt), thr, lim, np.nextafter(lim, FT(-1)), np.nextafter(lim, FT(1))):
            assert (fx.case.vl == special).sum() >= 20
        fx, ex = generated(f"mixed_{tag}")
        vl, ti = fx.case.vl.astype(np.float64), fx.case.ti.astype(np.float64)
        for lev in range(fx.case.om.nlev):     # every level of the one wavefront is mixed company
            assert np.any(ti[:, lev] > 0) and np.any(ti[:, lev] == 0)
            assert np.any(vl[:, lev] > 0.5 - ti[:, lev]) and np.any(vl[:, lev] < 0.5 - ti[:, lev])
            assert np.any(fx.case.vl[:, lev] == dt(0.05))


def test_bottom_sign_fixtures_differ_in_the_bottom_face_only():
    """clampcs_* is clamp_* under the consistent bottom sign, K_f (psi_f - psi_c - dz/2)/(dz/2), against the
    reference's K_f (psi_f - psi_c + dz/2)/(dz/2) (boundary_conditions.jl:395-398) -- the two differ
    by the gravity term 2 K_f in the bottom flux and in the bottom cell's tendency, and nowhere else"""
    for tag in ("f64", "f32"):
        (fa, a), (fb, b) = generated(f"clamp_{tag}"), generated(f"clampcs_{tag}")
        assert not fa.case.om.consistent_bottom_sign and fb.case.om.consistent_bottom_sign
        assert same_bits(fa.case.vl, fb.case.vl)
        for k in ("K", "psi", "fw_top"):
            assert same_bits(a[k], b[k]), k
        assert same_bits(a["dvl"][:, 1:], b["dvl"][:, 1:])
        moist = np.abs(a["fw_bot"]) < 1.0       # (a clamped bottom cell has psi ~ -1e15 ... -1e35: 2 K_f is below its ulp)
        assert moist.sum() >= 30 and np.all(a["fw_bot"][moist] != b["fw_bot"][moist])
        calm = moist & (np.abs(a["dvl"][:, 0]) < 1.0)         # (and so has the cell above it)
        assert calm.sum() >= 10 and np.all(a["dvl"][calm, 0] != b["dvl"][calm, 0])
        # the Dirichlet face state: vl = 0.2 with the column's own parameters; K_f from its exact closed form
        thr, n = fa.case.om.percol["vg_theta_r"].astype(fa.case.dtype).astype(float), fa.case.om.percol["vg_n"]
        S = (float(fa.case.dtype(0.2)) - thr) / (float(fa.case.dtype(0.5)) - thr)
        m = 1 - 1 / n.astype(fa.case.dtype).astype(float)
        Kf = np.sqrt(S) * (1 - (1 - S ** (1 / m)) ** m) ** 2 * float(fa.case.dtype(1.2e-7))
        assert np.allclose((a["fw_bot"] - b["fw_bot"])[moist], 2 * Kf[moist], rtol=1e-5 if tag == "f32" else 1e-9, atol=0)


# ------------------------------------------------------------------ known answers (tests/test_oracle_pins.py)

def _mpcase(model, n, zmin, zmax, vl, ti=None, rhoe=None, **kw):
    om = M.CaseModel(model, n, zmin, zmax, **kw)
    vl = np.atleast_2d(np.asarray(vl, np.float64))
    ti = np.zeros_like(vl) if ti is None else np.atleast_2d(ti)
    return pc.Case("ka", om, np.float64, vl.shape[0], vl=vl, ti=ti, rhoe=None if rhoe is None else np.atleast_2d(rhoe))


def test_known_answers_K1_water_closed_forms():
    """test_water_parameterizations.jl:1-63 in Float32: the values of the closed forms at S = 0.5, 1, 1.5"""
    F32 = np.float32
    vg = M.default_vg(theta_r=float(F32(0.2)))
    sp = M.default_soil(nu=float(F32(0.4)), S_s=float(F32(1e-2)))
    bc = pc._flux_bcs(hydrology=0.0)
    om = M.CaseModel(M.MODEL_RICHARDS, 3, -0.3, 0.0, soil=sp, vg=vg, bc=bc)
    case = pc.Case("k1", om, F32, 1, vl=np.array([[0.3, 0.4, 0.5]], F32), ti=np.zeros((1, 3), F32))
    ex = X.evaluate(case, 4.0)
    n, alpha, Ksat = float(F32(vg.n)), float(F32(vg.alpha)), float(F32(vg.Ksat))
    m = 1 - 1 / n
    S0 = (float(F32(0.3)) - float(F32(0.2))) / (float(F32(0.4)) - float(F32(0.2)))
    assert ex["psi"][0, 0] == pytest.approx(-((S0 ** (-1 / m) - 1) * alpha ** (-n)) ** (1 / n), rel=1e-12)
    assert ex["psi"][0, 1] == 0.0
    assert ex["psi"][0, 2] == pytest.approx((float(F32(0.5)) - float(F32(0.4))) / float(F32(1e-2)), rel=1e-12)   # :24-26: 10
    assert ex["psi"][0, 2] == pytest.approx(10.0, rel=1e-6)
    assert ex["K"][0, 0] == pytest.approx(math.sqrt(S0) * (1 - (1 - S0 ** (1 / m)) ** m) ** 2 * Ksat, rel=1e-12)
    assert ex["K"][0, 1] == Ksat and ex["K"][0, 2] == Ksat
    # the factors (:40-46): impedance 10^(-7 f_i) at f_i = 1 is 1e-7, viscosity exp(gamma (T - 288))
    om.cf = M.default_cf(viscosity=True, impedance=True)
    case2 = pc.Case("k1f", om, F32, 1, vl=np.array([[0.0, 0.3, 0.3]], F32), ti=np.array([[0.1, 0.0, 0.0]], F32),
                    T_aux=np.array([[288.0, 278.0, 298.0]], F32))
    ex2 = X.evaluate(case2, 4.0)
    base = X.evaluate(pc.Case("k1b", M.CaseModel(M.MODEL_RICHARDS, 3, -0.3, 0.0, soil=sp, vg=vg, bc=bc), F32, 1,
                              vl=case2.vl, ti=case2.ti), 4.0)
    g = float(F32(2.64e-2))
    assert ex2["K"][0, 0] / base["K"][0, 0] == pytest.approx(1e-7, rel=1e-12)
    assert ex2["K"][0, 1] / base["K"][0, 1] == pytest.approx(math.exp(g * -10.0), rel=1e-12)
    assert ex2["K"][0, 2] / base["K"][0, 2] == pytest.approx(math.exp(g * 10.0), rel=1e-12)


def test_known_answers_K2_heat_closed_forms():
    """test_heat_parameterizations.jl:22-80: temperature, heat capacity, Kersten number (both branches), the
    saturated and dry conductivities, in one heat-only column"""
    e = M.default_earth()
    sp = M.default_soil(nu=0.4, S_s=1e-3, nu_ss_om=0.1, nu_ss_gravel=0.1, nu_ss_quartz=0.1, rho_c_ds=1e6, kappa_solid=0.1,
                        rho_p=1.0, kappa_sat_unfrozen=0.57, kappa_sat_frozen=2.29)
    bc = pc._flux_bcs(energy=0.0)
    case = _mpcase(M.MODEL_HEAT, 2, 0.0, 1.0, [[0.25, 0.30]], ti=[[0.05, 0.0]], rhoe=[[5.4e7, 5.4e7]], soil=sp, bc=bc)
    ex = X.evaluate(case, 2.0)
    rcs = 1e6 + 0.25 * (e.cp_l * e.rho_liq) + 0.05 * (e.cp_i * e.rho_ice)
    assert ex["T"][0, 0] == pytest.approx(e.T_0 + (5.4e7 + 0.05 * e.rho_ice * e.LH_f0) / rcs, rel=1e-15)
    k = e.K_therm
    kdry = ((0.053 * 0.1 - k) * 0.6 + k * 1.0) / (1.0 - (1.0 - 0.053) * 0.6)
    ksat = 0.57 ** (0.25 / 0.30) * 2.29 ** (0.05 / 0.30)
    Ke = 0.75 ** 1.1
    assert ex["kappa"][0, 0] == pytest.approx(Ke * ksat + (1 - Ke) * kdry, rel=1e-14)
    Ke = (0.75 ** ((1.0 + 0.1 - 0.24 * 0.1 - 0.1) / 2.0)
          * ((1.0 + math.exp(-18.1 * 0.75)) ** (-3.0) - ((1.0 - 0.75) / 2.0) ** 3.0) ** (1.0 - 0.1))
    assert ex["kappa"][0, 1] == pytest.approx(Ke * 0.57 + (1 - Ke) * kdry, rel=1e-14)
    # heat_test_interface.jl:7 (K5's set-up): rho_c_ds = 0.43314518988433487 makes kappa / rho_c_s == 1 for dry soil
    sp5 = M.default_soil(nu=0.495, nu_ss_gravel=0.1, nu_ss_om=0.1, nu_ss_quartz=0.1, rho_c_ds=0.43314518988433487,
                         kappa_solid=8.0, kappa_sat_unfrozen=0.57, kappa_sat_frozen=2.29)
    dry = _mpcase(M.MODEL_HEAT, 2, 0.0, 1.0, [[0.0, 0.0]], rhoe=[[0.0, 0.0]], soil=sp5, bc=bc)
    assert X.evaluate(dry, 2.0)["kappa"] == pytest.approx(0.43314518988433487, rel=4e-16)   # (a Float64 literal)


def test_known_answers_K3_K4_grid_and_single_tendency():
    """coupled.jl:123-234: the default initial condition on 20 levels over (-2, 0): d rhoe = 0, d theta_i = 0 and
    d vartheta_l = -div of the gravity flux -K between zero-flux faces; the centres are -1.95:0.1:-0.05"""
    sp, vg = pc.coupled_soil()
    n = 20
    e = M.default_earth()
    rcs = sp.rho_c_ds + 0.25 * e.cp_l * e.rho_liq
    case = _mpcase(M.MODEL_COUPLED, n, -2.0, 0.0, np.full((1, n), 0.25), rhoe=np.full((1, n), rcs * (273.16 - e.T_0)),
                   soil=sp, vg=vg, bc=pc._flux_bcs(energy=0.0, hydrology=0.0))
    ex = X.evaluate(case, 2.0)
    assert np.all(ex["drhoe"] == 0.0) and np.all(ex["T"] == 273.16)
    K = math.sqrt(0.5) * (1 - (1 - 0.5 ** 2) ** 0.5) ** 2 * vg.Ksat
    flux = np.zeros(n + 1) - K
    flux[0] = flux[-1] = 0.0
    assert np.allclose(ex["dvl"][0], -(flux[1:] - flux[:-1]) / 0.1, rtol=1e-13, atol=1e-25)
    assert np.all(ex["dvl"][0, 1:-1] == 0.0)          # exactly: the centres are equally spaced, the state uniform


@pytest.mark.parametrize("nu,zi,n,zmin", [(0.5, -0.3, 20, -2.0), (0.495, -0.56, 50, -10.0)], ids=["K6", "K7"])
def test_known_answers_K6_K7_equilibrium_profile_is_stationary(nu, zi, n, zmin):
    """coupled.jl:1-120 / richards_equation.jl:1-95: the equilibrium the reference's runs end in, -S_s (z - z_i) +
    nu below the interface and nu (1 + (alpha (z - z_i))^n)^(-m) above, has a uniform head: with zero-flux faces
    its exact tendency is zero to the rounding of the Float64 STATE (|d psi / d vl| eps nu of head per cell)."""
    sp = M.default_soil(nu=nu, S_s=1e-3)
    vg = M.default_vg(n=2.0, alpha=2.6, Ksat=0.0443 / 3600 / 100, theta_r=0.0)
    zc, _ = pc.grid_np(zmin, 0.0, n)
    vl = np.where(zc < zi, -1e-3 * (zc - zi) + nu, nu * (1 + (2.6 * np.maximum(zc - zi, 0.0)) ** 2.0) ** -0.5)
    case = _mpcase(M.MODEL_RICHARDS, n, zmin, 0.0, vl[None, :], soil=sp, vg=vg, bc=pc._flux_bcs(hydrology=0.0))
    ex = X.evaluate(case, 2.0)
    head = ex["psi"][0] + zc
    assert np.max(np.abs(head - zi)) < 1e-9           # psi = -(z - z_i) on both sides of the interface
    dz = -zmin / n
    assert np.max(np.abs(ex["dvl"][0])) < vg.Ksat * 1e-9 / dz ** 2


def test_heat_only_tendency_matches_the_oracle():
    """the heat-only model has no fixture of its own (its closures are the coupled model's): the exact tendency of
    the suite's heat case, Dirichlet temperatures at both faces, next to the oracle's"""
    case = pc.make_case("heat_dirichlet_f64", ncols=16)
    fx = X.Fixture("heat", case, 2.0)
    ex = {k: v for k, v in X.evaluate(case, 2.0).items() if k.split("_")[-1] not in ("dvl",) and "fw" not in k}
    for k in ("K", "bK", "psi", "bpsi"):
        ex.pop(k)
    ex["c_w"] = 2.0
    u = X.assert_inside(X.working_type_values(fx), ex, "heat_dirichlet_f64")
    print(X.record_line("oracle", "heat_dirichlet_f64(16)", "cpu", u))


# ------------------------------------------------------------------ the oracle inside the bounds, unmasked

@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_inside_every_bound_unmasked(name):
    fx, ex = exact_of(name)
    got = X.working_type_values(fx)
    note = ""
    if name.startswith("overflow"):
        # the reference's own overflow (module docstring): psi = -Inf where the exact value is finite; those cells,
        # and the tendencies and fluxes that read them (NaN or +-Inf in the oracle), are the DEVICE's to meet
        lost = np.isneginf(got["psi"]) & np.isfinite(ex["psi"])
        assert np.all(np.isfinite(got["psi"]) | np.isneginf(got["psi"]))
        ex["psi"] = np.where(lost, np.nan, ex["psi"])
        ex["dvl"] = np.where(~np.isfinite(got["dvl"]), np.nan, ex["dvl"])
        assert np.all(np.isneginf(got["psi"]).any(axis=1) | np.isfinite(got["dvl"]).all(axis=1)), "non-finite only next to its overflow"
        note = f"reference overflowed in {int(lost.sum())} cells (not the oracle's to meet)"
    u = X.assert_inside(got, ex, name)
    print(X.record_line("oracle", name, "cpu", u, (X.ulp_summary(got, ex, fx.case.dtype) + " ulp med/max; " + note).strip("; ")))
