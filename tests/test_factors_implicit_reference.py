"""The NumPy references of the implicit integrators with conductivity factors (tests/factors_implicit_ref.py,
tests/factors_jacobian_ref.py) against the oracle, and the cases of tests/test_gpu_factors_implicit.py judged by the
references alone.  No GPU.

  - the closed-form tendency of factors_jacobian_ref equals the oracle's (Float64 round-off), in every Jacobian case;
  - its bands equal central differences of the oracle's tendency;
  - Newton's safeguard is inactive, with a factor 2 in hand, in EVERY cell of EVERY column of the Jacobian cases;
  - fed to the GPU test's assertion, each of the three mutants (a dropped impedance term, a dropped viscosity scale on
    dK, the impedance term kept on and above nu - theta_i) leaves at least 10 times the allowance, in every case whose
    Jacobian contains it (the third needs cells above nu - theta_i: the "above" cases);
  - the ceiling B <= q_1pc / 10 holds in the Float64 cases whose columns are equalised in stiffness.  The ensemble the
    other cases keep as it is (ice in every other column, so K differs by 10^2.6 between neighbours) has columns that
    are slack at any common step: their 1 % pin has no room whatever the kernel does, which is why the three mutants
    above, and not the 1 % ones, are what those cases guard against;
  - the reference Newton (stopping rule fixed_step_rule(1e-10), 50 iterations) converges in every column of every case
    the GPU tests use, and its residual meets the GPU test's bound (measured: 4 to 9 iterations, at most 1e-6 of it).
"""
import numpy as np
import pytest

import factors_implicit_cases as FC
import factors_implicit_ref as FR
import factors_jacobian_ref as FJ
import integrator_core as core

# B of the GPU assertion is C q32 per case: C is measured on the device and recorded in
# tests/test_gpu_factors_implicit.py; it lives here because the sensitivity tests feed the same assertion on the CPU.
C_BOUND = 8.0

JAC, JAC64 = FC.JACOBIAN, [s for s in FC.JACOBIAN if s.dtype == "f64"]


def bound(p):
    return C_BOUND * p.q32


def fd_bands(p):
    """Bands of I - dt df/dv by coloured central differences of the oracle's tendency
    (tests/test_newton_jacobian_reference.py::fd_bands)."""
    pr = p.pr
    v = pr.vl
    n = v.shape[1]
    por = pr.p["nu"] - pr.p["theta_r"]
    h = 1e-6 * np.maximum(np.abs(v - pr.p["theta_r"]), 1e-3 * por)
    a, b, c = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
    for k in range(3):
        hk = h * (np.arange(n) % 3 == k)[None, :]
        df = p.dt * (p.tendency(v + hk) - p.tendency(v - hk))
        for i in range(k, n, 3):
            hi = 2.0 * h[:, i]
            b[:, i] -= df[:, i] / hi
            if i > 0:
                c[:, i - 1] = -df[:, i - 1] / hi
            if i + 1 < n:
                a[:, i + 1] = -df[:, i + 1] / hi
    return a, b, c


@pytest.mark.parametrize("spec", JAC, ids=FC.IDS(JAC))
def test_closed_form_tendency_and_bands_equal_the_oracle(spec):
    p = FC.prepared(spec)
    f = FJ.tendency_and_slopes(p.pr)[0]
    et = float(np.max(np.abs(p.dt * f - p.dtf)) / np.max(np.abs(p.dtf)))
    fd = fd_bands(p)
    scale = np.max(np.abs(np.stack(p.J)), axis=(0, 2))[:, None]   # the column's largest band entry
    eb = max(float(np.max(np.abs(x - y) / scale)) for x, y in zip(p.J, fd))
    print("%s: tendency %.3g, bands against central differences %.3g" % (spec.id, et, eb))
    assert et <= 1e-13, et
    # (a cell above nu - theta_i has the slope 1 / S_s = 1000 of the saturated branch next to slopes of 1e-3: the
    # central difference itself rounds at 1e-6 of the column's largest entry there)
    assert eb <= 1e-6, eb


def test_the_above_cases_hold_cells_above_the_kink():
    for spec in JAC:
        p = FC.prepared(spec)
        above = p.pr.vl >= p.pr.p["nu"] - p.pr.ti
        assert above.any() == (spec.variant == "above"), spec.id
        if spec.variant == "above":
            assert (above & (p.pr.ti > 0)).sum() >= 10   # (the impedance factor is 1 without ice)


@pytest.mark.parametrize("spec", JAC, ids=FC.IDS(JAC))
def test_safeguard_inactive_in_every_cell_of_every_column(spec):
    p = FC.prepared(spec)
    ok = FJ.safeguard_inactive(p.pr, p.d)
    assert ok.shape == (FC.NCOLS, spec.nlev) and ok.all(), np.argwhere(~ok).tolist()
    assert np.max(np.abs(p.d)) > 0


def _excess(p, **kw):
    """The GPU assertion fed a d made with a mutated Jacobian: the worst |r_i| / allowed_i."""
    d = FJ.newton_update(p.pr, p.dt, p.dtf / p.dt, **kw)
    r, _ = FJ.residual_and_scale(p.J, d, p.dtf)
    return float(np.max(np.abs(r) / FJ.allowance(p.J, bound(p), d, p.pr.vl + d, p.dtf, p.pr.eps)))


@pytest.mark.parametrize("spec", JAC, ids=FC.IDS(JAC))
def test_each_mutant_leaves_ten_times_the_allowance(spec):
    p = FC.prepared(spec)
    own, f32 = _excess(p), _excess(p, dtype=np.float32)
    left = {m: _excess(p, mutant=m) for m in FC.mutants_of(spec)}
    print("%s: excess own %.3g, float32 slopes %.3g, mutants %s" % (spec.id, own, f32, left))
    assert own <= 1 and f32 <= 1
    assert left and min(left.values()) >= 10, left


def test_every_mutant_is_seen_somewhere():
    assert {m for s in JAC for m in FC.mutants_of(s)} == set(FJ.MUTANTS)


@pytest.mark.parametrize("spec", [s for s in JAC64 if s.variant == "equal"], ids=FC.IDS([s for s in JAC64 if s.variant == "equal"]))
def test_the_pin_has_room_where_the_columns_are_equalised(spec):
    p = FC.prepared(spec)
    print("%s: q32 %.3g, q_1pc %.3g, ratio %.3g" % (spec.id, p.q32, p.q_1pc, p.q_1pc / p.q32))
    assert bound(p) <= p.q_1pc / 10, (bound(p), p.q_1pc)


# ------------------------------------------------------------------ the reference Newton on the GPU tests' cases

def residual_specs():
    """tests/test_gpu_factors_implicit.py::test_residual_through_the_tendency's cases: all five boundary pairs at 10x
    and 100x the stable step, but free drainage on top over a Dirichlet bottom at 16 levels at 10x only (two columns
    cycle at 100x, the known cycle of DESIGN section 4.12); both factors, and one case each with only one."""
    out = []
    for dtype in ("f64", "f32"):
        for nlev in (2, 16):
            for kinds in FC.KINDS:
                for mult in (10.0, 100.0):
                    if not (mult == 100.0 and nlev == 16 and kinds == FC.KINDS[2]):
                        out.append(FC.Spec(dtype, nlev, kinds, "both", mult))
        out += [FC.Spec(dtype, 16, FC.KINDS[4], f, 10.0) for f in ("viscosity", "impedance")]
    return out


RESIDUAL = residual_specs()
PARITY = [FC.Spec(d, n, FC.KINDS[1], "both", 10.0) for d in ("f64", "f32") for n in (2, 16)]
NEWTON_CASES = RESIDUAL + [s for s in PARITY if s not in RESIDUAL]


def residual_bound(case, tol, mult):
    """10 tol nu (1 + 4 dt / stable_dt): tests/test_gpu_implicit.py's bound without its round-off term."""
    return 10 * tol * case.om.soil.nu * (1 + 4 * mult)


@pytest.mark.parametrize("spec", NEWTON_CASES, ids=FC.IDS(NEWTON_CASES))
def test_reference_newton_converges_in_every_column(spec):
    case, dt = FC.general(spec)
    vl, ti, T = FC.f64(case)
    v1, iters, conv = FR.implicit_euler(case.om, vl, ti, T, dt, 1, core.fixed_step_rule(1e-10), 50)
    res = np.max(np.abs(v1 - vl - dt * FR.tendency(case.om, v1, ti, T)), axis=1)
    print("%s: iterations %d..%d, residual / bound %.3g" % (spec.id, iters.min(), iters.max(),
                                                           float(res.max() / residual_bound(case, 1e-10, spec.mult))))
    assert conv.all(), np.flatnonzero(~conv[0]).tolist()
    # the reference itself meets the bound the device is held to (measured: at most 1e-6 of it)
    assert res.max() <= residual_bound(case, 1e-10, spec.mult)
