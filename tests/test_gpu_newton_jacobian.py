"""The analytic Newton Jacobian of the implicit Richards solvers, read off the device.

With max_iter = 1 a backward-Euler call returns exactly one Newton update from Y0: the first sweep has v - v_n = 0 and
the step length 1, so J(Y0) d = dt f(Y0) and Y1 = Y0 + d wherever the safeguard stays inactive.  d = Y1 - Y0 is read
off the device and must satisfy the closed-form reference Jacobian of tests/newton_jacobian_ref.py,
J_ref d = dt f(Y0) with f(Y0) from lh_rhs of the same context, for lh_step_implicit_euler,
lh_step_layered_implicit_euler, lh_step_coupled_implicit and lh_step_layered_coupled_implicit (flags 0, vartheta_l
only: the energy solve is linear and tested elsewhere).  A Newton iteration with a wrong Jacobian still converges to
the same root, so no test of the converged state sees a dropped dK h term, a slope of the wrong cell's class, a sign
slip in a Dirichlet face slope or the wrong saturation in a slope; this one does.

The cases and everything the reference alone says about them (the safeguard is inactive in every cell of every
column, q32, q_1pc) are tests/test_newton_jacobian_reference.py's; 67 columns, one full wave and a ragged one.

Per case, with r = J_ref d - dt f and s_i = sum_j |dt df_i/dv_j| |d_j| + |d_i|, every cell satisfies
    |r_i| <= B max_i s_i + 64 eps(FT) sum_j |J_ref,ij| max(|Y1_j|, |dt f_j|),
the second term being the suite's round_off convention (tests/test_gpu_implicit.py) and B = C q32: q32 is what the
same formulas leave with the two slopes evaluated in np.float32 (the device forms its slopes in Float32 on purpose),
and C allows for the device's Float32 log2 / exp2 not being IEEE.  Ceiling: B <= q_1pc / 10, a tenth of what either
slope off by 1 % leaves (asserted on the CPU, with the sensitivity of this very assertion).

In Float32 the round-off term dominates the allowance, so the Float32 cases guard against gross errors only (a
dropped dK or dn term leaves at least 10 times the allowance: the CPU module asserts it).

C = 8 (test_newton_jacobian_reference.C_BOUND): 4 x the largest Float64 ratio q / q32 measured, 1.6, rounded up to a
power of two.  Measured on an MI355X, 2026-10-21 (MEASURED below: the worst case of each family and type; every
Float64 case lies between 0.67 and 1.6).  The least room any Float64 case has is q_1pc = 167 q32, so the ceiling
B <= q_1pc / 10 would still hold at C = 16.  (While the layered cases were being chosen, two drafts of the 16-level
horizon case under a flux over free drainage measured 2.04 and 2.36; the case as it stands measures 1.2.)
"""
import ctypes as C

import numpy as np
import pytest

import newton_jacobian_ref as NJ
import parity_cases as pc
from test_newton_jacobian_reference import CASES, IDS, bound, prepared

pytestmark = pytest.mark.gpu
STATUS_UNCONVERGED = 8

# worst q / q32 over the columns and the cases of a family and type (each test prints its own figure).  Float32: the
# state is Float32, q is round-off of the state and not of the slopes, and the round-off term of the allowance judges it.
MEASURED = {"scalar-f64": 1.6, "layered-f64": 1.57, "coupled-f64": 1.1, "layered_coupled-f64": 0.883,
            "scalar-f32": 30.2, "layered-f32": 48.9}


def one_newton_update(p):
    """(Y0 as the device holds it, Y1, f(Y0) of lh_rhs, max_iters, unconverged, iterations, status) of one call with
    max_iter = 1 and nsteps = 1 on a fresh context."""
    spec, obj = p.spec, p.obj
    layered = spec.family in ("layered", "layered_coupled")
    g = pc.GpuModel(obj.case if layered else obj)
    with g:
        F, L = g.F, g.L
        if layered:
            g.set_soil_classes(obj.classes, obj.class_map, thermal=getattr(obj, "thermal", None))
        Y, Ya = g.prognostic_and_aux()
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        f = g.tendencies(dY)["vl"].astype(np.float64)
        y0 = g.download(Y, F.LH_VAR_VARTHETA_L).astype(np.float64)
        args = (g.ctx, Y, Ya, 0.0, p.dt, 1)
        if spec.family == "scalar":
            rc = L.lh_step_implicit_euler(*args, None, 0.0, 1)
        elif spec.family == "layered":
            rc = L.lh_step_layered_implicit_euler(*args, None, 0.0, 1)
        elif spec.family == "coupled":
            rc = L.lh_step_coupled_implicit(*args, 0, None, 0.0, 1)
        else:
            rc = L.lh_step_layered_coupled_implicit(*args, 0, None, 0.0, 1)
        F.check(rc, g.ctx)
        mi, un, tot = C.c_int32(), C.c_int64(), C.c_int64()
        F.check(L.lh_implicit_stats(g.ctx, C.byref(mi), C.byref(un)), g.ctx)
        F.check(L.lh_implicit_iterations(g.ctx, C.byref(tot)), g.ctx)
        y1 = g.download(Y, F.LH_VAR_VARTHETA_L).astype(np.float64)
        return y0, y1, f, mi.value, un.value, tot.value, g.status()


@pytest.mark.parametrize("spec", CASES, ids=IDS(CASES))
def test_first_newton_update_satisfies_the_reference_jacobian(spec):
    p = prepared(spec)
    y0, y1, f, mi, un, tot, status = one_newton_update(p)
    ncols = y0.shape[0]
    np.testing.assert_array_equal(y0, p.pr.vl)
    assert np.all(np.isfinite(y1)) and np.all(np.isfinite(f))
    assert mi == 1, mi
    assert tot == ncols, tot
    assert bool(status & STATUS_UNCONVERGED) == (un > 0), (status, un)
    assert (status & ~STATUS_UNCONVERGED) == 0, status
    d = y1 - y0
    dtf = float(spec.np_dtype(p.dt)) * f
    r, s = NJ.residual_and_scale(p.J, d, dtf)
    qdev = np.max(np.abs(r), axis=1) / np.max(s, axis=1)
    allowed = NJ.allowance(p.J, bound(p), d, y1, dtf, p.pr.eps)
    print("newton-jacobian %s: q %.3g, q32 %.3g, q/q32 %.3g, q_1pc %.3g, B %.3g, worst |r|/allowed %.3g, unconverged %d, "
          "|d|max %.3g" % (spec.id, qdev.max(), p.q32, qdev.max() / p.q32, p.q_1pc, bound(p),
                           float(np.max(np.abs(r) / allowed)), un, float(np.max(np.abs(d)))))
    assert np.max(np.abs(d)) > 0
    bad = np.abs(r) > allowed
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist(), float(np.max(np.abs(r) / allowed)))
