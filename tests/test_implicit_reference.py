"""The NumPy backward-Euler reference (tests/implicit_ref.py) on the CPU oracle's tendency: it
solves its own equations to round-off and is first order in dt.  No GPU."""
import numpy as np

import case_model as M
import implicit_ref as R
import parity_cases as pc


def test_reference_residual_is_round_off():
    case = pc.make_case("c2_richards_f64", ncols=4)
    sd = pc.O.stable_dt(case.om, case.vl, case.ti, None, 0.5)
    for mult in (10.0, 100.0):
        dt = mult * sd
        v1, iters = R.implicit_euler(case.om, case.vl, case.ti, dt, 1)
        res = R.residual(case.om, v1, case.vl, case.ti, dt)
        assert np.max(np.abs(res)) <= 1e-13, (mult, float(np.max(np.abs(res))))
        assert iters.max() < 60


def test_reference_residual_dirichlet_and_free_drainage():
    sp = M.default_soil(nu=0.287, S_s=1e-3)
    vg = M.default_vg(n=3.96, alpha=2.7, Ksat=34 / 3600 / 100, theta_r=0.075)
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, 0.267),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    om = M.CaseModel(M.MODEL_RICHARDS, 150, -1.5, 0.0, soil=sp, vg=vg, bc=bc)
    vl = np.full((1, 150), 0.1)
    ti = np.zeros((1, 150))
    v1, _ = R.implicit_euler(om, vl, ti, 4.0, 1)
    assert np.max(np.abs(R.residual(om, v1, vl, ti, 4.0))) <= 1e-13
    assert v1[0, -1] > 0.1


def test_reference_is_first_order():
    """Against the oracle's SSPRK33 at a quarter of the stable step, over 40 stable steps of a smooth
    wetting front: the error falls by 1.7-2.3x per halving of dt (measured 1.98, 1.99)."""
    case = pc.make_case("c2_richards_f64", ncols=3)
    sd = pc.O.stable_dt(case.om, case.vl, case.ti, None, 0.5)
    T = 40 * sd
    ref = case.vl.copy()
    pc.O.ssprk33(case.om, sd / 4, 160, vl=ref, ti=case.ti.copy())
    errs = []
    for k in (10, 20, 40):
        v, _ = R.implicit_euler(case.om, case.vl, case.ti, T / k, k)
        errs.append(np.max(np.abs(v - ref)))
    for a, b in zip(errs, errs[1:]):
        assert 1.7 <= a / b <= 2.3, errs
