"""The NumPy TR-BDF2 reference (tests/trbdf2_ref.py) on the CPU oracle's tendency: second order in dt,
an error estimate that tracks the true local error, adaptive runs that land on t1 and follow reltol;
and the new ABI entries refuse NULL arguments without a device.  No GPU."""
import ctypes as C

import numpy as np

import __graft_entry__ as g
import parity_cases as pc
import trbdf2_ref as R


def smooth_case(ncols=3):
    case = pc.make_case("c2_richards_f64", ncols=ncols)
    sd = pc.O.stable_dt(case.om, case.vl, case.ti, None, 0.5)
    return case, sd


def test_fixed_step_is_second_order():
    """Over 40 stable steps of a smooth wetting front, against the same scheme at 1/64 of the coarsest
    step: the global error falls 3.5-4.5x per halving of dt (measured 4.05, 4.04)."""
    case, sd = smooth_case()
    T = 40 * sd
    ref, _ = R.trbdf2(case.om, case.vl, case.ti, 0.0, T, T / 640, adaptive=False)
    errs = []
    for k in (10, 20, 40):
        v, info = R.trbdf2(case.om, case.vl, case.ti, 0.0, T, T / k, adaptive=False)
        assert np.all(info["t"] == T) and np.all(info["accepted"] == k)
        errs.append(np.max(np.abs(v - ref)))
    for a, b in zip(errs, errs[1:]):
        assert 3.5 <= a / b <= 4.5, errs


def test_error_estimate_tracks_the_local_error():
    """One step from the same state: |estimate| / |true local error| within [0.5, 2] (measured 1.003-1.02),
    and the estimate shrinks about 8x per halving of h (third-order local error; measured 6.8, 7.4)."""
    case, sd = smooth_case()
    y0, ti = case.vl.astype(np.float64), case.ti.astype(np.float64)
    fn = R.IR.tendency(case.om, y0, ti)
    est = []
    for hm in (0.25, 0.125, 0.0625):
        h = hm * sd
        y1, _, e, _ = R.attempt(case.om, y0, fn, ti, np.zeros(3), np.full(3, h))
        fine, _ = R.trbdf2(case.om, y0, ti, 0.0, h, h / 64, adaptive=False)
        ratio = np.max(np.abs(e)) / np.max(np.abs(y1 - fine))
        assert 0.5 <= ratio <= 2.0, (hm, ratio)
        est.append(np.max(np.abs(e)))
    for a, b in zip(est, est[1:]):
        assert 6.0 <= a / b <= 9.0, est


def test_adaptive_lands_on_t1_and_follows_reltol():
    case, sd = smooth_case()
    T = 40 * sd
    ref, _ = R.trbdf2(case.om, case.vl, case.ti, 0.0, T, T / 640, adaptive=False)
    errs = []
    for rtol in (1e-3, 1e-5):
        v, info = R.trbdf2(case.om, case.vl, case.ti, 0.0, T, sd, adaptive=True, reltol=rtol, abstol=1e-8)
        assert np.all(info["t"] == T) and not info["failed"].any()
        assert np.all(np.isfinite(info["h"])) and np.all(info["h"] > 0)
        errs.append(np.max(np.abs(v - ref)))
    assert errs[1] < errs[0], errs


def test_null_arguments_are_refused_without_a_device():
    pkg = g.load_package()
    F = pkg._ffi
    L = F.lib()
    assert L.lh_integrate_trbdf2(None, None, None, 0.0, 1.0, 1.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
    st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
    assert L.lh_trbdf2_stats(None, st) == F.LH_EINVAL
    assert L.lh_last_error(None)


def test_host_tolerances_default_each_on_its_own():
    soil = g.load_package().soil
    assert soil._trbdf2_tolerances(None, None) == (1e-6, 1e-3)
    assert soil._trbdf2_tolerances(None, 1e-5) == (1e-6, 1e-5)
    assert soil._trbdf2_tolerances(1e-8, None) == (1e-8, 1e-3)
    m = g.load_package().TRBDF2(reltol=1e-5)
    assert soil._trbdf2_tolerances(m.abstol, m.reltol) == (1e-6, 1e-5)
