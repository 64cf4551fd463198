"""Checks the CPU and the GPU tests of the layered coupled and heat-only models share (test infrastructure, no test
of its own): a column-uniform map against the oracle called once per class, the plain statistic over such an
ensemble, and conservation against a pair of boundary fluxes."""
import numpy as np

import case_model as M
import layered_heat_ref as H
import parity_cases as pc

CW = {np.dtype(np.float64): 2.0, np.dtype(np.float32): 4.0}   # the fixed cases' constants (tests/test_gpu_parity.py)


def oracle_per_class(lay):
    """The oracle's tendencies of a column-uniform map: one call per class with that class's numbers as the scalar
    parameters and the class's columns gathered; -> ([(columns, scalar case, the call's result)], the results
    assembled into [ncols, nlev] arrays)."""
    calls, full = [], {}
    for cols, case in H.per_class_cases(lay):
        want = pc.O.rhs(case.om, case.vl, case.ti, case.rhoe, None)
        calls.append((cols, case, want))
        for k, v in want.items():
            full.setdefault(k, np.zeros((lay.case.ncols,) + v.shape[1:], v.dtype))[cols] = v
    return calls, full


def assert_close_per_class(lay, got, label="", plain=True):
    """`got` (tendencies of a column-uniform map) against the oracle called once per class: every class's cells
    within the tolerance model of its own call (parity_cases.assert_tendencies_close at the fixed cases' Cw), and
    -- plain -- the plain statistic over the ENSEMBLE, every cell against the field's largest tendency, as
    assert_tendencies_close(plain=True) takes it for a case that is one oracle call.
    -> (the largest share of the tolerance model used, the plain shares), per field"""
    cw = CW[np.dtype(lay.case.dtype)]
    used = {}
    calls, full = oracle_per_class(lay)
    for cols, case, want in calls:
        g = {k: np.ascontiguousarray(v[cols]) for k, v in got.items()}
        if "vl" in g:
            g["ti"] = np.zeros_like(g["vl"])
        pc.assert_tendencies_close(case, g, want, Cw=cw, label=label)
        for k, v in pc.error_summary(case, g, want, cw).items():
            used[k] = max(used.get(k, 0.0), v)
    share = pc.plain_statistic(lay.case, got, {k: full[k] for k in got})
    if plain:
        for k, v in share.items():
            assert v >= pc.PLAIN_SHARE_MIN[np.dtype(lay.case.dtype)], (label, k, v)
    return used, share


def check_conservation(lay, d, faces):
    """sum d dz = F_bottom - F_top per column and field within nlev 4 eps sum|d| dz"""
    om = lay.case.om
    dz = (om.zmax - om.zmin) / om.nlev
    eps = float(np.finfo(lay.case.dtype).eps)
    worst = {}
    for k, j in (("rhoe", 0), ("vl", 1)):
        if k not in d:
            continue
        x = d[k].astype(np.float64)
        f_bot = faces[M.FACE_BOTTOM][j].astype(np.float64)
        f_top = faces[M.FACE_TOP][j].astype(np.float64)
        bound = om.nlev * 4 * eps * np.abs(x).sum(axis=1) * dz
        err = np.abs(x.sum(axis=1) * dz - (f_bot - f_top))
        worst[k] = float(np.max(err / bound))
        assert np.all(err <= bound), (k, worst[k])
    return worst
