"""NumPy reference for implicit steps of a LAYERED heat-only model (per-cell soil classes with their thermal
supplement): tests/heat_implicit_ref.py's construction with the tendency replaced by the NumPy restatement of
the layered tendency, layered_heat_ref.rhs in Float64.

With vartheta_l and theta_i prescribed the layered tendency is still affine in rhoe_int (every cell's T is
affine in its own rhoe_int, every face flux affine in its cells' T): f(Y, t) = A Y + b(t).  The bands of A come
from three coloured unit-vector evaluations, b(t) = f(0) under the boundary values of a bcv sample, a stage is one
Thomas solve in Float64.  thomas, matrix, cond_inf, stage_solve, _sample, with_energy_bc and the constants of the
two methods are heat_implicit_ref's, imported.  Needs neither the oracle nor the library.

Test infrastructure (tests/test_layered_heat_implicit_reference.py, tests/test_gpu_layered_heat_implicit.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

import case_model as M
import heat_implicit_ref as H
import layered_heat_ref as LH
import layered_ref as R

GAMMA, D = H.GAMMA, H.D
matrix, cond_inf, thomas, stage_solve, _sample = H.matrix, H.cond_inf, H.thomas, H.stage_solve, H._sample


def tendency(lay, rhoe, sample=None):
    """d rhoe_int / dt [ncols, nlev] of the Float64 twin of `lay` at the state rhoe, under the scalar energy
    boundary values of one bcv sample (None: the case's own)."""
    l64 = LH.as64(lay)
    if sample is not None:
        case = dataclasses.replace(l64.case, om=H.with_energy_bc(l64.case.om, sample))
        l64 = LH.LayeredHeat(case, l64.classes, l64.thermal, l64.class_map)
    return LH.rhs(l64, rhoe=np.asarray(rhoe, dtype=np.float64))["rhoe"].astype(np.float64)


def affine_parts(lay):
    """Bands (lo, di, up) of A as heat_implicit_ref.affine_parts returns them, and f(0)."""
    ncols, n = lay.case.vl.shape
    f0 = tendency(lay, np.zeros((ncols, n)))
    lo, di, up = np.zeros((ncols, n)), np.zeros((ncols, n)), np.zeros((ncols, n))
    s = 2.0 ** 30   # (a power of two: exact scaling; large, so that f(s e_j) - f(0) loses little to the constant)
    for k in range(3):
        e = np.zeros((ncols, n))
        e[:, k::3] = s
        df = (tendency(lay, e) - f0) / s
        for j in range(k, n, 3):
            di[:, j] = df[:, j]
            if j > 0:
                up[:, j - 1] = df[:, j - 1]
            if j + 1 < n:
                lo[:, j + 1] = df[:, j + 1]
    return (lo, di, up), f0


def heat_implicit(lay, rhoe, dt, nsteps, method="euler", bcv=None, bands=None):
    """nsteps steps of the [ncols, nlev] rhoe_int state (Float64) with heat_implicit_ref.heat_implicit's formulas;
    vartheta_l, theta_i and the class map of `lay` are held.  bands: affine_parts(lay)[0] where the caller has it."""
    assert method in ("euler", "trbdf2")
    y = np.array(rhoe, dtype=np.float64)
    if bcv is not None:
        assert np.asarray(bcv).shape == (nsteps + 1, 2, 2)
    if bands is None:
        bands, _ = affine_parts(lay)
    zero = np.zeros_like(y)
    b_at = lambda sample: tendency(lay, zero, sample)   # b(t) = f(0, t)
    b_const = None if bcv is not None else b_at(None)
    for k in range(nsteps):
        if method == "euler":
            b1 = b_const if bcv is None else b_at(_sample(bcv, k + 1))
            y = stage_solve(bands, dt, y + dt * b1)
            continue
        dh = D * dt
        fn = tendency(lay, y, _sample(bcv, k))
        bg = b_const if bcv is None else b_at(_sample(bcv, k, GAMMA))
        yg = stage_solve(bands, dh, y + dh * fn + dh * bg)
        w2 = (yg - (1.0 - GAMMA) ** 2 * y) / (GAMMA * (2.0 - GAMMA))
        b1 = b_const if bcv is None else b_at(_sample(bcv, k + 1))
        y = stage_solve(bands, dh, w2 + dh * b1)
    return y


def stable_dt(lay):
    """The explicit engines' cap of the Float64 twin, courant 1/2."""
    return LH.stable_dt(LH.as64(lay), 0.5)


def state64(lay):
    return np.asarray(lay.case.rhoe, dtype=np.float64)


# ------------------------------------------------------------------ cases shared by the two test files

NCLS = 5     # classes 1 and 4 are organic (layered_heat_ref.thermal_classes: every third): any_om is on


def cell_map(ncols, nlev, ncls=NCLS):
    """a different class in every cell: neighbours in a column differ by 2 (mod ncls), neighbouring columns by 1"""
    c, i = np.arange(ncols)[:, None], np.arange(nlev)[None, :]
    return ((c + 2 * i) % ncls).astype(np.uint8)


def three_horizons(ncols, nlev):
    """the same three horizons in every column (layered_ref.hydrostatic's proportions)"""
    row = np.zeros(nlev, dtype=np.uint8)
    row[nlev * 5 // 16:] = 1
    row[nlev * 11 // 16:] = 2
    return np.repeat(row[None, :], ncols, axis=0)


def column_map(ncols, nlev, ncls=3):
    """every column one class"""
    return R.uniform_map(ncols, nlev, ncls)


FLUX_TOP = (M.BC_FLUX, -0.8)   # layered_heat_ref.ENERGY_BC's top flux


def layered_case(dtype, ncols, nlev, kind="cells", bc="dirichlet", percol_bc=False, ice=False):
    """A heat-only case of layered_heat_ref.make_layered_heat.  kind: "cells" (cell_map, 5 classes), "horizons"
    (three_horizons, 3 classes with an organic one in the middle) or "columns" (column_map, 3 classes).
    bc: "dirichlet", "flux" or "mixed" (Dirichlet bottom, flux top).  percol_bc: the Dirichlet values vary by
    column (rounded to the working type, so that the device and the reference hold the same numbers)."""
    if kind == "cells":
        cmap, classes, thermal = cell_map(ncols, nlev), R.texture_classes()[:NCLS], LH.thermal_classes()[:NCLS]
        assert np.any(thermal[:, 6] > 0)
    elif kind == "horizons":
        cmap, classes, thermal = three_horizons(ncols, nlev), R.texture_classes()[[0, 5, 2]], LH.thermal_classes()[[0, 4, 2]]
    else:
        cmap, classes, thermal = column_map(ncols, nlev), R.texture_classes()[[0, 5, 2]], LH.thermal_classes()[[0, 4, 2]]
    lay = LH.make_layered_heat(dtype, ncols, nlev, cmap, model=M.MODEL_HEAT, classes=classes, thermal=thermal,
                               bc="flux" if bc == "flux" else "dirichlet", ice=ice, name="layered_heat_implicit")
    om = lay.case.om
    if bc == "mixed":
        om.bc[(M.FACE_TOP, M.COMP_ENERGY)] = FLUX_TOP
    if percol_bc:
        c = np.arange(ncols)
        om.percol_bc = {k: (v[1] + 2.0 * (H.pc.uhash(c, 77 + k[0], 1) - 0.5)).astype(dtype).astype(np.float64)
                        for k, v in om.bc.items() if v[0] == M.BC_DIRICHLET}
    return lay


# the order tests: three horizons, 24 levels, constant Dirichlet values over ORDER_SPAN stable steps
ORDER_SPAN = 2000.0
ORDER_STEPS = {"euler": (4, 8, 16, 32), "trbdf2": (8, 16, 32)}   # (TR-BDF2 from 4 to 8 steps: 4.8, not yet asymptotic)
ORDER_BANDS = {"euler": (1.8, 2.2), "trbdf2": (3.6, 4.4)}


def order_case(ncols=8, nlev=24):
    """Three horizons of eight levels (the first three classes, the middle one organic), Dirichlet faces, static ice
    in some columns, and -- as heat_implicit_ref's order case -- a smooth T(z) that meets the Dirichlet values at
    the faces: a start that is off them by several K puts a boundary-layer transient into the first steps, whose
    stiff components keep backward Euler's ratio above 2.2 at 4 and 8 steps of this span."""
    cmap = np.repeat(np.repeat(np.arange(3, dtype=np.uint8), nlev // 3)[None, :], ncols, axis=0)
    (_, vb), (_, vt) = LH.ENERGY_BC["dirichlet"]
    zc, _ = R.grid_np(-0.02 * nlev, 0.0, nlev)
    s = (zc + 0.02 * nlev) / (0.02 * nlev)
    T = vb + (vt - vb) * s + 3.0 * np.sin(np.pi * s)
    return LH.make_layered_heat(np.float64, ncols, nlev, cmap, model=M.MODEL_HEAT, classes=R.texture_classes()[:3],
                                thermal=LH.thermal_classes()[:3], bc="dirichlet", ice=True, T=T, name="layered_heat_order")


def order_errors(method, solve):
    """Max-norm errors of solve(lay, dt, nsteps) against the reference at dt / 16, per step count."""
    lay = order_case()
    bands, _ = affine_parts(lay)
    span = ORDER_SPAN * stable_dt(lay)
    errs = []
    for n in ORDER_STEPS[method]:
        ref = heat_implicit(lay, state64(lay), span / n / 16, 16 * n, method, bands=bands)
        errs.append(float(np.max(np.abs(solve(lay, span / n, n) - ref))))
    return errs
