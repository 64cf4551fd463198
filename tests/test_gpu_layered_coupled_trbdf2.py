"""lh_integrate_layered_coupled_trbdf2 / LayeredCoupledAdaptiveTRBDF2: adaptive TR-BDF2 of the coupled water and heat
model with per-cell soil classes on the device, every column with its own error-controlled step, against the NumPy
reference (tests/layered_coupled_trbdf2_ref.py), layered_heat_ref.ssprk33, lh_integrate_coupled_trbdf2 on the
per-class twins and the boundary fluxes' budget.  Mirrors tests/test_gpu_coupled_trbdf2.py; the contexts, hydrology
pairs and refusal words are tests/test_gpu_layered_coupled_implicit.py's."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import case_model as M
import layered_coupled_implicit_ref as LC
import layered_coupled_trbdf2_ref as LT
import layered_heat_ref as LH
import layered_ref as R
import parity_cases as pc
from test_gpu_coupled_trbdf2 import KEYS, STATUS_FAILED, _bcv_of
from test_gpu_coupled_trbdf2 import on_device as scalar_on_device
from test_gpu_layered_coupled_implicit import (ATMOS, COUPLED_ONLY, FACTORS, HYDS, LAYERED_OTHER_MODEL, LDEXP, LIBM,
                                               NOT_APPLICABLE, PERCOL, SCALAR_WITH_CLASSES, coupled_gpu, ptr, refused, tiny)

pytestmark = pytest.mark.gpu

NAME, SCALAR = "lh_integrate_layered_coupled_trbdf2", "lh_integrate_coupled_trbdf2"
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
NO_CLASS_MAP = ": the context has no class map (lh_set_soil_class_map); lh_integrate_coupled_trbdf2 steps a model without soil classes"


def on_device(lay, t0, t1, dt, abstol=0.0, abstol_e=0.0, reltol=0.0, bcv=None, h0=None, flags=0, form=None, calls=1):
    """(vl, rhoe at t1, stats dict, status, dt_cols after the call) of one lh_integrate_layered_coupled_trbdf2 call from
    the case's own state.  form: the closure form the context must report.  calls > 1: the same call again from the same
    state and the same dt_cols on the same context, which must give the same bits."""
    import torch
    with coupled_gpu(lay) as gm:
        F = gm.F
        Y, Ya = gm.prognostic_and_aux()
        ft = torch.float64 if lay.case.dtype == np.float64 else torch.float32
        cols = torch.zeros(lay.case.ncols, dtype=ft, device="cuda")
        b = None if bcv is None else np.ascontiguousarray(bcv, dtype=np.float64)
        out = None
        for _ in range(calls):
            gm.upload(Y, F.LH_VAR_VARTHETA_L, lay.case.vl)
            gm.upload(Y, F.LH_VAR_RHOE_INT, lay.case.rhoe)
            cols.zero_()
            if h0 is not None:
                cols.copy_(torch.as_tensor(np.asarray(h0), dtype=ft))
            torch.cuda.synchronize()
            F.check(getattr(gm.L, NAME)(gm.ctx, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, C.c_void_p(cols.data_ptr()),
                                        ptr(b)), gm.ctx)
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(gm.L.lh_trbdf2_stats(gm.ctx, st), gm.ctx)
            got = (gm.download(Y, F.LH_VAR_VARTHETA_L), gm.download(Y, F.LH_VAR_RHOE_INT), dict(zip(KEYS, list(st))), gm.status(),
                   cols.cpu().numpy().astype(np.float64))
            if out is not None:
                np.testing.assert_array_equal(got[0], out[0])
                np.testing.assert_array_equal(got[1], out[1])
                np.testing.assert_array_equal(got[4], out[4])
                assert got[2] == out[2] and got[3] == out[3]
            out = got
        if form is not None:
            assert gm.L.lh_closure_form(gm.ctx) == form
        return out


def take(lay, idx):
    """the columns idx of a layered case, in that order"""
    idx = np.asarray(idx)
    case = dataclasses.replace(pc._w.reorder_columns(lay.case, idx), ncols=len(idx))
    return LH.LayeredHeat(case, lay.classes, lay.thermal, np.ascontiguousarray(np.asarray(lay.class_map)[idx]))


# ------------------------------------------------------------------ 1. one attempted step against the reference

_ONE_STEP = {}   # per (key, dtype, step, boundary table): the reference's attempts, computed once, never modified


def one_step_reference(key, lay, h, bcv=None):
    """One step of h from the case's state by the reference: iterated to round-off (exact), stopped by the device's
    Newton rule (and, in Float32, with every stage output rounded to Float32), the error norms E of the exact one,
    and per variable d = max |other - exact|: what the device's stopping rule (and storing the state in FT) costs --
    from the reference alone (tests/test_gpu_coupled_trbdf2.py::one_step_reference)."""
    key = key + (np.dtype(lay.case.dtype).name, lay.case.ncols, float(h), None if bcv is None else np.asarray(bcv).tobytes())
    if key not in _ONE_STEP:
        exact, E = LT.first_attempt(lay, h, bcv)
        other, Eo = LT.first_attempt(lay, h, bcv, newton=LT.device_newton(),
                                     round_to=None if lay.case.dtype == np.float64 else np.float32)
        d = (float(np.max(np.abs(other["v1"] - exact["v1"]))), float(np.max(np.abs(other["e1"] - exact["e1"]))))
        _ONE_STEP[key] = (exact, E, d, other["conv"], Eo)
    return _ONE_STEP[key]


def check_one_step(lay, key, h, bcv=None, label="", form=None, got=None):
    """A call that spans exactly one step where the reference accepts in every column (E <= 1, both stages converged
    under the device's rule): the device accepts once per column, lands on the reference's Y_1 within
    4 d + c eps ||Y|| per variable, c = 64 (Float64) or 8 (Float32), and proposes h clamp(0.9 E^(-1/3), 0.2, 5) within
    5 % (tests/test_gpu_layered_implicit.py's tolerance on a proposal).  d is one_step_reference's, from the reference
    alone; the second term is the rounding of two evaluations of the same formulas in FT
    (tests/test_gpu_coupled_trbdf2.py::check_one_step, whose bound this is).  got: a result to judge instead of a
    call's."""
    exact, E, (dv, de), conv, _ = one_step_reference(key, lay, h, bcv)
    assert np.all(E <= 1.0) and np.all(conv), (label, E, conv)   # (the reference's own condition for this check)
    v1, e1, st, status, cols = got if got is not None else on_device(lay, 0.0, h, h, bcv=bcv, form=form)
    assert status == 0 and st["failed"] == 0, (label, status, st)
    n = lay.case.ncols
    eps = float(np.finfo(lay.case.dtype).eps)
    c = 64 if lay.case.dtype == np.float64 else 8
    bv = 4 * dv + c * eps * float(np.max(np.abs(exact["v1"])))
    be = 4 * de + c * eps * float(np.max(np.abs(exact["e1"])))
    gv = float(np.max(np.abs(v1.astype(np.float64) - exact["v1"])))
    ge = float(np.max(np.abs(e1.astype(np.float64) - exact["e1"])))
    want = h * LT.step_factor(E)
    print(f"one step {label} {np.dtype(lay.case.dtype).name}: E {E.min():.3g}..{E.max():.3g}, vl {gv:.3g} (4 d = {4 * dv:.3g}, bound {bv:.3g}), "
          f"rhoe {ge:.3g} (4 d = {4 * de:.3g}, bound {be:.3g}), proposal / reference {np.min(cols / want):.4f}..{np.max(cols / want):.4f}, {st}")
    assert st["accepted"] == n and st["rejected"] == 0, (label, E, st)
    np.testing.assert_allclose(cols, want, rtol=0.05, err_msg=f"{label} E={E}")
    assert gv <= bv, (label, gv, dv, bv)
    assert ge <= be, (label, ge, de, be)
    return v1, e1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mult", [0.25, 1.0])
@pytest.mark.parametrize("name", ["A", "C"])
def test_one_step_against_the_cpu_reference(name, mult, dtype):
    """Cases A (8 x 24, three horizons, flux / free drainage, Dirichlet energy, ice) and C (8 x 12, a class per cell,
    Dirichlet / free drainage, no ice) at 0.25 and 1 stable step: the reference measures E <= 0.0021 and 0.069 (A),
    0.0078 and 0.25 (C), every column accepts.  check_one_step's bounds."""
    lay = LT.make_case(name, dtype)
    check_one_step(lay, ("case", name), mult * LC.stable_dt(lay), label=f"{name} {mult}x")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["A", "C"])
def test_a_step_of_64_stable_steps_is_rejected_and_the_call_still_arrives(name, dtype):
    """At 64 stable steps the reference has E >= 2.5 in every column of A and C (tests/
    test_layered_coupled_trbdf2_reference.py): every column rejects its first attempt (at least ncols rejected steps
    in all) and the call still reaches t1 with status 0, no failed column and a positive proposal in every column."""
    lay = LT.make_case(name, dtype)
    h = 64.0 * LC.stable_dt(lay)
    _, _, _, conv, Eo = one_step_reference(("case", name), lay, h)
    assert np.all((Eo >= 1.4) | ~conv), (Eo, conv)
    v1, e1, st, status, cols = on_device(lay, 0.0, h, h)
    n = lay.case.ncols
    print(f"64x {name} {np.dtype(dtype).name}: reference E {Eo.min():.3g}..{Eo.max():.3g}, {st}")
    assert status == 0 and st["failed"] == 0, (status, st)
    # (a rejected attempt leaves at most 0.9 of the interval as the next step: two more steps at the least)
    assert st["rejected"] >= n and st["accepted"] >= 2 * n and st["max_steps"] >= 3, st
    assert np.all(cols > 0) and np.all(np.isfinite(v1)) and np.all(np.isfinite(e1))


# ------------------------------------------------------------------ 2. integration

_DEVICE = {}   # per (case, dtype, reltol): the device's integration over SPAN stable steps, computed once
_UNROUNDED = {}


def device_integration(name, dtype, reltol):
    key = (name, np.dtype(dtype).name, reltol)
    if key not in _DEVICE:
        lay = LT.make_case(name, dtype)
        sd = LC.stable_dt(lay)
        _DEVICE[key] = on_device(lay, 0.0, LT.SPAN * sd, sd, reltol=reltol)
    return _DEVICE[key]


def errors(v, e, want):
    return [float(np.max(np.abs(np.asarray(a, dtype=np.float64) - w))) for a, w in ((v, want[0]), (e, want[1]))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("reltol", [1e-3, 1e-4])
@pytest.mark.parametrize("name", sorted(LT.CASES))
def test_integration_against_ssprk33_and_the_reference_integrator(name, reltol, dtype):
    """Cases A-D over 64 stable steps from h0 = the stable step: status 0, no failed column; the errors in vartheta_l
    and rhoe_int against layered_heat_ref.ssprk33 at a quarter of the stable step are at most 2x the NumPy integrator's
    own (the device's Newton rule; in Float32 with everything the device keeps in a Float32 plane rounded to Float32).
    2x and not 1.5x: a column with E near 1 may accept on one side and reject on the other, which shifts its step
    sequence.  In Float64 the errors fall from reltol 1e-3 to 1e-4.  In Float32 the vartheta_l error is also held to
    the unrounded reference's error plus one eps32 max |vartheta_l| per attempted step
    (tests/test_gpu_coupled_trbdf2.py's rule).  Ratios and step counts are printed before they are asserted."""
    lay = LT.make_case(name, dtype)
    ssp = LT.ssprk33_reference(name, lay)
    vr, er, info = LT.integrated(name, lay, reltol, round_to=None if dtype == np.float64 else np.float32)
    v1, e1, st, status, cols = device_integration(name, dtype, reltol)
    n = lay.case.ncols
    dev, ref = errors(v1, e1, ssp), errors(vr, er, ssp)
    print(f"integration {name} {np.dtype(dtype).name} reltol {reltol}: errors device {dev[0]:.3g} {dev[1]:.3g}, reference {ref[0]:.3g} "
          f"{ref[1]:.3g}, ratios {dev[0] / ref[0]:.3f} {dev[1] / ref[1]:.3f}; accepted {st['accepted']} (reference "
          f"{int(info['accepted'].sum())}), rejected {st['rejected']} (reference {int(info['rejected'].sum())}), Newton per stage "
          f"{st['newton_iterations'] / (2.0 * (st['accepted'] + st['rejected'])):.2f}")
    assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (status, st)
    assert not info["failed"].any() and st["accepted"] >= n
    assert dev[0] <= 2.0 * ref[0] and dev[1] <= 2.0 * ref[1], (dev, ref)
    if dtype == np.float32:
        key = (name, reltol)
        if key not in _UNROUNDED:
            vu, _, iu = LT.integrated(name, lay, reltol)
            _UNROUNDED[key] = (float(np.max(np.abs(vu - ssp[0]))), int(np.max(iu["accepted"] + iu["rejected"])))
        own, steps = _UNROUNDED[key]
        unit = float(np.finfo(np.float32).eps) * float(np.max(np.abs(lay.case.vl)))
        print(f"  Float32 rounding: (device - unrounded reference) / (eps32 max|vl|) per attempted step "
              f"{(dev[0] - own) / unit / steps:.2f} ({steps} steps)")
        assert dev[0] <= own + steps * unit, (dev[0], own, steps, unit)
    elif reltol == 1e-4:
        loose = device_integration(name, dtype, 1e-3)
        last = errors(loose[0], loose[1], ssp)
        assert dev[0] < last[0] and dev[1] < last[1], (dev, last)


# ------------------------------------------------------------------ 3. shapes and independence

def shape_case(dtype, ncols, nlev, kind="cells"):
    return LC.layered_case(dtype, ncols, nlev, kind=kind, hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(c, n, "cells") for c in (1, 67, 130) for n in (1, 2, 3, 12)] + [(67, 24, "horizons")],
                         ids=lambda s: f"{s[0]}x{s[1]}_{s[2]}")
def test_shapes(shape, dtype):
    """A class per cell (5 classes, two organic) and 67 x 24 with three horizons; a ragged last wave, both faces on
    one cell, no interior face, one interior cell: 8 stable steps, every column reaches t1 finite with status 0, a
    repeated call from the same state gives the same bits, wave_steps >= accepted + rejected, and the last column is
    bitwise what it is in a call of its own."""
    ncols, nlev, kind = shape
    lay = shape_case(dtype, ncols, nlev, kind)
    sd = LC.stable_dt(lay)
    v1, e1, st, status, cols = on_device(lay, 0.0, 8 * sd, sd, calls=2)
    assert status == 0 and st["failed"] == 0 and st["accepted"] >= ncols, (status, st)
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(e1)) and np.all(cols > 0)
    assert np.max(np.abs(e1 - lay.case.rhoe)) > 0
    assert st["wave_steps"] >= st["accepted"] + st["rejected"] and st["unconverged"] == 0
    k = ncols - 1
    v_k, e_k, _, _, c_k = on_device(take(lay, [k]), 0.0, 8 * sd, sd)
    np.testing.assert_array_equal(v_k[0], v1[k])
    np.testing.assert_array_equal(e_k[0], e1[k])
    assert c_k[0] == cols[k]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_independence(dtype):
    """130 x 12 with a class per cell over 20 stable steps: a permutation of the columns (with their rows of the class
    map) permutes both planes and dt_cols bitwise; the first 67 columns are bitwise the 67-column run; the columns did
    choose their own steps."""
    lay = shape_case(dtype, 130, 12)
    sd = LC.stable_dt(lay)
    T = 20 * sd
    v_a, e_a, st, status, cols = on_device(lay, 0.0, T, sd)
    assert status == 0 and st["failed"] == 0 and np.all(cols > 0), (status, st)
    order = np.random.default_rng(5).permutation(130)
    v_p, e_p, _, _, cols_p = on_device(take(lay, order), 0.0, T, sd)
    np.testing.assert_array_equal(v_p, v_a[order])
    np.testing.assert_array_equal(e_p, e_a[order])
    np.testing.assert_array_equal(cols_p, cols[order])
    small = shape_case(dtype, 67, 12)
    np.testing.assert_array_equal(small.case.vl, lay.case.vl[:67])
    np.testing.assert_array_equal(small.class_map, lay.class_map[:67])
    v_s, e_s, _, _, cols_s = on_device(small, 0.0, T, sd)
    np.testing.assert_array_equal(v_s, v_a[:67])
    np.testing.assert_array_equal(e_s, e_a[:67])
    np.testing.assert_array_equal(cols_s, cols[:67])
    assert st["wave_steps"] >= st["accepted"] + st["rejected"]
    assert len(set(cols.tolist())) > 1


def test_sixteen_classes_keep_the_nibble_mask_path():
    """67 x 12 with all 16 classes of layered_ref.texture_classes, class (c + 2 i) mod 16 in cell (c, i): every index
    0..15 occurs, so the class byte's four-bit mask selects among a full table.  One attempt of 4 stable steps (the
    stable step is that of the most conductive class, 0.019 s; the reference has E <= 0.34 there) within
    check_one_step's bounds of the reference, which reads the same 16 classes; the first 8 columns run alone are
    bitwise their part of the 67-column call."""
    ncols, nlev = 67, 12
    cmap = LC.cell_map(ncols, nlev, 16)
    assert set(np.unique(cmap).tolist()) == set(range(16))
    lay = LH.make_layered_heat(np.float64, ncols, nlev, cmap, model=M.MODEL_COUPLED, classes=R.texture_classes()[:16],
                               thermal=LH.thermal_classes()[:16], bc="dirichlet", ice=True, name="layered_coupled_trbdf2_16")
    lay.case.om.percol_bc = {}
    h = 4.0 * LC.stable_dt(lay)
    whole = on_device(lay, 0.0, h, h)
    check_one_step(lay, ("sixteen",), h, label="16 classes", got=whole)
    got = on_device(take(lay, np.arange(8)), 0.0, h, h)
    np.testing.assert_array_equal(got[0], whole[0][:8])
    np.testing.assert_array_equal(got[1], whole[1][:8])
    np.testing.assert_array_equal(got[4], whole[4][:8])


# ------------------------------------------------------------------ 4. the clay form

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ice", [False, True], ids=["noice", "ice"])
def test_clay_form(ice, dtype):
    """67 x 12, a class per cell from the table whose fifth class has n = 1.06 (layered_adaptive_cases.clay_table: the
    host chooses the v_ldexp closure form for the whole table, so Float64 runs the VGF = false kernels;
    lh_closure_form is asserted, Float32 has one form): one attempt of one stable step within check_one_step's
    bounds."""
    import layered_adaptive_cases as AC
    classes = AC.clay_table()[[0, 1, 2, 3, AC.CLAY_CLASS]]
    assert classes[4, 0] == 1.06
    lay = LC.layered_case(dtype, 67, 12, kind="cells", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=ice, classes=classes)
    assert np.any(lay.class_map == 4)
    check_one_step(lay, ("clay", ice), LC.stable_dt(lay), label=f"clay ice={ice}", form=LDEXP if dtype == np.float64 else NOT_APPLICABLE)


# ------------------------------------------------------------------ 5. boundary values in time

def dirichlet_case(dtype, ncols, hyd="dirichlet"):
    return LC.layered_case(dtype, ncols, 12, kind="cells", hyd=HYDS[hyd], energy="dirichlet", ice=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constant_boundary_table_is_the_null_call(dtype):
    """A bcv whose two ends equal lh_set_bc's values is bitwise the bcv = NULL call."""
    lay = dirichlet_case(dtype, 67)
    sd = LC.stable_dt(lay)
    v0, e0, st0, s0, c0 = on_device(lay, 0.0, 16 * sd, sd)
    v1, e1, st1, s1, c1 = on_device(lay, 0.0, 16 * sd, sd, bcv=_bcv_of(lay.case))
    assert s0 == 0 and s1 == 0 and st0 == st1
    np.testing.assert_array_equal(v1, v0)
    np.testing.assert_array_equal(e1, e0)
    np.testing.assert_array_equal(c1, c0)


@pytest.mark.parametrize("face", ["top", "bottom"])
def test_ramped_dirichlet_values_against_the_reference(face):
    """Dirichlet T (+1.5 K) and vartheta_l (+0.02) at the top, or Dirichlet T (+0.5 K) at the bottom (its conductance
    in the pivot of cell 0, in the stage solves and in the homogeneous error solve), ramped over one step of half a
    stable step through bcv (the stage values at t + gamma h and t + h): check_one_step's bounds against the reference
    reading the same table, and another result than the constant table's."""
    lay = dirichlet_case(np.float64, 8, "dirichlet" if face == "top" else "dirichlet_drain")
    bc = lay.case.om.bc
    h = 0.5 * LC.stable_dt(lay)
    if face == "top":
        ramp = {(M.FACE_TOP, M.COMP_ENERGY): bc[(M.FACE_TOP, M.COMP_ENERGY)][1] + 1.5,
                (M.FACE_TOP, M.COMP_HYDROLOGY): bc[(M.FACE_TOP, M.COMP_HYDROLOGY)][1] + 0.02}
    else:
        ramp = {(M.FACE_BOTTOM, M.COMP_ENERGY): bc[(M.FACE_BOTTOM, M.COMP_ENERGY)][1] + 0.5}
    v1, e1 = check_one_step(lay, ("ramp", face), h, bcv=_bcv_of(lay.case, ramp), label=f"ramp {face}")
    v0, e0, *_ = on_device(lay, 0.0, h, h, bcv=_bcv_of(lay.case))
    assert np.max(np.abs(e1 - e0)) > 0
    assert face == "bottom" or np.max(np.abs(v1 - v0)) > 0


# ------------------------------------------------------------------ 6. against the scalar call

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_column_uniform_classes_against_the_scalar_call(dtype):
    """67 x 12 with every column one of 3 classes, one attempt of one stable step: within check_one_step's bounds of
    the reference, and lh_integrate_coupled_trbdf2 on the per-class scalar twins (layered_heat_ref.per_class_cases,
    tests/test_gpu_layered_coupled_implicit.py's construction) lands within the same bounds of the layered result (not
    bitwise: the layered water path carries true conductivities K_r Ksat)."""
    lay = LC.layered_case(dtype, 67, 12, kind="columns", hyd=HYDS["dirichlet_drain"], energy="dirichlet", ice=True)
    h = LC.stable_dt(lay)
    v1, e1 = check_one_step(lay, ("columns",), h, label="columns")
    exact, _, (dv, de), _, _ = one_step_reference(("columns",), lay, h)
    eps, c = float(np.finfo(dtype).eps), 64 if dtype == np.float64 else 8
    bv = 4 * dv + c * eps * float(np.max(np.abs(exact["v1"])))
    be = 4 * de + c * eps * float(np.max(np.abs(exact["e1"])))
    worst_v = worst_e = 0.0
    for cols, case in LH.per_class_cases(lay):
        vs, es, st, status, _ = scalar_on_device(case, 0.0, h, h)
        assert status == 0 and st["accepted"] == len(cols) and st["rejected"] == 0, (status, st)
        worst_v = max(worst_v, float(np.max(np.abs(vs.astype(np.float64) - v1[cols]))))
        worst_e = max(worst_e, float(np.max(np.abs(es.astype(np.float64) - e1[cols]))))
    print(f"layered against scalar {np.dtype(dtype).name}: vl {worst_v:.3g} (bound {bv:.3g}), rhoe {worst_e:.3g} (bound {be:.3g})")
    assert worst_v <= bv and worst_e <= be


# ------------------------------------------------------------------ 7. failure

def test_a_tolerance_float32_cannot_meet_fails_every_column():
    """All three tolerances 1e-14 in Float32 (case B's faces, 67 x 12): h shrinks to the floor, every column fails
    (status bit 4) with nothing accepted, both planes are bitwise the initial state and dt_cols is 0.  The controller's
    own exit, not a fault."""
    lay = LT.make_case("B", np.float32, ncols=67)
    sd = LC.stable_dt(lay)
    v, e, st, status, cols = on_device(lay, 0.0, 10 * sd, sd, abstol=1e-14, abstol_e=1e-14, reltol=1e-14)
    assert status & STATUS_FAILED and st["failed"] == 67 and np.all(cols == 0), (status, st)
    assert st["accepted"] == 0 and st["rejected"] >= 67
    np.testing.assert_array_equal(v, lay.case.vl)
    np.testing.assert_array_equal(e, lay.case.rhoe)


# ------------------------------------------------------------------ 8. conservation

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conservation_with_flux_faces(dtype):
    """Case B's faces (flux in both components, ice) on 67 x 12, 64 stable steps at reltol 1e-3: per column
    sum_i rhoe_int and sum_i vartheta_l change by (t1 - t0) (F_b - F_t) / dz however the column chose its steps, to
    nlev 4 eps sum |rhoe_int| and nlev (4 eps sum |vartheta_l| + kappa (abstol + reltol nu_max)), nu_max the largest
    class porosity: tests/test_gpu_coupled_trbdf2.py::test_conservation_with_flux_faces' forms.  Both expected changes
    are non-zero."""
    fe_t, fe_b, fw_t, fw_b = -2.0, 3.0, -2e-9, -5e-10
    lay = LT.make_case("B", dtype, ncols=67)
    om = lay.case.om
    om.bc[(M.FACE_TOP, M.COMP_ENERGY)], om.bc[(M.FACE_BOTTOM, M.COMP_ENERGY)] = (M.BC_FLUX, fe_t), (M.BC_FLUX, fe_b)
    om.bc[(M.FACE_TOP, M.COMP_HYDROLOGY)], om.bc[(M.FACE_BOTTOM, M.COMP_HYDROLOGY)] = (M.BC_FLUX, fw_t), (M.BC_FLUX, fw_b)
    sd = LC.stable_dt(lay)
    T = 64 * sd
    n, eps = om.nlev, float(np.finfo(dtype).eps)
    v1, e1, st, status, cols = on_device(lay, 0.0, T, sd)
    assert status == 0 and st["failed"] == 0 and len(set(cols.tolist())) > 1, (status, st)
    vl0, re0 = LC.state64(lay)
    dz = (om.zmax - om.zmin) / om.nlev
    newton = LT.NEWTON_KAPPA * (LT.ABSTOL + LT.RELTOL * float(lay.classes[:, 4].max()))
    for name, got, was, fb, ft, extra in (("rhoe", e1, re0, fe_b, fe_t, 0.0), ("vl", v1, vl0, fw_b, fw_t, newton)):
        change = got.astype(np.float64).sum(axis=1) - was.sum(axis=1)
        want = T * (fb - ft) / dz
        allowed = n * (4 * eps * np.abs(was).sum(axis=1) + extra)
        print(f"conservation {name} {np.dtype(dtype).name}: worst {np.max(np.abs(change - want) / allowed):.3g} of the bound, "
              f"expected change {want:.3g}, steps per column {st['accepted'] / 67.0:.1f}")
        assert abs(want) > 0
        assert np.all(np.abs(change - want) <= allowed), (name, float(np.max(np.abs(change - want) / allowed)))


# ------------------------------------------------------------------ 9. the contract

def test_each_tolerance_defaults_on_its_own():
    """A tolerance of 0 takes its own default (abstol 1e-6, abstol_e 1e-6 rho_l c_l, reltol 1e-3), bit for bit, also
    beside tolerances that are not the defaults; the energy's tolerance is read."""
    lay = LT.make_case("A", np.float64, ncols=67)
    sd = LC.stable_dt(lay)
    T = 16 * sd
    ae = LT.abstol_e_default(lay)
    ref = on_device(lay, 0.0, T, sd, abstol=1e-6, abstol_e=ae, reltol=1e-3)
    for a, b, r in ((0.0, ae, 1e-3), (1e-6, 0.0, 1e-3), (1e-6, ae, 0.0), (0.0, 0.0, 0.0)):
        got = on_device(lay, 0.0, T, sd, abstol=a, abstol_e=b, reltol=r)
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[4], ref[4])
    tight = on_device(lay, 0.0, T, sd, abstol=1e-8, abstol_e=ae, reltol=1e-4)
    got = on_device(lay, 0.0, T, sd, abstol=1e-8, abstol_e=0.0, reltol=1e-4)
    np.testing.assert_array_equal(got[1], tight[1])
    assert np.max(np.abs(tight[1] - ref[1])) > 0 and tight[3] == 0
    loose_e = on_device(lay, 0.0, T, sd, abstol_e=1e3 * ae)
    assert np.max(np.abs(loose_e[1] - ref[1])) > 0


def call(g, Y, Ya, t0=0.0, t1=1.0, dt=1.0, abstol=0.0, abstol_e=0.0, reltol=0.0, flags=0, name=NAME, bcv=None):
    return getattr(g.L, name)(g.ctx, Y, Ya, t0, t1, dt, abstol, abstol_e, reltol, flags, None, ptr(bcv))


def refused_with_zero_stats(g, rc, code, message):
    refused(g, rc, code, message)
    st = (C.c_int64 * g.F.LH_TRBDF2_NSTATS)(*([7] * g.F.LH_TRBDF2_NSTATS))   # a refused call reports zeros
    g.F.check(g.L.lh_trbdf2_stats(g.ctx, st), g.ctx)
    assert list(st) == [0] * g.F.LH_TRBDF2_NSTATS


def test_refusals_in_their_order():
    """The arguments first, then lh_step_layered_coupled_implicit's order: the model, a context without a map (the
    scalar call is named, and integrates it), layered_check (a prescribed atmosphere, per-column arrays, LH_MATH_LIBM),
    conductivity factors, the states.  A refused call leaves the statistics zeroed -- also after a call that
    counted -- and t1 == t0 leaves Y untouched."""
    lay = tiny()
    nan, inf = float("nan"), float("inf")
    tols = NAME + ": tolerances must be finite and >= 0"
    rich = R.make_layered(np.float64, 5, 6, R.uniform_map(5, 6, 2), classes=R.texture_classes()[:2])
    with pc.GpuModel(rich.case) as g:                                   # a Richards context with a map
        g.set_soil_classes(rich.classes, rich.class_map)
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        refused_with_zero_stats(g, call(g, Y, Ya, t0=1.0, t1=0.0), F.LH_EINVAL, NAME + ": need finite t0 <= t1")
        refused_with_zero_stats(g, call(g, Y, Ya, t1=inf), F.LH_EINVAL, NAME + ": need finite t0 <= t1")
        for dt in (0.0, -1.0, nan, inf):
            refused_with_zero_stats(g, call(g, Y, Ya, dt=dt), F.LH_EINVAL, NAME + ": need a finite dt > 0")
        for bad in (-1e-6, nan, inf):
            refused_with_zero_stats(g, call(g, Y, Ya, abstol=bad), F.LH_EINVAL, tols)
            refused_with_zero_stats(g, call(g, Y, Ya, abstol_e=bad), F.LH_EINVAL, tols)
            refused_with_zero_stats(g, call(g, Y, Ya, reltol=bad), F.LH_EINVAL, tols)
        refused_with_zero_stats(g, call(g, Y, Ya, flags=1), F.LH_EINVAL, NAME + ": unknown flags 0x1")
        refused_with_zero_stats(g, call(g, Y, Ya, flags=0x80000000), F.LH_EINVAL, NAME + ": unknown flags 0x80000000")
        refused_with_zero_stats(g, call(g, Y, Ya, bcv=np.full(8, nan)), F.LH_EINVAL, NAME + ": non-finite boundary value")
        assert getattr(g.L, NAME)(None, Y, Ya, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0, None, None) == F.LH_EINVAL
        refused_with_zero_stats(g, call(g, Y, Ya), F.LH_EMODEL, NAME + LAYERED_OTHER_MODEL)   # the arguments came first
    with pc.GpuModel(rich.case) as g:                                   # (the same model without a map)
        Y, Ya = g.prognostic_and_aux()
        refused_with_zero_stats(g, call(g, Y, Ya), g.F.LH_EMODEL, NAME + COUPLED_ONLY)
    with pc.GpuModel(lay.case) as g:                                    # a coupled context without a map
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        refused_with_zero_stats(g, call(g, Y, Ya), F.LH_EMODEL, NAME + NO_CLASS_MAP)
        g.set_soil_classes(lay.classes, None, thermal=lay.thermal)       # classes alone are not a map
        refused_with_zero_stats(g, call(g, Y, Ya), F.LH_EMODEL, NAME + NO_CLASS_MAP)
        F.check(call(g, Y, Ya, t1=100.0, dt=100.0, name=SCALAR), g.ctx)  # the scalar call it names integrates it
        assert g.status() == 0
    with coupled_gpu(lay) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        arr = np.full(lay.case.ncols, 0.45)
        a = M.AtmosForcing()
        f = F.lh_atmos_forcing(a.u_atm, a.theta_atm, a.z_atm, a.theta_scale, a.rho_a_sfc, a.q_atm, 0.001, 0.001, a.R_v, a.R_d,
                               a.grav, a.cp_d, a.cp_v, a.LH_v0, a.T_triple, a.press_triple, a.von_karman)
        F.check(L.lh_set_atmos_forcing(ctx, C.byref(f), None), ctx)
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], arr.ctypes.data_as(C.POINTER(C.c_double))), ctx)
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        refused_with_zero_stats(g, call(g, None, Ya, dt=0.0), F.LH_EINVAL, NAME + ": need a finite dt > 0")
        refused_with_zero_stats(g, call(g, None, Ya), F.LH_EMODEL, NAME + ATMOS)       # all three set: the atmosphere first
        F.check(L.lh_set_atmos_forcing(ctx, None, None), ctx)
        refused_with_zero_stats(g, call(g, None, Ya), F.LH_EMODEL, NAME + PERCOL)      # then the per-column arrays
        F.check(L.lh_set_percol_param(ctx, F.LH_PC["nu"], None), ctx)
        refused_with_zero_stats(g, call(g, None, Ya), F.LH_EMODEL, NAME + LIBM)        # then LH_MATH_LIBM
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        assert call(g, None, Ya) == F.LH_ESTATE                                        # then the states
        refused(g, call(g, Y, Ya, name=SCALAR), F.LH_EMODEL, SCALAR + SCALAR_WITH_CLASSES)   # the scalar call's old words
        # t1 == t0 does nothing
        F.check(call(g, Y, Ya, t0=2.0, t1=2.0), ctx)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_VARTHETA_L), lay.case.vl)
        np.testing.assert_array_equal(g.download(Y, F.LH_VAR_RHOE_INT), lay.case.rhoe)
        st = (C.c_int64 * F.LH_TRBDF2_NSTATS)(*([7] * F.LH_TRBDF2_NSTATS))
        F.check(L.lh_trbdf2_stats(ctx, st), ctx)
        assert list(st) == [0] * F.LH_TRBDF2_NSTATS
        # a call that counts, then a refused one: zeros again
        F.check(call(g, Y, Ya, t1=100.0, dt=100.0), ctx)
        F.check(L.lh_trbdf2_stats(ctx, st), ctx)
        assert st[0] >= lay.case.ncols and np.any(g.download(Y, F.LH_VAR_RHOE_INT) != lay.case.rhoe) and g.status() == 0
        refused_with_zero_stats(g, call(g, Y, Ya, flags=1), F.LH_EINVAL, NAME + ": unknown flags 0x1")
    fac = tiny(factors=True)
    with coupled_gpu(fac) as g:
        F, L, ctx = g.F, g.L, g.ctx
        Y, Ya = g.prognostic_and_aux()
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_LIBM), ctx)
        refused_with_zero_stats(g, call(g, None, Ya), F.LH_EMODEL, NAME + LIBM)        # layered_check before the factors
        F.check(L.lh_set_math_mode(ctx, F.LH_MATH_FAST), ctx)
        refused_with_zero_stats(g, call(g, None, Ya), F.LH_EMODEL, NAME + FACTORS)     # the factors before the states


# ------------------------------------------------------------------ 10. the host mirror

def horizon_model(lh, lay, top, bottom, fw):
    """the SoilModel of a three-horizon coupled case (tests/test_gpu_layered_coupled_implicit.py's host-mirror model)"""
    FT = np.float64
    om = lay.case.om
    n, N = om.nlev, lay.case.ncols
    hm = lambda k: lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3])
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=hm(k), ν=k[4], S_s=k[5], thermal=lh.SoilThermal(FT, **dict(zip(LH.THERMAL_FIELDS, t))))
                         for k, t in zip(lay.classes, lay.thermal)], lay.class_map[0].astype(np.int64))
    dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
    bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.Dirichlet(top), hydrology=lh.VerticalFlux(fw)),
                         bottom=lh.SoilComponentBC(energy=lh.Dirichlet(bottom), hydrology=lh.FreeDrainage()))
    model = lh.SoilModel(FT, domain=dom, boundary_conditions=bc, soil_param_set=lh.SoilParams(FT),
                         earth_param_set=lh.EarthParameterSet(), energy_model=lh.SoilEnergyModel(),
                         hydrology_model=lh.SoilHydrologyModel(FT), soil_classes=sc)
    return model, dom, bc


def test_host_mirror_through_simulation():
    """A three-horizon coupled SoilModel with a diurnal sine as its Dirichlet top temperature through
    Simulation(model, LayeredCoupledAdaptiveTRBDF2(), saveat=...): bitwise the chain of direct C calls, one per dt
    interval, with the table sampled at the interval's two ends and dt_cols carried from call to call (also across the
    saveat chunks).  The marker refuses a model without classes when the Simulation is built, in the library's words,
    and takes no forcing=; the scalar marker keeps refusing the layered model."""
    import torch
    lh = pc._pkg()
    FT = np.float64
    lay = LC.layered_case(FT, 5, 12, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    case = lay.case
    bottom, day, fw = 281.0, 86400.0, -2e-9
    top = lambda t: 287.0 + 4.0 * math.sin(2.0 * math.pi * t / day)
    model, dom, bc = horizon_model(lh, lay, top, bottom, fw)
    Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.2 + 0.0 * z, "θ_i": 0.0 * z, "ρe_int": 1e7 + 0.0 * z}, 0.0)
    Y.soil.ϑ_l, Y.soil.ρe_int = case.vl, case.rhoe
    dt, total, chunk = 20 * LC.stable_dt(lay), 6, 3
    sim = lh.Simulation(model, lh.LayeredCoupledAdaptiveTRBDF2(reltol=1e-4), Y_init=Y, dt=dt, tspan=(0.0, total * dt), Ya_init=Ya,
                        saveat=chunk * dt)
    sol = lh.run(sim)
    got_v, got_e = np.array(sim.integrator.u.soil.ϑ_l), np.array(sim.integrator.u.soil.ρe_int)
    stats = sim.integrator.trbdf2_stats
    assert len(sol.t) == total // chunk + 1 and sol.t[-1] == total * dt and stats["failed"] == 0, stats
    with coupled_gpu(lay) as g:
        F = g.F
        Yd, Yad = g.prognostic_and_aux()
        cols = torch.zeros(case.ncols, dtype=torch.float64, device="cuda")
        accepted = 0
        # the mirror's intervals: within a saveat chunk that starts at T the ends are T + dt, T + 2 dt, ... and the chunk's
        # own end, (c + 1) chunk dt, the run's tf for the last
        ends = []
        for c in range(total // chunk):
            T = ends[-1] if ends else 0.0
            ends += [T + (k + 1) * dt for k in range(chunk - 1)] + [total * dt if c == total // chunk - 1 else (c + 1) * chunk * dt]
        t = 0.0
        for te in ends:
            bcv = np.zeros((2, 2, 2))
            bcv[:, M.FACE_BOTTOM, M.COMP_ENERGY], bcv[:, M.FACE_TOP, M.COMP_HYDROLOGY] = bottom, fw
            bcv[:, M.FACE_TOP, M.COMP_ENERGY] = top(t), top(te)
            F.check(getattr(g.L, NAME)(g.ctx, Yd, Yad, t, te, dt, 0.0, 0.0, 1e-4, 0, C.c_void_p(cols.data_ptr()), ptr(bcv)), g.ctx)
            st = (C.c_int64 * F.LH_TRBDF2_NSTATS)()
            F.check(g.L.lh_trbdf2_stats(g.ctx, st), g.ctx)
            accepted += st[0]
            t = te
        want_v, want_e = g.download(Yd, F.LH_VAR_VARTHETA_L), g.download(Yd, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_e, want_e)
    assert stats["accepted"] == accepted
    assert np.max(np.abs(want_e - case.rhoe)) > 1e-3 * np.max(np.abs(case.rhoe)) and np.max(np.abs(want_v - case.vl)) > 0
    # refusals when the Simulation is built, and no forcing=
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.Simulation(model, lh.CoupledAdaptiveTRBDF2(), Y_init=Y, dt=dt, tspan=(0.0, dt), Ya_init=Ya)
    kw = dict(domain=dom, earth_param_set=lh.EarthParameterSet())
    plain = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.SoilHydrologyModel(FT), boundary_conditions=bc, **kw)
    ebc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)), bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0)))
    heat = lh.SoilModel(FT, energy_model=lh.SoilEnergyModel(), hydrology_model=lh.PrescribedHydrologyModel(), boundary_conditions=ebc, **kw)
    for other, words in ((plain, r"the context has no class map \(lh_set_soil_class_map\); lh_integrate_coupled_trbdf2 steps"),
                         (heat, "coupled models only")):
        with pytest.raises(NotImplementedError, match="LayeredCoupledAdaptiveTRBDF2: " + words):
            lh.Simulation(other, lh.LayeredCoupledAdaptiveTRBDF2(), Y_init=object(), dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
        with pytest.raises(NotImplementedError, match="LayeredCoupledAdaptiveTRBDF2: " + words):
            lh.integrate_layered_coupled_trbdf2(other, object(), None, 0.0, 1.0, 1.0)
    with pytest.raises(TypeError):
        lh.LayeredCoupledAdaptiveTRBDF2(forcing=object())
    assert isinstance(lh.LayeredCoupledAdaptiveTRBDF2(), lh.CoupledAdaptiveTRBDF2)
    model.close()


# ------------------------------------------------------------------ 11. a sand-over-clay column, end to end

def test_sand_over_clay_against_ssprk33():
    """8 x 60 with three horizons (conductive, tight, conductive: Ksat jumps of more than 100 at both interfaces), a
    flux top and a free-draining bottom, Dirichlet temperatures (tests/test_gpu_layered_coupled_implicit.py's column).
    One call over 120 stable steps at the default tolerances from h0 = the stable step against lh_step_ssprk33 at half
    a stable step over the same span on the same layered context: the device-minus-SSPRK33 distance in vartheta_l and
    in rhoe_int is at most 2x the NumPy integrator's own distance to layered_heat_ref.ssprk33 at the same size."""
    FT = np.float64
    lay = LC.layered_case(FT, 8, 60, kind="horizons", hyd=(M.BC_FLUX, M.BC_FREE_DRAINAGE), energy="dirichlet")
    sd = LC.stable_dt(lay)
    span = 120
    vl0, re0 = LC.state64(lay)
    v1, e1, st, status, cols = on_device(lay, 0.0, span * sd, sd)
    assert status == 0 and st["failed"] == 0, (status, st)
    with coupled_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        F.check(g.L.lh_step_ssprk33(g.ctx, Y, Ya, 0.0, 0.5 * sd, 2 * span, None), g.ctx)
        vs, es = g.download(Y, F.LH_VAR_VARTHETA_L), g.download(Y, F.LH_VAR_RHOE_INT)
        assert g.status() == 0
    vr, er, info = LT.integrate(lay, vl0, re0, 0.0, span * sd, sd, newton=LT.device_newton())
    ex = LH.ssprk33(LH.as64(lay), 0.5 * sd, 2 * span)
    dev = (float(np.max(np.abs(v1 - vs))), float(np.max(np.abs(e1 - es))))
    ref = (float(np.max(np.abs(vr - ex["vl"]))), float(np.max(np.abs(er - ex["rhoe"]))))
    print(f"sand over clay: device - SSPRK33 vl {dev[0]:.3g}, rhoe {dev[1]:.3g}; reference - SSPRK33 vl {ref[0]:.3g}, rhoe {ref[1]:.3g}; "
          f"accepted {st['accepted']} rejected {st['rejected']} (reference {int(info['accepted'].sum())} {int(info['rejected'].sum())}); "
          f"the state moved by vl {np.max(np.abs(vs - vl0)):.3g}, rhoe {np.max(np.abs(es - re0)):.3g}")
    assert not info["failed"].any() and ref[0] > 0 and ref[1] > 0
    assert dev[0] <= 2 * ref[0] and dev[1] <= 2 * ref[1]
