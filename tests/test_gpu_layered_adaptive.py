"""Adaptive SSPRK33 for layered Richards soils: lh_layered_step_bound_device,
lh_step_layered_ssprk33_device_dt and lh_step_layered_ssprk33_adaptive_hold, all served by the BOUND flavour of the
layered column stepper.

The hold call is DEFINED by a sequence of existing calls plus the bound entry: per chunk lh_layered_step_bound_device
into a word that is read, dt = min(bound, dt_max) in the working type, lh_set_tuning("persist=0") and
lh_step_ssprk33(Y, dt, hold) -- the fused stages with the step by value --, elapsed advanced by `hold` additions in
the working type.  vartheta_l, every chunk's dt, elapsed and lh_get_status must be those bits, as one call of three
chunks and as three calls of one chunk: that the two dt lists agree is what shows that the bound a launch leaves
after k steps equals the bound of a zero-step launch on the same state.

What the expectations of the flag, cap, Dirichlet and clay cases rest on is asserted on the CPU by
tests/test_layered_adaptive_cpu.py (tests/layered_adaptive_cases.py holds the cases)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import case_model as M
import layered_adaptive_cases as A
import layered_heat_ref as H
import layered_ref as R
import parity_cases as pc

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
FUSED, STEPPER = b"persist=0", b"persist=2"
COURANT, NCHUNKS = A.COURANT, A.NCHUNKS
# the project's tolerance for the Float32-accumulated rule against the working-type one (test_gpu_stepper.py)
BOUND_RTOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 2e-4}
DP = C.POINTER(C.c_double)


def layered_gpu(lay):
    g = pc.GpuModel(lay.case)
    g.set_soil_classes(lay.classes, lay.class_map)
    return g


def _word(dtype, value=0.0):
    import torch
    w = torch.full((1,), value, device="cuda", dtype=torch.float64 if np.dtype(dtype) == np.float64 else torch.float32)
    torch.cuda.synchronize()   # (the library works on its own stream)
    return w


def fresh_state(g, zero_ti_plane=False):
    """(Y, Ya) of the case; zero_ti_plane: the all-zero theta_i goes up as a plane, not as a fill"""
    Y, Ya = g.prognostic_and_aux()
    if zero_ti_plane:
        assert not np.any(g.case.ti)
        z = np.zeros_like(g.case.vl)
        g.F.check(g.L.lh_upload(g.ctx, Y, g.F.LH_VAR_THETA_I, z.ctypes.data, 1, g.case.om.nlev), g.ctx)
    return Y, Ya


def bound_device(g, Y, Ya, courant=COURANT, word=None):
    w = _word(g.case.dtype, -1.0) if word is None else word
    g.F.check(g.L.lh_layered_step_bound_device(g.ctx, Y, Ya, courant, w.data_ptr()), g.ctx)
    g.F.check(g.L.lh_synchronize(g.ctx), g.ctx)
    return float(w.item())


def host_stable_dt(g, Y, Ya, courant=COURANT):
    out = C.c_double()
    g.F.check(g.L.lh_stable_dt(g.ctx, Y, Ya, courant, C.byref(out)), g.ctx)
    return out.value


def defining_sequence(g, Y, Ya, courant, dt_max, nchunks, hold):
    """The defining sequence on Y.  -> (dt of every chunk, elapsed in FT, the bound before every chunk and after the last,
    the status the hold call must report: the sequence's own, plus bit 5 where a chunk's dt exceeds the bound of
    the state it ended on)"""
    F, L, ctx = g.F, g.L, g.ctx
    FT = np.dtype(g.case.dtype).type
    dts, bounds, elapsed = [], [], np.zeros(1, dtype=FT)
    for _ in range(nchunks):
        b = bound_device(g, Y, Ya, courant)
        bounds.append(b)
        dt = FT(b)
        if dt_max > 0 and not dt <= FT(dt_max):
            dt = FT(dt_max)
        F.check(L.lh_set_tuning(ctx, FUSED), ctx)
        F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, float(dt), hold, None), ctx)
        dts.append(float(dt))
        for _ in range(hold):
            elapsed += dt
    bounds.append(bound_device(g, Y, Ya, courant))
    status = g.status()
    if any(not (b > 0 and np.isfinite(b)) or b < d for b, d in zip(bounds[1:], dts)):
        status |= 32
    return dts, float(elapsed[0]), bounds, status


def hold_call(g, Y, Ya, courant, dt_max, nchunks, hold, calls=1):
    """`calls` calls of nchunks chunks.  -> (vartheta_l, the dt after every call, elapsed, status)"""
    F, L, ctx = g.F, g.L, g.ctx
    t, el = _word(g.case.dtype), _word(g.case.dtype)
    each = []
    for _ in range(calls):
        F.check(L.lh_step_layered_ssprk33_adaptive_hold(ctx, Y, Ya, 0.0, courant, dt_max, nchunks, hold, t.data_ptr(), el.data_ptr()), ctx)
        F.check(L.lh_synchronize(ctx), ctx)
        each.append(float(t.item()))
    return g.download(Y, F.LH_VAR_VARTHETA_L), each, float(el.item()), g.status()


def check_hold_is_its_defining_sequence(lay, hold, cap=0.0, courant=COURANT, zero_ti_plane=False, nchunks=NCHUNKS):
    """-> (dts, bounds, status) of the defining sequence, after the comparisons"""
    with layered_gpu(lay) as g:
        F = g.F
        Yr, Ya = fresh_state(g, zero_ti_plane)
        dt_max = cap * bound_device(g, Yr, Ya, courant)
        dts, elapsed, bounds, status = defining_sequence(g, Yr, Ya, courant, dt_max, nchunks, hold)
        want = g.download(Yr, F.LH_VAR_VARTHETA_L)
        for tuning in (FUSED, STEPPER):      # the calls have one engine: the key changes nothing
            F.check(g.L.lh_set_tuning(g.ctx, tuning), g.ctx)
            Y1, _ = fresh_state(g, zero_ti_plane)
            got1, last, el1, st1 = hold_call(g, Y1, Ya, courant, dt_max, nchunks, hold)
            assert np.array_equal(got1, want), "one call"
            assert (last, el1, st1) == ([dts[-1]], elapsed, status)
        Y2, _ = fresh_state(g, zero_ti_plane)
        got2, each, el2, st2 = hold_call(g, Y2, Ya, courant, dt_max, 1, hold, calls=nchunks)
        assert np.array_equal(got2, want), "chunk by chunk"
        assert (each, el2, st2) == (dts, elapsed, status)
    assert all(d > 0 for d in dts) and not status & 4
    if cap:
        assert all(d == float(np.dtype(lay.case.dtype).type(dt_max)) for d in dts), "the cap bites in every chunk"
    assert np.any(want != lay.case.vl), "the state did not move"
    return dts, bounds, status


# ------------------------------------------------------------ 1. the hold call is its defining sequence

# (ncols, nlev, nclasses): every nlev of {1, 2, 3, 64, 65, 97, 128} -- one and two cells per lane, a ragged top lane, a
# column of at most CW cells owning both faces -- and every ncols of {1, 67, 130} (spare slots of the last workgroup)
SHAPES = [(1, 1, 1), (67, 2, 3), (130, 3, 16), (1, 64, 16), (67, 65, 16), (130, 97, 3), (67, 128, 16), (130, 128, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d_%dcls" % s for s in SHAPES])
def test_hold_call_over_shapes(shape, hold, dtype):
    """(Dirichlet faces: the bound then covers the boundary terms too, so columns of one to three cells stay finite)"""
    ncols, nlev, ncls = shape
    lay = R.make_layered(dtype, ncols, nlev, R.horizon_map(ncols, nlev, ncls), classes=R.texture_classes()[:ncls], bc="dirichlet")
    check_hold_is_its_defining_sequence(lay, hold)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
@pytest.mark.parametrize("nlev", [64, 127])
def test_hold_call_with_every_face_a_class_interface(nlev, hold, dtype):
    """class(c, i) = (i + c) mod 16: every face joins two classes whose Ksat differ by a factor >= 100 and whose n
    differ -- the slopes of a face's two cells are scaled by different 1 / (n m)"""
    ncols = 7
    m = A.alternating_map(ncols, nlev)
    cls = R.texture_classes()
    K, n = cls[:, 3][m], cls[:, 0][m]
    assert np.all(np.maximum(K[:, 1:] / K[:, :-1], K[:, :-1] / K[:, 1:]) >= 100) and np.all(n[:, 1:] != n[:, :-1])
    check_hold_is_its_defining_sequence(R.make_layered(dtype, ncols, nlev, m), hold)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
def test_hold_call_over_boundary_kinds(bc, hold, dtype):
    check_hold_is_its_defining_sequence(R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc=bc), hold)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
@pytest.mark.parametrize("factors,ice", [(False, True), (True, False), (True, True)], ids=["ice", "factors", "factors_ice"])
def test_hold_call_with_factors_and_ice(factors, ice, hold, dtype):
    lay = R.make_layered(dtype, 67, 128, R.horizon_map(67, 128), bc="dirichlet", factors=factors, ice=ice)
    check_hold_is_its_defining_sequence(lay, hold)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
def test_hold_call_with_an_uploaded_zero_theta_i_plane(hold, dtype):
    """the kernel that reads theta_i, given an ice-free state: the same dt sequence as the one that knows the plane is zero"""
    lay = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet")
    known, _, st0 = check_hold_is_its_defining_sequence(lay, hold)
    plane, _, st1 = check_hold_is_its_defining_sequence(lay, hold, zero_ti_plane=True)
    assert plane == known and st0 == st1 == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hold", [1, 3, 16])
def test_hold_call_with_a_cap_that_bites_in_every_chunk(hold, dtype):
    """dt_max = 0.25 of the first bound (below every chunk's bound: tests/test_layered_adaptive_cpu.py)"""
    dts, bounds, status = check_hold_is_its_defining_sequence(A.capped_case(dtype), hold, cap=A.CAP_FRACTION)
    assert all(d < b for d, b in zip(dts, bounds)) and status == 0


# ------------------------------------------------------------ 2. the bound itself

BOUND_CASES = {"%dx%d_%dcls" % s: (lambda dtype, s=s: R.make_layered(dtype, s[0], s[1], R.horizon_map(s[0], s[1], s[2]),
                                                                    classes=R.texture_classes()[:s[2]], bc="dirichlet"))
               for s in SHAPES}
BOUND_CASES.update({
    "flux_drain": lambda dtype: R.make_layered(dtype, 67, 64, R.horizon_map(67, 64)),
    "alternating_127": lambda dtype: R.make_layered(dtype, 7, 127, A.alternating_map(7, 127)),
    "factors_ice": lambda dtype: R.make_layered(dtype, 67, 128, R.horizon_map(67, 128), bc="dirichlet", factors=True, ice=True),
    "dirichlet_consistent": lambda dtype: R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet_consistent"),
    "dirichlet_face_binds": A.dirichlet_binding_case,
})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_the_bound_is_the_stable_dt_rule_and_leaves_Y_untouched(name, dtype):
    lay = BOUND_CASES[name](dtype)
    if name == "dirichlet_face_binds":
        assert A.dirichlet_face_binds(lay)      # (the NumPy rule, on the CPU: the half-cell term is the binding one)
    with layered_gpu(lay) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        before = g.download(Y, F.LH_VAR_VARTHETA_L), g.download(Y, F.LH_VAR_THETA_I)
        got = bound_device(g, Y, Ya, COURANT)
        after = g.download(Y, F.LH_VAR_VARTHETA_L), g.download(Y, F.LH_VAR_THETA_I)
        host = host_stable_dt(g, Y, Ya, COURANT)
        twice = bound_device(g, Y, Ya, 2 * COURANT)
        assert g.status() == 0
    want = R.stable_dt(lay, COURANT)
    rtol = BOUND_RTOL[np.dtype(dtype)]
    print("%s %s: bound %.9g, lh_stable_dt %.9g (%.2g), NumPy %.9g (%.2g)" % (name, np.dtype(dtype).name, got, host, abs(got - host) / host,
                                                                            want, abs(got - want) / want))
    assert np.isfinite(got) and got > 0
    assert abs(got - host) <= rtol * host and abs(got - want) <= rtol * want
    assert abs(twice - 2 * got) <= 4 * np.finfo(dtype).eps * twice       # linear in the Courant factor
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[0], lay.case.vl)


def _column(lay, k):
    case = lay.case
    one = dataclasses.replace(case, ncols=1, vl=case.vl[k:k + 1], ti=case.ti[k:k + 1],
                              T_aux=None if case.T_aux is None else case.T_aux[k:k + 1])
    return R.Layered(one, lay.classes, np.ascontiguousarray(lay.class_map[k:k + 1]))


def _columns(lay, lo, hi):
    case = lay.case
    part = dataclasses.replace(case, ncols=hi - lo, vl=np.ascontiguousarray(case.vl[lo:hi]), ti=np.ascontiguousarray(case.ti[lo:hi]),
                               T_aux=None if case.T_aux is None else np.ascontiguousarray(case.T_aux[lo:hi]))
    return R.Layered(part, lay.classes, np.ascontiguousarray(lay.class_map[lo:hi]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_bound_does_not_depend_on_placement(dtype):
    """130 x 97: the bound of the ensemble is, bitwise, the minimum of the 130 bounds a one-column context gives for
    the same column (one context, reloaded with each column's map and state)"""
    lay = R.make_layered(dtype, 130, 97, R.horizon_map(130, 97), bc="dirichlet", ice=True)
    with layered_gpu(lay) as g:
        whole = bound_device(g, *g.prognostic_and_aux())
    singles = []
    with layered_gpu(_column(lay, 0)) as g:
        F = g.F
        Y, Ya = g.prognostic_and_aux()
        w = _word(dtype)
        for k in range(130):
            g.set_soil_class_map(lay.class_map[k:k + 1])
            F.check(g.L.lh_upload(g.ctx, Y, F.LH_VAR_VARTHETA_L, np.ascontiguousarray(lay.case.vl[k]).ctypes.data, 1, 97), g.ctx)
            F.check(g.L.lh_upload(g.ctx, Y, F.LH_VAR_THETA_I, np.ascontiguousarray(lay.case.ti[k]).ctypes.data, 1, 97), g.ctx)
            singles.append(bound_device(g, Y, Ya, word=w))
    assert len(set(singles)) > 10 and min(singles) == whole and whole > 0


# ------------------------------------------------------------ 3. the step from device memory

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tuning", [FUSED, STEPPER], ids=["persist0", "persist2"])
@pytest.mark.parametrize("nsteps", [1, 5])
@pytest.mark.parametrize("per_stage", [False, True], ids=["constant", "bcv"])
def test_device_dt_is_the_step_by_value(per_stage, nsteps, tuning, dtype):
    """lh_step_layered_ssprk33_device_dt against lh_step_ssprk33 with the same step by value, under either engine"""
    lay = R.make_layered(dtype, 67, 97, R.horizon_map(67, 97), bc="dirichlet")
    bcv = None
    if per_stage:
        Hy, top, bot = M.COMP_HYDROLOGY, M.FACE_TOP, M.FACE_BOTTOM
        bcv = np.zeros((nsteps, 3, 2, 2))
        bcv[:, :, bot, Hy] = lay.case.om.bc[(bot, Hy)][1]
        bcv[:, :, top, Hy] = lay.case.om.bc[(top, Hy)][1] + 0.002 * np.arange(3 * nsteps, dtype=np.float64).reshape(nsteps, 3)
    with layered_gpu(lay) as g:
        F, L, ctx = g.F, g.L, g.ctx
        F.check(L.lh_set_tuning(ctx, tuning), ctx)
        Y, Ya = g.prognostic_and_aux()
        dt = float(np.dtype(dtype).type(0.5 * bound_device(g, Y, Ya, 0.5)))
        b = None if bcv is None else np.ascontiguousarray(bcv).ctypes.data_as(DP)
        F.check(L.lh_step_ssprk33(ctx, Y, Ya, 0.0, dt, nsteps, b), ctx)
        want, st_want = g.download(Y, F.LH_VAR_VARTHETA_L), g.status()
        Y2, _ = g.prognostic_and_aux()
        w = _word(dtype, dt)
        F.check(L.lh_step_layered_ssprk33_device_dt(ctx, Y2, Ya, 0.0, w.data_ptr(), nsteps, b), ctx)
        got, st_got = g.download(Y2, F.LH_VAR_VARTHETA_L), g.status()
        assert float(w.item()) == dt                    # the word is read, not written
        if per_stage:                                   # ... and the values are read: constant ones end elsewhere
            Y3, _ = g.prognostic_and_aux()
            F.check(L.lh_step_layered_ssprk33_device_dt(ctx, Y3, Ya, 0.0, w.data_ptr(), nsteps, None), ctx)
            assert np.any(g.download(Y3, F.LH_VAR_VARTHETA_L) != got)
    assert np.array_equal(got, want) and st_got == st_want == 0
    assert np.any(got != lay.case.vl) and dt > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_contexts_over_column_blocks_step_like_one(dtype):
    """130 columns split 48 / 82 (37 / 63 %): the bound on each context, the minimum of the two words on the host,
    lh_step_layered_ssprk33_device_dt on both -- the concatenation is bitwise the single-context run"""
    import torch
    whole = R.make_layered(dtype, 130, 64, R.horizon_map(130, 64), bc="flux_drain")
    rounds, nsteps = 3, 4

    def run(lays):
        gs = [layered_gpu(lay) for lay in lays]
        try:
            st = [g.prognostic_and_aux() + (_word(dtype),) for g in gs]
            dts = []
            for _ in range(rounds):
                for g, (Y, Ya, t) in zip(gs, st):
                    g.F.check(g.L.lh_layered_step_bound_device(g.ctx, Y, Ya, COURANT, t.data_ptr()), g.ctx)
                for g in gs:
                    g.F.check(g.L.lh_synchronize(g.ctx), g.ctx)
                gmin = torch.min(torch.cat([t for *_, t in st]))        # the collective, on the host
                for *_, t in st:
                    t.copy_(gmin)
                torch.cuda.synchronize()
                dts.append(float(gmin.item()))
                for g, (Y, Ya, t) in zip(gs, st):
                    g.F.check(g.L.lh_step_layered_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, t.data_ptr(), nsteps, None), g.ctx)
            outs = [g.download(Y, g.F.LH_VAR_VARTHETA_L) for g, (Y, *_r) in zip(gs, st)]
            assert all(g.status() == 0 for g in gs)
            return outs, dts
        finally:
            for g in gs:
                g.close()

    (ref,), dts_ref = run([whole])
    outs, dts = run([_columns(whole, 0, 48), _columns(whole, 48, 130)])
    assert dts == dts_ref and all(d > 0 for d in dts) and len(set(dts)) > 1
    assert np.array_equal(np.concatenate(outs, axis=0), ref) and np.any(ref != whole.case.vl)


def test_one_rank_communicator_changes_nothing():
    lay = R.make_layered(np.float64, 67, 64, R.horizon_map(67, 64))
    out = []
    for attach in (False, True):
        with layered_gpu(lay) as g:
            F, L, ctx = g.F, g.L, g.ctx
            if attach:
                ident = (C.c_ubyte * F.LH_COMM_ID_BYTES)()
                F.check(L.lh_comm_unique_id(ident), None)
                F.check(L.lh_comm_init(ctx, 0, 1, ident), ctx)
            Y, Ya = g.prognostic_and_aux()
            b = bound_device(g, Y, Ya)
            out.append((b,) + hold_call(g, Y, Ya, COURANT, 0.0, 3, 5))
            if attach:
                F.check(L.lh_comm_destroy(ctx), ctx)
    assert out[0][0] == out[1][0] > 0 and out[0][2:] == out[1][2:] and out[0][2][0] > 0
    assert np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------ 4. the overrun flag (status bit 5)

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(A.FLAG_CASES))
def test_overrun_flag_is_what_the_defining_sequence_says(name, dtype):
    """Bit 5: some chunk ends on a state whose bound is below the step it was taken with.  In the NumPy reference alone
    the ratio bound / step stays 1 % away from 1 at every chunk end of both cases (tests/test_layered_adaptive_cpu.py),
    so the Float32 rounding of the bound cannot flip the flag."""
    lay, hold, courant, cap, expect = A.flag_case(name, dtype)
    with layered_gpu(lay) as g:
        F = g.F
        Yr, Ya = g.prognostic_and_aux()
        dt_max = cap * bound_device(g, Yr, Ya, courant)
        dts, elapsed, bounds, status = defining_sequence(g, Yr, Ya, courant, dt_max, NCHUNKS, hold)
        want = g.download(Yr, F.LH_VAR_VARTHETA_L)
        print(name, np.dtype(dtype).name, "dt", dts, "bounds", bounds, "ratios", [b / d for b, d in zip(bounds[1:], dts)])
        Y, _ = g.prognostic_and_aux()
        got, last, el, flags = hold_call(g, Y, Ya, courant, dt_max, NCHUNKS, hold)
    assert bool(status & 32) == expect, "the defining sequence itself"
    assert flags == status and bool(flags & 32) == expect and not flags & 4
    assert np.array_equal(got, want) and (last, el) == ([dts[-1]], elapsed)
    assert all(abs(b / d - 1.0) >= A.MARGIN for b, d in zip(bounds[1:], dts))


# ------------------------------------------------------------ 5. a clay-like table, a bone-dry column

@pytest.mark.parametrize("hold", [1, 3])
def test_a_bone_dry_clay_column_does_not_poison_the_bound(hold):
    lay = A.dry_clay_case()
    with layered_gpu(lay) as g:
        F = g.F
        assert g.L.lh_closure_form(g.ctx) == F.LH_CLOSURE_LDEXP
        Y, Ya = g.prognostic_and_aux()
        got = bound_device(g, Y, Ya)
        host = host_stable_dt(g, Y, Ya)
        # ... the dry column alone: its conductivity is 0 wherever its slope is saturated, no diffusivity, no bound
    with layered_gpu(_column(lay, A.DRY_COLUMN)) as g:
        alone = bound_device(g, *g.prognostic_and_aux())
    assert np.isfinite(got) and got > 0 and abs(got - host) <= 1e-6 * host
    assert alone == np.inf or (np.isfinite(alone) and alone > got)
    dts, bounds, status = check_hold_is_its_defining_sequence(lay, hold)
    assert not status & 4 and all(np.isfinite(b) and b > 0 for b in bounds)


# ------------------------------------------------------------ 6. a poisoned column

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_poisoned_column_is_flagged_and_left_out_of_the_bound(dtype):
    """column 40 is NaN: the others take the steps they take without it (a 66-column context), bit 0 is set"""
    sound = R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="dirichlet")
    bad = 40
    vl = np.array(sound.case.vl)
    vl[bad, :] = np.nan
    lay = A.at_state(sound, vl)
    others = np.arange(67) != bad
    rest = R.Layered(dataclasses.replace(sound.case, ncols=66, vl=np.ascontiguousarray(sound.case.vl[others]),
                                         ti=np.ascontiguousarray(sound.case.ti[others])),
                     sound.classes, np.ascontiguousarray(sound.class_map[others]))
    res = []
    for case in (lay, rest):
        with layered_gpu(case) as g:
            Y, Ya = g.prognostic_and_aux()
            b = bound_device(g, Y, Ya)
            assert g.status() == 0         # (a zero-step launch has no time loop: nothing to flag yet)
            res.append((b,) + hold_call(g, Y, Ya, COURANT, 0.0, 2, 3))
    (b_bad, v_bad, dt_bad, el_bad, st_bad), (b_rest, v_rest, dt_rest, el_rest, st_rest) = res
    assert b_bad == b_rest and np.isfinite(b_bad) and b_bad > 0
    assert st_bad & 1 and not st_bad & 4 and st_rest == 0
    assert (dt_bad, el_bad) == (dt_rest, el_rest) and dt_bad[0] > 0
    assert np.array_equal(v_bad[others], v_rest) and np.all(np.isfinite(v_rest)) and np.any(v_rest != rest.case.vl)
    assert not np.any(np.isfinite(v_bad[bad]))


# ------------------------------------------------------------ 7. error paths

def _refused(g, rc, code, *words):
    assert rc == code, (rc, g.L.lh_last_error(g.ctx))
    msg = g.L.lh_last_error(g.ctx).decode()
    for w in words:
        assert w in msg, msg


def test_refusals():
    F = pc._pkg()._ffi
    L = F.lib()
    B, D, A_ = "lh_layered_step_bound_device", "lh_step_layered_ssprk33_device_dt", "lh_step_layered_ssprk33_adaptive_hold"
    w = _word(np.float64, 1.0)
    p = w.data_ptr()

    def all_three(g, Y, Ya, code, *words, scalar=(None, None, None)):
        for name, call, sc in ((B, lambda: L.lh_layered_step_bound_device(g.ctx, Y, Ya, 0.3, p), scalar[0]),
                               (D, lambda: L.lh_step_layered_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, p, 1, None), scalar[1]),
                               (A_, lambda: L.lh_step_layered_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 4, p, p), scalar[2])):
            _refused(g, call(), code, name, *(words + ((sc,) if sc else ())))

    # NULL context
    assert L.lh_layered_step_bound_device(None, None, None, 0.3, p) == F.LH_EINVAL
    assert L.lh_step_layered_ssprk33_device_dt(None, None, None, 0.0, p, 1, None) == F.LH_EINVAL
    assert L.lh_step_layered_ssprk33_adaptive_hold(None, None, None, 0.0, 0.3, 0.0, 1, 4, p, p) == F.LH_EINVAL
    lay = R.make_layered(np.float64, 67, 8, R.horizon_map(67, 8, 3), classes=R.texture_classes()[:3])
    with layered_gpu(lay) as g:
        Y, Ya = g.prognostic_and_aux()
        # arguments
        _refused(g, L.lh_layered_step_bound_device(g.ctx, Y, Ya, 0.3, None), F.LH_EINVAL, B, "NULL")
        _refused(g, L.lh_layered_step_bound_device(g.ctx, Y, Ya, 0.0, p), F.LH_EINVAL, B, "courant")
        _refused(g, L.lh_layered_step_bound_device(g.ctx, Y, Ya, float("nan"), p), F.LH_EINVAL, B, "courant")
        _refused(g, L.lh_step_layered_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, None, 1, None), F.LH_EINVAL, D, "NULL")
        _refused(g, L.lh_step_layered_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, p, -1, None), F.LH_EINVAL, D, "nsteps")
        _refused(g, L.lh_step_layered_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 4, None, p), F.LH_EINVAL, A_, "NULL")
        for nchunks, hold, courant in ((-1, 4, 0.3), (1, 0, 0.3), (1, (1 << 20) + 1, 0.3), (1, 4, 0.0), (1, 4, -0.3)):
            _refused(g, L.lh_step_layered_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, courant, 0.0, nchunks, hold, p, p), F.LH_EINVAL,
                     A_, "nchunks", "hold", "courant")
        # nothing to do is legal and does nothing
        F.check(L.lh_step_layered_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 0, 4, p, p), g.ctx)
        F.check(L.lh_step_layered_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, p, 0, None), g.ctx)
        assert np.array_equal(g.download(Y, F.LH_VAR_VARTHETA_L), lay.case.vl) and float(w.item()) == 1.0
        # what every layered call refuses: per-column arrays, LH_MATH_LIBM
        arr = np.full(67, 0.45)
        F.check(L.lh_set_percol_param(g.ctx, F.LH_PC["nu"], arr.ctypes.data_as(DP)), g.ctx)
        all_three(g, Y, Ya, F.LH_EMODEL, "soil classes", "per-column")
        F.check(L.lh_set_percol_param(g.ctx, F.LH_PC["nu"], None), g.ctx)
        F.check(L.lh_set_math_mode(g.ctx, F.LH_MATH_LIBM), g.ctx)
        all_three(g, Y, Ya, F.LH_EMODEL, "soil classes", "LH_MATH_LIBM")
        F.check(L.lh_set_math_mode(g.ctx, F.LH_MATH_FAST), g.ctx)
        # a prescribed atmosphere cannot be set on a Richards context at all: the calls' own refusal of it is a guard
        atm = M.AtmosForcing()
        s = lay.case.om.soil
        f = F.lh_atmos_forcing(atm.u_atm, atm.theta_atm, atm.z_atm, atm.theta_scale, atm.rho_a_sfc, atm.q_atm, s.z_0m, s.z_0s, atm.R_v,
                               atm.R_d, atm.grav, atm.cp_d, atm.cp_v, atm.LH_v0, atm.T_triple, atm.press_triple, atm.von_karman)
        assert L.lh_set_atmos_forcing(g.ctx, C.byref(f), None) == F.LH_EMODEL
        # the scalar calls keep refusing a context with a map, and each names the layered call that takes its place
        t = _word(np.float64)
        dY = g.state(0)
        _refused(g, L.lh_step_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 4, t.data_ptr(), None), F.LH_EMODEL,
                 "lh_step_ssprk33_adaptive_hold", "soil classes", A_)
        _refused(g, L.lh_step_ssprk33_adaptive(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 1, t.data_ptr(), None), F.LH_EMODEL,
                 "lh_step_ssprk33_adaptive", "soil classes", A_)
        _refused(g, L.lh_step_ssprk33_device_dt(g.ctx, Y, Ya, 0.0, t.data_ptr(), None), F.LH_EMODEL, "lh_step_ssprk33_device_dt",
                 "soil classes", D)
        _refused(g, L.lh_rhs_stable_dt(g.ctx, 0.0, Y, Ya, dY, 0.3, t.data_ptr()), F.LH_EMODEL, "lh_rhs_stable_dt", "soil classes", B)
        # the map removed: the context is a scalar one again
        g.set_soil_class_map(None)
        all_three(g, Y, Ya, F.LH_EMODEL, "no class map", scalar=("lh_rhs_stable_dt", "lh_step_ssprk33_device_dt", "lh_step_ssprk33_adaptive_hold"))
        F.check(L.lh_step_ssprk33_adaptive_hold(g.ctx, Y, Ya, 0.0, 0.3, 0.0, 1, 4, t.data_ptr(), None), g.ctx)
    # a context that never had a map
    with pc.GpuModel(lay.case) as g:
        Y, Ya = g.prognostic_and_aux()
        all_three(g, Y, Ya, F.LH_EMODEL, "no class map", scalar=("lh_rhs_stable_dt", "lh_step_ssprk33_device_dt", "lh_step_ssprk33_adaptive_hold"))
    # more than 128 levels
    tall = R.make_layered(np.float64, 5, 130, R.horizon_map(5, 130))
    with layered_gpu(tall) as g:
        Y, Ya = g.prognostic_and_aux()
        all_three(g, Y, Ya, F.LH_EMODEL, "more than 128 levels")
    # any model but Richards: with a map (a layered coupled context) and without
    layh = H.make_layered_heat(np.float64, 5, 64, R.horizon_map(5, 64), model=M.MODEL_COUPLED)
    g = pc.GpuModel(layh.case)
    with g:
        Y, Ya = g.prognostic_and_aux()
        all_three(g, Y, Ya, F.LH_EMODEL, "Richards models only")
        g.set_soil_classes(layh.classes, layh.class_map, thermal=layh.thermal)
        all_three(g, Y, Ya, F.LH_EMODEL, "soil classes", "Richards models only")


# ------------------------------------------------------------ 8. the host mirror

def test_python_step_adaptive_on_a_layered_model():
    """step_adaptive(layered_model, hold=4, nsteps=3) is the C call with nchunks = 3; hold=1 works; without `hold` the
    call is lh_step_ssprk33_adaptive, which has no layered form"""
    import torch
    lh = pc._pkg()
    F, L = lh._ffi, lh._ffi.lib()
    FT = np.float64
    n, N = 48, 70
    classes = R.texture_classes()[[0, 5, 2]]
    horizons = np.zeros(n, dtype=np.int64)
    horizons[15:] = 1
    horizons[33:] = 2
    lay = R.make_layered(FT, N, n, np.repeat(horizons[None, :], N, axis=0), classes=classes, bc="flux_drain")
    om = lay.case.om
    sc = lh.SoilClasses([lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3]), ν=k[4], S_s=k[5])
                         for k in classes], horizons)

    def fresh():
        dom = lh.Column(FT, zlim=(om.zmin, om.zmax), nelements=n, ncolumns=N)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(hydrology=lh.VerticalFlux(-2e-8)),
                             bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage()))
        model = lh.SoilModel(FT, domain=dom, energy_model=lh.PrescribedTemperatureModel(),
                             hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT)),
                             boundary_conditions=bc, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet(),
                             soil_classes=sc)
        Y, Ya = lh.initialize_states(model, lambda z, m: {"ϑ_l": 0.3 + 0.0 * z, "θ_i": 0.0 * z}, 0.0)
        Y.soil.ϑ_l = lay.case.vl
        return model, Y, Ya

    model, Y, Ya = fresh()
    elapsed, dt = lh.step_adaptive(model, Y, Ya, t=0.0, courant=0.3, nsteps=3, hold=4)
    mirror = np.array(Y.soil.ϑ_l)
    with pytest.raises(NotImplementedError, match="soil classes"):
        lh.step_adaptive(model, Y, Ya)
    model.close()
    model, Y, Ya = fresh()
    be = model._backend()
    be.set_bcs(model, 0.0)
    buf = torch.zeros(2, device=torch.device("cuda", be.device_index()), dtype=torch.float64)
    torch.cuda.synchronize()
    ya = Ya.handle if hasattr(Ya, "handle") else None
    F.check(L.lh_step_layered_ssprk33_adaptive_hold(be.ctx, Y.handle, ya, 0.0, 0.3, 0.0, 3, 4, C.c_void_p(buf.data_ptr()),
                                                    C.c_void_p(buf.data_ptr() + 8)), be.ctx)
    F.check(L.lh_synchronize(be.ctx), be.ctx)
    assert (elapsed, dt) == (float(buf[1].item()), float(buf[0].item())) and dt > 0 and elapsed > 0
    assert np.array_equal(mirror, np.array(Y.soil.ϑ_l)) and np.any(mirror != lay.case.vl)
    model.close()
    model, Y, Ya = fresh()
    elapsed1, dt1 = lh.step_adaptive(model, Y, Ya, t=0.0, courant=0.3, nsteps=5, hold=1)
    assert dt1 > 0 and elapsed1 > dt1 and np.any(np.array(Y.soil.ϑ_l) != lay.case.vl)
    model.close()
