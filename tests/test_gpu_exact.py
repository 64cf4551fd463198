"""lh_diagnostics (K, psi, T, kappa), lh_rhs and lh_boundary_fluxes against the EXACT values of the fixtures under
tests/golden/exact/ (200-bit mpmath evaluations of the closed forms, tests/exact_ref.py), with no cell masked.

The rest of the suite compares the device with the oracle, which restates the reference op for op in the working
type: where the reference's own arithmetic loses its digits both sides are noise, and those tests widen the
tolerance or leave the cells out (tools/fuzz_closures.py: K where 1 - (1 - S^(1/m))^m < 64 eps, and every column
that holds such a cell; psi where S^(-1/m) overflows; the 1e12 cap and the 1e-300 floor of closure_tolerances).
Here the reference has its digits: bone-dry cells, the finite psi beyond the reference's overflow (up to the range
of the working type, -Inf beyond it: DESIGN.md section 2), the saturation edge, the theta_r + eps clamp, wavefronts of mixed
company, and every interval of the log2 table and every entry and rounding tie of the exp2 table of
lh_fastmath.hpp are compared cell by cell with bounds that are the project's tolerance model evaluated at the
exact values (exact_ref.bound_K, bound_psi; Cw = 2 / 4 on the fixed patterns, 4 / 16 on the fuzz states).

Configurations: the default closure form, `vgfast=0` (the v_ldexp form), LH_MATH_LIBM (the pow-for-pow debugging
policy; it HAS the reference's overflow, so the `overflow` fixtures are not its to meet) and Float32; the
zero-ice-plane launch next to the one that reads the plane, bitwise; the level-segmented launch; the layered
kernels with three classes; the Dirichlet bottom face with both settings of lh_set_bottom_sign_consistent
(`clamp_*`, `clampcs_*`); the heat-only model and its layered kernel (`heat_*`, `layered_heat_*`).  Every test prints `EXACT-USE device` lines (-s): the use of each bound and the
error in ulp next to the working-type reference's; profiles/exact_reference_use.txt keeps them.

Reads the fixture files only: no mpmath, no reference tree."""
import ctypes as C
import functools

import numpy as np
import pytest

import closure_form as CF
import exact_ref as X
import parity_cases as pc

pytestmark = pytest.mark.gpu

NAMES = X.fixture_names()
F64 = [n for n in NAMES if n.endswith("f64")]
F32 = [n for n in NAMES if n.endswith("f32")]


@functools.lru_cache(maxsize=None)
def fixture(name):
    fx = X.build_fixture(name)
    return fx, X.load_exact(fx)


@functools.lru_cache(maxsize=None)
def working_type(name):
    return X.working_type_values(fixture(name)[0])


def device_values(fx, tune=None, libm=False):
    """every quantity the fixture holds, from one context: lh_diagnostics, lh_rhs, lh_boundary_fluxes"""
    F = pc._pkg()._ffi
    with pc.GpuModel(fx.case, F.LH_MATH_LIBM if libm else None) as g:
        if tune is not None:
            F.check(g.L.lh_set_tuning(g.ctx, tune), g.ctx)
        if fx.classes is not None:
            g.set_soil_classes(fx.classes, fx.class_map, thermal=fx.thermal)
        if tune is not None and b"vgfast=0" in tune and CF.has_two_forms(g, F.LH_MATH_LIBM if libm else None):
            assert g.L.lh_closure_form(g.ctx) == CF.LDEXP
        Y, Ya = g.prognostic_and_aux()
        D = g.state(0b1111)
        F.check(g.L.lh_diagnostics(g.ctx, Y, Ya, D), g.ctx)
        out = dict(K=g.download(D, F.LH_DIAG_K), psi=g.download(D, F.LH_DIAG_PSI), kappa=g.download(D, F.LH_DIAG_KAPPA),
                   T=g.download(D, F.LH_DIAG_T))
        dY = g.state(0)
        g.rhs(Y, Ya, dY)
        t = g.tendencies(dY)
        out["dvl"], out["drhoe"] = t.get("vl"), t.get("rhoe")
        if "ti" in t:
            assert not np.any(t["ti"]), "d theta_i must be identically zero"
        for face, nm in ((pc.M.FACE_BOTTOM, "bot"), (pc.M.FACE_TOP, "top")):
            fe, fw = np.empty(fx.case.ncols), np.empty(fx.case.ncols)
            F.check(g.L.lh_boundary_fluxes(g.ctx, Y, Ya, 0.0, face, fe.ctypes.data_as(C.POINTER(C.c_double)),
                                           fw.ctypes.data_as(C.POINTER(C.c_double))), g.ctx)
            out["fe_" + nm], out["fw_" + nm] = fe, fw
        status = g.status()
    return {k: v for k, v in out.items() if v is not None}, status


def check(name, config, tune=None, libm=False):
    fx, ex = fixture(name)
    got, status = device_values(fx, tune, libm)
    if not name.startswith("overflow"):
        assert status == 0, "non-finite value flagged"
    wt = working_type(name)
    print(X.record_line("device", name, config, X.uses(got, ex),
                        "ulp med/max: device " + X.ulp_summary(got, ex, fx.case.dtype) + " | working-type reference "
                        + X.ulp_summary(wt, ex, fx.case.dtype)))
    X.assert_inside(got, ex, f"{name} [{config}]")
    return got


@pytest.mark.parametrize("name", F64)
def test_float64_default_form(name):
    check(name, "f64")


@pytest.mark.parametrize("name", F64)
def test_float64_ldexp_form(name):
    check(name, "f64 vgfast=0", tune=b"vgfast=0")


# (the layered kernels exist in the production math only: lh_diagnostics answers LH_EMODEL under LH_MATH_LIBM)
@pytest.mark.parametrize("name", [n for n in F64 if not n.startswith(("overflow", "layered"))])
def test_float64_libm(name):
    check(name, "f64 libm", libm=True)


@pytest.mark.parametrize("name", F32)
def test_float32(name):
    check(name, "f32")


ICE_FREE = ["overflow_f64", "overflow_f32", "clamp_f64", "clamp_f32", "clampcs_f64", "clampcs_f32", "sweep_log2_00_f64",
            "sweep_exp2_03_f64"]


@pytest.mark.parametrize("name", ICE_FREE)
def test_zero_ice_plane_and_ice_path_are_bitwise_equal_and_exact(name):
    fx, _ = fixture(name)
    assert not np.any(fx.case.ti)       # GpuModel.upload turns the all-zero field into a fill
    a = check(name, "zero=1", tune=b"zero=1")
    b = check(name, "zero=0", tune=b"zero=0")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")


SEGMENTED = ["fuzz_coupled_fac1_pc1_f64", "fuzz_richards_fac0_pc1_f64", "fuzz_coupled_fac1_pc1_f32", "mixed_f64", "edge_f32",
             "overflow_f64", "sweep_log2_05_f64", "layered_fuzzc_f64", "clampcs_f64", "heat_f64", "heat_f32", "layered_heat_f64"]


@pytest.mark.parametrize("name", SEGMENTED)
def test_level_segmented_launch(name):
    a = check(name, "seg=5", tune=b"seg=5,persist=0")
    b = check(name, "seg=-1", tune=b"seg=-1,persist=0")
    for k in ("dvl", "drhoe"):
        if k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
