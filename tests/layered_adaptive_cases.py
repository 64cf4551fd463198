"""The cases of tests/test_gpu_layered_adaptive.py whose expectations rest on conditions that the NumPy reference
alone must satisfy (layered_ref: `stable_dt`, `ssprk33`), and the NumPy run of the defining sequence of
lh_step_layered_ssprk33_adaptive_hold.  tests/test_layered_adaptive_cpu.py asserts those conditions without a GPU.

Test infrastructure: imports neither the oracle nor the HIP library.
"""
import dataclasses

import numpy as np

import case_model as M
import layered_ref as R

COURANT = 0.3
NCHUNKS = 3
MARGIN = 0.01             # the ratio bound / step stays this far from 1 at every chunk end of a flag case
CAP_FRACTION = 0.25       # dt_max of the capped case, as a fraction of the first bound


def at_state(lay, vl):
    """the same layered case at another vartheta_l"""
    return R.Layered(dataclasses.replace(lay.case, vl=np.ascontiguousarray(vl, dtype=lay.case.dtype)), lay.classes, lay.class_map)


def alternating_map(ncols, nlev, ncls=16):
    """class(c, i) = (i + c) mod ncls: every face of every column joins two classes"""
    return ((np.arange(nlev)[None, :] + np.arange(ncols)[:, None]) % ncls).astype(np.uint8)


def bound_terms(lay):
    """The three kinds of terms of layered_ref.stable_dt, each as twice the diffusivity D it bounds, [ncols] maxima:
    (the boundary cells' own 2 K s, the Dirichlet half-cell terms 4 max(K_f, K) s, the interior faces'
    (K_lo + K_hi) max(s_lo, s_hi)).  min courant dz^2 / D over all of them is stable_dt."""
    case, om = lay.case, lay.case.om
    FT = np.dtype(case.dtype).type
    vl, ti = np.asarray(case.vl, FT), np.asarray(case.ti, FT)
    n = om.nlev
    T = np.full_like(vl, FT(288)) if case.T_aux is None else np.asarray(case.T_aux, dtype=FT)
    p = R.cell_params(lay)
    with np.errstate(all="ignore"):
        K, psi = R.water_closures(om.cf, p, vl, ti, T)
        m = FT(1) - FT(1) / p["n"]
        nu_eff = p["nu"] - ti
        Se = R.P.effective_saturation(nu_eff, vl, p["theta_r"])
        u = Se ** (-FT(1) / m) - FT(1)
        slope = np.abs(psi) * (u + FT(1)) / (p["n"] * m * u * Se * (nu_eff - p["theta_r"]))
        s = np.where((Se <= 1) & (u > 0), slope, FT(1) / p["S_s"]).astype(np.float64)
        K = K.astype(np.float64)
        cell = np.zeros(vl.shape[0])
        face = np.zeros(vl.shape[0])
        for f, i in ((M.FACE_BOTTOM, 0), (M.FACE_TOP, n - 1)):
            cell = np.maximum(cell, 2.0 * K[:, i] * s[:, i])
            kind, val = R._bc(om, f, vl.shape[0], FT)
            if kind == M.BC_DIRICHLET:
                K_f, _ = R.water_closures(om.cf, {k: v[:, i] for k, v in p.items()}, val, ti[:, i], T[:, i])
                face = np.maximum(face, 4.0 * np.maximum(K_f.astype(np.float64), K[:, i]) * s[:, i])
        inner = np.zeros(vl.shape[0])
        if n > 1:
            inner = np.max((K[:, :-1] + K[:, 1:]) * np.maximum(s[:, :-1], s[:, 1:]), axis=1)
    return cell, face, inner


def dirichlet_face_binds(lay):
    """the half-cell term of a Dirichlet face is the largest term of the ensemble, strictly"""
    cell, face, inner = bound_terms(lay)
    return float(face.max()) > max(float(cell.max()), float(inner.max()))


def defining_sequence(lay, courant, dt_max, nchunks, hold):
    """The defining sequence in NumPy: per chunk dt = min(stable_dt(Y), dt_max) (dt_max <= 0: no cap), `hold`
    SSPRK33 steps at it.  -> (the dt of every chunk, the bound of Y before every chunk, the bound of the state every
    chunk ends on, the last state)"""
    FT = np.dtype(lay.case.dtype).type
    y = np.array(lay.case.vl, dtype=FT)
    dts, starts, ends = [], [], []
    b = R.stable_dt(lay, courant)
    for _ in range(nchunks):
        starts.append(b)
        dt = float(FT(min(b, dt_max) if dt_max > 0 else b))
        y = R.ssprk33(lay, dt, hold, vl=y)
        b = R.stable_dt(at_state(lay, y), courant)
        dts.append(dt)
        ends.append(b)
    return dts, starts, ends, y


# ---- the overrun flag (status bit 5)

SAND_OVER_LOAM = np.array([[2.8, 6.0, 0.03, 8e-5, 0.40, 1e-3],      # (n, alpha, theta_r, Ksat, nu, S_s): sand
                           [1.6, 1.5, 0.06, 4e-7, 0.45, 1e-3]])     # loam below


def wetting_front(dtype, ncols=5, nlev=24):
    """A wetting front into dry sand under a flux top: the sand (the upper two thirds, over loam) starts at
    S = 0.08 ... 0.12 and the top face infiltrates at 0.4 Ksat of the sand.  The wetted cells' diffusivity grows by
    orders of magnitude within a chunk of 16 steps, so a held step overruns the bound of the state it produces."""
    m = np.zeros((ncols, nlev), dtype=np.uint8)
    m[:, :nlev // 3] = 1
    H, top, bot = M.COMP_HYDROLOGY, M.FACE_TOP, M.FACE_BOTTOM
    lay = R.make_layered(dtype, ncols, nlev, m, classes=SAND_OVER_LOAM, bc="flux_drain", name="wetting_front")
    om = dataclasses.replace(lay.case.om, bc={(top, H): (M.BC_FLUX, -0.4 * SAND_OVER_LOAM[0, 3]), (bot, H): (M.BC_FREE_DRAINAGE, 0.0)})
    p = R.cell_params(lay)
    S = 0.08 + 0.01 * np.arange(ncols)[:, None] + np.zeros((1, nlev))
    vl = (p["theta_r"].astype(np.float64) + (p["nu"] - p["theta_r"]).astype(np.float64) * S).astype(dtype)
    return R.Layered(dataclasses.replace(lay.case, om=om, vl=vl), lay.classes, lay.class_map)


# name -> (builder(dtype), hold, courant, dt_max as a fraction of the first bound, the flag expected)
FLAG_CASES = {
    "wetting_front": (wetting_front, 16, 0.45, 0.0, True),
    "capped_horizons": (lambda dtype: R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="flux_drain"), 16, COURANT,
                        CAP_FRACTION, False),
}


def flag_case(name, dtype):
    build, hold, courant, cap, expect = FLAG_CASES[name]
    return build(dtype), hold, courant, cap, expect


# ---- the cap bites in every chunk

def capped_case(dtype):
    return R.make_layered(dtype, 67, 64, R.horizon_map(67, 64), bc="flux_drain")


# ---- Dirichlet faces whose half-cell term is the binding one

def dirichlet_binding_case(dtype, ncols=67, nlev=64):
    """Both faces Dirichlet, the top value close to saturation above a drier top cell: the face state's conductivity
    exceeds the cell's, and four times it times the cell's slope is the largest term of the ensemble."""
    lay = R.make_layered(dtype, ncols, nlev, R.horizon_map(ncols, nlev), bc="dirichlet")
    H = M.COMP_HYDROLOGY
    bc = dict(lay.case.om.bc)
    bc[(M.FACE_TOP, H)] = (M.BC_DIRICHLET, 0.34)
    return R.Layered(dataclasses.replace(lay.case, om=dataclasses.replace(lay.case.om, bc=bc)), lay.classes, lay.class_map)


# ---- a clay-like table with a bone-dry column among ordinary ones

CLAY_CLASS, DRY_COLUMN = 5, 7


def clay_table():
    """layered_ref.texture_classes with n = 1.06 in class 5 (m < 0.07: the whole table takes the v_ldexp form)"""
    classes = R.texture_classes().copy()
    classes[CLAY_CLASS, 0] = 1.06
    return classes


def dry_clay_case(dtype=np.float64, ncols=67, nlev=64):
    """... and column DRY_COLUMN all of that class at S = 1e-9: K underflows to 0 there while |psi| and its slope leave
    the Float32 range"""
    classes = clay_table()
    m = R.horizon_map(ncols, nlev).copy()
    m[DRY_COLUMN, :] = CLAY_CLASS
    lay = R.make_layered(dtype, ncols, nlev, m, classes=classes)
    vl = np.array(lay.case.vl)
    thr, nu = classes[CLAY_CLASS, 2], classes[CLAY_CLASS, 4]
    vl[DRY_COLUMN, :] = dtype(thr + (nu - thr) * 1e-9)
    return at_state(lay, vl)
