"""Clay-like ensembles: van Genuchten n in [1.03, 1.07] (m = 1 - 1/n in [0.029, 0.065], below the
0.07 of LH_VG_FAST_MIN_M), for which the host hands the Float64 water kernels the v_ldexp form of the
table-driven 2^(.) (lh_closure_form == LH_CLOSURE_LDEXP).

The states are MOIST on purpose: S in [0.5, 1.1].  For such n the reference's own closures are rounding
noise once a cell is drier than S ~ 0.5 (1 - S^(1/m) is within a few ulp of 1: K < 1e-25 Ksat), so a
comparison of values there says nothing about an implementation.  What the reference alone must satisfy
for a case of this module to be used by a GPU test is asserted on the CPU by
tests/test_clay_cases_cpu.py; the bone-dry behaviour (K exactly 0, psi up to 1e239 and beyond) is the
subject of `dry_clay_columns`.

Test infrastructure, imported by tests/test_gpu_closure_forms.py and tests/test_clay_cases_cpu.py.
"""
import numpy as np

import case_model as M
import parity_cases as pc

VARIANTS = ("percol", "scalar", "mixed", "ice", "factors")
MODELS = (M.MODEL_RICHARDS, M.MODEL_COUPLED)
SCALAR_N = 1.06                       # the uniform n of the `scalar` variant
MIXED_CLAY_N = 1.05                   # the two clay columns of the `mixed` variant: 17 and ncols - 3


def mixed_clay_columns(ncols):
    return (17, ncols - 3)


def moist_liquid(rng, thr, nu, shape):
    """90 % of the cells with S ~ U[0.5, 1.0], 10 % with S ~ U[1.0, 1.1] (oversaturated)."""
    S = np.where(rng.random(shape) < 0.9, rng.uniform(0.5, 1.0, shape), rng.uniform(1.0, 1.1, shape))
    return thr[:, None] + (nu - thr)[:, None] * S


def clay_case(model, variant, ncols=200, nlev=16, seed=1):
    """One ensemble of `ncols` columns x `nlev` levels of 5 cm.  Top face: a per-column hydrology
    Dirichlet value at S = 0.9 (a moist face state), bottom face: free drainage; the coupled model adds
    an energy Dirichlet value at the top and a flux at the bottom (as tools/fuzz_closures.fuzz_case)."""
    assert variant in VARIANTS and model in MODELS
    rng = np.random.default_rng([seed, VARIANTS.index(variant), model, ncols, nlev])
    N, n = ncols, nlev
    sp, vg = pc.coupled_soil() if model == M.MODEL_COUPLED else (M.default_soil(), M.default_vg())
    factors = variant == "factors"
    kw = {}
    # (every draw is made for every variant, so the variants share their streams where they share a range)
    vg_n = rng.uniform(1.03, 1.07, N)
    alpha = rng.uniform(0.5, 8.0, N)
    Ksat = 10.0 ** rng.uniform(-9, -6, N)
    nu = rng.uniform(0.4, 0.6, N)
    thr = rng.uniform(0.0, 0.1, N)
    if variant == "scalar":           # uniform parameters: the PERCOL = false instantiations
        vg = M.default_vg(n=SCALAR_N, alpha=vg.alpha, Ksat=vg.Ksat, theta_r=vg.theta_r)
        nu, thr = np.full(N, sp.nu), np.full(N, vg.theta_r)
    elif variant == "mixed":          # ordinary columns but two: the decision comes from the array's range
        vg_n = rng.uniform(1.2, 3.0, N)
        for c in mixed_clay_columns(N):
            vg_n[c] = MIXED_CLAY_N
        kw["percol"] = dict(vg_n=vg_n, vg_alpha=alpha, vg_Ksat=Ksat, vg_theta_r=thr, nu=nu)
    else:
        kw["percol"] = dict(vg_n=vg_n, vg_alpha=alpha, vg_Ksat=Ksat, vg_theta_r=thr, nu=nu)
    por = (nu - thr)[:, None]
    bc = {(M.FACE_TOP, M.COMP_HYDROLOGY): (M.BC_DIRICHLET, float(thr[0] + 0.9 * (nu[0] - thr[0]))),
          (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (M.BC_FREE_DRAINAGE, 0.0)}
    if model == M.MODEL_COUPLED:
        bc.update({(M.FACE_TOP, M.COMP_ENERGY): (M.BC_DIRICHLET, 277.0),
                   (M.FACE_BOTTOM, M.COMP_ENERGY): (M.BC_FLUX, 0.02)})
    if variant != "scalar":
        kw["percol_bc"] = {(M.FACE_TOP, M.COMP_HYDROLOGY): thr + 0.9 * (nu - thr)}
    om = M.CaseModel(model, n, -0.05 * n, 0.0, soil=sp, vg=vg, bc=bc,
                     cf=M.default_cf(viscosity=factors, impedance=factors), **kw)
    vl = moist_liquid(rng, thr, nu, (N, n))
    ti = np.zeros((N, n))
    icy = rng.integers(0, 3, N) < 2                         # two thirds of the columns
    u = rng.random((N, n))
    if variant in ("ice", "factors"):                       # theta_i <= 0.15 (nu - theta_r): the NOICE = false kernels
        ti = np.where(icy[:, None], 0.15 * u * por, 0.0)
    T = rng.uniform(274.0 if not factors else 262.0, 300.0, (N, n))
    e = om.earth
    tl = np.minimum(vl, nu[:, None] - ti)
    rho_c_s = sp.rho_c_ds + tl * (e.cp_l * e.rho_liq) + ti * (e.cp_i * e.rho_ice)
    rhoe = rho_c_s * (T - e.T_0) - ti * e.rho_ice * e.LH_f0
    args = dict(vl=vl, ti=ti)
    if model == M.MODEL_COUPLED:
        args["rhoe"] = rhoe
    elif factors:
        args["T_aux"] = T
    return pc.Case(f"clay_{variant}_{'coupled' if model == M.MODEL_COUPLED else 'richards'}_{N}x{n}_s{seed}",
                   om, np.float64, N, **args)


def ill_cells(case):
    """The rule of tools/fuzz_closures.py: cells whose K is rounding noise in the reference's own formula
    (1 - (1 - S^(1/m))^m below 64 eps)."""
    eps = np.finfo(case.dtype).eps
    with np.errstate(all="ignore"):
        n = pc._percol(case, "vg_n", case.om.vg.n)[:, None]
        m = 1.0 - 1.0 / n
        nu = pc._percol(case, "nu", case.om.soil.nu)[:, None]
        thr = pc._percol(case, "vg_theta_r", case.om.vg.theta_r)[:, None]
        S = (np.maximum(case.vl.astype(np.float64), thr + eps) - thr) / (nu - thr)
        t = np.where(S < 1, S ** (1.0 / m), 1.0)
        inner = np.where(S < 1, 1.0 - (1.0 - t) ** m, 1.0)
    return inner < 64 * eps


# ---- bone-dry clay: what the v_ldexp form exists for
DRY_N = (1.03, 1.05, 1.07)
DRY_S = (1e-15, 1e-12, 1e-9, 1e-6, 1e-3, 0.1)


def dry_clay_columns(nlev=16, moist=0, seed=3):
    """One Richards column per (n, S) of DRY_N x DRY_S, the whole column at that S, default loam
    otherwise, zero-flux faces; `moist` > 0 puts them in front of that many ordinary moist columns
    (n ~ U[1.2, 3], S in [0.5, 1.1]).  -> (case, number of dry columns)"""
    rng = np.random.default_rng([seed, nlev, moist])
    sp, vg = M.default_soil(), M.default_vg()
    nn, SS = np.meshgrid(DRY_N, DRY_S, indexing="ij")
    nd = nn.size
    N = nd + moist
    vg_n = np.concatenate([nn.ravel(), rng.uniform(1.2, 3.0, moist)])
    om = M.CaseModel(M.MODEL_RICHARDS, nlev, -0.05 * nlev, 0.0, soil=sp, vg=vg, bc=pc._flux_bcs(hydrology=0.0),
                     percol=dict(vg_n=vg_n))
    nu, thr = np.full(N, sp.nu), np.full(N, vg.theta_r)
    vl = np.empty((N, nlev))
    vl[:nd] = thr[:nd, None] + (nu - thr)[:nd, None] * SS.ravel()[:, None]
    if moist:
        vl[nd:] = moist_liquid(rng, thr[nd:], nu[nd:], (moist, nlev))
    return pc.Case(f"dry_clay_{N}x{nlev}", om, np.float64, N, vl=vl, ti=np.zeros((N, nlev))), nd


def take_columns(case, cols):
    """The sub-ensemble of the columns `cols` (every per-column array taken along)."""
    import dataclasses
    cols = np.asarray(cols)
    take = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[cols])
    om = dataclasses.replace(case.om, percol={k: take(v) for k, v in case.om.percol.items()},
                             percol_bc={k: take(v) for k, v in case.om.percol_bc.items()})
    return dataclasses.replace(case, name=case.name + "_sub", om=om, ncols=len(cols), vl=take(case.vl),
                               ti=take(case.ti), rhoe=take(case.rhoe), T_aux=take(case.T_aux))


# ---- one clay-like run per implicit / layered integrator family
# (FAMILY_SEED: the NumPy references themselves -- finite-difference Jacobians, iterated to round-off -- converge in
# every column of these; with seeds 2 and 3 one column of the Richards reference cycles at the saturation kink for
# 120 iterations, with seed 1 two columns of the coupled one do: tests/test_clay_cases_cpu.py)
FAMILY_SEED = 5
FAMILY_STEP = 10.0                    # one step of this many stable steps (Courant 0.5)


def family_case(model):
    return clay_case(model, "percol", 67, 16, FAMILY_SEED)


def layered_clay_case(ncols=48, nlev=16, seed=FAMILY_SEED):
    """16 soil classes (layered_ref.texture_classes) of which classes 3 and 11 have n = 1.05, up to four horizons
    per column (layered_ref.horizon_map), every cell moist: S in [0.5, 1.1] of its own class.  -> layered_ref.Layered"""
    import dataclasses

    import layered_ref as R
    classes = R.texture_classes()
    classes[[3, 11], 0] = MIXED_CLAY_N
    lay = R.make_layered(np.float64, ncols, nlev, R.horizon_map(ncols, nlev), classes=classes, bc="flux_drain",
                         name=f"clay_layered_{ncols}x{nlev}_s{seed}")
    p = R.cell_params(lay)
    rng = np.random.default_rng([seed, ncols, nlev, 16])
    S = np.where(rng.random((ncols, nlev)) < 0.9, rng.uniform(0.5, 1.0, (ncols, nlev)), rng.uniform(1.0, 1.1, (ncols, nlev)))
    vl = p["theta_r"] + (p["nu"] - p["theta_r"]) * S
    return R.Layered(dataclasses.replace(lay.case, vl=np.ascontiguousarray(vl)), classes, lay.class_map)


# ---- the cases the GPU tests use (one list, so that the CPU guard checks exactly those)
# The seed: a cell that happens to lie within 1e-6 or so of S = 1 makes the tolerance model wide in that
# cell (psi ~ (S^(-1/m) - 1)^(1/n) next to its root), up to 10x the plain statistic's 1e-13 of the field
# scale -- 3 of 88 (case, seed) pairs over seeds 1..4; with SEED every case uses 0.3 ... 0.6 of it.
SEED = 2
RHS_CASES = [(model, variant, 200, 16, SEED) for model in MODELS for variant in VARIANTS]
STEP_CASES = [(model, variant, 67, nlev, SEED) for model in MODELS for variant in ("percol", "ice")
              for nlev in (16, 96, 130)]
STEP_COUNT, STEP_COURANT, STEP_BOUND = 20, 0.5, 1e-11
