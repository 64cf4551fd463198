"""The closed-form Newton Jacobian of tests/newton_jacobian_ref.py against the oracle, and the cases of
tests/test_gpu_newton_jacobian.py judged by the reference alone.  No GPU.

For every case (CASES below, shared with the GPU test through prepared()):
  - the bands of J = I - dt df/dv equal a central finite difference of the oracle's tendency (oracle_py.rhs for
    scalar and per-column parameters, layered_ref / layered_coupled_implicit_ref for classes) to 1e-6 of the
    column's largest band entry;
  - Newton's safeguard is inactive, with a factor 2 in hand, in EVERY cell of EVERY column, judged on the
    reference's own first update d = J^-1 dt f(Y0): the GPU test leaves nothing out;
  - q32 (the same formulas with the two slopes in np.float32) and q_1pc (either slope off by 1 %, the smaller of
    the two, the minimum over the columns) are computed, and q_1pc >= 20 q32 in every Float64 case: the pin has room;
  - the GPU test's assertion (newton_jacobian_ref.allowance with the GPU module's bound) fails on a d made with
    either slope off by 1 % (Float64, in every case) and by a factor >= 100 with either slope dropped; in Float32,
    where the round-off term dominates, the whole allowance is at most 1/10 of the dropped-slope residuals.
"""
import dataclasses
import functools

import numpy as np
import pytest

import case_model as M
import coupled_implicit_ref as CR
import layered_coupled_implicit_ref as LC
import layered_heat_ref as LH
import layered_ref as R
import newton_jacobian_ref as NJ
import parity_cases as pc

NCOLS = 67          # one full wave and a ragged one
DZ = 0.02
KINDS = [(M.BC_FLUX, M.BC_FLUX), (M.BC_DIRICHLET, M.BC_FREE_DRAINAGE), (M.BC_FREE_DRAINAGE, M.BC_DIRICHLET),
         (M.BC_DIRICHLET, M.BC_DIRICHLET), (M.BC_FLUX, M.BC_FREE_DRAINAGE)]   # tests/test_gpu_implicit.py::KINDS (top, bottom)
KIND_IDS = {M.BC_FLUX: "flux", M.BC_DIRICHLET: "dir", M.BC_FREE_DRAINAGE: "drain"}
# The bound of the GPU assertion is C q32 per case: C is measured on the device and recorded in
# tests/test_gpu_newton_jacobian.py's docstring; it lives here because the sensitivity tests below feed the same
# assertion on the CPU.
C_BOUND = 8.0


@dataclasses.dataclass(frozen=True)
class Spec:
    """One case: the entry point's family, the shape, the boundary kinds (top, bottom), the variant and the step
    in units of the case's stable step."""
    family: str          # "scalar", "layered", "coupled", "layered_coupled"
    dtype: str           # "f64" / "f32"
    nlev: int
    kinds: tuple
    variant: str         # scalar: plain / ice / percol / consistent / regimes; layered: horizons|cells + _plain|_ice
    mult: float

    @property
    def id(self):
        k = "%s-%s" % (KIND_IDS[self.kinds[0]], KIND_IDS[self.kinds[1]])
        return "%s-%s-n%d-%s-%s-x%g" % (self.family, self.dtype, self.nlev, k, self.variant, self.mult)

    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32


def _specs():
    out = []
    for kinds in KINDS:
        for v in ("plain", "ice", "percol", "consistent"):
            if v == "consistent" and kinds[1] != M.BC_DIRICHLET:
                continue   # (the bottom-sign opt-out needs a Dirichlet bottom)
            out += [Spec("scalar", "f64", 16, kinds, v, mult) for mult in (1.0, 100.0)]
    for nlev in (1, 2, 3):   # one row with both boundary slopes; no interior cell; one interior cell
        out += [Spec("scalar", "f64", nlev, k, "plain", 10.0) for k in (KINDS[3], KINDS[4])]
    out.append(Spec("scalar", "f64", 16, KINDS[4], "regimes", 1.0))
    for cmap in ("horizons", "cells"):
        for nlev in (2, 16):
            for kinds in (KINDS[4], KINDS[3]):   # layered_ref's "flux_drain" and "dirichlet"
                # the step (the issue leaves it open): 10, 30, 60 or 300 stable steps: one at which the safeguard
                # stays inactive and the slackest column is stiff enough for the pin to have room
                mult = 10.0 if cmap == "cells" else (300.0 if nlev == 2 else 60.0) if kinds == KINDS[4] else 30.0
                out += [Spec("layered", "f64", nlev, kinds, "%s_%s" % (cmap, ice), mult) for ice in ("plain", "ice")]
    for fam in ("coupled", "layered_coupled"):
        out += [Spec(fam, "f64", 16, k, "ice", 10.0) for k in (KINDS[4], KINDS[3])]
    for kinds in KINDS:
        out += [Spec("scalar", "f32", 16, kinds, v, mult) for v in ("plain", "ice") for mult in (10.0, 100.0)]
    out.append(Spec("layered", "f32", 16, KINDS[4], "horizons_ice", 60.0))
    return out


CASES = _specs()
CASES64 = [s for s in CASES if s.dtype == "f64"]
CASES32 = [s for s in CASES if s.dtype == "f32"]
IDS = lambda specs: [s.id for s in specs]


# ------------------------------------------------------------------ the cases

def _hyd_bc(kinds, top_value=0.30, bottom_value=0.15):
    top, bottom = kinds
    vals = {M.BC_FLUX: -2e-9, M.BC_FREE_DRAINAGE: 0.0}
    if bottom == M.BC_FLUX:
        bottom_value = -2e-10   # (a tenth of the top's: at 100x the stable step the bottom cell keeps most of its water)
    return {(M.FACE_TOP, M.COMP_HYDROLOGY): (top, top_value if top == M.BC_DIRICHLET else vals[top]),
            (M.FACE_BOTTOM, M.COMP_HYDROLOGY): (bottom, vals[bottom] if bottom == M.BC_FREE_DRAINAGE else bottom_value)}


def scalar_case(spec):
    """tests/test_gpu_implicit.py::richards_case at NCOLS x nlev (dz = 0.02): the wetting front, static ice in every
    other column, per-column n, alpha, Ksat, nu and Dirichlet values; "regimes" adds the saturated branch, cells next
    to saturation and a clamped cell.  Where a state or a boundary value differs from richards_case's the comment says
    why: the reference alone must find the safeguard inactive everywhere and room for the pin."""
    n, dtype = spec.nlev, spec.np_dtype
    bc = _hyd_bc(spec.kinds)
    om = M.CaseModel(M.MODEL_RICHARDS, n, -DZ * n, 0.0, bc=bc, consistent_bottom_sign=spec.variant == "consistent")
    c = np.arange(NCOLS)
    if spec.variant == "percol":
        om.percol = dict(vg_n=1.4 + 1.2 * pc.uhash(c, 2, n), vg_alpha=1.5 + 4.0 * pc.uhash(c, 3, n),
                         vg_Ksat=10.0 ** (-7.0 + 2.0 * pc.uhash(c, 4, n)), nu=0.35 + 0.15 * pc.uhash(c, 6, n))
        om.percol_bc = {k: v[1] * (1.0 + 0.05 * (pc.uhash(c, 77 + k[0], 1) - 0.5)) for k, v in bc.items()
                        if v[0] == M.BC_DIRICHLET}
    vl = pc.wetting_front(NCOLS, n, -DZ * n, 0.0, 0.35)
    ti = np.zeros((NCOLS, n))
    if spec.variant == "ice":
        ti = np.where((c % 2 == 0)[:, None], 0.04 * pc.uhash(c[:, None], np.arange(n)[None, :] + 5, 1000), 0.0)
    if spec.variant == "regimes":
        # (a coarse sand, n = 6: psi of the clamped cell is 300 m and not the loam's 1e27; S_s = 0.05 so that the
        # saturated zone's diffusivity Ksat / S_s is the unsaturated cells' and not 100 times it)
        om.vg = M.default_vg(n=6.0, theta_r=0.05)
        om.soil = M.default_soil(S_s=0.05)
        nu, thr = om.soil.nu, om.vg.theta_r
        vl = np.maximum(vl, 0.15)
        sat, near, dry = c % 3 == 0, c % 3 == 1, c % 3 == 2
        # a saturated zone at the bottom: three cells above the porosity, hydrostatic among themselves
        for i in range(3):
            vl[sat, i] = nu + om.soil.S_s * (0.05 - DZ * i)
        # cells at S = 0.97 in the middle of the column
        vl[near, 6:9] = thr + 0.97 * (nu - thr)
        # one clamped bone-dry cell (just below theta_r: K and psi are constants of it) at the top, over a dry-down of
        # two cells: next to a conducting cell that one face would be the whole column (K falls by more than psi
        # grows from each of these cells to the next)
        for i, S in zip(range(n - 3, n - 1), (0.15, 0.02)):
            vl[dry, i] = thr + S * (nu - thr)
        vl[dry, n - 1] = thr - 1e-9
    if spec.variant == "percol":
        # two decades of Ksat: the columns equalised in stiffness (see equalised), and a Dirichlet face 10 % wetter (top)
        # or drier (bottom) than its boundary cell, so that a face's K_f is the column's own and not another decade
        def build(w):
            v = (w[:, None] * vl).astype(dtype)
            o = dataclasses.replace(om, percol_bc={k: np.float64(v[:, -1]) * 1.1 if k[0] == M.FACE_TOP else np.float64(v[:, 0]) * 0.9
                                                   for k in om.percol_bc})
            case = pc.Case("newton_jacobian", o, dtype, NCOLS, vl=v, ti=ti.astype(dtype))
            return case, NJ.problem_of_case(case)
        return equalised(build, 0.2, 1.1, lambda g: np.percentile(g, 25))[0]
    return pc.Case("newton_jacobian", om, dtype, NCOLS, vl=vl.astype(dtype), ti=ti.astype(dtype))


def stiffness(pr):
    """Per column: max_i |df_i/dv_i|, the size of the Jacobian's diagonal per unit of dt."""
    return np.max(np.abs(NJ.tendency_and_slopes(pr)[2]), axis=1)


def equalised(build, lo, hi, pick=np.median):
    """build(w [ncols]) -> (object, Problem), wetter for larger w.  Returns build(w) with w in [lo, hi] such that every
    column is as stiff as the median (pick) column of build(1), as far as [lo, hi] allows: one step then means the same
    in every column.  (q32 is the worst column's figure and q_1pc the slackest column's, so an ensemble whose columns
    differ by decades in stiffness has no room between the two, whatever the kernel does.)  Bisection: stiffness grows
    with w."""
    n = NCOLS
    target = float(pick(stiffness(build(np.ones(n))[1])))
    a, b = np.full(n, lo), np.full(n, hi)
    for _ in range(60):
        w = np.sqrt(a * b)
        up = stiffness(build(w)[1]) < target
        a, b = np.where(up, w, a), np.where(up, b, w)
    return build(np.sqrt(a * b))


PSI_TOP, PSI_DROP = -0.25, 2.5   # layered_ref.make_layered's front
SE_MAX = 0.85
# The classes of the cell maps: five of the conductive ones (n 1.68 ... 3.12, alpha, theta_r, nu all different).  With
# the tight classes in the map a two-cell column of two tight classes is three decades slacker than one that holds
# class 0 (n = 1.25, whose diffusivity hardly depends on the moisture), whatever the state: no room for the pin.  The
# Ksat jumps are the horizon maps'.
CELL_CLASSES = [2, 4, 6, 8, 10]
PSI_FACE = (1.05, 0.95)            # a Dirichlet face's potential in units of its boundary cell's (bottom: drier, top: wetter)


def _layered_water(lay, w):
    """layered_ref.make_layered's wetting front in psi, divided by w per column, through every cell's own class; the
    Dirichlet faces at 1.05 (bottom) and 0.95 (top) times the boundary cell's potential, through its class (per-column values)."""
    case, om = lay.case, lay.case.om
    nlev = om.nlev
    zc, _ = pc.grid_np(om.zmin, 0.0, nlev)
    zf = om.zmin + (0.2 + 0.6 * pc.uhash(np.arange(NCOLS), 0, nlev)) * (0.0 - om.zmin)
    psi = (PSI_TOP - PSI_DROP * (1.0 - pc.sigmoid((zc[None, :] - zf[:, None]) / 0.1))) / w[:, None]
    ti = case.ti.astype(np.float64)
    # no cell wetter than Se = SE_MAX: next to saturation the Float32 slopes lose digits to 1 - Se^(1/m) (eps / w: 1e-6 at
    # Se = 0.97 in a sand), and one such cell would set q32 for the whole case
    cls = np.asarray(lay.classes, dtype=np.float64)[np.asarray(lay.class_map)]
    n_, alpha_ = cls[..., 0], cls[..., 1]
    psi = np.minimum(psi, -(SE_MAX ** (-1.0 / (1.0 - 1.0 / n_)) - 1.0) ** (1.0 / n_) / alpha_)
    case.vl = R._state_from_potential(lay.classes, lay.class_map, psi, ti, case.dtype)
    om.percol_bc = {k: v for k, v in om.percol_bc.items() if k[1] != M.COMP_HYDROLOGY}
    for (face, comp), (kind, _) in om.bc.items():
        if comp == M.COMP_HYDROLOGY and kind == M.BC_DIRICHLET:
            i = 0 if face == M.FACE_BOTTOM else nlev - 1
            v = R._state_from_potential(lay.classes, lay.class_map[:, i], PSI_FACE[face] * psi[:, i], ti[:, i], case.dtype)
            om.percol_bc[(face, comp)] = v.astype(np.float64)
    return lay


def _target(spec):
    """The column whose stiffness the others take: the median under Dirichlet faces, the 60th percentile under a
    flux over free drainage (of the two-cell horizon columns too few are stiff enough at the median)."""
    return np.median if spec.kinds == KINDS[3] else (lambda g: np.percentile(g, 60))


def layered_case(spec):
    """layered_ref.make_layered with horizon_map (all 16 classes: every interface a Ksat jump >= 150) or a class per cell
    (layered_coupled_implicit_ref.cell_map over CELL_CLASSES), the columns equalised in stiffness."""
    cmap, ice = spec.variant.split("_")
    bc = {(M.BC_FLUX, M.BC_FREE_DRAINAGE): "flux_drain", (M.BC_DIRICHLET, M.BC_DIRICHLET): "dirichlet"}[spec.kinds]
    if cmap == "horizons":
        m, classes = R.horizon_map(NCOLS, spec.nlev), None
    else:
        m, classes = LC.cell_map(NCOLS, spec.nlev), R.texture_classes()[CELL_CLASSES]

    def build(w):
        lay = _layered_water(R.make_layered(spec.np_dtype, NCOLS, spec.nlev, m, classes=classes, bc=bc, ice=ice == "ice"), w)
        return lay, NJ.problem_of_layered(lay)
    return equalised(build, 0.1, 2.5, _target(spec))[0]


def coupled_case(spec):
    return CR.coupled_case(*spec.kinds, dtype=spec.np_dtype, ncols=NCOLS, nlev=spec.nlev, ice=True)


def layered_coupled_case(spec):
    """layered_coupled_implicit_ref.layered_case (a class per cell, 5 classes, two organic) with the water state and
    the hydrology faces of layered_case above; rho e_int from the case's own temperature field at that water state."""
    energy = "flux" if spec.kinds == KINDS[4] else "dirichlet"

    def build(w):
        lay = _layered_water(LC.layered_case(spec.np_dtype, NCOLS, spec.nlev, kind="cells", hyd=spec.kinds, energy=energy, ice=True,
                                              classes=R.texture_classes()[CELL_CLASSES]), w)
        return lay, NJ.problem_of_layered(lay)
    lay = equalised(build, 0.1, 2.5, _target(spec))[0]
    case, om = lay.case, lay.case.om
    zc, _ = pc.grid_np(om.zmin, om.zmax, spec.nlev)
    Tf = LH._temperature_field(NCOLS, spec.nlev, zc, True)
    Tf = np.where(np.any(case.ti != 0, axis=1)[:, None], Tf - 12.0, Tf)   # (make_layered_heat: the columns with ice are cold)
    case.rhoe = LH.rhoe_from_T(lay.classes, lay.thermal, lay.class_map, om, case.vl, case.ti.astype(np.float64), Tf, case.dtype)
    return lay


def _richards_twin64(lay):
    """The Float64 Richards twin of a layered (coupled) case: the same classes, map, water state, ice, hydrology faces."""
    om = dataclasses.replace(lay.case.om, model=M.MODEL_RICHARDS,
                             bc={k: v for k, v in lay.case.om.bc.items() if k[1] == M.COMP_HYDROLOGY})
    om.percol_bc = {k: v for k, v in lay.case.om.percol_bc.items() if k[1] == M.COMP_HYDROLOGY}
    case = dataclasses.replace(lay.case, om=om, dtype=np.float64, rhoe=None, T_aux=None,
                               vl=np.asarray(lay.case.vl, dtype=np.float64), ti=np.asarray(lay.case.ti, dtype=np.float64))
    return R.Layered(case, lay.classes, lay.class_map)


@dataclasses.dataclass
class Prepared:
    spec: Spec
    obj: object          # the Case or the layered case the GPU test runs
    pr: NJ.Problem
    dt: float
    tendency: object     # vl [ncols, nlev] Float64 -> the oracle's water tendency (Float64)
    J: tuple             # the reference bands
    dtf: np.ndarray      # dt f(Y0) of the oracle
    d: np.ndarray        # the reference's own first Newton update
    q32: float           # worst column of q with the slopes in Float32
    q_1pc: float         # the smaller of the 1 % mutants' q, the minimum over the columns
    slopes: tuple        # the slopes the case's Jacobian contains: "dK_scale", "dn_scale"


@functools.lru_cache(maxsize=None)
def prepared(spec):
    """Everything both test modules need of one case, computed once, shared and never written."""
    if spec.family == "scalar":
        obj = scalar_case(spec)
        pr = NJ.problem_of_case(obj)
        # (regimes: the stable step of the columns without the clamped cell -- with it the oracle's bound is 1e-38 s,
        # the slope of psi at theta_r + eps, and every J would be the identity)
        keep = ~np.any(pr.vl <= pr.p["theta_r"], axis=1)
        sd = pc.O.stable_dt(obj.om, np.ascontiguousarray(pr.vl[keep]), np.ascontiguousarray(pr.ti[keep]), None, 0.5)
        tendency = lambda v: pc.O.rhs(obj.om, np.ascontiguousarray(v), np.ascontiguousarray(pr.ti))["vl"]
    elif spec.family == "coupled":
        obj = coupled_case(spec)
        pr = NJ.problem_of_case(obj)
        twin = CR.coupled_case(*spec.kinds, dtype=spec.np_dtype, ncols=NCOLS, nlev=spec.nlev, ice=True, model=M.MODEL_RICHARDS)
        sd = pc.O.stable_dt(twin.om, pr.vl, pr.ti, None, 0.5)   # the water's stable step: only vartheta_l is judged
        tendency = lambda v: CR.water_tendency(obj.om, v, pr.ti)
    else:
        obj = layered_case(spec) if spec.family == "layered" else layered_coupled_case(spec)
        pr = NJ.problem_of_layered(obj)
        twin = _richards_twin64(obj)
        sd = R.stable_dt(twin)
        tendency = lambda v: R.rhs(twin, vl=v).astype(np.float64)
    dt = spec.mult * sd
    J = NJ.bands(pr, dt)
    dtf = dt * tendency(pr.vl)
    d = NJ.tri_solve(*J, dtf)
    q32 = float(np.max(NJ.q(J, NJ.newton_update(pr, dt, dtf / dt, dtype=np.float32), dtf)))
    # A slope the Jacobian of the case does not contain is no mutant of it: at nlev = 1 Dirichlet-Dirichlet rows hold no
    # dK and a flux over free drainage no dnpsi (the bands are bitwise the same with the slope scaled).
    slopes = tuple(k for k in ("dK_scale", "dn_scale")
                   if any(not np.array_equal(x, y) for x, y in zip(J, NJ.bands(pr, dt, **{k: 1.01}))))
    q_1pc = min(float(np.min(NJ.q(J, NJ.newton_update(pr, dt, dtf / dt, **{k: 1.01}), dtf))) for k in slopes)
    for a in (pr.vl, pr.ti, dtf, d) + J:
        a.setflags(write=False)
    return Prepared(spec, obj, pr, dt, tendency, J, dtf, d, q32, q_1pc, slopes)


def bound(p):
    """B of the GPU assertion for one case."""
    return C_BOUND * p.q32


def fd_bands(p):
    """Bands of I - dt df/dv by coloured central differences of the oracle's tendency."""
    pr = p.pr
    v = pr.vl
    n = v.shape[1]
    por = pr.p["nu"] - pr.p["theta_r"]
    h = 1e-6 * np.maximum(np.abs(v - pr.p["theta_r"]), 1e-3 * por)
    a, b, c = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
    for k in range(3):
        hk = h * (np.arange(n) % 3 == k)[None, :]
        df = p.dt * (p.tendency(v + hk) - p.tendency(v - hk))
        for i in range(k, n, 3):
            hi = 2.0 * h[:, i]
            b[:, i] -= df[:, i] / hi
            if i > 0:
                c[:, i - 1] = -df[:, i - 1] / hi
            if i + 1 < n:
                a[:, i + 1] = -df[:, i + 1] / hi
    return a, b, c


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("spec", CASES, ids=IDS(CASES))
def test_bands_equal_a_central_difference_of_the_oracle(spec):
    p = prepared(spec)
    fd = fd_bands(p)
    scale = np.max(np.abs(np.stack(p.J)), axis=(0, 2))[:, None]   # the column's largest band entry
    err = max(float(np.max(np.abs(x - y) / scale)) for x, y in zip(p.J, fd))
    print("%s: bands against central differences %.3g" % (spec.id, err))
    assert err <= 1e-6, err
    # and the reference's own tendency is the oracle's (the formulas above the slopes)
    f = NJ.tendency_and_slopes(p.pr)[0]
    assert np.max(np.abs(p.dt * f - p.dtf)) <= 1e-9 * np.max(np.abs(p.dtf)) + 1e-18


@pytest.mark.parametrize("spec", CASES, ids=IDS(CASES))
def test_safeguard_inactive_in_every_cell_of_every_column(spec):
    p = prepared(spec)
    ok = NJ.safeguard_inactive(p.pr, p.d)
    dmax = NJ.DMAX_FRAC * (p.pr.p["nu"] - p.pr.p["theta_r"])
    print("%s: largest |d| / dmax %.3g" % (spec.id, float(np.max(np.abs(p.d) / dmax))))
    assert ok.shape == (NCOLS, spec.nlev) and ok.all(), np.argwhere(~ok).tolist()
    assert np.max(np.abs(p.d)) > 0


def test_the_regimes_case_holds_its_regimes():
    p = prepared(next(s for s in CASES if s.variant == "regimes"))
    pr = p.pr
    num, por = pr.vl - pr.p["theta_r"], pr.p["nu"] - pr.p["theta_r"]
    assert (num >= por).sum() >= 3 and (num <= pr.eps).sum() >= 1 and np.isclose(num / por, 0.97).sum() >= 3
    _, _, dK, dn = NJ.closures(pr.p, pr.vl, pr.ti, pr.eps)
    assert np.all(dK[num >= por] == 0) and np.all(dn[num >= por] == -1.0 / pr.p["S_s"][num >= por])
    assert np.all(dK[num <= pr.eps] == 0) and np.all(dn[num <= pr.eps] == 0)


@pytest.mark.parametrize("spec", CASES64, ids=IDS(CASES64))
def test_the_pin_has_room(spec):
    """q_1pc >= 20 q32, and the GPU module's bound B = C q32 is within the ceiling q_1pc / 10."""
    p = prepared(spec)
    print("%s: q32 %.3g, q_1pc %.3g, ratio %.3g" % (spec.id, p.q32, p.q_1pc, p.q_1pc / p.q32))
    assert len(p.slopes) == (1 if spec.nlev == 1 else 2), p.slopes
    assert p.q_1pc >= 20 * p.q32, (p.q32, p.q_1pc)
    assert bound(p) <= p.q_1pc / 10, (bound(p), p.q_1pc)


def _excess(p, **kw):
    """The GPU assertion fed a d made with a mutated Jacobian: the worst |r_i| / allowed_i."""
    d = NJ.newton_update(p.pr, p.dt, p.dtf / p.dt, **kw)
    y1 = p.pr.vl + d
    r, _ = NJ.residual_and_scale(p.J, d, p.dtf)
    return float(np.max(np.abs(r) / NJ.allowance(p.J, bound(p), d, y1, p.dtf, p.pr.eps)))


@pytest.mark.parametrize("spec", CASES64, ids=IDS(CASES64))
def test_float64_assertion_is_sensitive(spec):
    p = prepared(spec)
    same = _excess(p)
    f32 = _excess(p, dtype=np.float32)
    one = [_excess(p, **{k: 1.01}) for k in p.slopes]
    drop = [_excess(p, **{k: 0.0}) for k in p.slopes]
    print("%s: excess own %.3g, float32 slopes %.3g, 1 %% %s, dropped %s" % (spec.id, same, f32, one, drop))
    assert same <= 1 and f32 <= 1
    assert min(one) > 1, one
    assert min(drop) >= 100, drop


@pytest.mark.parametrize("spec", CASES32, ids=IDS(CASES32))
def test_float32_assertion_catches_gross_errors(spec):
    """In Float32 the round-off term dominates the allowance: the whole of it is at most 1/10 of the residual a
    dropped dK or dn term leaves."""
    p = prepared(spec)
    drop = [_excess(p, **{k: 0.0}) for k in p.slopes]
    print("%s: excess dropped %s" % (spec.id, drop))
    assert _excess(p, dtype=np.float32) <= 1
    assert min(drop) >= 10, drop
