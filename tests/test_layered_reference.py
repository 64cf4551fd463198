"""The NumPy reference of the layered-soil tendency (tests/layered_ref.py) checked on the CPU: against the
oracle where a class map can be expressed as per-column parameters, and against what a layered column must
satisfy whatever computes it (hydrostatic equilibrium across horizons, conservation)."""
import numpy as np
import pytest

import layered_ref as R
import parity_cases as pc

DTYPES = [np.float64, np.float32]
CW = {np.dtype(np.float64): 2.0, np.dtype(np.float32): 4.0}   # the fixed cases' constants (tests/test_gpu_parity.py)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("bc", ["flux_drain", "dirichlet", "dirichlet_consistent", "flux"])
@pytest.mark.parametrize("factors,ice", [(False, False), (False, True), (True, True)], ids=["plain", "ice", "factors_ice"])
def test_column_uniform_maps_equal_the_oracle_with_percolumn_parameters(dtype, bc, factors, ice):
    """700 columns, column c of class c mod 16: the reference is then the oracle's tendency with the
    matching per-column parameter arrays."""
    lay = R.make_layered(dtype, 700, 64, R.uniform_map(700, 64), bc=bc, factors=factors, ice=ice)
    case = R.with_percol(lay)
    want = pc.O.rhs(case.om, case.vl, case.ti, None, case.T_aux)
    got = dict(vl=R.rhs(lay), ti=np.zeros_like(case.vl))
    pc.assert_tendencies_close(case, got, want, Cw=CW[np.dtype(dtype)], plain=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("ncols,nlev,ncls", [(1, 1, 1), (67, 3, 3), (5, 2, 16)])
def test_small_uniform_maps_equal_the_oracle(dtype, ncols, nlev, ncls):
    lay = R.make_layered(dtype, ncols, nlev, R.uniform_map(ncols, nlev, ncls), bc="dirichlet")
    case = R.with_percol(lay)
    want = pc.O.rhs(case.om, case.vl, case.ti, None, case.T_aux)
    pc.assert_tendencies_close(case, dict(vl=R.rhs(lay), ti=np.zeros_like(case.vl)), want, Cw=CW[np.dtype(dtype)], plain=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_layered_hydrostatic_column_is_at_rest(dtype):
    """64 levels, three horizons with Ksat ratios >= 100, psi = h0 - z in every cell by its own class's
    retention curve: K jumps by orders of magnitude at the interfaces, the head does not, nothing moves.
    The scale is what the same state does one level off its horizons."""
    rest = np.abs(R.rhs(R.hydrostatic(dtype))).max()
    shifted = np.abs(R.rhs(R.hydrostatic(dtype, shift=1))).max()
    assert shifted > 0
    assert rest <= 1e-6 * shifted, (rest, shifted)
    # (the case is what it says: unsaturated throughout, three horizons)
    lay = R.hydrostatic(dtype)
    p = R.cell_params(lay)
    assert np.all(lay.case.vl < p["nu"]) and len(np.unique(lay.class_map)) == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("bc", ["flux", "flux_drain", "dirichlet"])
def test_conservation_with_flux_faces(dtype, bc):
    """sum d vartheta_l dz = F_bottom - F_top: every interior face enters two cells with opposite signs."""
    lay = R.make_layered(dtype, 130, 64, R.horizon_map(130, 64), bc=bc)
    d, f_bot, f_top = R.rhs(lay, faces=True)
    check_conservation(lay, d, f_bot, f_top)


def check_conservation(lay, d, f_bot, f_top):
    om = lay.case.om
    eps = float(np.finfo(lay.case.dtype).eps)
    dz = (om.zmax - om.zmin) / om.nlev
    d8 = np.asarray(d, dtype=np.float64)
    total = d8.sum(axis=1) * dz
    want = np.asarray(f_bot, np.float64) - np.asarray(f_top, np.float64)
    bound = om.nlev * 4 * eps * np.abs(d8).sum(axis=1) * dz
    assert np.all(np.abs(total - want) <= bound), float(np.max(np.abs(total - want) / bound))


def test_horizon_map_has_an_interface_with_a_large_conductivity_jump():
    classes = R.texture_classes()
    m = R.horizon_map(130, 64)
    assert len(np.unique(m)) == 16
    K = classes[m, 3]
    ratio = np.maximum(K[:, 1:] / K[:, :-1], K[:, :-1] / K[:, 1:]).max(axis=1)
    assert np.all(ratio >= 100)
    # horizons of unequal thickness that differ per column
    assert len({tuple(np.flatnonzero(np.diff(row.astype(int)))) for row in m}) > 100


def test_host_mirror_refuses_at_construction_what_the_library_would_refuse():
    """SoilModel(..., soil_classes=...) without a device: the model kinds, the per-column arrays and the class
    maps the library answers with LH_EMODEL / LH_EINVAL are errors when the model is built."""
    lh = pc._pkg()
    FT = np.float64
    cls = [lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=k[0], α=k[1], θr=k[2], Ksat=k[3]), ν=k[4], S_s=k[5])
           for k in R.texture_classes()[:3]]
    assert cls[1].numbers() == tuple(R.texture_classes()[1])
    horizons = np.array([0, 0, 1, 1, 2, 2])

    def build(sc, ncolumns=4, **kw):
        args = dict(domain=lh.Column(FT, zlim=(-0.6, 0.0), nelements=6, ncolumns=ncolumns),
                    energy_model=lh.PrescribedTemperatureModel(),
                    hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT)),
                    boundary_conditions=None, soil_param_set=lh.SoilParams(FT), earth_param_set=lh.EarthParameterSet(),
                    soil_classes=sc)
        args.update(kw)
        return lh.SoilModel(FT, **args)

    sc = lh.SoilClasses(cls, horizons)
    assert build(sc).soil_classes is sc
    assert build(lh.SoilClasses(cls, np.repeat(horizons[None, :], 4, axis=0))).soil_classes.class_map.shape == (4, 6)
    with pytest.raises(lh.ModelError, match="soil classes"):
        build(sc, energy_model=lh.SoilEnergyModel())
    with pytest.raises(lh.ModelError, match="per-column"):
        build(sc, soil_param_set=lh.SoilParams(FT, ν=np.full(4, 0.45)))
    with pytest.raises(lh.ModelError, match="per-column"):
        build(sc, hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=lh.vanGenuchten(FT, n=np.full(4, 2.0))))
    with pytest.raises(lh.ModelError, match="class 3"):
        lh.SoilClasses(cls, np.array([0, 1, 3, 0, 0, 0]))
    with pytest.raises(lh.ModelError, match="16 classes"):
        lh.SoilClasses(cls * 6, horizons)
    with pytest.raises(ValueError, match="class_map has shape"):
        build(lh.SoilClasses(cls, horizons[:-1]))
    with pytest.raises(ValueError, match="scalar"):
        lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=np.full(4, 2.0)))
    # the integrators without layered kernels refuse in their check_scope
    model = build(sc)
    for method in (lh.ImplicitEuler(), lh.TRBDF2()):
        with pytest.raises(NotImplementedError, match="soil classes"):
            method.check_scope(model)
    lh.SSPRK33().check_scope(model)
