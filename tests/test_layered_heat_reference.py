"""The NumPy reference of the layered coupled and heat-only tendency (tests/layered_heat_ref.py) checked on the
CPU: against the oracle called once per class where every column has one class, and against what a layered
column must satisfy whatever computes it (an isothermal hydrostatic column at rest, conservation).  And the host
mirror's types for thermal classes, which need no device."""
import numpy as np
import pytest

import case_model as M
import layered_heat_ref as H
import layered_ref as R
import parity_cases as pc
from layered_heat_checks import assert_close_per_class, check_conservation

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
MODELS = [M.MODEL_COUPLED, M.MODEL_HEAT]
MODEL_IDS = ["coupled", "heat"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("bc", ["flux", "dirichlet", "dirichlet_consistent"])
@pytest.mark.parametrize("factors,ice", [(False, False), (True, True)], ids=["plain", "factors_ice"])
def test_one_class_per_column_equals_the_oracle_called_per_class(dtype, model, bc, factors, ice):
    lay = H.make_layered_heat(dtype, 700, 64, R.uniform_map(700, 64), model=model, bc=bc, factors=factors, ice=ice)
    used, share = assert_close_per_class(lay, H.rhs(lay))
    print("share of the model used:", used, "plain share:", share)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_coupled_flux_drain_equals_the_oracle_called_per_class(dtype):
    lay = H.make_layered_heat(dtype, 130, 64, R.uniform_map(130, 64), bc="flux_drain", ice=True)
    assert_close_per_class(lay, H.rhs(lay))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_isothermal_hydrostatic_column_is_at_rest(dtype, model):
    """Three horizons, T uniform (so rho e_int jumps at the horizons through rho_c_ds and nu), the water
    hydrostatic, zero-flux faces: nothing moves.  The scale is what the same state does with the map one level
    off its horizons; a tendency that takes any thermal constant from the scalars fails this."""
    rest = H.rhs(H.isothermal_hydrostatic(dtype, model))
    shifted = H.rhs(H.isothermal_hydrostatic(dtype, model, shift=1))
    for k in rest:
        r, s = np.abs(rest[k]).max(), np.abs(shifted[k]).max()
        print("%s: max|d| at rest %.3g, one level off its horizons %.3g" % (k, r, s))
        assert s > 0
        assert r <= 1e-6 * s, (k, r, s)
    lay = H.isothermal_hydrostatic(dtype, model)
    assert len(np.unique(lay.class_map)) == 3 and np.ptp(lay.case.rhoe) > 0.1 * np.abs(lay.case.rhoe).max()
    # the scalar tendency (every thermal constant the context's) does NOT rest
    scalar = H.LayeredHeat(lay.case, lay.classes, np.repeat(lay.thermal[:1], 3, axis=0), lay.class_map)
    assert np.abs(H.rhs(scalar)["rhoe"]).max() > 1e-3 * np.abs(shifted["rhoe"]).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("model,bc", [(M.MODEL_COUPLED, "flux"), (M.MODEL_COUPLED, "flux_drain"), (M.MODEL_COUPLED, "dirichlet"),
                                      (M.MODEL_HEAT, "flux"), (M.MODEL_HEAT, "dirichlet")])
def test_conservation(dtype, model, bc):
    lay = H.make_layered_heat(dtype, 130, 64, R.horizon_map(130, 64), model=model, bc=bc)
    d, faces = H.rhs(lay, faces=True)
    print("conservation: worst column uses", check_conservation(lay, d, faces), "of the bound")


@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_float32_reference_stays_within_the_plain_share_of_the_float64_one(model):
    """the inputs of the per-cell GPU test: the reference alone, Float32 against Float64"""
    lay = H.make_layered_heat(np.float32, 130, 64, R.horizon_map(130, 64), model=model, bc=H.PER_CELL_BC[model])
    got, want = H.rhs(lay), H.rhs(H.as64(lay))
    share = pc.plain_statistic(lay.case, got, want)
    print("Float32 reference against the Float64 one, share within %g: %s" % (pc.PLAIN_REL[np.dtype(np.float32)], share))
    for k, s in share.items():
        assert s >= pc.PLAIN_SHARE_MIN[np.dtype(np.float32)], (k, s)


def test_thermal_classes_differ_clearly():
    t = H.thermal_classes(16)
    assert np.any(t[:, 6] > 0) and np.any(t[:, 6] == 0)
    for j in (0, 3, 4):     # rho_c_ds, kappa_sat_unfrozen, kappa_sat_frozen of neighbouring classes
        assert np.all(np.abs(np.diff(t[:, j])) > 0.05 * np.abs(t[:-1, j])), j
    nu = R.texture_classes(16)[:, 4]
    assert np.all(np.abs(np.diff(nu)) > 0.01)


# ------------------------------------------------------------ the host mirror's types (no device needed)

def test_mirror_types_for_thermal_classes():
    lh = pc._pkg()
    FT = np.float64
    th = lh.SoilThermal(FT, ρc_ds=2.1e6, κ_solid=3.0, ρp=2600.0, κ_sat_unfrozen=1.4, κ_sat_frozen=2.9, ν_ss_gravel=0.05,
                        ν_ss_om=0.2, ν_ss_quartz=0.3)
    assert th.rho_c_ds == 2.1e6 and th.ν_ss_om == 0.2 and th.kappa_sat_frozen == 2.9
    d = lh.SoilThermal(FT)
    sp = lh.SoilParams(FT)
    for name in H.THERMAL_FIELDS:       # the defaults are SoilParams'
        assert getattr(d, name) == getattr(sp, name), name
    assert d.ρc_ds == sp.ρc_ds and d.κ_solid == sp.kappa_solid and d.ν_ss_quartz == sp.nu_ss_quartz
    with pytest.raises(TypeError):
        lh.SoilThermal(FT, κ_dry_parameter=0.05)           # stays a scalar of the model
    with pytest.raises((TypeError, ValueError)):
        lh.SoilThermal(FT, ρc_ds=np.full(3, 2e6))            # a class is scalars
    hm = lh.vanGenuchten(FT)
    with_th = [lh.SoilClass(FT, hydraulic_model=hm, ν=0.4 + 0.02 * k, thermal=th) for k in range(3)]
    assert with_th[0].thermal is th and lh.SoilClass(FT, hydraulic_model=hm).thermal is None
    horizons = np.array([0, 0, 1, 2])

    def build(classes):
        dom = lh.Column(FT, zlim=(-1.0, 0.0), nelements=4, ncolumns=3)
        bc = lh.SoilColumnBC(top=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0), hydrology=lh.VerticalFlux(0.0)),
                             bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0), hydrology=lh.VerticalFlux(0.0)))
        return lh.SoilModel(FT, domain=dom, energy_model=lh.SoilEnergyModel(),
                            hydrology_model=lh.SoilHydrologyModel(FT, hydraulic_model=hm), boundary_conditions=bc,
                            soil_param_set=sp, earth_param_set=lh.EarthParameterSet(),
                            soil_classes=lh.SoilClasses(classes, horizons))

    model = build(with_th)
    assert model.soil_classes.has_thermal
    with pytest.raises(lh.ModelError, match="soil classes"):
        build(with_th[:2] + [lh.SoilClass(FT, hydraulic_model=hm, ν=0.5)])
