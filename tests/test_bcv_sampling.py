"""The host mirror's one boundary-value sampler (soil._sampled_bcv) and the method markers' scope checks.
CPU only, and nothing here loads the library: the sampler reads the model's closures and nothing else.

Every expected array is written out directly from the closures; comparisons are np.array_equal (the
arrays go to the library as they are, so a last-bit difference in a sampling time is a different run)."""
import numpy as np
import pytest

import __graft_entry__ as g

lh = g.load_package()
S = lh.soil
F = lh._ffi
BOT, TOP = F.LH_FACE_BOTTOM, F.LH_FACE_TOP
EN, HY = F.LH_COMP_ENERGY, F.LH_COMP_HYDROLOGY
NCOLS = 4


def _model(top, bottom, energy=None, hydrology=None):
    FT = np.float64
    return lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-1.0, 0.0), nelements=4, ncolumns=NCOLS),
                        energy_model=energy or lh.SoilEnergyModel(),
                        hydrology_model=hydrology or lh.SoilHydrologyModel(FT),
                        boundary_conditions=lh.SoilColumnBC(top=top, bottom=bottom),
                        earth_param_set=lh.EarthParameterSet())


# closures whose value moves with the last bit of t
def T_bot(t):
    return 280.0 + 3.0 * np.sin(t)


def vl_top(t):
    return 0.3 + t / 7.0


def identity(t):
    return t


# (model, {(face, comp): closure or constant}): every entry not named is 0
def _cases():
    mixed = _model(top=lh.SoilComponentBC(energy=lh.VerticalFlux(12.5), hydrology=lh.Dirichlet(vl_top)),
                   bottom=lh.SoilComponentBC(energy=lh.Dirichlet(T_bot), hydrology=lh.VerticalFlux(-1e-7)))
    drain = _model(top=lh.SoilComponentBC(hydrology=lh.Dirichlet(identity)),      # energy: NoBC on both faces
                   bottom=lh.SoilComponentBC(hydrology=lh.FreeDrainage()),
                   energy=lh.PrescribedTemperatureModel())
    percol = _model(top=lh.SoilComponentBC(energy=lh.VerticalFlux(np.arange(float(NCOLS))),
                                           hydrology=lh.Dirichlet(lambda t: np.full(NCOLS, 0.2 + t))),
                    bottom=lh.SoilComponentBC(energy=lh.Dirichlet(7.0), hydrology=lh.Dirichlet(identity)))
    return {
        "mixed": (mixed, {(TOP, EN): 12.5, (TOP, HY): vl_top, (BOT, EN): T_bot, (BOT, HY): -1e-7}),
        "drain": (drain, {(TOP, HY): identity}),
        # the per-column flux and the per-column Dirichlet closure stay 0 (they reach the library through
        # set_bcs); Dirichlet(7.0) is a constant closure
        "percol": (percol, {(BOT, EN): 7.0, (BOT, HY): identity}),
    }


CASES = _cases()

T0, DT, N = 3.7, 0.1, 7
# the five callers' time lists, each with the caller's own floating-point expression, and its base time
TIME_LISTS = {
    "implicit_euler": ([T0 + (k + 1) * DT for k in range(N)], T0),
    "heat_implicit": ([T0 + k * DT for k in range(N + 1)], T0),
    "trbdf2": ((T0, T0 + N * DT), T0),
    "ssprk33": ([[(T0 + DT * np.arange(N))[k] + off for off in (0.0, DT, DT / 2)] for k in range(N)], T0),
    "ssprk33_refreshing_aux": ((T0, T0 + DT, T0 + DT / 2), T0),
}


def _expected(times, entries):
    times = np.asarray(times)
    want = np.zeros(times.shape + (2, 2))
    for k in np.ndindex(times.shape):
        for (f, c), v in entries.items():
            want[k + (f, c)] = v(times[k]) if callable(v) else v
    return want


@pytest.mark.parametrize("caller", sorted(TIME_LISTS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_sampled_values_are_the_closures_at_the_callers_times(case, caller):
    model, entries = CASES[case]
    times, base_t = TIME_LISTS[caller]
    got = S._sampled_bcv(model, times, base_t)
    want = _expected(times, entries)
    assert got.shape == np.shape(times) + (2, 2) and got.dtype == np.float64 and got.flags.c_contiguous
    assert np.array_equal(got, want)


def test_no_dirichlet_closure_means_no_array():
    model = _model(top=lh.SoilComponentBC(energy=lh.VerticalFlux(1.0), hydrology=lh.VerticalFlux(-2e-7)),
                   bottom=lh.SoilComponentBC(energy=lh.VerticalFlux(0.0), hydrology=lh.FreeDrainage()))
    for times, base_t in TIME_LISTS.values():
        assert S._sampled_bcv(model, times, base_t) is None


def test_ssprk33_stage_times_are_the_callers_expression_to_the_last_bit():
    """dt = 0.1, 7 steps from t = 0: t[k] + dt/2 and t + (k + 0.5) dt differ in the last bit for some k, and
    the identity closure makes every sampled value its own sampling time.  The values are those of the
    caller's expression (t + dt arange)[k] + off, which is also what Simulation's SSPRK33 driver builds."""
    t0, dt, n = 0.0, 0.1, 7
    tk = t0 + dt * np.arange(n)
    callers = np.array([[tk[k] + off for off in (0.0, dt, dt / 2)] for k in range(n)])
    other = np.array([[t0 + k * dt, t0 + (k + 1) * dt, t0 + (k + 0.5) * dt] for k in range(n)])
    assert not np.array_equal(callers[:, 2], other[:, 2])     # the premise: the two spellings are not the same
    assert np.array_equal(S._stage_times(t0, dt, n), callers)
    model, _ = CASES["drain"]
    got = S._sampled_bcv(model, S._stage_times(t0, dt, n), t0)
    assert np.array_equal(got[:, :, TOP, HY], callers)
    assert not np.array_equal(got[:, 2, TOP, HY], other[:, 2])
    got[:, :, TOP, HY] = 0.0
    assert not got.any()


# ---- scope refusals: the texts of the parent's _check_implicit_scope / _check_heat_implicit_scope

def _refused_models():
    FT = np.float64
    flux = lh.SoilComponentBC(energy=lh.VerticalFlux(0.0), hydrology=lh.VerticalFlux(0.0))
    wflux = lh.SoilComponentBC(hydrology=lh.VerticalFlux(0.0))
    atmos = lh.PrescribedAtmosForcing(FT, u_atm=2.0, theta_atm=290.0, z_atm=2.0, theta_scale=290.0,
                                      rho_a_sfc=1.2, q_atm=0.005)
    return {
        "coupled": _model(top=flux, bottom=flux),
        "viscosity": _model(top=wflux, bottom=wflux, energy=lh.PrescribedTemperatureModel(),
                            hydrology=lh.SoilHydrologyModel(FT, viscosity_factor=lh.TemperatureDependentViscosity(FT))),
        "atmos": _model(top=atmos, bottom=wflux, energy=lh.PrescribedTemperatureModel()),
    }


RICHARDS_TEXT = {
    "coupled": "{} is provided for Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)",
    "viscosity": "{} supports the NoEffect conductivity factors only",
    "atmos": "{} does not support a prescribed-atmosphere top",
}
HEAT_TEXT = "{} is provided for heat-only models only (SoilEnergyModel + PrescribedHydrologyModel)"


@pytest.mark.parametrize("which", ["coupled", "viscosity", "atmos"])
def test_scope_refusals_keep_their_words(which):
    model = _refused_models()[which]
    want = {
        lh.ImplicitEuler: RICHARDS_TEXT[which].format("ImplicitEuler"),
        lh.TRBDF2: RICHARDS_TEXT[which].format("TRBDF2"),
        lh.HeatImplicitEuler: HEAT_TEXT.format("HeatImplicitEuler"),
        lh.HeatTRBDF2: HEAT_TEXT.format("HeatTRBDF2"),
    }
    for marker, text in want.items():
        with pytest.raises(NotImplementedError) as e:
            marker().check_scope(model)
        assert str(e.value) == text
        with pytest.raises(NotImplementedError) as e:      # ... and Simulation asks the marker first of all
            lh.Simulation(model, marker(), Y_init=None, dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
        assert str(e.value) == text
    lh.SSPRK33().check_scope(model)                        # SSPRK33 refuses no model
    # the stepping functions carry their own names
    with pytest.raises(NotImplementedError) as e:
        lh.step_implicit(model, None)
    assert str(e.value) == want[lh.ImplicitEuler]
    with pytest.raises(NotImplementedError) as e:
        lh.integrate_trbdf2(model, None)
    assert str(e.value) == want[lh.TRBDF2]
    with pytest.raises(NotImplementedError) as e:
        lh.step_implicit_heat(model, None)
    assert str(e.value) == HEAT_TEXT.format("step_implicit_heat")


def test_unknown_method_is_refused_before_anything_else():
    with pytest.raises(NotImplementedError) as e:
        lh.Simulation(_refused_models()["coupled"], object(), Y_init=None, dt=1.0, tspan=(0.0, 1.0), Ya_init=None)
    assert str(e.value) == ("only SSPRK33, ImplicitEuler, TRBDF2, HeatImplicitEuler and HeatTRBDF2 are "
                            "provided on the device")
