"""CoupledFactorsImplicitEuler / CoupledFactorsTRBDF2 and step_implicit_coupled_factors at the host mirror's two seams
(tests/host_mirror_recorder.py), without a device and without the library: they issue the calls CoupledImplicitEuler /
CoupledTRBDF2 and step_implicit_coupled issue, under the new entry point's name (one library call per chunk), and
refuse at construction in the library's order and words: another model pair, soil classes, a viscosity factor, no
impedance factor, a prescribed-atmosphere top."""
import copy
import types

import pytest

import host_mirror_recorder as R

lh = R.lh
OLD, NEW = "lh_step_coupled_implicit", "lh_step_coupled_factors_implicit"


@pytest.fixture(autouse=True)
def table_length():
    """The recorder knows a call's boundary table by the entry point's name: the new call has its twin's layout."""
    R.TABLE_LENGTH[NEW] = R.TABLE_LENGTH[OLD]
    yield
    del R.TABLE_LENGTH[NEW]


def renamed(rec):
    """A recording of the plain call with the entry point's name replaced by the new one."""
    rec = copy.deepcopy(rec)
    for entry in rec["log"]:
        if entry[0] == "lib" and entry[1] == OLD:
            entry[1] = NEW
    return rec


def pair(flavour):
    """(a coupled model the plain call serves, the same model with the impedance factor)"""
    return (R.make_model("coupled", dirichlet=flavour == "dirichlet"),
            R.make_model("coupled", factor="impedance", dirichlet=flavour == "dirichlet"))


def with_both_factors(**kw):
    model = R.make_model("coupled", factor="impedance", **kw)
    model.hydrology_model.viscosity_factor = lh.TemperatureDependentViscosity(R.FT)
    return model


CALLS = [((R.T, R.DT, 3), {}),
         ((), {}),
         ((R.T, R.DT, 0), {}),
         ((R.T, R.DT, 3), dict(method="trbdf2")),
         ((R.T, R.DT, 3), dict(method="euler", tol=1e-9, max_iter=7)),
         ((R.T, R.DT, 5), dict(method="trbdf2", tol=1e-8))]


@pytest.mark.parametrize("flavour", ["dirichlet", "flux"])
@pytest.mark.parametrize("k", range(len(CALLS)))
def test_function_issues_the_plain_call_under_the_new_name(flavour, k):
    args, kw = CALLS[k]
    m0, m1 = pair(flavour)
    want = renamed(R.record(m0, lambda: lh.step_implicit_coupled(m0, R.StubState(), None, *args, **kw)))
    got = R.record(m1, lambda: lh.step_implicit_coupled_factors(m1, R.StubState(), None, *args, **kw))
    assert "raises" not in got, got
    calls = [e for e in got["log"] if e[0] == "lib" and e[1].startswith("lh_step")]
    assert [e[1] for e in calls] == [NEW]          # one library call, and it is the new one
    assert got == want


def test_the_call_s_arguments():
    """flags, the table of nsteps + 1 samples and the Newton arguments, as the entry point takes them."""
    _, m1 = pair("dirichlet")
    got = R.record(m1, lambda: lh.step_implicit_coupled_factors(m1, R.StubState(), None, R.T, R.DT, 3, "trbdf2", 1e-9, 7))
    (call,) = [e for e in got["log"] if e[0] == "lib" and e[1] == NEW]
    a = call[2]
    assert len(a) == 10
    assert a[3:7] == [R.enc(float(R.T)), R.enc(float(R.DT)), 3, lh._ffi.LH_COUPLED_TRBDF2]
    assert a[8:] == [R.enc(1e-9), 7]
    assert a[7] is not None                        # the sampled Dirichlet closures: 4 (nsteps + 1) doubles
    with pytest.raises(ValueError):
        lh.step_implicit_coupled_factors(m1, R.StubState(), None, method="rk4")


def advance_log(model, marker):
    """marker.advance over a first chunk, a middle chunk and the chunk that reaches tf, as the recorder drives it"""
    it = types.SimpleNamespace(u=R.StubState(), p=None, t=R.T, t0=R.T, tf=R.T + R.TOTAL * R.DT, dt=R.DT, _nsteps_done=0)
    sim = types.SimpleNamespace(integrator=it, method=marker, model=model)
    out, done = [], 0
    while done < R.TOTAL:
        n = min(R.CHUNK, R.TOTAL - done)
        rec = R.record(model, lambda: marker.advance(sim, n))
        assert "returns" in rec, rec
        it._nsteps_done += n
        it.t = it.t + n * it.dt if rec["returns"] is None else float.fromhex(rec["returns"])
        out.append(rec)
        done += n
    return out


@pytest.mark.parametrize("flavour", ["dirichlet", "flux"])
@pytest.mark.parametrize("plain,new,kw", [("CoupledImplicitEuler", "CoupledFactorsImplicitEuler", {}),
                                          ("CoupledImplicitEuler", "CoupledFactorsImplicitEuler", dict(tol=1e-9, max_iter=9)),
                                          ("CoupledTRBDF2", "CoupledFactorsTRBDF2", {}),
                                          ("CoupledTRBDF2", "CoupledFactorsTRBDF2", dict(tol=1e-8, max_iter=11))])
def test_markers_advance_as_the_plain_markers_under_the_new_name(flavour, plain, new, kw):
    m0, m1 = pair(flavour)
    want = [renamed(r) for r in advance_log(m0, getattr(lh, plain)(**kw))]
    got = advance_log(m1, getattr(lh, new)(**kw))
    assert got == want
    for chunk in got:                               # one library call per chunk
        assert [e[1] for e in chunk["log"] if e[0] == "lib" and e[1].startswith("lh_step")] == [NEW]


def test_markers_constructors():
    e, t = lh.CoupledFactorsImplicitEuler(), lh.CoupledFactorsTRBDF2(tol=1e-9, max_iter=20)
    assert isinstance(e, lh.CoupledImplicitEuler) and isinstance(t, lh.CoupledFactorsImplicitEuler)
    assert not isinstance(e, lh.CoupledTRBDF2)
    assert (e.method, e.tol, e.max_iter) == ("euler", None, None)
    assert (t.method, t.tol, t.max_iter) == ("trbdf2", 1e-9, 20)
    for cls, parent in ((lh.CoupledFactorsImplicitEuler, lh.CoupledImplicitEuler), (lh.CoupledFactorsTRBDF2, lh.CoupledTRBDF2)):
        assert list(R.inspect.signature(cls).parameters) == list(R.inspect.signature(parent).parameters) == ["tol", "max_iter"]


PAIR = "{name}: coupled models only (SoilEnergyModel + SoilHydrologyModel)"
CLASSES = ("{name} is not available with soil classes (a layered coupled model steps with SSPRK33, LayeredCoupledImplicitEuler, "
           "LayeredCoupledTRBDF2 or LayeredCoupledAdaptiveTRBDF2, a layered heat-only model with SSPRK33, "
           "LayeredHeatImplicitEuler or LayeredHeatTRBDF2)")
VISCOSITY = ("{name}: a viscosity factor other than NoEffect is not supported: the water then reads the unknown T and the "
             "stage is no longer block triangular")
NO_IMPEDANCE = ("{name}: the context has no impedance factor (lh_set_conductivity_factors); lh_step_coupled_implicit steps "
                "a model without conductivity factors")
ATMOS = "{name}: a prescribed-atmosphere top is not supported"
# every model violates what its row names and everything after it in the library's order
REFUSALS = [(lambda: R.make_model("richards", classes=True, factor="viscosity", atmos=True), PAIR),
            (lambda: R.make_model("heat", atmos=True), PAIR),
            (lambda: R.make_model("coupled", classes=True, factor="viscosity", atmos=True), CLASSES),
            (lambda: R.make_model("coupled", factor="viscosity", atmos=True), VISCOSITY),
            (lambda: with_both_factors(atmos=True), VISCOSITY),
            (lambda: R.make_model("coupled", atmos=True), NO_IMPEDANCE),
            (lambda: R.make_model("coupled", factor="impedance", atmos=True), ATMOS)]


@pytest.mark.parametrize("marker", ["CoupledFactorsImplicitEuler", "CoupledFactorsTRBDF2"])
@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusals_at_construction_in_the_library_s_order(marker, k):
    make, words = REFUSALS[k]
    model = make()
    rec = R.record(model, lambda: getattr(lh, marker)().check_scope(model))
    assert rec == {"log": [], "raises": ["NotImplementedError", words.format(name=marker)]}
    with pytest.raises(NotImplementedError) as e:
        lh.Simulation(model, getattr(lh, marker)(), Y_init=R.StubState(), dt=R.DT, tspan=(0.0, 1.0), Ya_init=None)
    assert str(e.value) == words.format(name=marker)
    rec = R.record(model, lambda: lh.step_implicit_coupled_factors(model, R.StubState(), None))
    assert rec == {"log": [], "raises": ["NotImplementedError", words.format(name="step_implicit_coupled_factors")]}


def test_scope_passes_with_the_impedance_factor_and_the_plain_markers_still_refuse_it():
    model = R.make_model("coupled", factor="impedance")
    for marker in ("CoupledFactorsImplicitEuler", "CoupledFactorsTRBDF2"):
        assert R.record(model, lambda: getattr(lh, marker)().check_scope(model)) == {"log": [], "returns": None}
    for marker in ("CoupledImplicitEuler", "CoupledTRBDF2", "CoupledAdaptiveTRBDF2"):
        rec = R.record(model, lambda: getattr(lh, marker)().check_scope(model))
        assert rec["raises"] == ["NotImplementedError", "%s: conductivity factors other than NoEffect are not supported" % marker]
