"""FactorsImplicitEuler / FactorsTRBDF2 and step_implicit_factors / integrate_factors_trbdf2 at the host mirror's two
seams (tests/host_mirror_recorder.py), without a device and without the library: they issue the calls ImplicitEuler /
TRBDF2 and step_implicit / integrate_trbdf2 issue, under the new names, and refuse at construction in the library's
order: another model pair, soil classes, factors that are both NoEffect, a prescribed-atmosphere top."""
import copy
import types

import pytest

import host_mirror_recorder as R

lh = R.lh
NEW = {"lh_step_implicit_euler": "lh_step_factors_implicit_euler", "lh_integrate_trbdf2": "lh_integrate_factors_trbdf2"}


@pytest.fixture(autouse=True)
def table_lengths():
    """The recorder knows a call's boundary table by the entry point's name: the new calls have their twins' layouts."""
    for old, new in NEW.items():
        R.TABLE_LENGTH[new] = R.TABLE_LENGTH[old]
    yield
    for new in NEW.values():
        del R.TABLE_LENGTH[new]


def renamed(rec):
    """A recording of the plain calls with the entry points' names replaced by the factors calls'."""
    rec = copy.deepcopy(rec)
    for entry in rec["log"]:
        if entry[0] == "lib":
            entry[1] = NEW.get(entry[1], entry[1])
    return rec


def pair(flavour, factor):
    """(a model the plain calls serve, the same model with a conductivity factor)"""
    return (R.make_model("richards", dirichlet=flavour == "dirichlet"),
            R.make_model("richards", factor=factor, dirichlet=flavour == "dirichlet"))


CALLS = [("step_implicit", "step_implicit_factors", (R.T, R.DT, 3), {}),
         ("step_implicit", "step_implicit_factors", (), {}),
         ("step_implicit", "step_implicit_factors", (R.T, R.DT, 0), {}),
         ("step_implicit", "step_implicit_factors", (R.T, R.DT, 3), dict(tol=1e-9, max_iter=7)),
         ("integrate_trbdf2", "integrate_factors_trbdf2", (R.T0, R.T1, R.DT), {}),
         ("integrate_trbdf2", "integrate_factors_trbdf2", (), {}),
         ("integrate_trbdf2", "integrate_factors_trbdf2", (R.T0, R.T1, R.DT), dict(abstol=1e-8, reltol=1e-5)),
         ("integrate_trbdf2", "integrate_factors_trbdf2", (R.T0, R.T1, R.DT), dict(reltol=0.0, adaptive=False))]


@pytest.mark.parametrize("flavour", ["dirichlet", "flux"])
@pytest.mark.parametrize("factor", ["viscosity", "impedance"])
@pytest.mark.parametrize("k", range(len(CALLS)))
def test_functions_issue_the_plain_calls_under_the_new_names(flavour, factor, k):
    plain, new, args, kw = CALLS[k]
    m0, m1 = pair(flavour, factor)
    want = renamed(R.record(m0, lambda: getattr(lh, plain)(m0, R.StubState(), None, *args, **kw)))
    got = R.record(m1, lambda: getattr(lh, new)(m1, R.StubState(), None, *args, **kw))
    assert "raises" not in got, got
    assert [e[1] for e in got["log"] if e[0] == "lib"][0] in NEW.values()
    assert got == want


def test_dt_cols_reach_the_new_adaptive_call():
    import torch
    m0, m1 = pair("flux", "impedance")
    kw = dict(dt_cols=R.FakeDeviceTensor(R.NCOLS, torch.float64))
    want = renamed(R.record(m0, lambda: lh.integrate_trbdf2(m0, R.StubState(), None, R.T0, R.T1, R.DT, **kw)))
    assert R.record(m1, lambda: lh.integrate_factors_trbdf2(m1, R.StubState(), None, R.T0, R.T1, R.DT, **kw)) == want


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
@pytest.mark.parametrize("plain,new,kw", [("ImplicitEuler", "FactorsImplicitEuler", {}),
                                          ("ImplicitEuler", "FactorsImplicitEuler", dict(tol=1e-9, max_iter=9)),
                                          ("TRBDF2", "FactorsTRBDF2", {}),
                                          ("TRBDF2", "FactorsTRBDF2", dict(abstol=1e-8, reltol=1e-5, adaptive=False))])
def test_markers_advance_as_the_plain_markers_under_the_new_names(flavour, plain, new, kw):
    m0, m1 = pair(flavour, "viscosity")
    want = [renamed(r) for r in advance_log(m0, getattr(lh, plain)(**kw))]
    assert advance_log(m1, getattr(lh, new)(**kw)) == want


def test_markers_take_no_forcing():
    assert "forcing" not in R.inspect.signature(lh.FactorsTRBDF2).parameters
    assert "forcing" not in R.inspect.signature(lh.FactorsImplicitEuler).parameters
    assert lh.FactorsTRBDF2().forcing is None
    assert isinstance(lh.FactorsTRBDF2(), lh.TRBDF2) and isinstance(lh.FactorsImplicitEuler(), lh.ImplicitEuler)


PAIR = "{name} is provided for Richards models only (SoilHydrologyModel + PrescribedTemperatureModel)"
CLASSES = "{name} is not available with soil classes (layered soils step with SSPRK33, LayeredImplicitEuler or LayeredTRBDF2)"
NO_FACTORS = "{name} is provided for models with a conductivity factor other than NoEffect (without one: ImplicitEuler, TRBDF2)"
ATMOS = "{name} does not support a prescribed-atmosphere top"
# every model violates what its row names and everything after it in the library's order
REFUSALS = [(dict(family="coupled", classes=True, atmos=True), PAIR),
            (dict(family="richards", classes=True, atmos=True), CLASSES),
            (dict(family="richards", atmos=True), NO_FACTORS),
            (dict(family="richards", factor="impedance", atmos=True), ATMOS)]


@pytest.mark.parametrize("marker", ["FactorsImplicitEuler", "FactorsTRBDF2"])
@pytest.mark.parametrize("kw,words", REFUSALS)
def test_refusals_at_construction_in_the_library_s_order(marker, kw, words):
    model = R.make_model(**kw)
    rec = R.record(model, lambda: getattr(lh, marker)().check_scope(model))
    assert rec == {"log": [], "raises": ["NotImplementedError", words.format(name=marker)]}
    Y = R.StubState()
    with pytest.raises(NotImplementedError) as e:
        lh.Simulation(model, getattr(lh, marker)(), Y_init=Y, dt=R.DT, tspan=(0.0, 1.0), Ya_init=None)
    assert str(e.value) == words.format(name=marker)


@pytest.mark.parametrize("factor", ["viscosity", "impedance"])
def test_scope_passes_with_a_factor_and_the_plain_markers_still_refuse_it(factor):
    model = R.make_model("richards", factor=factor)
    for marker in ("FactorsImplicitEuler", "FactorsTRBDF2"):
        assert R.record(model, lambda: getattr(lh, marker)().check_scope(model)) == {"log": [], "returns": None}
    for marker in ("ImplicitEuler", "TRBDF2"):
        rec = R.record(model, lambda: getattr(lh, marker)().check_scope(model))
        assert rec["raises"] == ["NotImplementedError", "%s supports the NoEffect conductivity factors only" % marker]
