"""BoundarySeries on the host (no GPU): its validation with the library's own rules, its breakpoints and its
end values against the formula of include/landhydro.h; and the four entry points of the series in the header,
the ctypes table, the Julia shim and INTEGRATION.md."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lh_bc_series_create", "lh_bc_series_set", "lh_bc_series_destroy", "lh_integrate_series")


@pytest.fixture(scope="module")
def lh():
    return g.load_package()


def test_validation_with_the_librarys_rules(lh):
    S = lh.BoundarySeries
    ok = {("top", "hydrology"): [1.0, 2.0, 3.0]}
    for bad, word in (([0.0], "nknots"), ([[0.0, 1.0], [2.0, 3.0]], "nknots"), ([0.0, 1.0, 1.0], "knot 2"),
                      ([0.0, 2.0, 1.0], "knot 2"), ([0.0, float("nan"), 2.0], "knot 1"), ([0.0, 1.0, float("inf")], "knot 2")):
        with pytest.raises(ValueError, match=word):
            S(bad, {})
    with pytest.raises(ValueError, match="shape"):
        S([0.0, 1.0, 2.0], {("top", "hydrology"): [1.0, 2.0]})
    with pytest.raises(ValueError, match="shape"):
        S([0.0, 1.0, 2.0], {("top", "hydrology"): np.zeros((3, 2, 2))})
    with pytest.raises(ValueError, match="not a \\(face, component\\)"):
        S([0.0, 1.0, 2.0], {("side", "hydrology"): [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError, match="not a \\(face, component\\)"):
        S([0.0, 1.0, 2.0], {"top": [1.0, 2.0, 3.0]})
    with pytest.raises(ValueError, match="twice"):
        S([0.0, 1.0, 2.0], {("top", "hydrology"): [1.0, 2.0, 3.0], (1, 1): [1.0, 2.0, 3.0]})
    s = S([0.0, 1.0, 2.0], ok)
    assert s.nknots == 3 and list(s.values) == [(lh._ffi.LH_FACE_TOP, lh._ffi.LH_COMP_HYDROLOGY)]
    # values are not judged
    S([0.0, 1.0], {("bottom", "energy"): [float("nan"), float("inf")]})
    # names and the C enums are the same keys
    a = S([0.0, 1.0], {(lh._ffi.LH_FACE_BOTTOM, lh._ffi.LH_COMP_ENERGY): [1.0, 2.0]})
    assert a.value_at(("bottom", "energy"), 0.5) == 1.5


def test_breakpoints(lh):
    s = lh.BoundarySeries([0.0, 1.0, 2.5, 4.0, 7.0], {})
    assert s.breakpoints(0.5, 6.0) == [0.5, 1.0, 2.5, 4.0, 6.0]
    assert s.breakpoints(0.0, 7.0) == [0.0, 1.0, 2.5, 4.0, 7.0]      # knots on t0 and t1 are not interior
    assert s.breakpoints(1.0, 4.0) == [1.0, 2.5, 4.0]
    assert s.breakpoints(1.2, 2.0) == [1.2, 2.0]
    assert s.breakpoints(3.0, 3.0) == [3.0, 3.0]
    for t0, t1 in ((-0.1, 1.0), (0.0, 7.5)):
        with pytest.raises(ValueError, match="no extrapolation"):
            s.breakpoints(t0, t1)


def test_end_values_are_the_formula(lh):
    rng = np.random.default_rng(11)
    T = np.cumsum(rng.uniform(0.1, 3.0, 6))
    u = rng.normal(size=6)
    pcv = rng.normal(size=(6, 9))
    s = lh.BoundarySeries(T, {("top", "hydrology"): u, ("bottom", "energy"): pcv})
    for t in np.concatenate([rng.uniform(T[0], T[-1], 40), T]):
        k = min(int(np.searchsorted(T, t, side="right")) - 1, 4)
        for key, v in ((("top", "hydrology"), u), (("bottom", "energy"), pcv)):
            if t == T[k]:
                want = v[k]
            elif t == T[k + 1]:
                want = v[k + 1]
            else:
                want = v[k] + (v[k + 1] - v[k]) * ((t - T[k]) / (T[k + 1] - T[k]))
            got = s.value_at(key, t)
            assert np.array_equal(np.asarray(got), np.asarray(want)), (key, t)
    assert s.value_at(("top", "hydrology"), T[3]) == u[3]              # exactly the knot's value on a knot
    assert isinstance(s.value_at(("top", "hydrology"), T[0] + 0.01), float)
    assert s.value_at(("bottom", "energy"), T[-1]).shape == (9,)
    with pytest.raises(ValueError, match="no extrapolation"):
        s.value_at(("top", "hydrology"), T[-1] + 1.0)
    with pytest.raises(KeyError):
        s.value_at(("top", "energy"), T[0])


def test_methods_take_a_forcing(lh):
    s = lh.BoundarySeries([0.0, 1.0], {})
    assert lh.TRBDF2().forcing is None and lh.LayeredTRBDF2().forcing is None and lh.CoupledAdaptiveTRBDF2().forcing is None
    assert lh.TRBDF2(forcing=s).forcing is s and lh.LayeredTRBDF2(forcing=s).forcing is s
    assert lh.CoupledAdaptiveTRBDF2(forcing=s).forcing is s
    with pytest.raises(TypeError):
        lh.integrate_series(None, None, None, object(), 0.0, 1.0, 1.0)


def test_the_four_names_are_everywhere(lh):
    header = open(os.path.join(ROOT, "include", "landhydro.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    shim = open(os.path.join(g.PKG_DIR, "julia", "LandHydrologyHIP.jl"), encoding="utf-8").read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    api = open(os.path.join(g.PKG_DIR, "csrc", "lh_api.hip")).read()
    assert "typedef struct lh_bc_series lh_bc_series;" in header
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), f"{n} is not declared in landhydro.h"
        assert n in lh._ffi.SIGNATURES, f"{n} is not in _ffi.SIGNATURES"
        assert f"ccall((:{n}, lib)" in shim, f"the Julia shim never calls {n}"
        assert f"`{n}" in doc, f"INTEGRATION.md does not list {n}"
        assert re.search(r"^int %s\(" % n, api, flags=re.M), f"{n} is not defined in lh_api.hip"
    assert len(lh._ffi.SIGNATURES["lh_integrate_series"][1]) == 12
