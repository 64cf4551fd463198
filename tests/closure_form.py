"""Selecting and asserting the closure form (lh_closure_form) in GPU tests.

The Float64 water kernels exist in two forms of the table-driven 2^(.): the
integer-exponent form, which ordinary ensembles take, and the v_ldexp form, which the host chooses for
clay-like parameters and which `vgfast=0` forces.  `ldexp_form` runs a test in the second: LH_TUNE is
read at lh_create, so every context the test creates -- through whatever helper -- starts with
`vgfast=0`; and every parity_cases.GpuModel that is left without an error is asked, at that moment,
which form its next launch would take, so a helper that resets the tuning (lh_set_tuning resets the keys
it is not given) or a context that silently runs the other form fails the test.

Test infrastructure (fixtures are imported by the test modules that use them), no test of its own.
"""
import numpy as np
import pytest

import case_model as M
import parity_cases as pc

LDEXP, INTEGER_EXPONENT, NOT_APPLICABLE = 0, 1, 2


def has_two_forms(g, math_mode=None):
    """Float64, a model with water, the production math: the contexts lh_closure_form answers 0 or 1 for."""
    return (np.dtype(g.case.dtype) == np.float64 and g.case.om.model != M.MODEL_HEAT
            and math_mode in (None, g.F.LH_MATH_FAST))


def assert_form(g, want, math_mode=None):
    got = g.L.lh_closure_form(g.ctx)
    assert got == (want if has_two_forms(g, math_mode) else NOT_APPLICABLE), (g.case.name, got, want)


class _Checked:
    contexts = 0


def _watch(monkeypatch, want):
    """Every GpuModel left without an error asserts its form; -> the counter of contexts that had two forms to choose from."""
    checked = _Checked()
    cls = pc.GpuModel
    init, leave = cls.__init__, cls.__exit__

    def __init__(self, case, math_mode=None, stream=None):
        self._math_mode = math_mode
        init(self, case, math_mode, stream)

    def __exit__(self, *a):
        try:
            if self.ctx:
                checked.contexts += has_two_forms(self, self._math_mode)
                if a[0] is None:     # (a test that is failing already keeps its own error)
                    assert_form(self, want, self._math_mode)
        finally:
            leave(self, *a)

    monkeypatch.setattr(cls, "__init__", __init__)
    monkeypatch.setattr(cls, "__exit__", __exit__)
    return checked


@pytest.fixture
def ldexp_form(monkeypatch):
    """The test runs with `vgfast=0`; at least one of its contexts must have had the two forms to choose from."""
    monkeypatch.setenv("LH_TUNE", "vgfast=0")
    checked = _watch(monkeypatch, LDEXP)
    yield checked
    assert checked.contexts > 0, "no Float64 water context was created: the test did not run the v_ldexp form"


@pytest.fixture
def host_chosen_ldexp_form(monkeypatch):
    """No tuning: the host's interval test must itself choose the v_ldexp form in every context of the test."""
    monkeypatch.delenv("LH_TUNE", raising=False)
    checked = _watch(monkeypatch, LDEXP)
    yield checked
    assert checked.contexts > 0
