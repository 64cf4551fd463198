"""lh_step_ssprk33_series without a device: the tests' sampler (the interpolation formula and the stage times, written
out once more; the knots and value tables the GPU tests in test_gpu_ssprk33_series.py share with this file) against a
brute-force restatement, and the host mirror's argument checks, forcing-type check and calls through
tests/host_mirror_recorder.py."""
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

import case_model as M
import host_mirror_recorder as R

lh = R.lh
STEP_SERIES = lh.step_series     # (every test here is about this call: on a build without it the module does not import)
S = sys.modules[__name__]        # (the sampler below, under the name the GPU tests import this module by)
DT = 0.0123

# ------------------------------------------------------------------ the sampler, the knots and the tables
NSTEPS = 5
TOP_H, TOP_E = (M.FACE_TOP, M.COMP_HYDROLOGY), (M.FACE_TOP, M.COMP_ENERGY)
BOT_H, BOT_E = (M.FACE_BOTTOM, M.COMP_HYDROLOGY), (M.FACE_BOTTOM, M.COMP_ENERGY)


def series_value(T, v, t):
    """v_k + (v_k+1 - v_k) ((t - T_k) / (T_k+1 - T_k)) in double with k the largest index that has T_k <= t, capped at
    nknots - 2; exactly v_k or v_k+1 on a knot (tests/test_gpu_bc_series.py::series_value)."""
    k = min(int(np.searchsorted(T, t, side="right")) - 1, len(T) - 2)
    if t == T[k]:
        return v[k]
    if t == T[k + 1]:
        return v[k + 1]
    return v[k] + (v[k + 1] - v[k]) * ((t - T[k]) / (T[k + 1] - T[k]))


def stage_times(t, dt, nsteps):
    """[nsteps][3]: t_k, t_k + dt, t_k + dt / 2 with t_k = t + dt * double(k) (the host mirror's _stage_times)."""
    return (t + dt * np.arange(nsteps))[:, None] + np.array((0.0, dt, dt / 2))


def sample_bcv(T, values, base, t, dt, nsteps):
    """bc_stage_values[nsteps][3][2][2] of lh_step_ssprk33: `base` ({(face, comp): value}, lh_set_bc's) with the
    components of `values` ({(face, comp): [nknots]}) sampled at the stage times."""
    bcv = np.zeros((nsteps, 3, 2, 2))
    for (f, c), v in base.items():
        bcv[:, :, f, c] = v
    st = stage_times(t, dt, nsteps)
    for (f, c), v in values.items():
        for s in range(nsteps):
            for stage in range(3):
                bcv[s, stage, f, c] = series_value(T, v, st[s, stage])
    return bcv


def start_time(dt):
    return 3.7 * dt


def knots(dt, nsteps=NSTEPS):
    """Six irregular knots around the `nsteps` steps of dt from start_time(dt): the first step spans two knots (+0.2 dt,
    +0.7 dt), the last interval holds the steps 2, 3 and 4 whole, the knot 3 IS the third stage time of step 1 (same
    arithmetic, and the tables below have a kink there), and the last knot IS the last stage time of the call."""
    t0 = start_time(dt)
    st = stage_times(t0, dt, nsteps)
    T = np.array([t0 - 0.3 * dt, t0 + 0.2 * dt, t0 + 0.7 * dt, st[1, 2], t0 + 1.9 * dt, st[nsteps - 1, 1]])
    assert np.all(np.diff(T) > 0)
    return T


# per knot: factors on a flux or a Dirichlet water content, shifts of a Dirichlet temperature (a kink at knot 3)
SHAPE = {"flux": np.array([1.0, 3.0, 0.5, 2.0, 1.5, 0.8]), "dirichlet": np.array([1.0, 0.9, 1.05, 0.95, 1.0, 0.97]),
         "temperature": np.array([0.0, 2.0, -1.0, 3.0, 1.0, -2.0])}


def uniform_table(key, kind, value):
    """[nknots] values of one (face, component) whose lh_set_bc kind and value are given"""
    if kind == M.BC_FLUX:
        return value * SHAPE["flux"]
    assert kind == M.BC_DIRICHLET
    return value + SHAPE["temperature"] if key[1] == M.COMP_ENERGY else value * SHAPE["dirichlet"]


def uniform_values(om, keys):
    return {k: uniform_table(k, *om.bc[k]) for k in keys}


def percol_table(T, key, kind, value, ncols):
    """[nknots, ncols]: every column its own table -- the uniform one scaled and shifted in time (resampled at
    T - shift), column 1 constant in time and, for a flux, column 2 with a sign change between the knots 2 and 3."""
    u = uniform_table(key, kind, value)
    c = np.arange(ncols)
    shift = ((c * 5) % 11 - 5) * 0.13 * (T[-1] - T[0]) / 11.0
    out = np.stack([np.interp(T - shift[j], T, u) for j in range(ncols)], axis=1)
    m = (c * 7) % 13
    if kind == M.BC_FLUX:
        out = out * (0.4 + 0.1 * m)[None, :]
    elif key[1] == M.COMP_HYDROLOGY:        # a water content: stays inside the pore space
        out = out * (1.0 + 0.02 * (m - 6) / 6.0)[None, :]
    else:                                   # a temperature
        out = out + (0.25 * (m - 6))[None, :]
    if ncols > 1:
        out[:, 1] = u[0]
    if ncols > 2 and kind == M.BC_FLUX:
        out[3:, 2] = -out[3:, 2]
    return np.ascontiguousarray(out)


def percol_values(T, om, keys, ncols):
    return {k: percol_table(T, k, *om.bc[k], ncols) for k in keys}


def many_knots(dt, nknots=300, nsteps=NSTEPS):
    """`nknots` irregular knots around the `nsteps` steps of dt from start_time(dt), for the bisection of the wave's
    search (more than 65 knots): the first stage time lies in the FIRST interval, the last interval holds the third
    stage of the last step and ends ON the call's last stage time, everything between falls into intervals far above
    index 64, and one knot above index 64 IS the third stage time of step 2 (same arithmetic)."""
    t0 = start_time(dt)
    st = stage_times(t0, dt, nsteps)
    j = np.arange(nknots - 3)
    gaps = 0.25 + ((j * 7919) % 101) / 101.0                       # irregular, a ratio of 5 between neighbours at most
    inner = t0 + 0.3 * dt + (nsteps - 0.9) * dt * np.cumsum(gaps) / (gaps.sum() + 1.0)     # in (t0 + 0.3 dt, t0 + (nsteps - 0.6) dt)
    hit = int(np.argmin(np.abs(inner - st[2, 2])))
    inner[hit] = st[2, 2]
    T = np.concatenate([[t0 - 0.1 * dt], [t0 + 0.3 * dt], inner, [st[nsteps - 1, 1]]])
    assert len(T) == nknots and np.all(np.diff(T) > 0) and hit + 2 > 64 and T[hit + 2] == st[2, 2]
    assert T[-2] < st[nsteps - 1, 2] < T[-1] and T[0] < st[0, 0] < T[1]
    return T


def many_knot_values(value, nknots=300):
    """a flux table with a kink at every knot"""
    k = np.arange(nknots)
    return value * (0.5 + 2.0 * ((k * 6151) % 89) / 89.0)


# ------------------------------------------------------------------ the sampler against the definition


def brute_value(T, v, t):
    """The definition, by a scan: on a knot its value; otherwise the interval [T_k, T_k+1] that holds t (the last one
    for t = T_last) and the formula evaluated in double, operation by operation."""
    for k in range(len(T)):
        if t == T[k]:
            return float(v[k])
    k = max(j for j in range(len(T) - 1) if T[j] <= t)
    num = np.float64(t) - np.float64(T[k])
    den = np.float64(T[k + 1]) - np.float64(T[k])
    return float(np.float64(v[k]) + (np.float64(v[k + 1]) - np.float64(v[k])) * (num / den))


def test_the_knots_are_the_ones_the_issue_names():
    T, t0 = S.knots(DT), S.start_time(DT)
    st = S.stage_times(t0, DT, S.NSTEPS)
    interval = lambda t: min(int(np.searchsorted(T, t, side="right")) - 1, len(T) - 2)
    # a step spans two knots; a knot interval holds three whole steps; a stage time IS a knot, with a kink there
    assert np.sum((T > st[0, 0]) & (T < st[0, 1])) == 2
    assert [interval(st[k, 0]) == interval(st[k, 1]) == 4 for k in range(S.NSTEPS)] == [False, False, True, True, True]
    assert st[1, 2] == T[3] and st[-1, 1] == T[-1] and st[0, 0] > T[0]
    for shape in S.SHAPE.values():
        left = (shape[3] - shape[2]) / (T[3] - T[2])
        right = (shape[4] - shape[3]) / (T[4] - T[3])
        assert abs(left - right) > 0.1 * abs(left)
    # the stage times of a step are not monotone
    assert np.all(st[:, 2] < st[:, 1]) and np.all(st[:, 0] < st[:, 2])


def test_stage_times_are_formed_as_the_issue_states():
    t0 = S.start_time(DT)
    st = S.stage_times(t0, DT, S.NSTEPS)
    for k in range(S.NSTEPS):
        tk = t0 + DT * float(k)
        assert st[k, 0] == tk and st[k, 1] == tk + DT and st[k, 2] == tk + DT / 2
    np.testing.assert_array_equal(st, lh.soil._stage_times(t0, DT, S.NSTEPS))


@pytest.mark.parametrize("shape", sorted(S.SHAPE))
def test_sampler_against_the_brute_force_restatement(shape):
    T, t0 = S.knots(DT), S.start_time(DT)
    v = -2e-9 * S.SHAPE[shape]
    times = list(S.stage_times(t0, DT, S.NSTEPS).ravel()) + list(T) + [np.nextafter(x, d) for x in T[1:-1] for d in (-np.inf, np.inf)]
    for t in times:
        got, want = S.series_value(T, v, t), brute_value(T, v, t)
        assert got == want, (t, got, want)
        # ... and it is the piecewise-linear interpolant: within a few ulps of the exact rational value
        k = min(int(np.searchsorted(T, t, side="right")) - 1, len(T) - 2)
        exact = Fraction(v[k]) + (Fraction(v[k + 1]) - Fraction(v[k])) * (Fraction(t) - Fraction(T[k])) / (Fraction(T[k + 1]) - Fraction(T[k]))
        assert abs(Fraction(got) - exact) <= 4 * Fraction(np.spacing(np.abs(v).max()))
    assert S.series_value(T, v, T[3]) == v[3] and S.series_value(T, v, T[-1]) == v[-1] and S.series_value(T, v, T[0]) == v[0]
    # the mirror's BoundarySeries.value_at states the same rule
    fs = lh.BoundarySeries(T, {("top", "hydrology"): v})
    for t in times:
        assert fs.value_at(("top", "hydrology"), t) == S.series_value(T, v, t)


def test_many_knots_put_stage_times_where_the_waves_search_branches():
    T, t0 = S.many_knots(DT), S.start_time(DT)
    v = S.many_knot_values(-2e-9)
    st = S.stage_times(t0, DT, S.NSTEPS)
    interval = lambda t: min(int(np.searchsorted(T, t, side="right")) - 1, len(T) - 2)
    ks = sorted({interval(t) for t in st.ravel()})
    assert ks[0] == 0 and ks[-1] == len(T) - 2 and sum(64 < k < len(T) - 2 for k in ks) >= 4
    assert any(t == T[interval(t)] and interval(t) > 64 for t in st.ravel())      # a stage time ON a knot above index 64
    for t in st.ravel():
        assert S.series_value(T, v, t) == brute_value(T, v, t)


def test_sample_bcv_fills_the_existing_calls_table():
    T, t0 = S.knots(DT), S.start_time(DT)
    v = 0.34 * S.SHAPE["dirichlet"]
    bcv = S.sample_bcv(T, {S.TOP_H: v}, {S.TOP_H: 0.34, S.BOT_H: -2e-9}, t0, DT, S.NSTEPS)
    assert bcv.shape == (S.NSTEPS, 3, 2, 2)
    assert np.all(bcv[:, :, S.BOT_H[0], S.BOT_H[1]] == -2e-9) and np.all(bcv[:, :, :, 0] == 0.0)
    assert bcv[1, 2, S.TOP_H[0], S.TOP_H[1]] == v[3] and bcv[-1, 1, S.TOP_H[0], S.TOP_H[1]] == v[-1]


# ------------------------------------------------------------------ the host mirror, between the recorder's seams

def _series(dt=R.DT, t=R.T, nsteps=3):
    T = S.knots(dt, nsteps) - S.start_time(dt) + t
    return lh.BoundarySeries(T, {("top", "hydrology"): -2e-7 * S.SHAPE["flux"]})


def test_step_series_makes_one_call_behind_set_bcs():
    model, Y = R.make_model("richards"), R.StubState()
    fs = _series()
    rec = R.record(model, lambda: lh.step_series(model, Y, None, fs, R.T, R.DT, 3))
    assert "raises" not in rec, rec
    names = [e[1] if e[0] == "lib" else e[0] for e in rec["log"]]
    assert names == ["set_bcs", "lh_bc_series_create", "lh_bc_series_set", "lh_step_ssprk33_series"]
    assert rec["log"][0] == ["set_bcs", R.enc(R.T)]
    args = rec["log"][-1][2]
    assert args[0] == "ctx" and args[2] is None and args[4:] == [R.enc(R.T), R.enc(R.DT), 3]
    assert rec["returns"] == R.enc(R.T + 3 * R.DT)
    rec = R.record(model, lambda: lh.step_series_engine(model, 3))
    assert rec["log"] == [["lib", "lh_step_series_engine", ["ctx", 3]]] and rec["returns"] == 0


@pytest.mark.parametrize("kw, error, words", [
    (dict(series=None), TypeError, "step_series: series must be a BoundarySeries"),
    (dict(series=[0.0, 1.0]), TypeError, "step_series: series must be a BoundarySeries"),
    (dict(nsteps=-1), ValueError, "step_series: need nsteps >= 0 and dt > 0"),
    (dict(dt=0.0), ValueError, "step_series: need nsteps >= 0 and dt > 0"),
    (dict(dt=float("nan")), ValueError, "step_series: need nsteps >= 0 and dt > 0"),
    (dict(t=float("inf")), ValueError, "step_series: t is not finite"),
    (dict(t=R.T - R.DT), ValueError, "leaves the knots"),
    (dict(nsteps=4), ValueError, "leaves the knots"),
])
def test_step_series_checks_its_arguments_before_any_call(kw, error, words):
    model, Y = R.make_model("richards"), R.StubState()
    a = dict(series=_series(), t=R.T, dt=R.DT, nsteps=3)
    a.update(kw)
    rec = R.record(model, lambda: lh.step_series(model, Y, None, a["series"], a["t"], a["dt"], a["nsteps"]))
    assert rec["log"] == [] and rec["raises"][0] == error.__name__ and words in rec["raises"][1], rec


def test_step_series_with_no_steps_checks_no_span():
    model, Y = R.make_model("richards"), R.StubState()
    rec = R.record(model, lambda: lh.step_series(model, Y, None, _series(), R.T - 100.0, R.DT, 0))
    assert rec["log"][-1][1] == "lh_step_ssprk33_series" and rec["log"][-1][2][-1] == 0


def test_the_marker_takes_a_series_only_and_advances_by_one_call_per_chunk():
    for bad in (None, 3.0, {("top", "hydrology"): [1.0]}):
        with pytest.raises(TypeError, match="SeriesSSPRK33: forcing must be a BoundarySeries"):
            lh.SeriesSSPRK33(forcing=bad)
    fs = _series(nsteps=7)
    m = lh.SeriesSSPRK33(forcing=fs)
    assert isinstance(m, lh.SSPRK33) and m.forcing is fs
    for flavour in ("dirichlet", "flux"):      # (a closure on the series' component is not sampled: the series wins)
        model = R.make_model("richards", dirichlet=flavour == "dirichlet")
        m.check_scope(model)
        it = types.SimpleNamespace(u=R.StubState(), p=None, t=R.T, t0=R.T, tf=R.T + 7 * R.DT, dt=R.DT, _nsteps_done=0)
        sim = types.SimpleNamespace(integrator=it, method=m, model=model)
        for n in (3, 3, 1):
            rec = R.record(model, lambda: m.advance(sim, n))
            assert "raises" not in rec, rec
            calls = [e for e in rec["log"] if e[0] == "set_bcs" or e[1].startswith("lh_step")]
            assert [c[0] if c[0] == "set_bcs" else c[1] for c in calls] == ["set_bcs", "lh_step_ssprk33_series"]
            assert calls[0][1] == R.enc(it.t) and calls[1][2][4:] == [R.enc(it.t), R.enc(R.DT), n]
            it.t = float.fromhex(rec["returns"])
            it._nsteps_done += n
    # SSPRK33 itself is what it was: no parameters, no attributes, lh_step_ssprk33
    assert vars(lh.SSPRK33()) == {}
    with pytest.raises(TypeError):
        lh.SSPRK33(forcing=fs)
