"""What the host mirror's integrator block (soil.py, the method markers through _advance_trbdf2) does at its two seams,
without a device and without the library: a transcript of every scope refusal, of every call that reaches the library
(entry point and arguments, floats by their bits) or the backend's set_bcs, of every return value, of the markers'
constructors and of their advance.  tests/golden/host_mirror/make_transcript.py writes it to the fixture;
tests/test_host_mirror_contract_cpu.py regenerates it and compares entry by entry.

The seams: soil.F.lib is replaced by a function that returns a RecordingLib, and a model's _backend by a function that
returns a StubBackend.  Besides them the recorder uses the package's exported names only.  _advance_trbdf2 makes its
per-column step buffer with torch.zeros on the context's device and _dt_cols_pointer synchronises that device: these
two torch functions are replaced by stand-ins while a run is between the seams, since there is no device here."""
import contextlib
import ctypes as C
import inspect
import types

import numpy as np

import __graft_entry__ as g

lh = g.load_package()
F = lh._ffi            # (soil.F is this module)
FT = np.float64
NLEV, NCOLS = 4, 3
DOUBLE_P = C.POINTER(C.c_double)

# ------------------------------------------------------------------------------------------------- encoding


class Tables:
    """Every distinct table of doubles once; an entry names it by its index."""

    def __init__(self):
        self.rows, self.index = [], {}

    def add(self, values):
        row = tuple(float(v).hex() for v in values)
        if row not in self.index:
            self.index[row] = len(self.rows)
            self.rows.append(list(row))
        return {"table": self.index[row]}


TABLES = Tables()


def enc(x):
    """JSON form of a value: floats by their bits (float.hex), None as None, tuples as lists."""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, C.c_void_p):
        return {"ptr": x.value}
    if isinstance(x, (StubState, FakeDeviceTensor, lh.BoundarySeries)):
        return repr(x) if not isinstance(x, lh.BoundarySeries) else "<series>"
    if isinstance(x, (tuple, list)):
        return [enc(v) for v in x]
    if isinstance(x, dict):
        return {str(k): enc(v) for k, v in x.items()}
    raise TypeError(f"the recorder cannot encode {type(x).__name__}")


# ---------------------------------------------------------------------------------------------------- seams

# doubles behind the one double pointer of an entry point, from its contract (a: the call's arguments)
TABLE_LENGTH = {
    "lh_step_implicit_euler": lambda a: 4 * a[5],
    "lh_step_layered_implicit_euler": lambda a: 4 * a[5],
    "lh_step_heat_implicit": lambda a: 4 * (a[5] + 1),
    "lh_step_layered_heat_implicit": lambda a: 4 * (a[5] + 1),
    "lh_step_coupled_implicit": lambda a: 4 * (a[5] + 1),
    "lh_step_layered_coupled_implicit": lambda a: 4 * (a[5] + 1),
    "lh_step_ssprk33": lambda a: 12 * a[5],
    "lh_integrate_trbdf2": lambda a: 8,
    "lh_integrate_layered_trbdf2": lambda a: 8,
    "lh_integrate_coupled_trbdf2": lambda a: 8,
    "lh_integrate_layered_coupled_trbdf2": lambda a: 8,
    "lh_integrate_heat_trbdf2": lambda a: 8,
    "lh_integrate_layered_heat_trbdf2": lambda a: 8,
    "lh_integrate_dense": lambda a: a[12],            # the save times
    "lh_bc_series_create": lambda a: a[1],            # the knots
}


class RecordingLib:
    """Stands for the library: every entry point records (name, arguments) and returns LH_OK.  The two statistics
    read-backs and lh_bc_series_create fill their outputs with numbers that differ from call to call."""

    def __init__(self, log):
        self.log = log
        self.outputs = 0
        self.nknots = {}

    def __getattr__(self, name):
        def entry(*args):
            self.log.append(["lib", name, [self._arg(name, args, k) for k in range(len(args))]])
            if name == "lh_bc_series_create":     # (lh_bc_series_set's values have one entry per knot)
                self.nknots[args[3]._obj.value] = args[1]
            return F.LH_OK
        return entry

    def _arg(self, name, args, k):
        a = args[k]
        if isinstance(a, DOUBLE_P):
            if name == "lh_bc_series_set":
                n = self.nknots[args[1].value]
            else:
                n = TABLE_LENGTH[name](args)
            return TABLES.add(a[i] for i in range(n))
        if type(a).__name__ == "CArgObject":      # C.byref(x): an output
            return self._output(name, a._obj)
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:            # the snapshots' handles
                return [v for v in a]
            return self._output(name, a)
        return enc(a)

    def _output(self, name, obj):
        self.outputs += 1
        if isinstance(obj, C.Array):              # lh_trbdf2_stats
            for i in range(len(obj)):
                obj[i] = (i + 1) * self.outputs
            return "<out %d>" % len(obj)
        if name == "lh_bc_series_create":
            obj.value = 0xB000 + self.outputs
            return "<out series>"
        obj.value = 3 + self.outputs              # lh_implicit_stats
        return "<out>"


class StubBackend:
    """Stands for soil._Backend: a context, the model kind, and a set_bcs that records its time."""

    def __init__(self, model, log):
        self.ctx = "ctx"
        self.log = log
        em, hm = model.energy_model, model.hydrology_model
        if isinstance(em, lh.SoilEnergyModel):
            self.kind = F.LH_MODEL_COUPLED if isinstance(hm, lh.SoilHydrologyModel) else F.LH_MODEL_HEAT
        else:
            self.kind = F.LH_MODEL_RICHARDS

    def set_bcs(self, model, t):
        self.log.append(["set_bcs", enc(t)])

    def device_index(self):
        return 0


class StubState:
    """Stands for a FieldVector: a handle, and similar() for the snapshots of integrate_dense."""

    def __init__(self, number=0xA000):
        self.handle = C.c_void_p(number)
        self.made = 0

    def similar(self):
        self.made += 1
        return StubState(self.handle.value + self.made)

    def __repr__(self):
        return "<state %#x>" % self.handle.value


class FakeDeviceTensor:
    """What _dt_cols_pointer asks of a device tensor."""
    is_cuda = True

    def __init__(self, n, dtype):
        import torch
        self.n, self.dtype, self.device = n, dtype, torch.device("cuda", 0)

    def numel(self):
        return self.n

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0xD000

    def __repr__(self):
        return "<device tensor %d>" % self.n


@contextlib.contextmanager
def no_device():
    import torch
    zeros, sync = torch.zeros, torch.cuda.synchronize
    torch.zeros = lambda n, dtype=None, device=None: FakeDeviceTensor(n, dtype)
    torch.cuda.synchronize = lambda device=None: None
    try:
        yield
    finally:
        torch.zeros, torch.cuda.synchronize = zeros, sync


@contextlib.contextmanager
def seams(model, log):
    """The two seams around one run; a fresh library and backend stub each time."""
    lib, be = RecordingLib(log), StubBackend(model, log)
    saved = F.lib
    F.lib = lambda: lib
    model._backend = lambda: be
    try:
        with no_device():
            yield
    finally:
        F.lib = saved
        del model._backend


def record(model, fn):
    """fn() between the seams: {"raises": [type, message]} or {"log": [...], "returns": value}."""
    log = []
    with seams(model, log):
        try:
            out = fn()
        except Exception as e:   # noqa: BLE001  (the exception IS the result)
            return {"log": log, "raises": [type(e).__name__, str(e)]}
    return {"log": log, "returns": enc(out)}


# ------------------------------------------------------------------------------------------- the model matrix


# Dirichlet closures whose value moves with the last bit of t (arithmetic only: the same bits everywhere)
def vl_of(t):
    return 0.3 + t / 7.0


def T_of(t):
    return 280.0 + t / 3.0


def _component_bc(family, which, dirichlet):
    water, heat = family != "heat", family != "richards"
    if dirichlet:
        en = lh.Dirichlet(T_of) if heat else None
        hy = lh.Dirichlet(vl_of) if water else None
        if which == "bottom" and family == "coupled":
            hy = lh.VerticalFlux(-1e-7)          # (a flux next to closures: sampled at the base time only)
    else:
        en = lh.VerticalFlux(12.5 if which == "top" else 0.0) if heat else None
        hy = (lh.VerticalFlux(-2e-7) if which == "top" else lh.FreeDrainage()) if water else None
    return lh.SoilComponentBC(energy=en, hydrology=hy)


def _classes():
    def one(n, nu):
        return lh.SoilClass(FT, hydraulic_model=lh.vanGenuchten(FT, n=n, alpha=2.0, Ksat=1e-6, theta_r=0.02), nu=nu, S_s=1e-3,
                            thermal=lh.SoilThermal(FT))
    return lh.SoilClasses([one(2.0, 0.4), one(1.4, 0.5)], [0, 0, 1, 1])


FAMILIES = ("richards", "heat", "coupled")
FACTORS = ("noeffect", "viscosity", "impedance")


def make_model(family, classes=False, factor="noeffect", atmos=False, dirichlet=False):
    energy = lh.PrescribedTemperatureModel() if family == "richards" else lh.SoilEnergyModel()
    if family == "heat":
        hydrology = lh.PrescribedHydrologyModel()
    else:
        hydrology = lh.SoilHydrologyModel(
            FT, viscosity_factor=lh.TemperatureDependentViscosity(FT) if factor == "viscosity" else None,
            impedance_factor=lh.IceImpedance(FT) if factor == "impedance" else None)
    top = _component_bc(family, "top", dirichlet)
    if atmos:
        top = lh.PrescribedAtmosForcing(FT, u_atm=2.0, theta_atm=290.0, z_atm=2.0, theta_scale=290.0, rho_a_sfc=1.2,
                                        q_atm=0.005)
    bcs = lh.SoilColumnBC(top=top, bottom=_component_bc(family, "bottom", dirichlet))
    # (SoilModel refuses soil classes under an atmosphere top when it is built; the integrators' own order of refusals
    # is what is recorded, so the class map is attached afterwards there)
    model = lh.SoilModel(FT, domain=lh.Column(FT, zlim=(-1.0, 0.0), nelements=NLEV, ncolumns=NCOLS), energy_model=energy,
                         hydrology_model=hydrology, boundary_conditions=bcs, earth_param_set=lh.EarthParameterSet(),
                         soil_classes=_classes() if classes and not atmos else None)
    if classes and atmos:
        model.soil_classes = _classes()
    return model


def matrix():
    """name -> keyword arguments of make_model, without the boundary-condition flavour"""
    out = {}
    for family in FAMILIES:
        for classes in (False, True):
            for factor in (FACTORS if family != "heat" else FACTORS[:1]):
                for atmos in (False, True):
                    name = "%s/%s/%s/%s" % (family, "classes" if classes else "one-soil", factor, "atmos" if atmos else "plain")
                    out[name] = dict(family=family, classes=classes, factor=factor, atmos=atmos)
    return out


MARKERS = ("SSPRK33", "ImplicitEuler", "TRBDF2", "LayeredImplicitEuler", "LayeredTRBDF2", "HeatImplicitEuler", "HeatTRBDF2",
           "LayeredHeatImplicitEuler", "LayeredHeatTRBDF2", "HeatAdaptiveTRBDF2", "LayeredHeatAdaptiveTRBDF2",
           "HeatSeriesTRBDF2", "LayeredHeatSeriesTRBDF2", "CoupledImplicitEuler", "CoupledTRBDF2",
           "LayeredCoupledImplicitEuler", "LayeredCoupledTRBDF2", "CoupledAdaptiveTRBDF2", "LayeredCoupledAdaptiveTRBDF2",
           "LayeredCoupledSeriesTRBDF2")
SERIES_MARKERS = ("HeatSeriesTRBDF2", "LayeredHeatSeriesTRBDF2", "LayeredCoupledSeriesTRBDF2")


def series(family="richards"):
    key = ("top", "energy") if family == "heat" else ("top", "hydrology")
    return lh.BoundarySeries([0.0, 0.5, 2.0], {key: [0.25, 0.375, 0.3125], ("bottom", "energy"): [280.0, 281.5, 279.25]})


def make_marker(name, forcing=None, **kw):
    cls = getattr(lh, name)
    if name in SERIES_MARKERS or forcing is not None:
        return cls(forcing=forcing, **kw)
    return cls(**kw)


# ---------------------------------------------------------------------------------------------------- scope


def record_scope(out):
    for mname, kw in matrix().items():
        for marker in MARKERS:
            model = make_model(**kw)
            m = make_marker(marker, series(kw["family"]) if marker in SERIES_MARKERS else None)
            out["scope|%s|%s" % (marker, mname)] = record(model, lambda: m.check_scope(model))


# ---------------------------------------------------------------------------------------------------- calls

T, DT = 0.3, 0.1
T0, T1 = 0.3, 1.1

FIXED = {   # name -> (has method, has tol / max_iter)
    "step_implicit": (False, True), "step_implicit_layered": (False, True),
    "step_implicit_heat": (True, False), "step_implicit_layered_heat": (True, False),
    "step_implicit_coupled": (True, True), "step_implicit_layered_coupled": (True, True),
}
ADAPTIVE = {   # name -> the keyword arguments it has besides dt_cols
    "integrate_trbdf2": ("abstol", "reltol", "adaptive"), "integrate_layered_trbdf2": ("abstol", "reltol", "adaptive"),
    "integrate_heat_trbdf2": ("abstol_e", "reltol"), "integrate_layered_heat_trbdf2": ("abstol_e", "reltol"),
    "integrate_coupled_trbdf2": ("abstol", "abstol_e", "reltol"),
    "integrate_layered_coupled_trbdf2": ("abstol", "abstol_e", "reltol"),
}
SERIES = {
    "integrate_series": ("abstol", "abstol_e", "reltol", "adaptive"), "integrate_heat_series": ("abstol_e", "reltol"),
    "integrate_layered_coupled_series": ("abstol", "abstol_e", "reltol"),
    "integrate_dense": ("abstol", "abstol_e", "reltol", "adaptive"),
}
EXPLICIT = {"abstol": 1e-8, "abstol_e": 2.5, "reltol": 1e-5}
SAVEAT = {
    "saveat=[]": [], "saveat=one": [0.7], "saveat=ends": [T0, 0.55, T1], "saveat=2d": [[0.4, 0.5]],
    "saveat=65537": np.arange(65537.0), "saveat=nan": [0.4, float("nan")], "saveat=inf": [float("inf")],
    "saveat=equal": [0.4, 0.4], "saveat=back": [0.5, 0.4], "saveat=before": [0.2, 0.4], "saveat=after": [0.4, 1.2],
}


def _tolerance_variants(names):
    """each tolerance in {None, 0.0, an explicit value} and `adaptive` in {True, False}, one at a time"""
    out = {}
    for n in names:
        if n == "adaptive":
            out["adaptive=False"] = dict(adaptive=False)
        else:
            for v in (None, 0.0, EXPLICIT[n]):
                out["%s=%r" % (n, v)] = {n: v}
    return out


def _dt_cols_variants():
    import torch
    return {"dt_cols=cpu": dict(dt_cols=torch.zeros(NCOLS, dtype=torch.float64)),
            "dt_cols=device": dict(dt_cols=FakeDeviceTensor(NCOLS, torch.float64)),
            "dt_cols=device-f32": dict(dt_cols=FakeDeviceTensor(NCOLS, torch.float32)),
            "dt_cols=device-short": dict(dt_cols=FakeDeviceTensor(NCOLS - 1, torch.float64))}


def call_cases(family):
    """[(function name, variant name, callable(model, Y))]: the default call of every function and its variants"""
    cases = []

    def add(name, variant, *args, **kw):
        cases.append((name, variant, lambda model, Y: getattr(lh, name)(model, Y, None, *args, **kw)))

    for name, (has_method, has_tol) in FIXED.items():
        add(name, "default", T, DT, 3)
        add(name, "signature-defaults")
        for n in (0, 1):
            add(name, "nsteps=%d" % n, T, DT, n)
        if has_method:
            for m in ("euler", "trbdf2", "bogus"):
                add(name, "method=" + m, T, DT, 3, method=m)
        if has_tol:
            for v in (0.0, 1e-9):
                add(name, "tol=%r" % v, T, DT, 3, tol=v)
            for v in (0, 7):
                add(name, "max_iter=%r" % v, T, DT, 3, max_iter=v)
    for name, names in ADAPTIVE.items():
        add(name, "default", T0, T1, DT)
        add(name, "signature-defaults")
        for variant, kw in {**_tolerance_variants(names), **_dt_cols_variants()}.items():
            add(name, variant, T0, T1, DT, **kw)
    fs = series(family)
    for name, names in SERIES.items():
        if name == "integrate_dense":
            def add_s(variant, s, t0=T0, t1=T1, saveat=(0.4, 0.9), **kw):
                add(name, variant, t0, t1, DT, saveat, s, **kw)
            for variant, s in SAVEAT.items():
                add_s(variant, fs, saveat=s)
                add_s(variant + ",series=None", None, saveat=s)
        else:
            def add_s(variant, s, t0=T0, t1=T1, **kw):
                add(name, variant, s, t0, t1, DT, **kw)
        add_s("default", fs)
        add_s("series=None", None)
        add_s("series=list", [0.0, 1.0])
        add_s("span-before", fs, t0=-0.5)
        add_s("span-after", fs, t1=2.5)
        for variant, kw in {**_tolerance_variants(names), **_dt_cols_variants()}.items():
            add_s(variant, fs, **kw)
    return cases


def record_calls(out):
    """The default call of every function on every model of the matrix, with and without Dirichlet closures; every
    variant on the models without factors and with a plain top (both boundary flavours, with and without soil classes:
    a variant that ends in a scope refusal shows what is checked before the scope)."""
    for mname, kw in matrix().items():
        everything = kw["factor"] == "noeffect" and not kw["atmos"]
        for flavour in ("dirichlet", "flux"):
            for name, variant, fn in call_cases(kw["family"]):
                if variant != "default" and not everything:
                    continue
                model, Y = make_model(dirichlet=flavour == "dirichlet", **kw), StubState()
                out["call|%s|%s|%s/%s" % (name, variant, mname, flavour)] = record(model, lambda: fn(model, Y))


# -------------------------------------------------------------------------------------------------- markers


def _explicit_arguments(cls, fs):
    sig = inspect.signature(cls)
    special = {"adaptive": False, "forcing": fs, "max_iter": 9}
    return {p: special.get(p, 1e-7 * (k + 1)) for k, p in enumerate(sig.parameters)}


def _attributes(m):
    return {"vars": enc(vars(m)), "method": getattr(m, "method", None),
            "hooks": [h for h in ("check_scope", "advance", "integrate", "integrate_forcing", "step") if hasattr(m, h)]}


def record_markers(out):
    fs = series()
    for name in MARKERS:
        cls = getattr(lh, name)
        kw = _explicit_arguments(cls, fs)
        rec = {"signature": str(inspect.signature(cls)), "mro": [k.__name__ for k in cls.__mro__],
               "default": _attributes(make_marker(name, fs if name in SERIES_MARKERS else None)),
               "explicit": _attributes(cls(**kw)), "positional": _attributes(cls(*kw.values()))}
        if name in SERIES_MARKERS:
            try:
                cls()
                rec["no forcing"] = "passes"
            except TypeError as e:   # (the interpreter's own words for a missing argument are not the project's)
                rec["no forcing"] = type(e).__name__
            for label, bad in (("None", None), ("number", 3.0), ("dict", {("top", "energy"): [1.0]})):
                try:
                    cls(forcing=bad)
                    rec["forcing=" + label] = "passes"
                except Exception as e:   # noqa: BLE001
                    rec["forcing=" + label] = [type(e).__name__, str(e)]
        out["marker|" + name] = rec


# -------------------------------------------------------------------------------------------------- advance

CHUNK, TOTAL = 3, 7


def _family_of(marker):
    return "heat" if "Heat" in marker else "coupled" if "Coupled" in marker else "richards"


def record_advance(out):
    """marker.advance(sim, nsteps) on a stub sim with it.p = None over a first chunk, a middle chunk and the chunk that
    reaches tf (3 + 3 + 1 intervals of dt), the step count and the time kept as Simulation's driver keeps them."""
    for marker in MARKERS:
        family = _family_of(marker)
        takes = "forcing" in inspect.signature(getattr(lh, marker)).parameters
        forcings = [True] if marker in SERIES_MARKERS else [False, True] if takes else [False]
        for forced in forcings:
            for flavour in ("dirichlet", "flux"):
                model = make_model(family, classes=marker.startswith("Layered"), dirichlet=flavour == "dirichlet")
                m = make_marker(marker, series(family) if forced else None)
                it = types.SimpleNamespace(u=StubState(), p=None, t=T, t0=T, tf=T + TOTAL * DT, dt=DT, _nsteps_done=0)
                sim = types.SimpleNamespace(integrator=it, method=m, model=model)
                done, chunk = 0, 0
                while done < TOTAL:
                    n = min(CHUNK, TOTAL - done)
                    rec = record(model, lambda: m.advance(sim, n))
                    if "returns" in rec:
                        t = rec["returns"]
                        it._nsteps_done += n
                        it.t = it.t + n * it.dt if t is None else float.fromhex(t)
                    rec["t"] = enc(it.t)
                    rec["trbdf2_stats"] = enc(getattr(it, "trbdf2_stats", None))
                    rec["implicit_stats"] = enc(getattr(it, "implicit_stats", None))
                    out["advance|%s|%s|%s|chunk %d" % (marker, "forcing" if forced else "no forcing", flavour, chunk)] = rec
                    done += n
                    chunk += 1


def transcript():
    """{key: entry} and the tables the entries name"""
    global TABLES
    TABLES = Tables()
    out = {}
    record_scope(out)
    record_calls(out)
    record_markers(out)
    record_advance(out)
    return out, TABLES.rows
