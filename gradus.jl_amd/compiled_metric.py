"""A user's `metric_components(r, θ)` compiled into kernels of its own (GR_METRIC_COMPILED).

`TabulatedMetric` carries a metric to the device as samples; `CompiledMetric` carries it as code.  The callable runs ONCE on a
recording scalar; what it did becomes straight-line C++ on the typed dual numbers of csrc/gr_device.hpp -- the body of
`GenericMetricT<12>::components` (csrc/gr_usermetric.hpp) -- and `hipcc` builds the library's own kernels_tu.hip around it: the
fp64 set, the area factor, both tangent shapes, both sky-cell shapes and the offset solve, linked into one shared module that
the library loads at run time (gr_metric_module_load).  The reference does the same through ForwardDiff
(src/tracing/method-implementations/auto-diff.jl:206-211): there a user's metric costs what a catalogue metric costs.

No fit, no radial range, no table.  A metric with branches cannot be traced this way and keeps the table.
"""
from __future__ import annotations

import ctypes
import hashlib
import inspect
import math
import os
import subprocess

import numpy as np

from .metrics import AbstractMetric, AbstractStaticAxisSymmetric

GR_METRIC_COMPILED = 12


class UntraceableMetric(TypeError):
    """The callable did something a straight-line component function cannot express."""

    def __init__(self, what):
        super().__init__(f"{what}.  A compiled metric is straight-line arithmetic in r, sin θ and cos θ (+ - * /, integer powers, "
                         "np.sqrt / np.exp / np.log, np.sin(θ) / np.cos(θ) of θ itself): trace this metric through "
                         "TabulatedMetric instead, and name the radii where a piecewise metric changes form in its `breaks`")


# ---------------------------------------------------------------------------------------------------------------------------
# the recording scalar
# ---------------------------------------------------------------------------------------------------------------------------
class _Graph:
    """Hash-consed expression DAG: node = (op, args...); equal sub-expressions are one node.  Nothing is reordered or
    simplified beyond folding operations on two literals: the generated code rounds in the order the callable wrote."""

    def __init__(self):
        self.nodes = []          # (op, *args)
        self.index = {}

    def add(self, op, *args):
        key = (op,) + args
        i = self.index.get(key)
        if i is None:
            i = len(self.nodes)
            self.nodes.append(key)
            self.index[key] = i
        return i

    def const(self, x):
        x = float(x)
        if not math.isfinite(x):
            raise UntraceableMetric(f"the callable produced the constant {x!r}")
        return self.add("const", x.hex())        # (the hex form keeps -0.0 and every bit)


_UFUNCS = {np.add: "add", np.subtract: "sub", np.multiply: "mul", np.true_divide: "div", np.negative: "neg", np.positive: "pos",
           np.sqrt: "sqrt", np.exp: "exp", np.log: "log", np.sin: "sin", np.cos: "cos", np.power: "pow", np.square: "square",
           np.reciprocal: "recip"}


class _Sym:
    """One value of the recording: a node of the graph.  Arithmetic records; anything that would need the VALUE refuses."""

    __slots__ = ("g", "i")
    __array_priority__ = 1000.0

    def __init__(self, g, i):
        self.g, self.i = g, i

    # -- lifting --
    def _lift(self, o):
        if isinstance(o, _Sym):
            if o.g is not self.g:
                raise UntraceableMetric("the callable mixed values of two different traces")
            return o
        if isinstance(o, (bool, np.bool_)):
            raise UntraceableMetric("the callable used a truth value as a number (a branch)")
        if isinstance(o, (int, float, np.integer, np.floating)):
            return _Sym(self.g, self.g.const(o))
        if isinstance(o, np.ndarray) and o.ndim == 0:
            return self._lift(o.item())
        raise UntraceableMetric(f"the callable combined a metric value with a {type(o).__name__}")

    def _is_const(self):
        return self.g.nodes[self.i][0] == "const"

    def _value(self):
        return float.fromhex(self.g.nodes[self.i][1])

    def _bin(self, op, a, b):
        a, b = self._lift(a), self._lift(b)
        if a._is_const() and b._is_const():
            x, y = a._value(), b._value()
            return _Sym(self.g, self.g.const({"add": x + y, "sub": x - y, "mul": x * y}[op] if op != "div" else x / y))
        return _Sym(self.g, self.g.add(op, a.i, b.i))

    def _un(self, op):
        return _Sym(self.g, self.g.add(op, self.i))

    def __add__(self, o): return self._bin("add", self, o)
    def __radd__(self, o): return self._bin("add", o, self)
    def __sub__(self, o): return self._bin("sub", self, o)
    def __rsub__(self, o): return self._bin("sub", o, self)
    def __mul__(self, o): return self._bin("mul", self, o)
    def __rmul__(self, o): return self._bin("mul", o, self)
    def __truediv__(self, o): return self._bin("div", self, o)
    def __rtruediv__(self, o): return self._bin("div", o, self)
    def __neg__(self): return self._un("neg")
    def __pos__(self): return self

    def __pow__(self, n):
        if isinstance(n, (float, np.floating)) and float(n) == int(n):
            n = int(n)
        if isinstance(n, _Sym) or not isinstance(n, (int, np.integer)) or isinstance(n, (bool, np.bool_)):
            raise UntraceableMetric("the callable raised a value to a power that is not an integer literal (write np.sqrt, or "
                                    "np.exp(p * np.log(x)))")
        n = int(n)
        if n == 0:
            return _Sym(self.g, self.g.const(1.0))
        base = self if abs(n) == 1 else _Sym(self.g, self.g.add("powi", self.i, abs(n)))
        return base if n > 0 else self._bin("div", 1.0, base)

    def __rpow__(self, o):
        raise UntraceableMetric("the callable raised a number to a power that depends on the coordinates (write np.exp(x * log(b)))")

    # -- the functions of the list --
    def sqrt(self): return self._fn("sqrt")
    def exp(self): return self._fn("exp")
    def log(self): return self._fn("log")

    def _fn(self, op):
        if self.g.nodes[self.i][0] == "theta":
            raise UntraceableMetric(f"the callable took {op} of θ itself: θ enters a compiled metric through np.sin(θ) and np.cos(θ) only")
        return self._un(op)

    def sin(self): return self._trig("sin")
    def cos(self): return self._trig("cos")

    def _trig(self, op):
        if self.g.nodes[self.i][0] != "theta":
            raise UntraceableMetric(f"the callable took np.{op} of something other than θ")
        return _Sym(self.g, self.g.add(op + "_theta"))

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        op = _UFUNCS.get(ufunc)
        if method != "__call__" or kwargs or op is None:
            raise UntraceableMetric(f"the callable called np.{getattr(ufunc, '__name__', ufunc)}, which a compiled metric does not have")
        if op in ("add", "sub", "mul", "div"):
            return self._bin(op, inputs[0], inputs[1])
        if op == "pow":
            if not isinstance(inputs[0], _Sym):
                return self.__rpow__(inputs[0])
            return inputs[0] ** inputs[1]
        x = inputs[0]
        return {"neg": x.__neg__, "pos": x.__pos__, "sqrt": x.sqrt, "exp": x.exp, "log": x.log, "sin": x.sin, "cos": x.cos,
                "square": lambda: x * x, "recip": lambda: 1.0 / x}[op]()

    # -- what needs the value --
    def __bool__(self):
        raise UntraceableMetric("the callable took the truth value of a metric value (an `if`, `and`, `or`, `max` or `abs`: a branch)")

    def _cmp(self, o):
        raise UntraceableMetric("the callable compared a metric value (a branch)")

    __lt__ = __le__ = __gt__ = __ge__ = __eq__ = __ne__ = _cmp
    __hash__ = None

    def __float__(self):
        raise UntraceableMetric("the callable asked for the numerical value of a coordinate (math.sin and friends, float(), an index): "
                                "use the numpy functions")

    __int__ = __index__ = __float__

    def __abs__(self):
        raise UntraceableMetric("the callable took an absolute value (a branch)")

    def __getattr__(self, name):
        # np.tanh(x) on an object looks for x.tanh(); anything else a callable might ask of a float
        if name.startswith("__"):
            raise AttributeError(name)
        raise UntraceableMetric(f"the callable called `{name}` on a metric value, which a compiled metric does not have")


def _positional_arity(f):
    try:
        ps = [p for p in inspect.signature(f).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        var = any(p.kind == p.VAR_POSITIONAL for p in inspect.signature(f).parameters.values())
    except (TypeError, ValueError):
        return 2
    return 3 if (len(ps) >= 3 or var) else 2


class Trace:
    """The recorded component function: `source` (the generated C++ body), `sha256`, and `evaluate(r, s, c, params)` -- the same
    graph on floats, numpy arrays or special_radii.Jet, which is where the host-side quantities (ISCO, redshift, tetrads) come from."""

    def __init__(self, f, n_params=0, from_rsc=False):
        if n_params > 6:
            raise ValueError("a compiled metric has at most 6 run-time parameters (gr_config.params[0..5])")
        g = _Graph()
        r = _Sym(g, g.add("r"))
        if from_rsc:
            # a catalogue metric's own formula takes (r, sin θ, cos θ)
            out = f(r, _Sym(g, g.add("sin_theta")), _Sym(g, g.add("cos_theta")))
        else:
            th = _Sym(g, g.add("theta"))
            if n_params and _positional_arity(f) >= 3:
                out = f(r, th, tuple(_Sym(g, g.add("param", k)) for k in range(n_params)))
            else:
                out = f(r, th)
        try:
            out = tuple(out)
        except TypeError:
            out = None
        if out is None or len(out) != 5:
            raise UntraceableMetric("the callable must return the five components (g_tt, g_rr, g_θθ, g_ϕϕ, g_tϕ)"
                                    + (f", it returned {len(out)} values" if out is not None else ""))
        r0 = _Sym(g, 0)
        self.graph = g
        self.outputs = [r0._lift(o).i for o in out]
        for i in self.outputs:
            if g.nodes[i][0] == "theta":
                raise UntraceableMetric("a component is θ itself: θ enters a compiled metric through np.sin(θ) and np.cos(θ) only")
        self.n_params = int(n_params)
        self.source = self._emit()
        self.sha256 = hashlib.sha256(self.source.encode()).hexdigest()

    # reachable nodes in creation order (a node's arguments are always older than the node)
    def _live(self):
        g = self.graph
        live, stack = set(), list(self.outputs)
        while stack:
            i = stack.pop()
            if i in live:
                continue
            live.add(i)
            n = g.nodes[i]
            stack.extend(a for a in (n[1:3] if n[0] in ("add", "sub", "mul", "div") else n[1:2] if n[0] in ("neg", "sqrt", "exp", "log", "powi") else ()))
        return sorted(live)

    def _coord_dependent(self, live):
        dep = {}
        for i in live:
            n = self.graph.nodes[i]
            if n[0] in ("r", "sin_theta", "cos_theta", "theta"):
                dep[i] = True
            elif n[0] in ("const", "param"):
                dep[i] = False
            elif n[0] == "powi":
                dep[i] = dep[n[1]]
            else:
                dep[i] = any(dep[a] for a in n[1:])
        return dep

    def _emit(self):
        g = self.graph
        live = self._live()
        dep = self._coord_dependent(live)
        name = {}
        lines = ["// generated by gradus_jl_amd.compiled_metric: the body of GenericMetricT<12>::components(r, s, c, g)"]

        def lit(h):
            t = "%.17g" % float.fromhex(h)
            return t if any(ch in t for ch in ".en") else t + ".0"

        def ref(i):
            n = g.nodes[i]
            if n[0] == "const":
                x = lit(n[1])
                return f"({x})" if x.startswith("-") else x
            return name[i]

        for i in live:
            n = g.nodes[i]
            op = n[0]
            if op == "const":
                continue
            if op == "theta":
                raise UntraceableMetric("the callable used θ outside np.sin(θ) and np.cos(θ)")
            if op in ("r", "sin_theta", "cos_theta"):
                name[i] = {"r": "r", "sin_theta": "s", "cos_theta": "c"}[op]
                continue
            if op == "param":
                name[i] = f"p{n[1]}"
                lines.append(f"const real p{n[1]} = P[{n[1]}];")
                continue
            t = f"t{i}"
            name[i] = t
            if op in ("add", "sub", "mul"):
                expr = f"{ref(n[1])} {'+-*'[('add', 'sub', 'mul').index(op)]} {ref(n[2])}"
            elif op == "div":
                num = ref(n[1])
                expr = f"inv_({ref(n[2])})" if (g.nodes[n[1]][0] == "const" and float.fromhex(g.nodes[n[1]][1]) == 1.0) else f"{num} * inv_({ref(n[2])})"
            elif op == "neg":
                expr = f"-{ref(n[1])}"
            elif op == "powi":
                expr = f"dpowi<{n[2]}>({ref(n[1])})"
            else:
                expr = f"d{op}({ref(n[1])})"
            # a sub-expression of parameters and literals alone is a plain number (a literal operand would otherwise make it a double)
            lines.append(f"const auto {t} = {expr};" if dep[i] else f"const real {t} = {expr};")
        for k, i in enumerate(self.outputs):
            # a component that depends on neither coordinate: (r - r) + k, as the catalogue's flat space writes it
            lines.append(f"dput(g[{k}], {ref(i)});" if dep[i] else f"dput(g[{k}], (r - r) + {ref(i)});")
        return "\n".join(lines) + "\n"

    def evaluate(self, r, s, c, params=()):
        """The five components with r, s = sin θ, c = cos θ floats, arrays or Jets (r) -- the arithmetic of the generated code."""
        from .special_radii import Jet

        g = self.graph
        val = {}

        def fn(op, x):
            if isinstance(x, Jet):
                return getattr(x, op)()
            return getattr(np, op)(x)

        for i in self._live():
            n = g.nodes[i]
            op = n[0]
            if op == "const":
                val[i] = float.fromhex(n[1])
            elif op == "r":
                val[i] = r
            elif op == "sin_theta":
                val[i] = s
            elif op == "cos_theta":
                val[i] = c
            elif op == "param":
                val[i] = float(params[n[1]])
            elif op == "add":
                val[i] = val[n[1]] + val[n[2]]
            elif op == "sub":
                val[i] = val[n[1]] - val[n[2]]
            elif op == "mul":
                val[i] = val[n[1]] * val[n[2]]
            elif op == "div":
                val[i] = val[n[1]] / val[n[2]]
            elif op == "neg":
                val[i] = -val[n[1]]
            elif op == "powi":
                y = val[n[1]]
                for _ in range(n[2] - 1):
                    y = y * val[n[1]]
                val[i] = y
            else:
                val[i] = fn(op, val[n[1]])
        return tuple(val[i] for i in self.outputs)


# ---------------------------------------------------------------------------------------------------------------------------
# compile
# ---------------------------------------------------------------------------------------------------------------------------
def default_cache_dir():
    base = os.environ.get("GRADUS_MI355X_MODULE_CACHE") or os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.expanduser("~/.cache"),
                                                                         "gradus_mi355x", "modules")
    return base


def _entry():
    """__graft_entry__: the one place the library's compile flags live (HIP_FLAGS), shared, not copied."""
    import importlib
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module("__graft_entry__")


_HIPCC_VERSION = {}


def _hipcc_version(hipcc):
    if hipcc not in _HIPCC_VERSION:
        _HIPCC_VERSION[hipcc] = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
    return _HIPCC_VERSION[hipcc]


def module_key(source: str):
    """(sha256 of everything a module is made from, its 64-bit build id): the generated source, the kernel sources, the flags and
    the compiler's version."""
    E = _entry()
    try:
        hipcc = E._hipcc()
    except RuntimeError as e:
        raise RuntimeError("CompiledMetric needs hipcc to compile the metric's kernels and found none (looked on PATH and in "
                           "/opt/rocm/bin); TabulatedMetric traces a metric without a compiler") from e
    h = hashlib.sha256()
    for part in (source, E.csrc_hash(), "\0".join(E.HIP_FLAGS), "\0".join("\0".join(f) for _, _, f in E.module_units("BODY", 0)),
                 _hipcc_version(hipcc)):
        h.update(part.encode() + b"\0\0")
    key = h.hexdigest()
    return key, (int(key[:16], 16) & 0x7FFFFFFFFFFFFFFF) | 1          # (a positive int64, never 0: 0 is "no module" in the library's cache keys)


def build_module(source: str, cache_dir=None) -> str:
    """The kernel module of a generated component body: `<cache_dir>/<sha256>.so`, compiled when it is not there yet -- seven
    kernels_tu.hip units side by side (as many as __graft_entry__.job_limit() allows), one link."""
    import tempfile

    E = _entry()
    key, build_id = module_key(source)
    cache_dir = os.path.abspath(cache_dir or default_cache_dir())          # (the body is #included by its absolute path)
    out = os.path.join(cache_dir, key + ".so")
    if os.path.exists(out):
        return out
    os.makedirs(cache_dir, exist_ok=True)
    body = os.path.join(cache_dir, key + ".inc")
    with open(body, "w") as f:
        f.write(source)
    with tempfile.TemporaryDirectory(dir=cache_dir, prefix=key[:12] + ".build.") as tmp:
        units = E.module_units(body, build_id)
        E.compile_units(units, E.CSRC, tmp, force=True)
        partial = os.path.join(tmp, "module.so")
        E.link_module([os.path.join(tmp, o) for o, _, _ in units], partial)
        os.replace(partial, out)          # (atomic: a second process never sees half a module)
    return out


def module_info(path):
    """gr_user_module_info of a module file, as a dict (loads the file, no device needed)."""
    from . import _lib

    h = ctypes.CDLL(path, mode=os.RTLD_LOCAL)
    h.gr_user_module_info.restype = ctypes.POINTER(_lib.gr_user_module_info_t)
    i = h.gr_user_module_info().contents
    return {"abi_version": int(i.abi_version), "metric_id": int(i.metric_id), "build_id": int(i.build_id),
            "header_hash": "".join("%016x" % (int(w) & 0xFFFFFFFFFFFFFFFF) for w in i.header_hash)}


# the launchers every module exports (kernels_tu.hip)
MODULE_LAUNCHERS = ("gr64_launch_trace_m12", "gr64_launch_path_m12", "gr64_launch_apply_m12", "gr64_launch_classify_m12",
                    "gr64_launch_areafactor_m12", "grt_launch_trace_m12", "grt1_launch_trace_m12", "grts_launch_trace_m12",
                    "grts1_launch_trace_m12", "grv1_launch_offset_m12")

_LOADED = {}          # module path -> metric id in this process


def load_module(path) -> int:
    """The metric id of a module in this process: loaded once (gr_metric_module_load)."""
    from . import _lib

    if path not in _LOADED:
        mid = ctypes.c_int64(-1)
        _lib.check(_lib.load().gr_metric_module_load(os.fsencode(path), ctypes.byref(mid)))
        _LOADED[path] = int(mid.value)
    return _LOADED[path]


def unload_module(path):
    from . import _lib

    mid = _LOADED.pop(path, None)
    if mid is not None:
        _lib.check(_lib.load().gr_metric_module_unload(mid))


def unload_all():
    """Free every slot this process has loaded through `load_module` (each module is loaded again at its next use)."""
    for path in list(_LOADED):
        unload_module(path)


# ---------------------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------------------
class CompiledMetric(AbstractStaticAxisSymmetric):
    """ANY branch-free static, axis-symmetric metric on the device through kernels compiled for it.

    `source`: a callable `f(r, θ)` or `f(r, θ, p)` -> (g_tt, g_rr, g_θθ, g_ϕϕ, g_tϕ) written with numpy functions, or a metric of
    this package (its own formula is recorded).  `params`: up to six run-time parameters, handed to the callable as `p` and to the
    kernels as gr_config.params -- `with_params(...)` gives the same kernels other values, nothing is compiled again.  A bare
    callable must bring `inner_radius` (the event horizon); `isco` defaults to the source's, or is found from the callable's own
    derivatives.  `cache_dir`: where `<sha256>.so` is kept (default: $GRADUS_MI355X_MODULE_CACHE, else ~/.cache/gradus_mi355x/modules).

    The callable is recorded at construction (`UntraceableMetric` if it branches, compares, or calls a function a component
    body does not have); the module is compiled at first use on the device (or by `compile()`), once per source, kernel sources,
    flags and compiler.  Host-side quantities come from the recorded function itself: there is no table and no fit error.
    """

    def __init__(self, source, params=(), *, inner_radius=None, isco=None, cache_dir=None):
        self.source = source
        self.params = tuple(float(p) for p in params)
        if isinstance(source, AbstractMetric):
            if not hasattr(source, "_components"):
                raise UntraceableMetric(f"{type(source).__name__} has no component formula to record")
            self.trace = Trace(source._components, 0, from_rsc=True)
        else:
            self.trace = Trace(source, len(self.params))
        if inner_radius is None:
            if not isinstance(source, AbstractMetric):
                raise ValueError("a callable metric needs `inner_radius` (the event horizon radius)")
            inner_radius = source.inner_radius()
        self._inner_radius = float(inner_radius)
        self._isco = isco
        self.cache_dir = cache_dir
        self._module = None

    # -- the module --
    @property
    def generated_source(self):
        return self.trace.source

    @property
    def sha256(self):
        return module_key(self.trace.source)[0]

    @property
    def build_id(self):
        return module_key(self.trace.source)[1]

    def compile(self):
        """Path of this metric's kernel module (compiled now if no earlier construction left it in the cache)."""
        if self._module is None:
            self._module = build_module(self.trace.source, self.cache_dir)
        return self._module

    @property
    def metric_id(self):
        """GR_METRIC_COMPILED + the slot the module has in this process (loaded at first use)."""
        return load_module(self.compile())

    def unload(self):
        """Free the module's slot in this process (the next use loads it again)."""
        if self._module is not None:
            unload_module(self._module)

    @property
    def resources(self):
        """{kernel: {vgprs, scratch_bytes, lds_bytes, max_threads}} of the trace kernels (thin disc): scratch_bytes > 0 means
        the metric spills.  Needs a device."""
        from . import _lib

        out = (_lib.gr_metric_resources * len(_lib.MODULE_KERNELS))()
        _lib.check(_lib.load().gr_metric_module_resources(self.metric_id, None, out))
        return {k: {"vgprs": int(o.vgprs), "scratch_bytes": int(o.scratch_bytes), "lds_bytes": int(o.lds_bytes), "max_threads": int(o.max_threads)}
                for k, o in zip(_lib.MODULE_KERNELS, out)}

    def with_params(self, *params):
        """The same kernels with other run-time parameters."""
        if len(params) != len(self.params):
            raise ValueError(f"this metric has {len(self.params)} parameters")
        m = object.__new__(CompiledMetric)
        m.__dict__.update(self.__dict__)
        m.params = tuple(float(p) for p in params)
        return m

    def cache_key(self):
        """What a cache of per-metric results keys on: the module's build id and the parameters (never the slot number)."""
        return ("compiled", self.build_id) + self.params

    # -- AbstractMetric --
    def abi_params(self):
        return list(self.params)

    def _components(self, r, s, c):
        return self.trace.evaluate(r, s, c, self.params)

    def metric_components(self, r, theta):
        return self.trace.evaluate(r, np.sin(theta), np.cos(theta), self.params)

    def inner_radius(self):
        return self._inner_radius

    def isco(self):
        if self._isco is not None:
            return float(self._isco)
        if isinstance(self.source, AbstractMetric):
            return self.source.isco()
        from .special_radii import generic_isco

        return generic_isco(self)
