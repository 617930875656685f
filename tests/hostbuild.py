"""Builds a host harness (tests/host_harness*.cpp: a header of the library compiled for the CPU) into a shared object next to its
source and loads it.  One place for what every ctypes binding of a harness did for itself."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_loaded = {}


def so_path(source, suffix=""):
    return os.path.join(HERE, "lib" + os.path.splitext(source)[0] + suffix + ".so")


def build(source, flags=(), defines=(), suffix="", compiler="g++"):
    """so_path(source, suffix), compiled (-O2 -std=c++17 `flags`, -D per entry of `defines`) if it is missing or older than what it
    may include: the source, tests/*.hpp, every header of the library and the C ABI.  All of them, not the ones the source names: a
    list kept by hand goes stale, and a harness too many rebuilt costs seconds.  `suffix` keeps the builds of one source with
    different `defines` apart."""
    src, so = os.path.join(HERE, source), so_path(source, suffix)
    deps = [src, os.path.join(ROOT, "include", "gradus_mi355x.h")] + glob.glob(os.path.join(HERE, "*.hpp")) \
        + glob.glob(os.path.join(ROOT, "gradus.jl_amd", "csrc", "*.hpp"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([compiler, "-O2", "-std=c++17", *flags, *("-D" + d for d in defines), "-fPIC", "-shared", "-o", so, src])
    return so


def load(source, suffix="", **kw):
    """ctypes.CDLL of build(source, ...): built and loaded once per shared object and process."""
    so = so_path(source, suffix)
    if so not in _loaded:
        _loaded[so] = C.CDLL(build(source, suffix=suffix, **kw))
    return _loaded[so]
