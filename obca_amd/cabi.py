"""The C ABI as the Python side sees it, read ONCE from the public headers (include/obca_hip.h, obca_path_ws.h, obca_clearance.h, obca_refine.h, obca_quad_subdivide.h, obca_plan_device.h, obca_plan_scenes.h, obca_plan_resident.h, obca_plan_resident_check.h, obca_quad_plan_resident.h, obca_rollout.h, obca_track.h, obca_ensemble.h, obca_advance.h, obca_scene_edit.h, obca_certify.h, obca_predict.h, obca_plan.h, obca_plan3d.h, obca_diag.h): `bind(lib, header)` gives every
function `lib` exports the `restype` and `argtypes` its prototype declares, `Opts` is `typedef struct obca_opts`.  The call sites of api.py, planner.py and diag.py then pass
Python numbers and prepared numpy arrays and say nothing about C types; a miscounted argument, an array of another dtype, a non-contiguous view or a read-only output buffer
is a TypeError on the CPU, before anything reaches the library.  The subset of C the headers use is all that is parsed; a parameter of another kind raises when the library is
bound."""
import ctypes as C
import os
import re
import numpy as np
from . import buildflags

_PROTO = re.compile(r"\b(int|const char \*)\s*(obca_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", re.S)      # (also the two under #ifdef OBCA_PROFILE: the profiling build exports them)
_PARAM = re.compile(r"(const )?(long long|[a-z_]+) ?(\*{0,2}) ?\w+ ?(\[\w*\])?")
_HANDLES = ("void", "obca_ctx", "obca_batch", "obca_quad_batch")


def _text(header):
    """a header of include/ (or any path) without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(buildflags.INCLUDE, header)).read(), flags=re.S)


def opts_fields(header="obca_hip.h"):
    """the fields of `typedef struct obca_opts` as a ctypes _fields_ list"""
    body = re.search(r"typedef struct obca_opts \{(.*?)\} obca_opts;", _text(header), flags=re.S).group(1)
    kinds = {"double": C.c_double, "int": C.c_int}
    return [(n.strip(), kinds[kind]) for kind, names in (d.split(None, 1) for d in body.split(";") if d.strip()) for n in names.split(",")]


class Opts(C.Structure):
    _fields_ = opts_fields()


class ArrayParam:
    """argtypes entry of a `[const] double *` / `[const] int *` parameter: None, a numpy array of exactly that dtype, C-contiguous (and writeable unless the parameter is
    const), or whatever POINTER(ctype) takes itself (byref(), ctypes arrays, data_as pointers).  Nothing is converted: a silent copy of an output array would lose the results."""

    def __init__(self, ctype, const):
        self.ptr, self.view, self.dtype, self.const = C.POINTER(ctype), ctype * 0, np.dtype(ctype), const

    def from_param(self, a):
        if not isinstance(a, np.ndarray):
            return self.ptr.from_param(a)
        f = a.flags
        if a.dtype != self.dtype or not f.c_contiguous or not (self.const or f.writeable):
            raise TypeError(f"need a C-contiguous {'' if self.const else 'writeable '}{self.dtype} array, got {a.dtype}, contiguous={f.c_contiguous}, writeable={f.writeable}")
        # the array's own memory, kept alive by what is returned: a zero-length ctypes array laid over it goes to C as its address and costs a seventh of numpy's data_as
        # (0.6 against 3.9 us, and a host-pointer solve passes 24 arrays); from_buffer wants writeable memory, so a read-only input takes the slow way
        return self.view.from_buffer(a) if f.writeable else a.ctypes.data_as(self.ptr)


def _ctype(param, name):
    m = _PARAM.fullmatch(" ".join(param.split()))
    const, base, depth = (bool(m.group(1)), m.group(2), len(m.group(3)) + bool(m.group(4))) if m else (False, None, 0)
    if depth == 0 and base in ("int", "double"):
        return {"int": C.c_int, "double": C.c_double}[base]
    if depth == 1 and base in ("int", "double"):
        return ArrayParam({"int": C.c_int, "double": C.c_double}[base], const)
    if depth == 1 and base in ("float", "long long", "char", "obca_opts"):
        return {"float": C.POINTER(C.c_float), "long long": C.POINTER(C.c_longlong), "char": C.c_char_p, "obca_opts": C.POINTER(Opts)}[base]
    if depth in (1, 2) and base in _HANDLES:
        return C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)
    raise TypeError(f"{name}: no ctypes type for the parameter `{param.strip()}`")


def prototypes(header):
    """name -> (restype, argtypes) of every function the header declares"""
    out = {}
    for ret, name, params in _PROTO.findall(_text(header)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (C.c_int if ret == "int" else C.c_char_p, [_ctype(p, name) for p in params])
    return out


def bind(lib, header):
    """declare every function of `header` that `lib` exports (a profiling, poisoned or older build exports another set); returns lib"""
    for name, (restype, argtypes) in prototypes(header).items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib
