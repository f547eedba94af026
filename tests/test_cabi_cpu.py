"""obca_amd/cabi.py reads the four public headers as the one statement of the C ABI on the Python side.  Its reading is checked here against an independent one (the classifier
of the Julia shim's test, a literal table for the two headers that one does not read), on the real libraries (they cross-compile without a GPU; nothing here touches a device),
and on what the bound parameter types take and refuse."""
import ctypes as C
import numpy as np
import pytest
from obca_amd import api, cabi, diag, planner
from test_julia_shim_cpu import c_prototypes

HEADERS = {"obca_hip.h": 44, "obca_plan.h": 9, "obca_plan3d.h": 6, "obca_diag.h": 1}      # prototypes per header: 42 exported + the two of the profiling build, ...
# obca_plan3d.h and obca_diag.h, parameter by parameter as include/ declares them
LITERAL = {"obca_plan3d_create": ["int", "ptr"], "obca_plan3d_destroy": ["ptr"], "obca_plan3d_last_error": ["ptr"], "obca_plan3d_kernel_ms": ["ptr", "ptr"],
           "obca_plan3d_paths_batch": ["ptr", "int", "ptr", "ptr", "int", "ptr", "double", "ptr", "double", "ptr", "int", "ptr", "ptr"],
           "obca_plan3d_warm_start_batch": ["ptr", "int", "int", "ptr", "ptr", "int", "ptr", "double", "ptr", "double", "ptr", "ptr"],
           "obca_diag_leave_pattern": ["int", "int", "double", "ptr", "ptr"]}


def kind(t):
    return {C.c_int: "int", C.c_double: "double"}.get(t, "ptr")


def test_the_reading_of_the_headers_agrees_with_the_independent_classifier():
    protos = {h: cabi.prototypes(h) for h in HEADERS}
    assert {h: len(p) for h, p in protos.items()} == HEADERS
    assert "obca_batch_debug_phase_cycles" in protos["obca_hip.h"] and "obca_quad_batch_debug_phase_cycles" in protos["obca_hip.h"]      # phase_cycles() calls them in the profiling build
    mine = {n: [kind(t) for t in args] for h in ("obca_hip.h", "obca_plan.h") for n, (_, args) in protos[h].items()}
    assert mine == c_prototypes()
    assert {n: [kind(t) for t in args] for h in ("obca_plan3d.h", "obca_diag.h") for n, (_, args) in protos[h].items()} == LITERAL
    res = {n: r for p in protos.values() for n, (r, _) in p.items()}
    assert {n for n, r in res.items() if r is C.c_char_p} == {"obca_last_error", "obca_plan3d_last_error"} and all(r in (C.c_int, C.c_char_p) for r in res.values())


def test_the_parameter_types():
    sig = cabi.prototypes("obca_hip.h")
    a = sig["obca_parking_signed_dist_batch"][1]
    assert a[0] is C.c_void_p and a[1] is C.c_int and a[4] is C.c_double and a[21] is C.POINTER(api.Opts)
    assert all(isinstance(a[k], cabi.ArrayParam) and a[k].const and a[k].dtype == np.float64 for k in (3, 5, 6, 8, 9, 12, 20)) and a[10].dtype == np.int32 and a[10].const      # Ts, ego[4], ..., nOb
    assert all(isinstance(a[k], cabi.ArrayParam) and not a[k].const for k in range(22, 30)) and a[25].dtype == np.int32      # the outputs; exitflag
    assert sig["obca_create"][1] == [C.POINTER(C.c_void_p), C.c_int] and sig["obca_batch_create"][1][3] is C.POINTER(C.c_void_p)
    assert sig["obca_device_name"][1][1] is C.c_char_p and sig["obca_batch_scratch_bytes"][1][1] is C.POINTER(C.c_longlong) and sig["obca_batch_kernel_ms"][1][1] is C.POINTER(C.c_float)
    assert cabi.prototypes("obca_plan3d.h")["obca_plan3d_create"][1] == [C.c_int, C.POINTER(C.c_void_p)]
    assert cabi.opts_fields() == api.Opts._fields_ and len(api.Opts._fields_) == 35


@pytest.fixture(scope="module")
def libs():
    import obca_amd
    obca_amd.build_library(); planner.build_library(); planner.build_plan3d_library(); diag.build_library()
    return {"obca_hip.h": api._load(), "obca_plan.h": planner._load(), "obca_plan3d.h": planner._load3d(), "obca_diag.h": diag._load()}


def test_every_exported_function_is_declared_on_the_loaded_libraries(libs):
    n = 0
    for h, lib in libs.items():
        for name, (restype, argtypes) in cabi.prototypes(h).items():
            if "debug_phase_cycles" in name:
                assert not hasattr(lib, name)      # (the product library does not export them: bind() skipped them)
                continue
            fn = getattr(lib, name)
            assert fn.restype is restype and len(fn.argtypes) == len(argtypes) and [kind(t) for t in fn.argtypes] == [kind(t) for t in argtypes], name
            n += 1
    assert n == 42 + 9 + 6 + 1 and set(api.EXPORTS + planner.PLAN3D_EXPORTS) <= {n_ for h in libs for n_ in cabi.prototypes(h)}


def test_bound_functions_still_work_and_refuse_a_miscounted_call(libs):
    o = api.Opts()
    assert libs["obca_hip.h"].obca_default_opts(o) == 0 and o.tol == 1e-5 and o.max_iter == 200      # (POINTER(Opts) takes the record itself, or byref of it)
    q = api.Opts()
    assert libs["obca_hip.h"].obca_quadcopter_reference_opts(C.byref(q)) == 0 and q.max_iter == 3000
    assert libs["obca_diag.h"].obca_diag_leave_pattern(-1, 4, 1e30, None, None) == -1      # (argument check only: no device is touched)
    with pytest.raises(TypeError):
        libs["obca_diag.h"].obca_diag_leave_pattern(-1, 4, 1e30, None)      # too few
    with pytest.raises(TypeError):
        libs["obca_hip.h"].obca_batch_sync()
    with pytest.raises(C.ArgumentError):
        libs["obca_diag.h"].obca_diag_leave_pattern(-1, 4, 1e30, np.zeros(1), None)      # a float64 array where int * is declared


def test_what_an_array_parameter_takes_and_refuses():
    out, cin, iout = cabi.ArrayParam(C.c_double, False), cabi.ArrayParam(C.c_double, True), cabi.ArrayParam(C.c_int, False)
    a = np.arange(12.0).reshape(3, 4)
    ro = a.copy(); ro.flags.writeable = False
    for p in (out, cin):
        assert p.from_param(None) is None
        assert C.cast(p.from_param(a), C.c_void_p).value == a.ctypes.data      # the array's own memory: nothing is copied
        assert p.from_param(a.ctypes.data_as(C.POINTER(C.c_double))) is not None and p.from_param(C.byref(C.c_double(1.0))) is not None and p.from_param((C.c_double * 3)()) is not None
        for bad in (a.astype(np.float32), a[:, ::2], a.T, a.astype(np.int64), [1.0, 2.0], 3.0, C.byref(C.c_int(1))):
            with pytest.raises(TypeError):
                p.from_param(bad)
    assert C.cast(cin.from_param(ro), C.c_void_p).value == ro.ctypes.data      # read-only: fine where the header says const ...
    with pytest.raises(TypeError):
        out.from_param(ro)                                                      # ... refused where the library writes
    i = np.zeros(3, np.int32)
    assert C.cast(iout.from_param(i), C.c_void_p).value == i.ctypes.data and iout.from_param(C.byref(C.c_int(0))) is not None and iout.from_param(None) is None
    for bad in (np.zeros(3, np.int64), np.zeros(3), np.zeros(3, np.uint32)):
        with pytest.raises(TypeError):
            iout.from_param(bad)


def test_an_unknown_parameter_type_fails_when_the_library_is_bound(tmp_path):
    class Lib:
        obca_new = staticmethod(lambda *a: 0)
    good = tmp_path / "good.h"; good.write_text("/* a header */\nint obca_new(const double *x /* n */, int n);\nint obca_absent(int n);\n")
    lib = cabi.bind(Lib(), str(good))
    assert lib.obca_new.restype is C.c_int and [kind(t) for t in lib.obca_new.argtypes] == ["ptr", "int"] and not hasattr(lib, "obca_absent")
    for decl in ("unsigned n", "const float x", "short *x", "double **x", "obca_opts o", "size_t n"):
        bad = tmp_path / "bad.h"; bad.write_text("int obca_new(%s);\n" % decl)
        with pytest.raises(TypeError, match="obca_new"):
            cabi.bind(Lib(), str(bad))
