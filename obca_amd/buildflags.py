"""ONE place for how every native piece is built: the compile flags, the table of the pieces (PIECES: product library, its diagnostic variants, device and host planner, the
host emulations of the tests; TEST_PIECES, CHECK_PIECES, EMU_PIECES: emulations only their own tests build) and the one rule that compiles them (compile_if_stale: globbed dependencies, compile aside, rename into place).  The build functions of the
package, the lazy builds of the tests, __graft_entry__.build() and the shell scripts under tools/ all go through build(NAME):

    python -m obca_amd.buildflags build NAME...     builds the named pieces (those that are out of date)
    python -m obca_amd.buildflags hipcc|gxx|warn    prints a flag set

Warnings are errors everywhere.  Round 4 lost two stores of the stage assembly behind a `//` comment; `hipcc -Wall` prints that as "variable 'sumz' set but not used" -- the
build scripts of rounds 1-5 never passed -Wall and filtered the compiler's output, and the bug cost two rounds.  tests/test_abi_cpu.py compiles the
device sources with these flags (-fsyntax-only, seconds) and asserts that the compiler prints nothing.
  -Wno-unused-parameter: phase functions share signatures (dw, dc, ... are passed to every variant, used by some) -- the one warning class that is interface, not accident.
"""
import collections
import glob
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(_HERE, "..", "include")
WARN = ["-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
# -fno-optimize-sibling-calls: the phases of the solve are non-inlined local device functions that use the whole register file.  LLVM drops the
# callee-saved-register saves of such functions (every caller is known) only if no call site is marked `tail`, and -O3 marks them all; with the
# flag the 112 VGPR + ~150 AGPR saves / restores per phase call disappear: 0.23 MB less scratch traffic per factorisation pass, 140 k -> 154 k solves/s.
HIPCC = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-optimize-sibling-calls", "-I" + INCLUDE] + WARN
# host C++ (planner; the emulation of the kernels under tests/emu, which sees `#pragma unroll`)
GXX = ["g++", "-std=c++17", "-fPIC", "-shared"] + WARN + ["-Wno-unknown-pragmas", "-Wno-misleading-indentation"]

_CSRC = os.path.join(_HERE, "csrc")
_EMU = os.path.join(os.path.dirname(_HERE), "tests", "emu")
Piece = collections.namedtuple("Piece", "cc flags out sources libs")


def _piece(cc, flags, out, *sources, libs=()):
    return Piece(cc, list(flags), out, list(sources), list(libs))


_HIP = os.path.join(_CSRC, "obca_hip.hip")
PIECES = {
    "hip": _piece(HIPCC, [], os.path.join(_CSRC, "libobca_hip.so"), _HIP),                                          # the product: both IPM kernels + the C ABI (include/obca_hip.h)
    "hip_prof": _piece(HIPCC, ["-DOBCA_PROFILE"], os.path.join(_CSRC, "libobca_hip_prof.so"), _HIP),                # per-phase clocks (tools/phase_profile.py); loaded through OBCA_HIP_LIBRARY
    "hip_poison": _piece(HIPCC, ["-DOBCA_POISON"], os.path.join(_CSRC, "variants", "libobca_hip_poison.so"), _HIP),      # work buffers and LDS filled with NaN at entry ...
    "hip_poison_1e30": _piece(HIPCC, ["-DOBCA_POISON", "-DOBCA_POISON_VALUE=1e30"], os.path.join(_CSRC, "variants", "libobca_hip_poison_1e30.so"), _HIP),      # ... and with 1e30: NaN hides behind fmax
    "diag": _piece(HIPCC, [], os.path.join(_CSRC, "libobca_diag.so"), os.path.join(_CSRC, "obca_diag.hip")),        # the pattern kernel of the bit-equality tests (include/obca_diag.h)
    "plan3d": _piece(HIPCC, [], os.path.join(_CSRC, "libobca_plan3d.so"), os.path.join(_CSRC, "obca_plan3d.hip")),  # the quadcopter's grid planner on the device (include/obca_plan3d.h)
    "plan": _piece(GXX, ["-O2", "-pthread", "-I" + INCLUDE], os.path.join(_CSRC, "libobca_plan.so"),               # the host planner (Hybrid A*; REFERENCE mode in the second file)
                   os.path.join(_CSRC, "obca_planner.cpp"), os.path.join(_CSRC, "obca_planner_ref.cpp")),
}
# test infrastructure, listed here so that it is built by the same rule (nothing in the package loads it): the kernel text compiled for the host, tests/emu/NAME.cpp -> libobca_NAME.so
for _name, _src, _flags, _libs in (("emu", "obca_emu.cpp", ["-O1"], ["-ldl"]), ("validate_emu", "validate_emu.cpp", ["-O1"], []),
                                   ("quad_shift_emu", "quad_shift_emu.cpp", ["-O1"], []), ("plan3d_emu", "plan3d_emu.cpp", ["-O2"], [])):
    PIECES[_name] = _piece(GXX, _flags, os.path.join(_EMU, "libobca_%s.so" % _name), os.path.join(_EMU, _src), libs=_libs)
# Emulations that only their own tests build (lazily, through build(NAME) like every piece; __graft_entry__.build() does not compile them): tests/emu/NAME.cpp -> libobca_NAME.so.
# tests/test_path_ws_cpu.py pins the argv and walks the include closure of path_ws_emu as tests/test_build_cpu.py does for the pieces of PIECES.
TEST_PIECES = {"path_ws_emu": _piece(GXX, ["-O1"], os.path.join(_EMU, "libobca_path_ws_emu.so"), os.path.join(_EMU, "path_ws_emu.cpp"))}      # obca_amd/csrc/obca_path_ws.h for the host
# The same kind of piece, in a table of its own because tests/test_path_ws_cpu.py pins TEST_PIECES at its one entry: obca_amd/csrc/obca_clearance.h for the host
# (tests/test_clearance_cpu.py pins this one's argv and walks its include closure).
CHECK_PIECES = {"clearance_emu": _piece(GXX, ["-O1"], os.path.join(_EMU, "libobca_clearance_emu.so"), os.path.join(_EMU, "clearance_emu.cpp"))}
# Every later emulation of this kind joins THIS table (the two above are pinned at their one entry by their tests): tests/emu/NAME.cpp -> libobca_NAME.so, -O1, built
# lazily by its own tests through build(NAME), not by __graft_entry__.build().  refine_emu: obca_amd/csrc/obca_refine.h for the host (tests/test_refine_cpu.py);
# quad_subdivide_emu: obca_amd/csrc/obca_quad_subdivide.h for the host (tests/test_quad_refine_cpu.py); hybrid_emu: obca_amd/csrc/obca_hybrid.h for the host
# (tests/test_hybrid_cpu.py); scenes_emu: the same header's per-instance route (tests/test_scenes_cpu.py); plan_resident_emu: obca_amd/csrc/obca_plan_resident.h with the
# search and the path warm start behind it, the resident route (tests/test_plan_resident_cpu.py); quad_plan_resident_emu: obca_amd/csrc/obca_quad_plan_resident.h over
# obca_plan3d.h, the quadcopter's resident route (tests/test_quad_plan_resident_cpu.py); rollout_emu: obca_amd/csrc/obca_rollout.h for the host (tests/test_rollout_cpu.py);
# track_emu: obca_amd/csrc/obca_track.h over it for the host (tests/test_track_cpu.py); ensemble_emu: obca_amd/csrc/obca_ensemble.h over both (tests/test_ensemble_cpu.py);
# certify_emu: obca_amd/csrc/obca_certify.h over obca_clearance.h (tests/test_certify_cpu.py); shift_emu: obca_amd/csrc/obca_shift.h, the parking receding-horizon
# restart (tests/test_shift_cpu.py); advance_emu: obca_amd/csrc/obca_advance.h over the rollout and both shifts, the closed-loop step (tests/test_advance_cpu.py);
# scene_edit_emu: obca_amd/csrc/obca_scene_edit.h over obca_validate.h, the obstacles of a resident batch moved in place (tests/test_scene_edit_cpu.py);
# predict_emu: obca_amd/csrc/obca_predict.h over obca_clearance.h, the clearance of a held plan against obstacles that move (tests/test_predict_cpu.py).
EMU_PIECES = {_n: _piece(GXX, ["-O1"], os.path.join(_EMU, "libobca_%s.so" % _n), os.path.join(_EMU, _n + ".cpp"))
              for _n in ("refine_emu", "quad_subdivide_emu", "hybrid_emu", "scenes_emu", "plan_resident_emu", "quad_plan_resident_emu", "rollout_emu", "track_emu", "ensemble_emu", "certify_emu",
                         "shift_emu", "advance_emu", "scene_edit_emu", "predict_emu")}
DEFAULT = [n for n in PIECES if n not in ("hip_prof", "hip_poison", "hip_poison_1e30")]      # what __graft_entry__.build() compiles


def dependencies(sources):
    """What a piece is checked against: its sources, EVERY header of the project and this file (it holds the flags).  Globbed, not listed by hand: a header edit may
    rebuild a piece that does not include it, never the other way round (tests/test_build_cpu.py walks the #include lines of every piece)."""
    return list(sources) + glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")) + [os.path.abspath(__file__)]


def compile_if_stale(out, cmd, sources, force=False, libs=()):
    """Run `cmd -o out sources libs` if `out` is missing or older than one of dependencies(sources); returns `out`.  The compiler writes to a temporary beside `out` (its
    name ends in .so: .gitignore covers it) that is renamed into place: a process that has the old library mapped keeps the old file, and several builders at once (xdist
    workers, the `&` of tools/build.sh) each replace a whole file.  A failed compile removes its temporary and leaves the previous `out` as it was."""
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in dependencies(sources)):
        return out
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    tmp = "%s.%d.tmp.so" % (out, os.getpid())
    try:
        subprocess.check_call(list(cmd) + ["-o", tmp] + list(sources) + list(libs))
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return out


def build(name, force=False, out=None, flags=None):
    """build a piece of the table (PIECES, TEST_PIECES, CHECK_PIECES or EMU_PIECES); `out` / `flags` replace the entry's output path / extra flags (the OBCA_HIP_LIBRARY override, the checking builds of the emulation,
    the tuning variants of tools/plan3d_rate.py)"""
    p = {**EMU_PIECES, **CHECK_PIECES, **TEST_PIECES, **PIECES}[name]
    return compile_if_stale(out or p.out, p.cc + (p.flags if flags is None else list(flags)), p.sources, force, p.libs)


def main(argv):
    which = argv[0] if argv else "hipcc"
    if which == "build":
        for n in argv[1:]:
            print(build(n))
    else:
        print(" ".join({"hipcc": HIPCC, "gxx": GXX, "warn": WARN}[which]))


if __name__ == "__main__":
    main(sys.argv[1:])
