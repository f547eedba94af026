"""The one build rule of obca_amd/buildflags.py (compile_if_stale) and its table of the native pieces (PIECES); no GPU, and no product library is compiled here:
the include closure of every piece lies inside what the rule checks, the argv of every piece is pinned, the rule itself is exercised on a three-line C++ file."""
import ctypes as C
import os
import re
import shutil
import subprocess
import pytest
from conftest import ROOT
from obca_amd import buildflags as BF

CSRC = os.path.join(ROOT, "obca_amd", "csrc"); EMU = os.path.join(ROOT, "tests", "emu"); INC = os.path.join(ROOT, "obca_amd", "..", "include")
HIPCC = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-optimize-sibling-calls", "-I" + INC, "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]
GXX = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
# name -> (what stands in front of `-o <output>`, the output, what stands behind it)
ARGV = {
    "hip": (HIPCC, CSRC + "/libobca_hip.so", [CSRC + "/obca_hip.hip"]),
    "hip_prof": (HIPCC + ["-DOBCA_PROFILE"], CSRC + "/libobca_hip_prof.so", [CSRC + "/obca_hip.hip"]),
    "hip_poison": (HIPCC + ["-DOBCA_POISON"], CSRC + "/variants/libobca_hip_poison.so", [CSRC + "/obca_hip.hip"]),
    "hip_poison_1e30": (HIPCC + ["-DOBCA_POISON", "-DOBCA_POISON_VALUE=1e30"], CSRC + "/variants/libobca_hip_poison_1e30.so", [CSRC + "/obca_hip.hip"]),
    "diag": (HIPCC, CSRC + "/libobca_diag.so", [CSRC + "/obca_diag.hip"]),
    "plan3d": (HIPCC, CSRC + "/libobca_plan3d.so", [CSRC + "/obca_plan3d.hip"]),
    "plan": (GXX + ["-O2", "-pthread", "-I" + INC], CSRC + "/libobca_plan.so", [CSRC + "/obca_planner.cpp", CSRC + "/obca_planner_ref.cpp"]),
    "emu": (GXX + ["-O1"], EMU + "/libobca_emu.so", [EMU + "/obca_emu.cpp", "-ldl"]),
    "validate_emu": (GXX + ["-O1"], EMU + "/libobca_validate_emu.so", [EMU + "/validate_emu.cpp"]),
    "quad_shift_emu": (GXX + ["-O1"], EMU + "/libobca_quad_shift_emu.so", [EMU + "/quad_shift_emu.cpp"]),
    "plan3d_emu": (GXX + ["-O2"], EMU + "/libobca_plan3d_emu.so", [EMU + "/plan3d_emu.cpp"]),
}


def test_table_holds_the_eleven_pieces_and_the_default_set():
    assert sorted(BF.PIECES) == sorted(ARGV)
    assert sorted(BF.DEFAULT) == sorted(set(ARGV) - {"hip_prof", "hip_poison", "hip_poison_1e30"})


@pytest.mark.parametrize("name", sorted(ARGV))
def test_include_closure_lies_inside_the_dependency_set(name):
    """every file reached over `#include "..."` from a piece's sources is one the rule compares the output's age with (at the hand-written lists this replaced that was
    false for plan, plan3d, validate_emu and quad_shift_emu)"""
    p = BF.PIECES[name]
    deps = {os.path.realpath(d) for d in BF.dependencies(p.sources)}
    assert os.path.realpath(BF.__file__) in deps                       # the file that holds the flags
    search = [a[2:] for a in p.cc + p.flags if a.startswith("-I")]
    todo = [os.path.realpath(s) for s in p.sources]; seen = set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        assert f in deps, (name, f)
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), flags=re.M):
            found = [c for c in (os.path.join(d, inc) for d in [os.path.dirname(f)] + search) if os.path.exists(c)]
            assert found, (name, f, inc)
            todo.append(os.path.realpath(found[0]))
    assert len(seen) > len(p.sources)                                      # (the walk found headers: every piece includes at least one)


@pytest.mark.parametrize("name", sorted(ARGV))
def test_argv_of_every_piece_is_pinned(name, tmp_path, monkeypatch):
    """optimisation levels, -pthread, -ldl, -DOBCA_PROFILE, the poison defines: an edit of the table cannot change a build silently"""
    calls = []

    def recorder(argv):
        calls.append(list(argv)); open(argv[argv.index("-o") + 1], "w").close()
    monkeypatch.setattr(BF.subprocess, "check_call", recorder)
    front, out, back = ARGV[name]
    assert os.path.realpath(BF.PIECES[name].out) == os.path.realpath(out)
    aside = str(tmp_path / os.path.basename(out))                          # (the product's own output is not touched)
    assert BF.build(name, force=True, out=aside) == aside and os.path.exists(aside)
    (argv,) = calls
    i = argv.index("-o")
    assert argv[:i] == front and argv[i + 2:] == back
    assert os.path.dirname(argv[i + 1]) == str(tmp_path) and argv[i + 1] != aside and argv[i + 1].endswith(".so")      # compiled aside, under a name .gitignore covers
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(out)]


def test_command_line(monkeypatch, capsys):
    built = []
    monkeypatch.setattr(BF, "build", lambda n: built.append(n) or "/x/" + n)
    BF.main(["build", "emu", "plan"])
    assert built == ["emu", "plan"] and capsys.readouterr().out.split() == ["/x/emu", "/x/plan"]
    for which, flags in (("hipcc", HIPCC), ("gxx", GXX), ("warn", ["-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"])):
        BF.main([which])
        assert capsys.readouterr().out == " ".join(flags) + "\n"


# ---------------------------------------------------------------- the rule itself, on a three-line C++ file
class Tiny:
    def __init__(self, d, monkeypatch):
        self.d = d; self.src = str(d / "tiny.cpp"); self.out = str(d / "libtiny.so"); self.compiles = 0
        real = subprocess.check_call

        def counting(argv):
            self.compiles += 1
            return real(argv)
        monkeypatch.setattr(BF.subprocess, "check_call", counting)

    def write(self, text, age=-100.0):
        """the source, `age` seconds younger than the output (older than it by default; than now if there is no output yet)"""
        with open(self.src, "w") as f:
            f.write(text)
        t = (os.stat(self.out).st_mtime if os.path.exists(self.out) else os.stat(self.src).st_mtime) + age
        os.utime(self.src, (t, t))

    def build(self, **kw):
        return BF.compile_if_stale(self.out, BF.GXX + ["-O0"], [self.src], **kw)

    def answer(self):
        """what the library on disk returns (loaded from a copy under a fresh name: the loader hands a path it has open back as it is)"""
        self.n = getattr(self, "n", 0) + 1
        return C.CDLL(shutil.copy(self.out, str(self.d / ("copy%d.bin" % self.n)))).answer()


SRC = 'extern "C" int answer() {\n    return %d;\n}\n'


@pytest.fixture
def tiny(tmp_path, monkeypatch):
    t = Tiny(tmp_path, monkeypatch)
    t.write(SRC % 1)
    assert t.build() == t.out and t.compiles == 1 and t.answer() == 1      # built because it is missing
    return t


def test_fresh_output_is_left_alone(tiny):
    st = os.stat(tiny.out)
    assert tiny.build() == tiny.out and tiny.compiles == 1
    assert (os.stat(tiny.out).st_mtime_ns, os.stat(tiny.out).st_ino) == (st.st_mtime_ns, st.st_ino)


def test_newer_source_rebuilds_by_replacing_the_file(tiny):
    old = C.CDLL(tiny.out); ino = os.stat(tiny.out).st_ino
    tiny.write(SRC % 2, age=+10.0)
    assert tiny.build() == tiny.out and tiny.compiles == 2
    assert os.stat(tiny.out).st_ino != ino                                 # replaced, not rewritten:
    assert old.answer() == 1 and tiny.answer() == 2                        # a process that has the old library open keeps it


def test_newer_buildflags_rebuilds(tiny, monkeypatch):
    real = os.path.getmtime; flags = os.path.abspath(BF.__file__); newer = os.stat(tiny.out).st_mtime + 10.0
    monkeypatch.setattr(BF.os.path, "getmtime", lambda p: newer if os.path.abspath(p) == flags else real(p))
    assert tiny.build() == tiny.out and tiny.compiles == 2


def test_newer_project_header_rebuilds(tiny, monkeypatch):
    real = os.path.getmtime; hdr = os.path.join(ROOT, "include", "obca_plan.h"); newer = os.stat(tiny.out).st_mtime + 10.0
    monkeypatch.setattr(BF.os.path, "getmtime", lambda p: newer if os.path.realpath(p) == os.path.realpath(hdr) else real(p))
    assert tiny.build() == tiny.out and tiny.compiles == 2


def test_force_rebuilds(tiny):
    ino = os.stat(tiny.out).st_ino
    assert tiny.build(force=True) == tiny.out and tiny.compiles == 2 and os.stat(tiny.out).st_ino != ino


def test_failed_compile_leaves_the_previous_output_and_no_temporary(tiny):
    before = open(tiny.out, "rb").read(); st = os.stat(tiny.out)
    tiny.write('extern "C" int answer( {\n', age=+10.0)
    listing = sorted(os.listdir(tiny.d))
    with pytest.raises(subprocess.CalledProcessError):
        tiny.build()
    assert tiny.compiles == 2
    assert open(tiny.out, "rb").read() == before and os.stat(tiny.out).st_ino == st.st_ino
    assert sorted(os.listdir(tiny.d)) == listing


def test_the_rule_is_written_once():
    """no file of the package, the tests or the tools compares file ages on its own (oracle/ keeps its Makefile and is not looked at)"""
    needle = b"getmtime" + b"("
    files = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(ROOT, "obca_amd")) for f in fs if not f.endswith((".so", ".pyc"))]
    files += [os.path.join(ROOT, d, f) for d in ("tests", "tools") for f in os.listdir(os.path.join(ROOT, d)) if f.endswith(".py")]
    assert len(files) > 40
    hits = [os.path.relpath(f, ROOT) for f in files if needle in open(f, "rb").read()]
    assert hits == [os.path.join("obca_amd", "buildflags.py")]
