#!/usr/bin/env python3
"""SHA-256 of the device code of obca_hip.hip, per build of the table: what a "kernels untouched" change compares before and after.

    python tools/code_sections.py [BUILD...]        default: hip hip_prof hip_poison hip_poison_1e30; prints one JSON object

Each build is compiled with its product flags plus `--cuda-device-only -c`, the gfx950 code object is taken out of the bundle and its .text, .rodata and .note
sections are hashed.  Sections, not the file: two compiles of one source differ in a per-compile unit id inside the dynamic symbol and hash tables, the three
sections do not, and they do not move with host code or with the path of the tree either.  Needs no GPU; one build takes a minute or two, the builds run side by side.
"""
import concurrent.futures
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from obca_amd import buildflags  # noqa: E402

BUILDS = ("hip", "hip_prof", "hip_poison", "hip_poison_1e30")
SECTIONS = (".text", ".rodata", ".note")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _llvm(tool):
    """the LLVM tool that belongs to hipcc: on the PATH, or beside the compiler of the ROCm installation"""
    found = shutil.which(tool)
    if found:
        return found
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for d in ("lib/llvm/bin", "llvm/bin"):
        if os.path.exists(os.path.join(rocm, d, tool)):
            return os.path.join(rocm, d, tool)
    raise FileNotFoundError(tool)


def sections(name):
    p = buildflags.PIECES[name]
    with tempfile.TemporaryDirectory() as tmp:
        bundle, elf = os.path.join(tmp, "dev.o"), os.path.join(tmp, "dev.elf")
        subprocess.check_call([f for f in p.cc if f != "-shared"] + p.flags + ["--cuda-device-only", "-c", "-o", bundle] + p.sources)
        subprocess.check_call([_llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + elf])
        out = {}
        for sec in SECTIONS:
            raw = os.path.join(tmp, "sec.bin")
            subprocess.check_call([_llvm("llvm-objcopy"), "--dump-section", "%s=%s" % (sec, raw), elf, os.path.join(tmp, "unused.elf")])
            with open(raw, "rb") as f:
                data = f.read()
            out[sec] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        return out


def main(argv):
    names = argv or list(BUILDS)
    with concurrent.futures.ThreadPoolExecutor(len(names)) as pool:
        print(json.dumps(dict(zip(names, pool.map(sections, names))), indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
