#!/bin/bash
# diagnostic builds of libobca_hip.so, loaded through OBCA_HIP_LIBRARY (git-ignored, not part of the product; the entries hip_poison* of the table in obca_amd/buildflags.py):
#   poison  -DOBCA_POISON [-DOBCA_POISON_VALUE]   work buffers and the kernels' LDS filled with a pattern at entry: NaN (default) AND 1e30 -- NaN hides behind fmax
# (the -DOBCA_HWID and -DOBCA_DRAIN builds of the round-5 search are gone with the switches they served: docs/HISTORY.md, "Round 5")
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
for P in hip_poison hip_poison_1e30; do python -m obca_amd.buildflags build $P & done      # warnings are errors in the variants too
wait; ls -la $R/obca_amd/csrc/variants
