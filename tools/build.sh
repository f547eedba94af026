#!/bin/bash
# builds libobca_hip.so (product), the -DOBCA_PROFILE diagnostic variant, the diagnostic library, the device planner of the quadcopter, the host emulation, the host planner and the
# oracle, side by side.  The commands, the flags -- warnings are errors -- and the dependency rule live in the table of obca_amd/buildflags.py (a piece that is up to date is not
# compiled again); the compiler's diagnostics are NOT filtered (rounds 1-5 piped them through grep and missed "variable 'sumz' set but not used").
R=$(cd "$(dirname "$0")/.." && pwd); cd $R
for P in hip hip_prof diag plan3d emu plan; do python -m obca_amd.buildflags build $P & done
make -C $R/oracle -s &
wait
# register / scratch usage per kernel: python tools/regs.py
