// TEST INFRASTRUCTURE ONLY.  Host build of the parking warm start from planner paths: obca_amd/csrc/obca_path_ws.h compiled with -DOBCA_EMU, where every PAR(lane) region is a
// plain loop over the 64 lanes, SYNC is nothing and the LDS arrays are locals.  tests/test_path_ws_cpu.py compares it with planner.path_to_warm_start on a machine without a
// GPU, tests/test_gpu_path_ws.py compares the device with it bit for bit.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_path_ws.h"
using namespace obca;

static std::string g_pw_err;

extern "C" {
// obca_parking_path_warm_start_batch of include/obca_path_ws.h, instance after instance, on the caller's arrays as they are (rows of `cap` nodes)
const char *emu_path_ws_last_error() { return g_pw_err.c_str(); }
int emu_path_ws_limits(int *maxnodes, int *nmax) { *maxnodes = PW_MAXNODES; *nmax = OB_NMAX; return 0; }
int emu_path_ws_batch(int B, int N, const double *paths, const int *dirs, const int *counts, int cap, const double *xF, double v_nom, double L, double a_max,
                      double *Ts, double *xWS, double *uWS, int *status) {
    if (const char *bad = pw::path_ws_check_args(B, N, cap, v_nom, L, a_max, paths && dirs && counts && Ts && xWS && uWS && status)) { g_pw_err = bad; return -1; }
    for (int i = 0; i < B; i++) {
        double *ts = Ts + i, *x = xWS + (size_t)i * 4 * (N + 1), *u = uWS + (size_t)i * 2 * N;
        int st = pw::path_ws_count_status(counts[i], cap);
        if (!st) st = pw::path_ws_instance(N, counts[i], paths + (size_t)i * cap * 3, dirs + (size_t)i * cap, xF ? xF + (size_t)i * 4 : nullptr, v_nom, L, a_max, ts, x, u);
        if (st) pw::path_ws_zero(N, ts, x, u);
        status[i] = st;
    }
    return 0;
}
// one instance of obca_batch_set_path_warm_start: prob / z0 as tests/packing.py packs them, zlen doubles in z0
int emu_path_ws_record(int N, int count, int cap, const double *path, const int *dir, int use_xF, double v_nom, double a_max, double *prob, double *z0, int zlen) {
    return pw::path_ws_record(N, count, cap, path, dir, use_xF, v_nom, a_max, prob, z0, zlen);
}
}
