// TEST INFRASTRUCTURE ONLY.  Host build of the closed-loop rollout: obca_amd/csrc/obca_track.h (over obca_rollout.h) compiled with -DOBCA_EMU, where every PAR(lane) region
// is a plain loop over the 64 lanes, SYNC is nothing and the work buffers are the caller's memory.  tests/test_track_cpu.py compares it with the numpy statements of
// obca_amd/validate.py on a machine without a GPU, tests/test_gpu_track.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_clearance.h"
#include "../../obca_amd/csrc/obca_rollout.h"
#include "../../obca_amd/csrc/obca_track.h"
using namespace obca;

static std::string g_tk_err;

extern "C" {
const char *emu_track_last_error() { return g_tk_err.c_str(); }
int emu_track_sizes(int *out, int *roll_out, int *smax) { *out = TK_OUT; *roll_out = RO_OUT; *smax = CL_SMAX; return 0; }
// one instance: prob / z / ts / vmax as emu_rollout_parking takes them; q 4, r 2, qf 4; dx0 4 or NULL; rev: deal the linearisation and clearance items to the lanes
// backwards; AB N x 4 x 6, pose 3 x (N S + 1), X (N + 1) x 4, K N x 2 x 4: the work buffers' slices
int emu_track_parking(int N, const double *prob, const double *z, const double *ts, int vmax, int substeps, int feedback, int clamp, const double *q, const double *r, const double *qf,
                      const double *dx0, double need, int rev, double *AB, double *pose, double *X, double *K, double *out) {
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, 4, 2, need)) { g_tk_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !AB || !pose || !X || !K || !out) { g_tk_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    const trk::Weights w = trk::make_weights(q, r, qf, 4, 2);
    std::vector<double> Ua((size_t)2 * N);      // the applied inputs: the work buffer's region behind [A|B]
    if (vmax <= 2) trk::track_parking_instance<2>(N, prob, z, ts, substeps, feedback, clamp, w, dx0, need, rev, AB, Ua.data(), pose, X, K, out);
    else if (vmax <= OB_VMID) trk::track_parking_instance<OB_VMID>(N, prob, z, ts, substeps, feedback, clamp, w, dx0, need, rev, AB, Ua.data(), pose, X, K, out);
    else trk::track_parking_instance<OB_VMAX>(N, prob, z, ts, substeps, feedback, clamp, w, dx0, need, rev, AB, Ua.data(), pose, X, K, out);
    return 0;
}
// one instance: prob, x, u, ts, tstride as emu_rollout_quad takes them; q 12, r 4, qf 12; dx0 12 or NULL; AB N x 12 x 16, K N x 4 x 12
int emu_track_quad(int N, const double *prob, const double *x, const double *u, const double *ts, int tstride, int substeps, int feedback, int clamp, const double *q, const double *r,
                   const double *qf, const double *dx0, double need, int rev, double *AB, double *pose, double *X, double *K, double *out) {
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, QX, QU, need)) { g_tk_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !u || !ts || !AB || !pose || !X || !K || !out) { g_tk_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    const trk::Weights w = trk::make_weights(q, r, qf, QX, QU);
    std::vector<double> Ua((size_t)QU * N);
    trk::track_quad_instance(N, prob, x, u, ts, tstride, substeps, feedback, clamp, w, dx0, need, rev, AB, Ua.data(), pose, X, K, out);
    return 0;
}
}
