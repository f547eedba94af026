// TEST INFRASTRUCTURE ONLY.  Host build of the closed-loop ensemble: obca_amd/csrc/obca_ensemble.h (over obca_track.h and obca_rollout.h) compiled with -DOBCA_EMU, where
// every PAR(lane) region is a plain loop over the 64 lanes, SYNC is nothing and the work buffers are the caller's memory.  tests/test_ensemble_cpu.py compares it with the
// numpy statements of obca_amd/validate.py on a machine without a GPU, tests/test_gpu_ensemble.py compares the device with it.  It is never linked into libobca_hip.so.
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
#include "../../obca_amd/csrc/obca_ensemble.h"
using namespace obca;

static std::string g_en_err;

extern "C" {
const char *emu_ensemble_last_error() { return g_en_err.c_str(); }
int emu_ensemble_sizes(int *mem, int *out, int *mmax) { *mem = EN_MEM; *out = EN_OUT; *mmax = EN_MMAX; return 0; }
// one instance: prob / z / ts / vmax as emu_track_parking takes them; members M; q 4, r 2, qf 4; dx0 4 x M or NULL, dub 2 x M or NULL (zeros); rev: deal the linearisation
// items to the lanes backwards; mem M x EN_MEM, fin M x 4, out EN_OUT
int emu_ensemble_parking(int N, const double *prob, const double *z, const double *ts, int vmax, int substeps, int members, int feedback, int clamp, const double *q, const double *r,
                         const double *qf, const double *dx0, const double *dub, double need, int rev, double *mem, double *fin, double *out) {
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, 4, 2, need)) { g_en_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !mem || !fin || !out) { g_en_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    const trk::Weights w = trk::make_weights(q, r, qf, 4, 2);
    std::vector<double> AB(ens::ensemble_ab_len(N, 4, 2)), K(trk::track_gain_len(N, 4, 2)), d0((size_t)4 * members, 0.0), db((size_t)2 * members, 0.0);      // the work buffers; what the library packs
    if (dx0) memcpy(d0.data(), dx0, sizeof(double) * d0.size());
    if (dub) memcpy(db.data(), dub, sizeof(double) * db.size());
    if (vmax <= 2) ens::ensemble_parking_instance<2>(N, prob, z, ts, substeps, members, feedback, clamp, w, d0.data(), db.data(), need, rev, AB.data(), K.data(), mem, fin, out);
    else if (vmax <= OB_VMID) ens::ensemble_parking_instance<OB_VMID>(N, prob, z, ts, substeps, members, feedback, clamp, w, d0.data(), db.data(), need, rev, AB.data(), K.data(), mem, fin, out);
    else ens::ensemble_parking_instance<OB_VMAX>(N, prob, z, ts, substeps, members, feedback, clamp, w, d0.data(), db.data(), need, rev, AB.data(), K.data(), mem, fin, out);
    return 0;
}
// one instance: prob, x, u, ts, tstride as emu_track_quad takes them; q 12, r 4, qf 12; dx0 12 x M or NULL, dub 4 x M or NULL; fin M x 12
int emu_ensemble_quad(int N, const double *prob, const double *x, const double *u, const double *ts, int tstride, int substeps, int members, int feedback, int clamp, const double *q,
                      const double *r, const double *qf, const double *dx0, const double *dub, double need, int rev, double *mem, double *fin, double *out) {
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, QX, QU, need)) { g_en_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !u || !ts || !mem || !fin || !out) { g_en_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    const trk::Weights w = trk::make_weights(q, r, qf, QX, QU);
    std::vector<double> AB(ens::ensemble_ab_len(N, QX, QU)), K(trk::track_gain_len(N, QX, QU)), d0((size_t)QX * members, 0.0), db((size_t)QU * members, 0.0);
    if (dx0) memcpy(d0.data(), dx0, sizeof(double) * d0.size());
    if (dub) memcpy(db.data(), dub, sizeof(double) * db.size());
    ens::ensemble_quad_instance(N, prob, x, u, ts, tstride, substeps, members, feedback, clamp, w, d0.data(), db.data(), need, rev, AB.data(), K.data(), mem, fin, out);
    return 0;
}
// the instance record of a member table (M x EN_MEM), as phase 4 forms it
int emu_ensemble_reduce(int members, int substeps, int feedback, int clamp, int inst_bad, const double *mem, double *out) {
    if (members < 1 || members > EN_MMAX || !mem || !out) { g_en_err = "need 1 <= members <= 64 and no NULL argument"; return -1; }
    ens::ensemble_reduce(members, substeps, feedback, clamp, inst_bad, mem, out);
    return 0;
}
}
