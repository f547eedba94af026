// TEST INFRASTRUCTURE ONLY.  Host build of the clearance certificate: obca_amd/csrc/obca_certify.h (over obca_clearance.h) compiled with -DOBCA_EMU, where every PAR(lane)
// region is a plain loop over the 64 lanes, SYNC is nothing and the item table is the caller's memory.  tests/test_certify_cpu.py compares it with the numpy statements of
// obca_amd/validate.py on a machine without a GPU, tests/test_gpu_certify.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_clearance.h"
#include "../../obca_amd/csrc/obca_certify.h"
using namespace obca;

static std::string g_ct_err;

extern "C" {
const char *emu_certify_last_error() { return g_ct_err.c_str(); }
int emu_certify_sizes(int *out, int *ticks, int *item) { *out = CT_OUT; *ticks = CT_TICKS; *item = CT_ITEM; return 0; }
// the refusal of certify_check_args for these arguments ("" if none)
const char *emu_certify_check_args(double need, double slack, int max_steps) { const char *bad = cert::certify_check_args(need, slack, max_steps); return bad ? bad : ""; }
// Lambda of one parking interval: x 4, u 2, h = timeScale[k] Ts, ego as the problem record holds it (off = PH_OFF, g = PH_G ..); and of one quadcopter node (xk 12)
double emu_certify_lipschitz_parking(const double *x, const double *u, double h, double L, double off, const double *g) { return cert::lipschitz_parking(x, u, h, L, cert::car_radius(off, g[0], g[1])); }
double emu_certify_lipschitz_quad(const double *xk) { return cert::lipschitz_quad(xk); }
// one instance: prob / z as tests/packing.py packs them (x, u and t of z are read), ts (N + 1) or NULL; vmax: the widest obstacle of the BATCH the instance belongs to
// (the row class, as launch_dualws picks it); rev: deal the items to the lanes backwards; iv 2 (N + 1), out CT_OUT; items: the item table (3 x (N + 1) x nOb) or NULL
int emu_certify_parking(int N, const double *prob, const double *z, const double *ts, int vmax, double need, double slack, int max_steps, int rev, double *iv, double *out, double *items) {
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { g_ct_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !iv || !out) { g_ct_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    std::vector<double> work(cert::certify_work_len(N, (int)prob[PH_NOB]), 0.0);
    if (vmax <= 2) cert::certify_parking_instance<2>(N, prob, z, ts, need, slack, max_steps, rev, work.data(), iv, out);
    else if (vmax <= OB_VMID) cert::certify_parking_instance<OB_VMID>(N, prob, z, ts, need, slack, max_steps, rev, work.data(), iv, out);
    else cert::certify_parking_instance<OB_VMAX>(N, prob, z, ts, need, slack, max_steps, rev, work.data(), iv, out);
    if (items) memcpy(items, work.data(), sizeof(double) * work.size());
    return 0;
}
// one instance: prob as tests/packing.py packs it (Ts, R and the boxes are read), x (N + 1) x 12, ts[k * tstride]
int emu_certify_quad(int N, const double *prob, const double *x, const double *ts, int tstride, double need, double slack, int max_steps, int rev, double *iv, double *out, double *items) {
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { g_ct_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !ts || !iv || !out) { g_ct_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    std::vector<double> work(cert::certify_work_len(N, QOB), 0.0);
    cert::certify_quad_instance(N, prob, x, ts, tstride, need, slack, max_steps, rev, work.data(), iv, out);
    if (items) memcpy(items, work.data(), sizeof(double) * work.size());
    return 0;
}
// the parking clearance of ONE pose against obstacle j of the problem record, as the item loop computes it (the host build's own distance, for the numpy statement):
// pose (x, y, yaw)
double emu_certify_pose_clearance(const double *prob, int vmax, const double *pose, int j) {
    const int v = (int)prob[PH_VOB + j], r0 = (int)prob[PH_ROFF + j];
    double a1[OB_VMAX], a2[OB_VMAX], bj[OB_VMAX], g[4], lm[OB_VMAX], mu[4], d;
    for (int i = 0; i < OB_VMAX; i++) { const bool on = i < v; a1[i] = on ? prob[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? prob[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? prob[PH_B + r0 + i] : 0.0; }
    for (int i = 0; i < 4; i++) g[i] = prob[PH_G + i];
    const double sn = sin(pose[2]), cs = cos(pose[2]), off = prob[PH_OFF];
    if (vmax <= 2) dualws_one<2>(v, a1, a2, bj, g, pose[0] + cs * off, pose[1] + sn * off, cs, sn, lm, mu, &d);
    else if (vmax <= OB_VMID) dualws_one<OB_VMID>(v, a1, a2, bj, g, pose[0] + cs * off, pose[1] + sn * off, cs, sn, lm, mu, &d);
    else dualws_one<OB_VMAX>(v, a1, a2, bj, g, pose[0] + cs * off, pose[1] + sn * off, cs, sn, lm, mu, &d);
    return d < CL_TOUCH ? 0.0 : d;
}
// the same for n poses (n x 3) against every obstacle of the record: out n x nOb
int emu_certify_pose_table(const double *prob, int vmax, const double *poses, int n, double *out) {
    const int nOb = (int)prob[PH_NOB];
    for (int q = 0; q < n; q++)
        for (int j = 0; j < nOb; j++) out[(size_t)q * nOb + j] = emu_certify_pose_clearance(prob, vmax, poses + 3 * (size_t)q, j);
    return 0;
}
}
