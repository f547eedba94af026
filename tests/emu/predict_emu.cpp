// TEST INFRASTRUCTURE ONLY.  Host build of the clearance prediction against moving obstacles: obca_amd/csrc/obca_predict.h (over the validate and clearance kernel texts)
// compiled with -DOBCA_EMU, where every PAR(lane) region is a plain loop over the 64 lanes, SYNC is nothing and the LDS marks and cum[] are local arrays.
// tests/test_predict_cpu.py compares it with the numpy statements of obca_amd/validate.py on a machine without a GPU, tests/test_gpu_predict.py compares the device with
// it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_clearance.h"
#include "../../obca_amd/csrc/obca_predict.h"
using namespace obca;

static std::string g_pr_err;

extern "C" {
const char *emu_predict_last_error() { return g_pr_err.c_str(); }
int emu_predict_sizes(int *out, int *pin, int *qin, int *clr_out) { *out = PR_OUT; *pin = PR_PIN; *qin = PR_QIN; *clr_out = CL_OUT; return 0; }
// one instance: prob / z as tests/packing.py packs them (x, u and t of z are read), ts (N + 1) or NULL, rates PR_PIN per obstacle; vmax: the widest obstacle of the BATCH
// the instance belongs to; rev: deal the samples to the lanes backwards; prof: N S + 1 doubles or NULL
int emu_predict_parking(int N, const double *prob, const double *z, const double *ts, const double *rates, int vmax, int substeps, double need, int rev, double *out, double *prof) {
    if (const char *bad = clr::clearance_check_args(substeps, need)) { g_pr_err = bad; return -1; }
    if (N < 1 || N > OB_NMAX || !prob || !z || !rates || !out) { g_pr_err = "need 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    if (vmax <= 2) prd::predict_parking_instance<2>(N, prob, z, ts, rates, substeps, need, rev, out, prof);
    else if (vmax <= OB_VMID) prd::predict_parking_instance<OB_VMID>(N, prob, z, ts, rates, substeps, need, rev, out, prof);
    else prd::predict_parking_instance<OB_VMAX>(N, prob, z, ts, rates, substeps, need, rev, out, prof);
    return 0;
}
// the distance the numpy statement is given: dualws_one of the class of vmax (geometry and centre offset of the record `prob`) for the car at pose (x, y, yaw) against the
// v rows A (v x 2), b the CALLER has moved -- no clamp
double emu_predict_pose_distance(const double *prob, int vmax, const double *pose, int v, const double *A, const double *b) {
    double a1[OB_VMAX] = {0}, a2[OB_VMAX] = {0}, bj[OB_VMAX] = {0}, g[4], lam[OB_VMAX], mu[4], d = 0.0;
    for (int i = 0; i < v && i < OB_VMAX; i++) { a1[i] = A[2 * i]; a2[i] = A[2 * i + 1]; bj[i] = b[i]; }
    for (int i = 0; i < 4; i++) g[i] = prob[PH_G + i];
    const double sn = sin(pose[2]), cs = cos(pose[2]), X = pose[0] + cs * prob[PH_OFF], Y = pose[1] + sn * prob[PH_OFF];
    if (vmax <= 2) { double p1[2] = {a1[0], a1[1]}, p2[2] = {a2[0], a2[1]}, pb[2] = {bj[0], bj[1]}; dualws_one<2>(v, p1, p2, pb, g, X, Y, cs, sn, lam, mu, &d); }
    else if (vmax <= OB_VMID) { double p1[OB_VMID], p2[OB_VMID], pb[OB_VMID]; for (int i = 0; i < OB_VMID; i++) { p1[i] = a1[i]; p2[i] = a2[i]; pb[i] = bj[i]; } dualws_one<OB_VMID>(v, p1, p2, pb, g, X, Y, cs, sn, lam, mu, &d); }
    else dualws_one<OB_VMAX>(v, a1, a2, bj, g, X, Y, cs, sn, lam, mu, &d);
    return d;
}
// one instance: prob as tests/packing.py packs it (Ts, R and the boxes are read), x (N + 1) x 12, ts[k * tstride], rates PR_QIN per box
int emu_predict_quad(int N, const double *prob, const double *x, const double *ts, int tstride, const double *rates, int substeps, double need, int rev, double *out, double *prof) {
    if (const char *bad = clr::clearance_check_args(substeps, need)) { g_pr_err = bad; return -1; }
    if (N < 1 || N > QNMAX || !prob || !x || !ts || !rates || !out) { g_pr_err = "need 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    prd::predict_quad_instance(N, prob, x, ts, tstride, rates, substeps, need, rev, out, prof);
    return 0;
}
}
