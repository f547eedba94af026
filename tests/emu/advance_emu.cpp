// TEST INFRASTRUCTURE ONLY.  Host build of the closed-loop step: obca_amd/csrc/obca_advance.h (over obca_rollout.h, obca_shift.h and obca_quad_shift.h) compiled with
// -DOBCA_EMU, where every PAR(lane) region is a plain loop over the 64 lanes, SYNC is nothing and the work buffers are the caller's memory.  tests/test_advance_cpu.py
// compares it with the numpy statements of obca_amd/validate.py and of the shift tests on a machine without a GPU, tests/test_gpu_advance.py compares the device with it.
// It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_clearance.h"
#include "../../obca_amd/csrc/obca_rollout.h"
#include "../../obca_amd/csrc/obca_shift.h"
#include "../../obca_amd/csrc/obca_quad_shift.h"
#include "../../obca_amd/csrc/obca_advance.h"
using namespace obca;

static std::string g_av_err;

extern "C" {
const char *emu_advance_last_error() { return g_av_err.c_str(); }
int emu_advance_sizes(int *out, int *clr, int *smax) { *out = AV_OUT; *clr = RO_CLR; *smax = CL_SMAX; return 0; }
// B instances addressed as the kernel addresses them: prob (rw) at stride s_prob, z / z0 (w) / tmp at stride s_z as tests/packing.py packs them; vmax: the widest obstacle
// of the batch; kick: 4 x B or NULL; st: 4 x B; log: B x cap x 4 or NULL with `logged` nodes in it; out: AV_OUT x B.  Refuses what the C ABI refuses, before anything is written.
int emu_advance_parking(int B, int N, int shift, double *prob, long long s_prob, const double *z, double *z0, double *tmp, long long s_z, int vmax, int substeps, const double *kick,
                        double need, int rev, double *st, double *log, int cap, int logged, double *out) {
    if (B < 1 || N < 1 || N > OB_NMAX || !prob || !z || !z0 || !tmp || !st || !out) { g_av_err = "need B >= 1, 1 <= N <= OBCA_NMAX and no NULL argument"; return -1; }
    if (const char *bad = adv::advance_check_args(N, shift, substeps, need)) { g_av_err = bad; return -1; }
    if (log && logged + shift > cap) { g_av_err = "the log is full"; return -1; }
    std::vector<double> pose(adv::advance_pose_len(shift, substeps)), X(adv::advance_state_len(shift, 4));      // the work buffer of one instance
    for (int i = 0; i < B; i++) {
        double *p = prob + (size_t)i * s_prob, *lg = log ? log + ((size_t)i * cap + logged) * 4 : nullptr;
        const double *zi = z + (size_t)i * s_z, *kk = kick ? kick + (size_t)i * 4 : nullptr;
        double *z0i = z0 + (size_t)i * s_z, *ti = tmp + (size_t)i * s_z, *si = st + (size_t)i * 4, *oi = out + (size_t)i * AV_OUT;
        const double lgd = log ? (double)(logged + shift) : -1.0;
        if (vmax <= 2) adv::advance_parking_instance<2>(N, shift, p, zi, z0i, ti, substeps, kk, need, rev, pose.data(), X.data(), si, lg, lgd, oi);
        else if (vmax <= OB_VMID) adv::advance_parking_instance<OB_VMID>(N, shift, p, zi, z0i, ti, substeps, kk, need, rev, pose.data(), X.data(), si, lg, lgd, oi);
        else adv::advance_parking_instance<OB_VMAX>(N, shift, p, zi, z0i, ti, substeps, kk, need, rev, pose.data(), X.data(), si, lg, lgd, oi);
    }
    return 0;
}
// B instances: prob (rw) at stride s_prob, z at stride s_z, info 8 x B; kick / xF_new: 12 x B or NULL; st: 12 x B; log: B x cap x 12 or NULL
int emu_advance_quad(int B, int N, int shift, double *prob, long long s_prob, const double *z, long long s_z, const double *info, int substeps, const double *kick, const double *xF_new,
                     double need, int rev, double *st, double *log, int cap, int logged, double *out) {
    if (B < 1 || N < 1 || N > QNMAX || !prob || !z || !info || !st || !out) { g_av_err = "need B >= 1, 1 <= N <= OBCA_QUAD_NMAX and no NULL argument"; return -1; }
    if (const char *bad = adv::advance_check_args(N, shift, substeps, need)) { g_av_err = bad; return -1; }
    if (log && logged + shift > cap) { g_av_err = "the log is full"; return -1; }
    std::vector<double> pose(adv::advance_pose_len(shift, substeps)), X(adv::advance_state_len(shift, QX));
    for (int i = 0; i < B; i++)
        adv::advance_quad_instance(N, shift, prob + (size_t)i * s_prob, z + (size_t)i * s_z, info + (size_t)i * 8, substeps, kick ? kick + (size_t)i * QX : nullptr,
                                   xF_new ? xF_new + (size_t)i * QX : nullptr, need, rev, pose.data(), X.data(), st + (size_t)i * QX,
                                   log ? log + ((size_t)i * cap + logged) * QX : nullptr, log ? (double)(logged + shift) : -1.0, out + (size_t)i * AV_OUT);
    return 0;
}
}
