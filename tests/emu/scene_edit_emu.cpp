// TEST INFRASTRUCTURE ONLY.  Host build of the scene edit: obca_amd/csrc/obca_scene_edit.h (over obca_validate.h) compiled with -DOBCA_EMU, where every PAR(lane) region is
// a plain loop over the 64 lanes and a value fetched from another lane is an array element.  tests/test_scene_edit_cpu.py compares it with the numpy statements of
// obca_amd/validate.py on a machine without a GPU, tests/test_gpu_scene_edit.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <string>
#include "../../obca_amd/csrc/obca_validate.h"
#include "../../obca_amd/csrc/obca_scene_edit.h"
using namespace obca;

static std::string g_se_err;

extern "C" {
const char *emu_scene_edit_last_error() { return g_se_err.c_str(); }
int emu_scene_edit_sizes(int *pin, int *qin, int *nobmax, int *mmax) { *pin = SE_PIN; *qin = SE_QIN; *nobmax = OB_NOBMAX; *mmax = OB_MMAX; return 0; }
// B parking records (rw) at stride s_prob; in: s_in doubles per instance, SE_PIN per obstacle; status: B doubles.  Refuses a record whose counts leave the header.
int emu_move_parking(int B, double *prob, long long s_prob, const double *in, long long s_in, int rev, double *status) {
    if (B < 1 || !prob || !in || !status || s_prob < OB_HDR) { g_se_err = "need B >= 1, s_prob >= OB_HDR and no NULL argument"; return -1; }
    for (int i = 0; i < B; i++) {
        const double *p = prob + (size_t)i * s_prob;
        if (!(p[PH_NOB] >= 0 && p[PH_NOB] <= OB_NOBMAX && p[PH_M] >= 0 && p[PH_M] <= OB_MMAX && SE_PIN * p[PH_NOB] <= (double)s_in)) { g_se_err = "counts out of range"; return -1; }
    }
    for (int i = 0; i < B; i++) sed::move_parking_instance(prob + (size_t)i * s_prob, in + (size_t)i * s_in, rev, status + i);
    return 0;
}
// B quadcopter records (rw) at stride s_prob; in: SE_QIN x 5 doubles per instance; status: B doubles
int emu_move_quad(int B, double *prob, long long s_prob, const double *in, int rev, double *status) {
    if (B < 1 || !prob || !in || !status || s_prob < QPH_SIZE) { g_se_err = "need B >= 1, s_prob >= QPH_SIZE and no NULL argument"; return -1; }
    for (int i = 0; i < B; i++) sed::move_quad_instance(prob + (size_t)i * s_prob, in + (size_t)i * QOB * SE_QIN, rev, status + i);
    return 0;
}
}
