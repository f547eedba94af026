// TEST INFRASTRUCTURE ONLY.  Host build of the parking receding-horizon shift: obca_amd/csrc/obca_shift.h compiled with -DOBCA_EMU, where every PAR(lane) region is a plain
// loop over the 64 lanes and SYNC is nothing.  tests/test_shift_cpu.py compares it bit for bit with a numpy statement of the same rules (tests/shift_common.py) on a machine
// without a GPU.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include "../../obca_amd/csrc/obca_shift.h"
using namespace obca;

extern "C" {
// the solver's layout of an instance, in the order of tests/packing.py (LAYOUT_FIELDS: 26 ints), and the header length
int emu_shift_layout(int N, int nOb, int M, int *out, int *hdr) {
    Lay l; make_layout(N, nOb, M, l);
    const int v[26] = {l.x, l.u, l.t, l.lam, l.mu, l.sl, l.so, l.ss, l.pi, l.nu, l.yg, l.yo, l.zxL, l.zxU, l.zuL, l.zuU, l.ztL, l.ztU, l.zlam, l.zmu, l.zso, l.zssL, l.zssU, l.zs1,
                       l.nprimal, l.len};
    memcpy(out, v, sizeof v); *hdr = OB_HDR;
    return 0;
}
// B instances addressed as the kernel addresses them: record strides s_prob / s_z (the batch's widest instance), tmp with the stride of z (the direction buffer);
// prob (rw) / z / z0 (w) as tests/packing.py packs them; x0_new: 4 x B or NULL; rev: deal the items to the lanes backwards.  Refuses what the C ABI refuses.
int emu_shift_batch(int B, int N, int shift, double *prob, long long s_prob, const double *z, double *z0, double *tmp, long long s_z, const double *x0_new, int rev) {
    if (B < 1 || N < 1 || N > OB_NMAX || shift < 0 || shift > N || !prob || !z || !z0 || !tmp) return -1;
    if (s_prob < OB_HDR + 3 * (N + 1) || s_z < 3 * (N + 1)) return -1;
    for (int i = 0; i < B; i++) {
        const double *p = prob + (size_t)i * s_prob;
        const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
        if (nOb < 1 || nOb > OB_NOBMAX || M < nOb || M > OB_MMAX) return -1;
        Lay l; make_layout(N, nOb, M, l);
        if (l.len > s_z) return -1;
    }
    for (int i = 0; i < B; i++)
        shf::shift_instance(N, shift, prob + (size_t)i * s_prob, z + (size_t)i * s_z, z0 + (size_t)i * s_z, tmp + (size_t)i * s_z, x0_new ? x0_new + (size_t)i * 4 : nullptr, rev);
    return 0;
}
}
