// TEST INFRASTRUCTURE ONLY.  A stand-alone program (its own main) around the host build of obca_amd/csrc/obca_quad_subdivide.h, for the host compiler's address and
// undefined-behaviour sanitizers: tests/test_quad_refine_cpu.py compiles it with -fsanitize=address,undefined and runs it.  Every buffer comes from malloc with exactly the
// size the HIP host code of obca_hip.hip gives it -- the staging block of obca_quadcopter_subdivide_batch, [ Ts B | x | timeScale | Ts_f B | x_f ]; the problem records,
// iterates and info of a source and a destination obca_quad_batch -- and the instances are addressed as the two kernels address them, so an access one double outside any of
// them ends the run.  Shapes: those of the tests, with B = 1 (the block ends behind the only instance) and B = 3.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include "../../obca_amd/csrc/obca_quad_subdivide.h"
using namespace obca;

static double *block(size_t n, double fill) {
    double *p = (double *)malloc(n * sizeof(double));
    if (!p) { fprintf(stderr, "malloc failed\n"); exit(2); }
    for (size_t i = 0; i < n; i++) p[i] = fill;
    return p;
}
static void wave(double *x, size_t n, double a) { for (size_t i = 0; i < n; i++) x[i] = a + 0.01 * (double)(i % 97); }

static int host_call(int B, int N, int r, bool with_ts, int nan_inst) {
    const size_t Nf = (size_t)N * r, nx = (size_t)B * QX * (N + 1), nt = with_ts ? (size_t)B * (N + 1) : 0, nin = B + nx + nt, nxf = (size_t)B * QX * (Nf + 1);
    double *d = block(nin + B + nxf, -7.25);
    wave(d, B, 0.3); wave(d + B, nx, 1.0); if (nt) wave(d + B + nx, nt, 0.9);
    if (nan_inst >= 0) d[B + (size_t)nan_inst * QX * (N + 1) + 5] = NAN;
    const double *Ts = d, *x = d + B, *ts = nt ? d + B + nx : nullptr;
    double *Tsf = d + nin, *xf = Tsf + B;
    int bad = 0;
    for (int rev = 0; rev < 2; rev++)
        for (size_t i = 0; i < (size_t)B; i++) {
            const int rc = qsd::subdivide_host_instance(N, r, Ts[i], x + i * QX * (N + 1), ts ? ts + i * (N + 1) : nullptr, rev, Tsf + i, xf + i * QX * (Nf + 1));
            if (rc != ((int)i == nan_inst)) bad++;
            for (size_t k = 0; k < QX * (Nf + 1); k++) if ((xf[i * QX * (Nf + 1) + k] != xf[i * QX * (Nf + 1) + k]) != ((int)i == nan_inst)) bad++;
        }
    free(d);
    return bad;
}

static int resident_call(int B, int n, int N, int r, double margin, int failed) {
    quad::QLay ls; quad::q_make_layout(N, ls);
    const size_t Nf = (size_t)N * r, sp = QPH_SIZE + QX * (N + 1), dp = QPH_SIZE + QX * (Nf + 1);
    double *prob = block((size_t)B * sp, 0.0), *z = block((size_t)B * ls.len, 0.5), *info = block((size_t)B * 8, 1.0), *pd = block((size_t)n * dp, -7.25);
    wave(prob, (size_t)B * sp, 0.2); wave(z, (size_t)B * ls.len, 1.1);
    if (failed >= 0) info[(size_t)failed * 8 + 7] = 0.0;
    int bad = 0;
    for (int rev = 0; rev < 2; rev++)
        for (int j = 0; j < n; j++) {
            const size_t i = (size_t)((j * 2 + 1) % B);      // a selection with repeats
            const int st = qsd::subdivide_record(N, r, margin, prob + i * sp, z + i * ls.len, info + i * 8, rev, pd + (size_t)j * dp);
            if (st != ((int)i == failed)) bad++;
        }
    for (size_t k = 0; k < (size_t)n * dp; k++) if (pd[k] == -7.25) bad++;      // every word of every record was written
    free(prob); free(z); free(info); free(pd);
    return bad;
}

int main() {
    const int shapes[][2] = {{1, 1}, {2, 3}, {7, 4}, {60, 2}, {4, 32}, {128, 1}};
    int bad = 0, runs = 0;
    for (const auto &s : shapes)
        for (int B : {1, 3}) {
            bad += host_call(B, s[0], s[1], true, -1) + host_call(B, s[0], s[1], false, B - 1);
            bad += resident_call(B, B, s[0], s[1], 0.0, -1) + resident_call(B, B + 1, s[0], s[1], 0.02, 0);
            runs += 4;
        }
    printf("quad_subdivide_check: %d calls, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
