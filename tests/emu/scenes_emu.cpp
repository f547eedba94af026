// TEST INFRASTRUCTURE ONLY.  Host build of the device planner's PER-INSTANCE route (obca_scene_astar_batch, include/obca_plan_scenes.h): obca_amd/csrc/obca_hybrid.h
// compiled with -DOBCA_EMU as in hybrid_emu.cpp, the searches called the way the kernel's per-instance instantiation calls them -- the field of instance i from its
// record in the packed arrays (hy::field_of), no blocked map from the host.  tests/test_scenes_cpu.py checks the route with it on a machine without a GPU,
// tests/test_gpu_scenes.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_hybrid.h"
using namespace obca;

static std::string g_sc_err;

extern "C" {
const char *emu_scene_last_error() { return g_sc_err.c_str(); }
// obca_scene_astar_batch with the slot configuration and the loop order as arguments, as emu_hybrid_astar_batch.  which: the instance whose holonomic map goes to map_out
// (nx * ny floats, or NULL) and whose blocked cells -- hy::cell_blocked, the function the search calls -- go to blocked_out (nx * ny bytes, or NULL); dims (2, or NULL): nx, ny.
int emu_scene_astar_batch(int B, const double *starts, const double *goals, const int *nOb, const int *vOb, const double *A, const double *b, const double *ego, double L,
                          const double *XYbounds, const double *opts, int nopts, double bucket_width, double *paths, int *dirs, int cap, int *counts, int *expansions,
                          int *rounds, int slots, int max_nodes, int max_chunks, int order, int which, float *map_out, unsigned char *blocked_out, int *dims) {
    if (!paths || !dirs || !counts) { g_sc_err = "NULL output"; return -1; }
    if (slots < 1 || slots > OBCA_HYBRID_MAXSLOTS || max_nodes < 0 || max_nodes > OBCA_HYBRID_MAXNODES || max_chunks < 0 || order < 0 || order > 2) { g_sc_err = "slot configuration out of range"; return -1; }
    const int mn = max_nodes ? max_nodes : OBCA_HYBRID_MAXNODES, mc = max_chunks ? max_chunks : hy::default_chunks(mn);
    hy::Params P; hy::HostFields W; std::vector<double> inst;
    const std::string bad = hy::make_scenes(B, starts, goals, nOb, vOb, A, b, ego, L, XYbounds, opts, nopts, bucket_width, cap, mn, mc, P, W, inst);
    if (!bad.empty()) { g_sc_err = bad; return -1; }
    hy::Fields S; S.rec = W.rec.data(); S.v = W.v.data(); S.off = W.off.data(); S.voff = W.voff.data();
    S.A = W.A.data(); S.b = W.b.data(); S.rn = W.rn.data(); S.nrm = W.nrm.data(); S.vert = W.vert.data();
    if (dims) { dims[0] = P.nx; dims[1] = P.ny; }
    if (blocked_out && which >= 0 && which < B) {
        const hy::Field F = hy::field_of(S, which);
        for (int c = 0; c < P.nmap; c++) blocked_out[c] = hy::cell_blocked(P, F, c % P.nx, c / P.nx);
    }
    const size_t sb = hy::slot_bytes(P.ncell, mn, mc);
    std::vector<float> hmap((size_t)P.nmap); std::vector<int> li(HY_LDS_INTS);
    hy::emu_order = order;
    for (int s = 0; s < slots && s < B; s++) {
        void *block = malloc(sb);
        if (!block) { g_sc_err = "malloc failed"; return -2; }
        memset(block, 0xFF, hy::slot_init_bytes(P.ncell));
        const hy::SlotMem M = hy::carve(block, P.ncell, mn, mc);
        for (int i = s; i < B; i += slots) {
            hy::emu_map_out = (map_out && i == which) ? map_out : nullptr;
            hy::search(P, hy::field_of(S, i), nullptr, &inst[(size_t)i * 10], M, hmap.data(), li.data(), paths + (size_t)i * cap * 3, dirs + (size_t)i * cap, counts + i,
                       expansions ? expansions + i : nullptr, rounds ? rounds + i : nullptr);
        }
        free(block);
    }
    hy::emu_map_out = nullptr; hy::emu_order = 0;
    return 0;
}
}
