// TEST INFRASTRUCTURE ONLY.  Host build of the round-synchronous Hybrid A* of the device: obca_amd/csrc/obca_hybrid.h compiled with -DOBCA_EMU, where every parallel loop
// is a sequential one (ascending, descending or in a fixed shuffled order), a barrier is nothing and an atomic is the plain operation.  tests/test_hybrid_cpu.py checks the
// design with it on a machine without a GPU, tests/test_gpu_hybrid.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_hybrid.h"
using namespace obca;

static std::string g_hy_err;

extern "C" {
const char *emu_hybrid_last_error() { return g_hy_err.c_str(); }
int emu_hybrid_sizes(int *maxmap, int *window, int *chunk, int *lds_bytes, int *node_bytes) {
    *maxmap = OBCA_HYBRID_MAXMAP; *window = HY_W; *chunk = HY_CH; *lds_bytes = (int)(OBCA_HYBRID_MAXMAP * sizeof(float) + HY_LDS_INTS * sizeof(int)); *node_bytes = (int)sizeof(hy::Node);
    return 0;
}
// obca_hybrid_astar_batch with the slot configuration and the loop order as arguments: `slots` slots take the instances slot, slot + slots, ... one after the other, as the
// persistent workgroups of the device do.  map_out (nx * ny floats, or NULL): the holonomic map of the LAST instance; blocked_out (nx * ny bytes, or NULL); dims (2, or NULL): nx, ny.
int emu_hybrid_astar_batch(int B, const double *starts, const double *goals, int nOb, const int *vOb, const double *A, const double *b, const double *ego, double L,
                           const double *XYbounds, const double *opts, int nopts, double bucket_width, double *paths, int *dirs, int cap, int *counts, int *expansions,
                           int *rounds, int slots, int max_nodes, int max_chunks, int order, float *map_out, unsigned char *blocked_out, int *dims) {
    if (!paths || !dirs || !counts) { g_hy_err = "NULL output"; return -1; }
    if (slots < 1 || slots > OBCA_HYBRID_MAXSLOTS || max_nodes < 0 || max_nodes > OBCA_HYBRID_MAXNODES || max_chunks < 0 || order < 0 || order > 2) { g_hy_err = "slot configuration out of range"; return -1; }
    const int mn = max_nodes ? max_nodes : OBCA_HYBRID_MAXNODES, mc = max_chunks ? max_chunks : hy::default_chunks(mn);
    hy::Params P; hy::HostField W; std::vector<unsigned char> blocked; std::vector<double> inst;
    if (const char *bad = hy::make_params(B, starts, goals, nOb, vOb, A, b, ego, L, XYbounds, opts, nopts, bucket_width, cap, mn, mc, P, W, blocked, inst)) { g_hy_err = bad; return -1; }
    hy::Field F; F.nOb = nOb; F.v = W.v.data(); F.off = W.off.data(); F.voff = W.voff.data(); F.A = W.A.data(); F.b = W.b.data(); F.rn = W.rn.data(); F.vert = W.vert.data();
    if (dims) { dims[0] = P.nx; dims[1] = P.ny; }
    if (blocked_out) memcpy(blocked_out, blocked.data(), blocked.size());
    const size_t sb = hy::slot_bytes(P.ncell, mn, mc);
    std::vector<float> hmap((size_t)P.nmap); std::vector<int> li(HY_LDS_INTS);
    hy::emu_order = order;
    for (int s = 0; s < slots && s < B; s++) {
        void *block = malloc(sb);
        if (!block) { g_hy_err = "malloc failed"; return -2; }
        memset(block, 0xFF, hy::slot_init_bytes(P.ncell));
        const hy::SlotMem M = hy::carve(block, P.ncell, mn, mc);
        for (int i = s; i < B; i += slots) {
            hy::emu_map_out = (map_out && i == B - 1) ? map_out : nullptr;
            hy::search(P, F, blocked.data(), &inst[(size_t)i * 10], M, hmap.data(), li.data(), paths + (size_t)i * cap * 3, dirs + (size_t)i * cap, counts + i,
                       expansions ? expansions + i : nullptr, rounds ? rounds + i : nullptr);
        }
        free(block);
    }
    hy::emu_map_out = nullptr; hy::emu_order = 0;
    return 0;
}
}
