// TEST INFRASTRUCTURE ONLY.  Host build of the planner's RESIDENT route (obca_batch_plan_warm_start, include/obca_plan_resident.h): obca_amd/csrc/obca_plan_resident.h,
// obca_hybrid.h and obca_path_ws.h compiled with -DOBCA_EMU, called in the order the host layer launches them -- the packing over problem records as tests/packing.py packs
// them, the per-instance search over exactly that packed block, pw::path_ws_record behind it.  tests/test_plan_resident_cpu.py checks the route with it on a machine
// without a GPU, tests/test_gpu_plan_resident.py compares the device with it.  It is never linked into libobca_hip.so.
#define OBCA_EMU 1
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include "../../obca_amd/csrc/obca_hybrid.h"
#include "../../obca_amd/csrc/obca_path_ws.h"
#include "../../obca_amd/csrc/obca_plan_resident.h"
using namespace obca;

static std::string g_plr_err;

static void pack_all(int B, const double *prob, long long s_prob, int nObMax, int MMax, const double *XYbounds, int order, const plr::Block &blk) {
    const double far_ = hy::host_far(XYbounds);
    hy::emu_order = order;
    for (int i = 0; i < B; i++) plr::plan_pack_instance(i, nObMax, MMax, far_, prob + (size_t)i * s_prob, blk);
    hy::emu_order = 0;
}

// the whole route.  block_given: NULL, or a whole packed block (plr::layout's bytes: the device's own) that stands in for the one the packing would write here
static int plan_impl(int B, int N, double *prob, long long s_prob, double *z0, int zlen, int nObMax, int MMax, const double *ego, double L, const double *XYbounds,
                     const double *opts, int nopts, double bucket_width, int cap, int use_xF, double v_nom, double a_max, int slots, int max_nodes, int max_chunks, int order,
                     const char *block_given, double *paths, int *dirs, int *counts, int *expansions, int *rounds, int *status, double *inst_out) {
    if (!prob || !z0 || !paths || !dirs || !counts || !status || !expansions || !rounds) { g_plr_err = "NULL argument"; return -1; }
    if (slots < 1 || slots > OBCA_HYBRID_MAXSLOTS || max_nodes < 0 || max_nodes > OBCA_HYBRID_MAXNODES || max_chunks < 0 || order < 0 || order > 2) { g_plr_err = "slot configuration out of range"; return -1; }
    if (cap < 2 || cap > PW_MAXNODES) { g_plr_err = "need 2 <= cap <= OBCA_PATH_WS_MAXNODES"; return -1; }
    if (const char *bad = pw::path_ws_check_args(B, N, cap, v_nom, 1.0, a_max, true)) { g_plr_err = bad; return -1; }
    if (nObMax < 1 || nObMax > OB_NOBMAX || MMax < 1 || MMax > OB_MMAX) { g_plr_err = "nObMax or MMax out of range"; return -1; }
    const int mn = max_nodes ? max_nodes : OBCA_HYBRID_MAXNODES, mc = max_chunks ? max_chunks : hy::default_chunks(mn);
    hy::Params P; hy::HostField none; std::vector<unsigned char> free_map; std::vector<double> pose;
    const double origin[3] = {0.0, 0.0, 0.0};
    if (const char *bad = hy::make_params(1, origin, origin, 0, nullptr, nullptr, nullptr, ego, L, XYbounds, opts, nopts, bucket_width, cap, mn, mc, P, none, free_map, pose)) { g_plr_err = bad; return -1; }
    const plr::Layout lay = plr::layout(B, nObMax, MMax);
    std::vector<double> mem(lay.bytes / 8, 0.0);
    const plr::Block blk = plr::block_at((char *)mem.data(), lay);
    if (block_given) memcpy(mem.data(), block_given, lay.bytes);
    else pack_all(B, prob, s_prob, nObMax, MMax, XYbounds, order, blk);
    // a block from outside is read through field_of like any other: its offsets are checked against the block first
    for (int i = 0; block_given && i < B; i++) {
        const int *rec = blk.rec + 4 * (size_t)i; const int nOb = rec[3];
        bool ok = rec[0] == i * nObMax && rec[1] == i * MMax && rec[2] == i * nObMax * PLR_NV && nOb >= 0 && nOb <= nObMax;
        for (int j = 0; ok && j < nOb; j++) {
            const int v = blk.v[rec[0] + j], o = blk.off[rec[0] + i + j], vo = blk.voff[rec[0] + i + j], vn = blk.voff[rec[0] + i + j + 1];
            ok = v >= 0 && o >= 0 && o + v <= MMax && vo >= 0 && vn >= vo && vn <= nObMax * PLR_NV;
        }
        if (!ok) { g_plr_err = "the given block's offsets leave the block"; return -1; }
    }
    if (inst_out) memcpy(inst_out, blk.inst, (size_t)B * 80);
    const hy::Fields S = plr::fields_of(blk);
    const size_t sb = hy::slot_bytes(P.ncell, mn, mc);
    std::vector<float> hmap((size_t)P.nmap); std::vector<int> li(HY_LDS_INTS);
    hy::emu_order = order;
    for (int s = 0; s < slots && s < B; s++) {
        void *block = malloc(sb);
        if (!block) { g_plr_err = "malloc failed"; hy::emu_order = 0; return -2; }
        memset(block, 0xFF, hy::slot_init_bytes(P.ncell));
        const hy::SlotMem M = hy::carve(block, P.ncell, mn, mc);
        for (int i = s; i < B; i += slots)
            hy::search(P, hy::field_of(S, i), nullptr, blk.inst + (size_t)i * 10, M, hmap.data(), li.data(), paths + (size_t)i * cap * 3, dirs + (size_t)i * cap, counts + i, expansions + i, rounds + i);
        free(block);
    }
    hy::emu_order = 0;
    for (int i = 0; i < B; i++)
        status[i] = pw::path_ws_record(N, counts[i], cap, paths + (size_t)i * cap * 3, dirs + (size_t)i * cap, use_xF, v_nom, a_max, prob + (size_t)i * s_prob, z0 + (size_t)i * zlen, zlen);
    return 0;
}

extern "C" {
const char *emu_plr_last_error() { return g_plr_err.c_str(); }
// byte offsets of plr::Layout (inst, A, b, rn, nrm, vert, rec, v, off, voff, bytes) and the vertices of an obstacle's block
int emu_plr_layout(int B, int nObMax, int MMax, long long *out /* 11 */, int *nv) {
    const plr::Layout l = plr::layout(B, nObMax, MMax);
    const size_t v[11] = {l.inst, l.A, l.b, l.rn, l.nrm, l.vert, l.rec, l.v, l.off, l.voff, l.bytes};
    for (int i = 0; i < 11; i++) out[i] = (long long)v[i];
    *nv = PLR_NV;
    return 0;
}
// plan_pack_instance over B records of s_prob doubles each into `block` (emu_plr_layout's bytes); order: the obstacles (and rows) of an instance ascending, descending, shuffled
int emu_plr_pack(int B, const double *prob, long long s_prob, int nObMax, int MMax, const double *XYbounds, int order, char *block) {
    if (!prob || !XYbounds || !block || B < 1 || nObMax < 1 || nObMax > OB_NOBMAX || MMax < 1 || MMax > OB_MMAX || order < 0 || order > 2) { g_plr_err = "bad arguments"; return -1; }
    pack_all(B, prob, s_prob, nObMax, MMax, XYbounds, order, plr::block_at(block, plr::layout(B, nObMax, MMax)));
    return 0;
}
// what the host route makes of the same scenes (hy::make_scenes): the fields of hy::make_fields, flat as `Fields` reads them, and make_params' instance records.
// The arrays hold at least: rec 4 B, v sum(nOb), off / voff sum(nOb) + B, A 2 rows, b / rn / nrm rows, vert 2 x 17 per obstacle, inst 10 B.  sizes: rows, obstacles, vertices.
int emu_plr_host_fields(int B, const double *starts, const double *goals, const int *nOb, const int *vOb, const double *A, const double *b, const double *ego, double L,
                        const double *XYbounds, int *rec, int *v, int *off, int *voff, double *A_, double *b_, double *rn, double *nrm, double *vert, double *inst, int *sizes) {
    hy::Params P; hy::HostFields W; std::vector<double> in;
    const std::string bad = hy::make_scenes(B, starts, goals, nOb, vOb, A, b, ego, L, XYbounds, nullptr, 0, 0.0, 2, 16, 16, P, W, in);
    if (!bad.empty()) { g_plr_err = bad; return -1; }
    memcpy(rec, W.rec.data(), W.rec.size() * 4); memcpy(v, W.v.data(), W.v.size() * 4); memcpy(off, W.off.data(), W.off.size() * 4); memcpy(voff, W.voff.data(), W.voff.size() * 4);
    memcpy(A_, W.A.data(), W.A.size() * 8); memcpy(b_, W.b.data(), W.b.size() * 8); memcpy(rn, W.rn.data(), W.rn.size() * 8); memcpy(nrm, W.nrm.data(), W.nrm.size() * 8);
    memcpy(vert, W.vert.data(), W.vert.size() * 8); memcpy(inst, in.data(), in.size() * 8);
    sizes[0] = (int)W.b.size(); sizes[1] = (int)W.v.size(); sizes[2] = (int)(W.vert.size() / 2);
    return 0;
}
// obca_batch_plan_warm_start on host memory: prob B x s_prob and z0 B x zlen are the batch's records and start iterates (rewritten where status is 0); the slot
// configuration and the loop order as arguments, as emu_scene_astar_batch.  inst_out: NULL, or B x 10 for the instance records the search read.
int emu_plr_plan(int B, int N, double *prob, long long s_prob, double *z0, int zlen, int nObMax, int MMax, const double *ego, double L, const double *XYbounds,
                 const double *opts, int nopts, double bucket_width, int cap, int use_xF, double v_nom, double a_max, int slots, int max_nodes, int max_chunks, int order,
                 double *paths, int *dirs, int *counts, int *expansions, int *rounds, int *status, double *inst_out) {
    return plan_impl(B, N, prob, s_prob, z0, zlen, nObMax, MMax, ego, L, XYbounds, opts, nopts, bucket_width, cap, use_xF, v_nom, a_max, slots, max_nodes, max_chunks, order,
                     nullptr, paths, dirs, counts, expansions, rounds, status, inst_out);
}
// the same over a packed block GIVEN by the caller (emu_plr_layout's bytes: the device's own, from obca_batch_packed_block): nothing is packed here, the search reads the
// caller's instance records and fields
int emu_plr_plan_given(int B, int N, double *prob, long long s_prob, double *z0, int zlen, int nObMax, int MMax, const double *ego, double L, const double *XYbounds,
                       const double *opts, int nopts, double bucket_width, int cap, int use_xF, double v_nom, double a_max, int slots, int max_nodes, int max_chunks, int order,
                       const char *block, double *paths, int *dirs, int *counts, int *expansions, int *rounds, int *status) {
    if (!block) { g_plr_err = "NULL block"; return -1; }
    return plan_impl(B, N, prob, s_prob, z0, zlen, nObMax, MMax, ego, L, XYbounds, opts, nopts, bucket_width, cap, use_xF, v_nom, a_max, slots, max_nodes, max_chunks, order,
                     block, paths, dirs, counts, expansions, rounds, status, nullptr);
}
}
