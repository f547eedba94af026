// obca_hybrid.h -- the parking planner on the device: a ROUND-SYNCHRONOUS Hybrid A*, one workgroup per search (include/obca_plan_device.h is the ABI).
//
// The host search (hybrid_astar_impl, obca_planner.cpp) pops one node at a time from a priority queue; that does not map onto a workgroup.  Here the
// open set lies in buckets of width bw in f = g + h and a ROUND takes every entry of the lowest non-empty bucket that is there when the round starts:
//   pass 1  : every entry whose node is no longer the one recorded for its cell is stale and is struck out; the others count as expansions and try to FINISH (goal
//             tolerances without the analytic expansion; else the shortest Reeds-Shepp curve to the goal, collision-tested every <= 0.2 m).  The cheapest finish of the
//             round wins through one 64-bit atomic minimum of (fp32 bits of g + curve length) << 32 | cell.
//   phase A : every (entry, primitive) pair is one item: integrate, collision-test each sub-step, g (fp32) and the cell.  Candidates no cheaper than what the cell holds
//             since the round started are dropped, the others do atomicMin(claim[cell], (bits of g) << 32 | parent cell * nprim + primitive).
//   phase B : after a barrier every item integrates again (no collision test) and the one whose word stands in the claim is the cell's winner: it takes a node from the
//             append-only pool (the handle comes from an atomic counter; handles are never compared with each other and never leave the search), records itself in the cell table,
//             clears the claim and takes a position in bucket max(current, floor(f / bw)) -- or in the far list, if that bucket lies beyond the window of bucket heads.
//             Then the buckets that grew take chunks from the slot's pool (one thread per bucket), the new nodes write their entries, the buckets are closed.
// Every decision is a minimum over a set fixed at the start of the round: the cell table is read in pass 1 and phase A and written in phase B only, a cell has one winner,
// a round one finish.  So paths, counts, expansions and rounds do not depend on the order in which lanes, waves or the entries of a bucket run; the host build
// (tests/emu/hybrid_emu.cpp, -DOBCA_EMU: every parallel loop a sequential one, ascending, descending or shuffled) returns the same bits, and so does the device as long as
// no libm result enters: the search itself calls none (heading as (sin, cos), rotated by per-primitive constants from the host; distances by sqrt), the Reeds-Shepp curves do.
// No contraction of a * b + c into an fma anywhere in this file.
// The holonomic map (2-D fp32 cost-to-go of a disc robot, per search: goals differ) is relaxed in LDS until nothing changes, as obca_plan3d.h does; the blocked cells, row
// norms, obstacle vertices and edge weights come from the host.
// Per-instance obstacle fields (include/obca_plan_scenes.h): the same search, called with the field of its own instance (field_of: a record of offsets into arrays that
// hold the fields of the whole batch, make_fields) and without a blocked map -- it then finds the blocked cells itself while it initialises the map (cell_blocked: the
// disc test the host's map comes from, the row norm read from memory, so still no libm), 512 threads sharing the cells.  Nothing else of a search depends on which route
// called it.
// The collision test, the disc test, the polygons and the Reeds-Shepp curves are obca_plan_geom.h's: ONE text, which the host search (obca_planner.cpp) compiles too.  The
// search loop, the holonomic map (relaxed here, a Dijkstra there), the primitives' integration and wrap() are each search's own.
// Every loop is bounded: rounds by P.maxrounds, expansions by maxexp (a round whose live entries would pass it is not expanded), sweeps by the cell count, the chain walk
// by the node count, wrap() by its own count.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/obca_plan.h"
#include "../../include/obca_plan_device.h"
#include "../../include/obca_plan_scenes.h"

#ifndef OBCA_EMU
// A file-scope pragma lasts to the end of the translation unit (the target knows no float_control push / pop): obca_hip.hip includes this header LAST, behind every
// other definition, so nothing but the planner is compiled under it.
#pragma clang fp contract(off)
#endif
#include "obca_plan_geom.h"      // behind the pragma: the geometry and the Reeds-Shepp curves this search shares with the host search (HY_FN, HY_HD, HY_PI come with them)
#ifndef HY_NT
#define HY_NT 512      // threads per workgroup = per search: 8 waves, two per SIMD (256 VGPRs each: the collision test clips polygons in registers)
#endif

namespace obca {
namespace hy {
using namespace geom;

#define HY_W OBCA_HYBRID_WINDOW
#define HY_CH OBCA_HYBRID_CHUNK
#define HY_CE (OBCA_HYBRID_CHUNK - 1)              // entries of a chunk (word 0 is the link)
#define HY_NSI (2 * OBCA_HYBRID_MAXSTEER + 1)
#define HY_CLIP (4 + OBCA_HYBRID_MAXROWS + 1)      // every half-plane adds at most one vertex to a convex polygon
#define HY_NONE 0xFFFFFFFFFFFFFFFFull
typedef unsigned long long u64;

// control words in LDS (ints), behind the five bucket arrays
enum { C_VOTE = 0, C_NNODES = 3, C_NTOUCH = 4, C_NFAR = 5, C_NCHUNK = 6, C_MINB = 7, C_OVER = 8, C_NFAR2 = 9, C_ALIVE = 10, C_CNT = 11, C_FIN = 16 /* u64 */, C_WORDS = 32 };
#define HY_LDS_INTS (5 * HY_W + 32)      // the five bucket arrays and C_WORDS control words

struct Params {      // one per call, built on the host (make_params)
    int nx, ny, nyaw, ncell, nmap, nst, nsi, nprim, sub, maxexp, analytic, rs_heur, cap, maxnodes, maxchunks, maxrounds, nOb, nrows, nvert, pad_;
    double xmin, xmax, ymin, ymax, res, yres, step, dsub, smax, margin, gtol, ytol, crev, csw, cst, cchg, hweight, L, Rmin, RminH, bw, ego[4];
    float w1, w2;                                          // edge weights of the holonomic map: (float)(res hypot(1, 0)), (float)(res hypot(1, 1))
    double kap[HY_NSI], steer[HY_NSI], sd[HY_NSI], cd[HY_NSI];      // per steering command: curvature, angle, sin / cos of the heading change of one forward sub-step
    double rad;                                            // radius of the disc robot of the holonomic map: 0.9 of the car's half width (or half length, if that is less)
};
struct Field : geom::Field {};      // the obstacle field of a search: the batch's (obca_hybrid_astar_batch), or the instance's own (obca_scene_astar_batch: field_of); under
                                    // the name the kernel's argument always had, so the kernels keep their symbols
// The fields of a batch of scenes, instance after instance in flat arrays (make_fields).  rec: four ints per instance -- where its obstacles, rows and polygon vertices
// start, and how many obstacles it has; off and voff carry one entry more than obstacles per instance (so instance i starts at its obstacle offset + i) and count from
// the instance's own first row / vertex.
struct Fields { const int *rec, *v, *off, *voff; const double *A, *b, *rn, *nrm, *vert; };
struct Node { double x, y, yaw, s, c; float g; int parent, cell, bucket, pos; signed char dir, si; };
struct SlotMem { Node *nodes; unsigned *cell_g; int *cell_node; u64 *claim; int *touched, *far, *chunks, *chunklist; };
struct Pose { double x, y, yaw, s, c; };

// ---------------------------------------------------------------- atomics, loops
#ifdef OBCA_EMU
static int emu_order = 0;      // items of a parallel loop in ascending (0), descending (1) or a fixed shuffled (2) order
static inline int emu_perm(int i, int n) { return emu_order == 0 ? i : (emu_order == 1 ? n - 1 - i : (n % 7919 ? (int)(((long long)i * 7919 + 13) % n) : n - 1 - i)); }
#define HY_FOR(i, n) for (int i##_ = 0, i##n_ = (n), i = 0; i##_ < i##n_ && ((i = emu_perm(i##_, i##n_)), true); i##_++)
#define HY_LFOR(i, n) for (int i = 0; i < (n); i++)
#define HY_TID0 1
#define HY_WAVE0 1
#define HY_LANE0 1
#define HY_BARRIER() ((void)0)
static inline int aadd(int *p, int v) { const int o = *p; *p = o + v; return o; }
static inline void amin32(int *p, int v) { if (v < *p) *p = v; }
static inline void amin64(u64 *p, u64 v) { if (v < *p) *p = v; }
static inline u64 aload64(const u64 *p) { return *p; }
static inline void astore64(u64 *p, u64 v) { *p = v; }
#else
#define HY_FOR(i, n) for (int i = (int)threadIdx.x, i##n_ = (n); i < i##n_; i += HY_NT)
#define HY_LFOR(i, n) for (int i = (int)(threadIdx.x & 63); i < (n); i += 64)
#define HY_TID0 (threadIdx.x == 0)
#define HY_WAVE0 (threadIdx.x < 64)
#define HY_LANE0 (threadIdx.x == 0)
#define HY_BARRIER() __syncthreads()
HY_FN int aadd(int *p, int v) { return atomicAdd(p, v); }
HY_FN void amin32(int *p, int v) { (void)atomicMin(p, v); }
HY_FN void amin64(u64 *p, u64 v) { (void)atomicMin(p, v); }
// the claim words and the finish word are written by atomics (which act beyond the first-level cache): they are read and cleared the same way
HY_FN u64 aload64(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
HY_FN void astore64(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

HY_FN unsigned fbits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }      // g, f >= 0: the bits order as the numbers do
HY_FN double wrap(double a) {      // this search's own, not the host search's: bounded at 1 024 turns like every loop here (the host's takes any yaw)
    for (int i = 0; i < 1024 && a > HY_PI; i++) a -= 2 * HY_PI;
    for (int i = 0; i < 1024 && a < -HY_PI; i++) a += 2 * HY_PI;
    return a;
}
HY_FN double dist2(double dx, double dy) { return sqrt(dx * dx + dy * dy); }

// ---------------------------------------------------------------- collision: the shared test, its clip scratch two local arrays (at most OBCA_HYBRID_MAXROWS rows per obstacle)
// The shared test makes its scratch from the carrier where a clip starts (the host search's points into the carrier's heap buffers): this one takes P and needs nothing of it.
struct ClipLocal { P2 a[HY_CLIP], b[HY_CLIP]; HY_MEMBER ClipLocal(const Params &) {} };
HY_FN bool collides_cs(const Params &P, const Field &w, double x, double y, double c, double s) { return geom::collides_cs<ClipLocal>(P, w, x, y, c, s); }

// The field of instance i of a batch of scenes (the values are the same in every lane of the workgroup)
HY_HD Field field_of(const Fields &S, int i) {
    const int ob = S.rec[4 * i], row = S.rec[4 * i + 1], vx = S.rec[4 * i + 2];
    Field F; F.nOb = S.rec[4 * i + 3]; F.v = S.v + ob; F.off = S.off + ob + i; F.voff = S.voff + ob + i;
    F.A = S.A + 2 * (size_t)row; F.b = S.b + row; F.rn = S.rn + row; F.nrm = S.nrm + row; F.vert = S.vert + 2 * (size_t)vx;
    return F;
}
// Can a disc of radius P.rad stand on cell (ix, iy) of the holonomic map?  The shared disc test at the cell's corner: the byte the host's map holds for the cell.
HY_HD bool cell_blocked(const Params &P, const Field &F, int ix, int iy) { return disc_collides(F, P.xmin + ix * P.res, P.ymin + iy * P.res, P.rad); }

// ---------------------------------------------------------------- the analytic expansion
// the shortest curve from the pose to the goal (unit = Rmin); the walk along it, sampled every <= 0.2 m: test (path == NULL: false at the first pose that collides)
// or record (cap - at poses from `at`; returns the count through *nout)
HY_FN RsPath rs_to_goal(const Params &P, const Pose &q, const double *goal) {
    const double dx = goal[0] - q.x, dy = goal[1] - q.y;
    return rs_shortest((q.c * dx + q.s * dy) / P.Rmin, (-q.s * dx + q.c * dy) / P.Rmin, wrap(goal[2] - q.yaw));
}
HY_FN int rs_samples(const Params &P, const RsPath &p) {
    int tot = 0;
    for (int i = 0; i < p.n; i++) { const double L_ = fabs(p.len[i]); if (L_ < 1e-12) continue; const int m = (int)ceil(L_ * P.Rmin / 0.2); tot += m > 1 ? m : 1; }
    return tot;
}
HY_FN bool rs_walk(const Params &P, const Field &F, const Pose &q, const RsPath &p, double *path, int *dirs) {
    double x = 0, y = 0, yaw = 0, sy = 0.0, cy = 1.0; int k = 0;
    for (int i = 0; i < p.n; i++) {
        const double L_ = fabs(p.len[i]); if (L_ < 1e-12) continue;
        const int d = p.len[i] >= 0 ? 1 : -1; int m = (int)ceil(L_ * P.Rmin / 0.2); if (m < 1) m = 1;
        for (int j = 0; j < m; j++) {
            advance_sc(p.type[i], p.len[i] / m, x, y, yaw, sy, cy);
            const double wx = q.x + P.Rmin * (q.c * x - q.s * y), wy = q.y + P.Rmin * (q.s * x + q.c * y);
            if (path) { path[3 * k] = wx; path[3 * k + 1] = wy; path[3 * k + 2] = wrap(q.yaw + yaw); dirs[k] = d; k++; }
            else if (collides_cs(P, F, wx, wy, q.c * cy - q.s * sy, q.s * cy + q.c * sy)) return false;
        }
    }
    return true;
}

// ---------------------------------------------------------------- primitives, cells, heuristic
// one primitive from the pose: direction d, steering command si; check: collision-test every sub-step (false at the first that collides).  This search's own integration:
// the heading is rotated by per-primitive constants, where the host search asks libm per sub-step.
HY_FN bool prim_apply(const Params &P, const Field &F, Pose &q, int d, int si, bool check) {
    const double kap = P.kap[si], ds = d * P.dsub, sd = d * P.sd[si], cd = P.cd[si];
    for (int j = 0; j < P.sub; j++) {
        if (fabs(kap) < 1e-9) { q.x += ds * q.c; q.y += ds * q.s; }
        else {
            const double s1 = q.s * cd + q.c * sd, c1 = q.c * cd - q.s * sd;
            q.x += (s1 - q.s) / kap; q.y += -(c1 - q.c) / kap; q.yaw = q.yaw + ds * kap; q.s = s1; q.c = c1;
        }
        if (check && collides_cs(P, F, q.x, q.y, q.c, q.s)) return false;
    }
    return true;
}
HY_FN int cell_of(const Params &P, double x, double y, double yaw) {
    const double fx = floor((x - P.xmin) / P.res), fy = floor((y - P.ymin) / P.res);
    if (!(fx >= 0 && fx <= P.nx && fy >= 0 && fy <= P.ny)) return -1;
    double fa = floor((wrap(yaw) + HY_PI) / P.yres); if (fa >= P.nyaw) fa = P.nyaw - 1; if (!(fa >= 0)) return -1;
    const long long k = ((long long)fy * (P.nx + 1) + (long long)fx) * P.nyaw + (long long)fa;
    return k >= 0 && k < P.ncell ? (int)k : -1;
}
HY_FN int round_idx(double v, int n) {      // lround, cut to 0 .. n - 1
    if (!(v > 0)) return 0;
    if (v >= n) return n - 1;
    int r = (int)v; if (v - r >= 0.5) r++;
    return r > n - 1 ? n - 1 : r;
}
HY_FN double heur(const Params &P, const float *hmap, const Pose &q, const double *goal) {
    const int ix = round_idx((q.x - P.xmin) / P.res, P.nx), iy = round_idx((q.y - P.ymin) / P.res, P.ny);
    const float hv = hmap[iy * P.nx + ix];
    const double h2 = (hv >= 0.f && hv < 1e8f) ? (double)hv : dist2(q.x - goal[0], q.y - goal[1]) + 5.0;
    double h = max2(h2, P.RminH * fabs(wrap(q.yaw - goal[2])) * 0.5);
    if (P.rs_heur) {
        const double dx = goal[0] - q.x, dy = goal[1] - q.y;
        const RsPath p = rs_shortest((q.c * dx + q.s * dy) / P.RminH, (-q.s * dx + q.c * dy) / P.RminH, wrap(goal[2] - q.yaw));
        if (p.n > 0) h = max2(h, P.RminH * p.total);
    }
    return P.hweight * h;
}
HY_FN float step_g(const Params &P, const Node &par, int d, int si) {
    const double steer = P.steer[si];
    double g = (double)par.g + P.step * (d > 0 ? 1.0 : P.crev) + P.cst * fabs(steer) * P.step + P.cchg * fabs(steer - P.steer[par.si]);
    if (par.dir != 0 && par.dir != d) g += P.csw;
    return (float)g;
}
HY_FN int bucket_of(const Params &P, double f, int cur) {
    double fb = floor(f / P.bw); if (!(fb < 1e9)) fb = 1e9; if (!(fb >= 0)) fb = 0;
    const int b = (int)fb;
    return b < cur ? cur : b;
}

// ---------------------------------------------------------------- buckets: chains of chunks, heads in LDS (bh head, bt tail, bc entries, ba entries being added, bn first new chunk)
struct Buckets { int *bh, *bt, *bc, *ba, *bn, *ctl; };
HY_FN int tail_space(int cnt) { return cnt == 0 ? 0 : HY_CE - ((cnt - 1) % HY_CE + 1); }
HY_FN int new_chunks(int cnt, int add) { const int need = add - tail_space(cnt); return need > 0 ? (need + HY_CE - 1) / HY_CE : 0; }
// the buckets that grew take their chunks (one thread per bucket); the caller's barrier follows
HY_FN void bucket_alloc(const Params &P, const Buckets &K, const SlotMem &M) {
    HY_FOR(i, HY_W) {
        if (K.ba[i] <= 0) continue;
        const int nnew = new_chunks(K.bc[i], K.ba[i]);
        K.bn[i] = -1;
        if (!nnew) continue;
        const int c0 = aadd(&K.ctl[C_NCHUNK], nnew);
        if (c0 + nnew > P.maxchunks) { K.ctl[C_OVER] = 1; continue; }
        for (int j = 0; j < nnew; j++) M.chunks[(size_t)(c0 + j) * HY_CH] = j + 1 < nnew ? c0 + j + 1 : -1;
        if (K.bt[i] >= 0) M.chunks[(size_t)K.bt[i] * HY_CH] = c0; else K.bh[i] = c0;
        K.bn[i] = c0;
    }
}
// a node that took position `pos` of the additions to its bucket writes its entry
HY_FN void entry_write(const Buckets &K, const SlotMem &M, int h, int base) {
    const int pos = M.nodes[h].pos;
    if (pos < 0) return;
    const int i = M.nodes[h].bucket - base, cnt = K.bc[i], space = tail_space(cnt);
    int chunk, slot;
    if (pos < space) { chunk = K.bt[i]; slot = (cnt - 1) % HY_CE + 1 + pos; }
    else { chunk = K.bn[i] + (pos - space) / HY_CE; slot = (pos - space) % HY_CE; }
    M.chunks[(size_t)chunk * HY_CH + 1 + slot] = h;
}
HY_FN void bucket_close(const Buckets &K) {
    HY_FOR(i, HY_W) {
        if (K.ba[i] <= 0) continue;
        const int nnew = new_chunks(K.bc[i], K.ba[i]);
        if (nnew) K.bt[i] = K.bn[i] + nnew - 1;
        K.bc[i] += K.ba[i]; K.ba[i] = 0;
    }
}

#ifdef OBCA_EMU
static float *emu_map_out = nullptr;      // the holonomic map of the last search, if the caller wants it (nmap floats)
#endif

// ---------------------------------------------------------------- one search
// in: start x, y, yaw, sin, cos; goal x, y, yaw, sin, cos.  hmap: P.nmap floats and li: HY_LDS_INTS ints, in LDS.  path cap x 3, dirs cap.
// blocked: the cells of the holonomic map a disc cannot stand on, P.nmap bytes from the host -- or NULL: the search finds them itself from F (cell_blocked, needs F.nrm),
// the threads sharing the cells as they share the relaxation.  Everything else the search knows of the obstacles it reads through F, nothing through P.
HY_FN void search(const Params &P, const Field &F, const unsigned char *blocked, const double *in, const SlotMem &M, float *hmap, int *li,
                  double *path, int *dirs, int *count, int *nexp_out, int *rounds_out) {
    Buckets K; K.bh = li; K.bt = li + HY_W; K.bc = li + 2 * HY_W; K.ba = li + 3 * HY_W; K.bn = li + 4 * HY_W; K.ctl = li + 5 * HY_W;
    int *ctl = K.ctl; u64 *fin = (u64 *)(ctl + C_FIN);
    const double *start = in, *goal = in + 5;
    int status = 0, nexp = 0, nround = 0, found_cell = -1;
    if (collides_cs(P, F, start[0], start[1], start[4], start[3]) || collides_cs(P, F, goal[0], goal[1], goal[4], goal[3])) status = -2;      // (every thread decides the same)
    Pose p0; p0.x = start[0]; p0.y = start[1]; p0.yaw = wrap(start[2]); p0.s = start[3]; p0.c = start[4];
    const int k0 = cell_of(P, p0.x, p0.y, p0.yaw);
    bool run = status == 0 && k0 >= 0;
    // ---- the control words, the buckets, the holonomic map
    HY_FOR(i, HY_W) { K.bh[i] = -1; K.bt[i] = -1; K.bc[i] = 0; K.ba[i] = 0; K.bn[i] = -1; }
    if (HY_TID0) { for (int i = 0; i < C_WORDS; i++) ctl[i] = 0; *fin = HY_NONE; }
    if (run) {
        const int gx = round_idx((goal[0] - P.xmin) / P.res, P.nx), gy = round_idx((goal[1] - P.ymin) / P.res, P.ny), gid = gy * P.nx + gx;
        HY_FOR(c, P.nmap) hmap[c] = c == gid ? 0.f : ((blocked ? blocked[c] != 0 : cell_blocked(P, F, c % P.nx, c / P.nx)) ? -1.f : HUGE_VALF);
        HY_BARRIER();
        bool settled = false;
        for (int s = 0; !settled && s < P.nmap; s++) {
            bool low = false;
            HY_FOR(c, P.nmap) {
                const float g0 = hmap[c];
                if (g0 < 0.f) continue;
                const int x = c % P.nx, y = c / P.nx; float best = g0;
                for (int dy = -1; dy <= 1; dy++) {
                    if ((dy < 0 && y == 0) || (dy > 0 && y == P.ny - 1)) continue;
                    for (int dx = -1; dx <= 1; dx++) {
                        if ((!dx && !dy) || (dx < 0 && x == 0) || (dx > 0 && x == P.nx - 1)) continue;
                        const float v = hmap[c + dy * P.nx + dx], cand = v + (dx && dy ? P.w2 : P.w1);
                        if (v >= 0.f && cand < best) best = cand;
                    }
                }
                if (best < g0) { hmap[c] = best; low = true; }
            }
            if (low) ctl[C_VOTE + s % 3] = 1;
            HY_BARRIER();
            settled = ctl[C_VOTE + s % 3] == 0;
            if (HY_TID0) ctl[C_VOTE + (s + 2) % 3] = 0;
        }
        // (a map that did not settle within its bound cannot be: every sweep that lowers a word lowers the finite sum of a monotone field; the search would still be valid)
#ifdef OBCA_EMU
        if (emu_map_out) for (int c = 0; c < P.nmap; c++) emu_map_out[c] = hmap[c];
#endif
    }
    HY_BARRIER();
    // ---- the start node
    int base = 0;
    if (run) {
        base = bucket_of(P, heur(P, hmap, p0, goal), 0);
        if (HY_TID0) {
            Node n; n.x = p0.x; n.y = p0.y; n.yaw = p0.yaw; n.s = p0.s; n.c = p0.c; n.g = 0.f; n.parent = -1; n.cell = k0; n.bucket = base; n.pos = 0; n.dir = 0; n.si = (signed char)P.nst;
            if (P.maxnodes < 1 || P.maxchunks < 1) ctl[C_OVER] = 1;
            else {
                M.nodes[0] = n; M.cell_g[k0] = 0u; M.cell_node[k0] = 0; M.touched[0] = k0;
                M.chunks[0] = -1; M.chunks[1] = 0; K.bh[0] = 0; K.bt[0] = 0; K.bc[0] = 1;
                ctl[C_NNODES] = 1; ctl[C_NTOUCH] = 1; ctl[C_NCHUNK] = 1;
            }
        }
        HY_BARRIER();
        if (ctl[C_OVER]) { status = -3; run = false; }
    }
    int *far = M.far, *far2 = M.far + P.maxnodes;
    // ---- rounds
    for (int it = 0; run && it < P.maxrounds; it++) {
        if (HY_TID0) ctl[C_MINB] = HY_W;
        HY_BARRIER();
        HY_FOR(i, HY_W) if (K.bc[i] > 0) amin32(&ctl[C_MINB], i);
        HY_BARRIER();
        const int mb = ctl[C_MINB];
        if (mb == HY_W) {      // the window is empty: done, or move it to the lowest bucket of the far list
            const int nfar = ctl[C_NFAR];
            if (nfar == 0) break;
            HY_BARRIER();
            if (HY_TID0) { ctl[C_MINB] = 0x7FFFFFFF; ctl[C_NFAR2] = 0; }
            HY_BARRIER();
            HY_FOR(i, nfar) amin32(&ctl[C_MINB], M.nodes[far[i]].bucket);
            HY_BARRIER();
            base = ctl[C_MINB];
            HY_FOR(i, nfar) {
                const int h = far[i], b = M.nodes[h].bucket;
                if (b - base < HY_W) M.nodes[h].pos = aadd(&K.ba[b - base], 1);
                else { M.nodes[h].pos = -1; far2[aadd(&ctl[C_NFAR2], 1)] = h; }
            }
            HY_BARRIER();
            bucket_alloc(P, K, M);
            HY_BARRIER();
            if (ctl[C_OVER]) { status = -3; break; }
            HY_FOR(i, nfar) entry_write(K, M, far[i], base);
            HY_BARRIER();
            bucket_close(K);
            if (HY_TID0) ctl[C_NFAR] = ctl[C_NFAR2];
            { int *t = far; far = far2; far2 = t; }
            continue;
        }
        const int cur = base + mb, n = K.bc[mb], head = K.bh[mb];
        HY_BARRIER();
        if (HY_TID0) {      // the round's entries leave the bucket: what phase B adds to it belongs to the next round
            const int nch = (n + HY_CE - 1) / HY_CE; int c = head;
            for (int j = 0; j < nch && c >= 0; j++) { M.chunklist[j] = c; c = M.chunks[(size_t)c * HY_CH]; }
            K.bh[mb] = -1; K.bt[mb] = -1; K.bc[mb] = 0; ctl[C_ALIVE] = 0;
        }
        HY_BARRIER();
#define HY_ENTRY(i) M.chunks[(size_t)M.chunklist[(i) / HY_CE] * HY_CH + 1 + (i) % HY_CE]
        // pass 1: stale entries are struck out; the others are expansions and try to finish
        HY_FOR(i, n) {
            const int h = HY_ENTRY(i);
            const Node nd = M.nodes[h];
            if (M.cell_node[nd.cell] != h) { HY_ENTRY(i) = -1; continue; }
            (void)aadd(&ctl[C_ALIVE], 1);
            Pose q; q.x = nd.x; q.y = nd.y; q.yaw = nd.yaw; q.s = nd.s; q.c = nd.c;
            const double dgoal = dist2(nd.x - goal[0], nd.y - goal[1]);
            if (!P.analytic) {
                if (dgoal <= P.gtol && fabs(wrap(nd.yaw - goal[2])) <= P.ytol) amin64(fin, ((u64)fbits(nd.g) << 32) | (unsigned)nd.cell);
            } else if (dgoal < 6.0 * P.Rmin || nd.cell % 16 == 0) {
                const RsPath p = rs_to_goal(P, q, goal);
                if (p.n > 0 && rs_walk(P, F, q, p, nullptr, nullptr)) amin64(fin, ((u64)fbits((float)((double)nd.g + P.Rmin * p.total)) << 32) | (unsigned)nd.cell);
            }
        }
        HY_BARRIER();
        if ((long long)nexp + ctl[C_ALIVE] > P.maxexp) break;      // the live entries of this round would pass maxexp: the round is not counted, not expanded and cannot finish
        nexp += ctl[C_ALIVE]; nround++;
        { const u64 f = *fin; if (f != HY_NONE) { found_cell = (int)(f & 0xFFFFFFFFull); break; } }
        // phase A: every (entry, primitive) pair claims its cell
        HY_FOR(item, n * P.nprim) {
            const int i = item / P.nprim, pr = item % P.nprim, h = HY_ENTRY(i);
            if (h < 0) continue;
            const Node nd = M.nodes[h];
            const int d = pr < P.nsi ? 1 : -1, si = pr % P.nsi;
            Pose q; q.x = nd.x; q.y = nd.y; q.yaw = nd.yaw; q.s = nd.s; q.c = nd.c;
            if (!prim_apply(P, F, q, d, si, true)) continue;
            const int k = cell_of(P, q.x, q.y, q.yaw);
            if (k < 0) continue;
            const unsigned gb = fbits(step_g(P, nd, d, si));
            if (M.cell_g[k] <= gb) continue;
            amin64(&M.claim[k], ((u64)gb << 32) | (unsigned)(nd.cell * P.nprim + pr));
        }
        HY_BARRIER();
        const int n0 = ctl[C_NNODES];
        HY_BARRIER();
        // phase B: the winner of every claimed cell commits
        HY_FOR(item, n * P.nprim) {
            const int i = item / P.nprim, pr = item % P.nprim, h = HY_ENTRY(i);
            if (h < 0) continue;
            const Node nd = M.nodes[h];
            const int d = pr < P.nsi ? 1 : -1, si = pr % P.nsi;
            Pose q; q.x = nd.x; q.y = nd.y; q.yaw = nd.yaw; q.s = nd.s; q.c = nd.c;
            (void)prim_apply(P, F, q, d, si, false);
            const int k = cell_of(P, q.x, q.y, q.yaw);
            if (k < 0) continue;
            const float g = step_g(P, nd, d, si);
            const unsigned gb = fbits(g);
            if (aload64(&M.claim[k]) != (((u64)gb << 32) | (unsigned)(nd.cell * P.nprim + pr))) continue;
            astore64(&M.claim[k], HY_NONE);
            const int h2 = aadd(&ctl[C_NNODES], 1);
            if (h2 >= P.maxnodes) { ctl[C_OVER] = 1; continue; }
            if (M.cell_g[k] == 0xFFFFFFFFu) M.touched[aadd(&ctl[C_NTOUCH], 1)] = k;
            M.cell_g[k] = gb; M.cell_node[k] = h2;
            Node nn; nn.x = q.x; nn.y = q.y; nn.yaw = wrap(q.yaw); nn.s = q.s; nn.c = q.c; nn.g = g; nn.parent = h; nn.cell = k; nn.dir = (signed char)d; nn.si = (signed char)si;
            nn.bucket = bucket_of(P, (double)g + heur(P, hmap, q, goal), cur);
            if (nn.bucket - base < HY_W) nn.pos = aadd(&K.ba[nn.bucket - base], 1);
            else { nn.pos = -1; far[aadd(&ctl[C_NFAR], 1)] = h2; }
            M.nodes[h2] = nn;
        }
        HY_BARRIER();
        if (ctl[C_OVER]) { status = -3; break; }
        const int n1 = ctl[C_NNODES];
        bucket_alloc(P, K, M);
        HY_BARRIER();
        if (ctl[C_OVER]) { status = -3; break; }
        HY_FOR(j, n1 - n0) entry_write(K, M, n0 + j, base);
        HY_BARRIER();
        bucket_close(K);
#undef HY_ENTRY
    }
    HY_BARRIER();
    // ---- the path, on one wavefront: every lane walks the chain (the same numbers in all), the lanes share the segments
    if (HY_WAVE0) {
        int cnt = status;
        if (found_cell >= 0) {
            int *chain = M.far;      // (the far list is no longer needed)
            int Lc = 0;
            for (int h = M.cell_node[found_cell]; h >= 0 && Lc < P.maxnodes; h = M.nodes[h].parent) chain[Lc++] = h;      // found node first
            const Node fn = M.nodes[chain[0]];
            Pose q; q.x = fn.x; q.y = fn.y; q.yaw = fn.yaw; q.s = fn.s; q.c = fn.c;
            RsPath tail; tail.n = 0; tail.total = 0;
            int nt = 0;
            if (P.analytic) { tail = rs_to_goal(P, q, goal); nt = rs_samples(P, tail); }
            cnt = 1 + (Lc - 1) * P.sub + nt;
            if (cnt > P.cap) cnt = -1;
            else {
                HY_LFOR(c, Lc) {
                    const Node pn = M.nodes[chain[Lc - 1 - c]];
                    if (c == 0) {
                        path[0] = pn.x; path[1] = pn.y; path[2] = pn.yaw;
                        dirs[0] = Lc > 1 ? M.nodes[chain[Lc - 2]].dir : (nt > 0 ? (tail.len[0] >= 0 ? 1 : -1) : pn.dir);
                    }
                    if (c + 1 < Lc) {      // the primitive that leads to the next node of the chain, replayed at its sub-steps
                        const Node nn = M.nodes[chain[Lc - 2 - c]];
                        Pose r; r.x = pn.x; r.y = pn.y; r.yaw = pn.yaw; r.s = pn.s; r.c = pn.c;
                        const double kap = P.kap[nn.si], ds = nn.dir * P.dsub, sd = nn.dir * P.sd[nn.si], cd = P.cd[nn.si];
                        for (int j = 0; j < P.sub; j++) {
                            if (fabs(kap) < 1e-9) { r.x += ds * r.c; r.y += ds * r.s; }
                            else { const double s1 = r.s * cd + r.c * sd, c1 = r.c * cd - r.s * sd; r.x += (s1 - r.s) / kap; r.y += -(c1 - r.c) / kap; r.yaw = r.yaw + ds * kap; r.s = s1; r.c = c1; }
                            const int o = 1 + c * P.sub + j;
                            path[3 * o] = r.x; path[3 * o + 1] = r.y; path[3 * o + 2] = r.yaw; dirs[o] = nn.dir;
                        }
                    }
                }
                if (HY_LANE0 && nt > 0) { const int o = 1 + (Lc - 1) * P.sub; (void)rs_walk(P, F, q, tail, path + 3 * o, dirs + o); }
            }
        }
        if (HY_LANE0) { *count = cnt; if (nexp_out) *nexp_out = nexp; if (rounds_out) *rounds_out = nround; ctl[C_CNT] = cnt; }
    }
    HY_BARRIER();
    // ---- the rest of the caller's rows is zero, whatever the buffer held; the cells this search touched are as they were
    {
        const int Kn = ctl[C_CNT] > 0 ? ctl[C_CNT] : 0;
        HY_FOR(qi, 3 * (P.cap - Kn)) path[3 * Kn + qi] = 0.0;
        HY_FOR(qi, P.cap - Kn) dirs[Kn + qi] = 0;
        const int ntouch = ctl[C_NTOUCH];
        HY_FOR(i, ntouch) { const int k = M.touched[i]; M.cell_g[k] = 0xFFFFFFFFu; M.cell_node[k] = -1; }
    }
    HY_BARRIER();
}

// ================================================================ host code: the arguments, the parameter block, the obstacle field, the blocked cells
struct HostField { std::vector<int> v, off, voff; std::vector<double> A, b, rn, vert, nrm; };
// the fields of a batch of scenes as `Fields` reads them (make_fields)
struct HostFields { std::vector<int> rec, v, off, voff; std::vector<double> A, b, rn, nrm, vert; };

static inline bool finite_(double v) { return v - v == 0.0; }
static inline Field view(const HostField &W, int nOb) {
    Field F; F.nOb = nOb; F.v = W.v.data(); F.off = W.off.data(); F.voff = W.voff.data(); F.A = W.A.data(); F.b = W.b.data(); F.rn = W.rn.data(); F.vert = W.vert.data(); F.nrm = W.nrm.data();
    return F;
}
// one obstacle as a polygon, the vertices appended to `vert`
static inline void host_polygon(const double *A, const double *b, int rows, double far_, std::vector<double> &vert) {
    P2 pa[HY_CLIP], pb[HY_CLIP];
    append_polygon(A, b, rows, far_, pa, pb, vert);
}

// NULL if the call is good (then P, W, blocked and inst -- B x 10 doubles: start and goal with sin, cos of their headings -- are filled), else what is wrong
static inline const char *make_params(int B, const double *starts, const double *goals, int nOb, const int *vOb, const double *A, const double *b, const double *ego, double L,
                                      const double *XYbounds, const double *opts_in, int nopts, double bucket_width, int cap, int maxnodes, int maxchunks,
                                      Params &P, HostField &W, std::vector<unsigned char> &blocked, std::vector<double> &inst) {
    if (B < 1 || !starts || !goals || nOb < 0 || (nOb > 0 && (!vOb || !A || !b)) || !ego || !XYbounds) return "need B >= 1 and non-NULL starts, goals, ego, XYbounds (and vOb, A, b if nOb > 0)";
    if (cap < 2) return "need cap >= 2";
    if (opts_in && (nopts < 0 || nopts > OBCA_PLAN_NOPTS)) return "need 0 <= nopts <= OBCA_PLAN_NOPTS";
    if (nOb > OBCA_HYBRID_MAXOB) return "more than OBCA_HYBRID_MAXOB obstacles";
    double o[OBCA_PLAN_NOPTS] = HY_DEFAULT_OPTS;
    for (int i = 0; opts_in && i < nopts; i++) o[i] = opts_in[i];
    for (int i = 0; i < OBCA_PLAN_NOPTS; i++) if (!finite_(o[i])) return "an option is not finite";
    if (!finite_(L) || !(L > 0) || !finite_(bucket_width)) return "need L > 0 and a finite bucket_width";
    for (int i = 0; i < 4; i++) if (!finite_(ego[i]) || !finite_(XYbounds[i])) return "ego or XYbounds is not finite";
    for (long long i = 0; i < 3LL * B; i++) if (!finite_(starts[i]) || !finite_(goals[i]) || fabs(starts[i]) > 1e6 || fabs(goals[i]) > 1e6) return "a start or goal coordinate is not finite (or beyond 1e6)";
    if (o[16] != 0.0) return "the lattice heuristic (option 16) is not available on the device";
    if (!(o[14] > 0.0)) return "need a positive heuristic weight";
    if (!(o[0] >= 0.01) || !(o[1] >= 0.1) || !(o[2] > 0) || !(o[2] <= 100.0) || !(o[3] > 0) || !(o[3] < 1.5) || !(o[4] >= 1) || !(o[4] <= OBCA_HYBRID_MAXSTEER) || !(o[11] >= 0) || !(o[12] >= 0))
        return "an option is out of range (resolutions, step, max steer below 1.5 rad, 1 .. OBCA_HYBRID_MAXSTEER steering samples)";
    if (!(o[8] >= 0) || !(o[9] >= 0) || !(o[10] >= 0) || !(o[13] >= 0)) return "a cost option (reverse, switch, steer, steer change) is negative: g must not fall along a path";
    memset(&P, 0, sizeof P);
    P.xmin = XYbounds[0]; P.xmax = XYbounds[1]; P.ymin = XYbounds[2]; P.ymax = XYbounds[3];
    if (!(P.xmax > P.xmin) || !(P.ymax > P.ymin)) return "XYbounds is empty";
    P.res = o[0]; P.yres = o[1] * HY_PI / 180; P.step = o[2]; P.smax = o[3]; P.nst = (int)o[4]; P.nsi = 2 * P.nst + 1; P.nprim = 2 * P.nsi;
    P.margin = o[5]; P.gtol = o[6]; P.ytol = o[7] * HY_PI / 180; P.crev = o[8]; P.csw = o[9]; P.cst = o[10]; P.cchg = o[13]; P.hweight = o[14]; P.rs_heur = o[15] != 0.0; P.L = L;
    P.maxexp = o[11] > 2e9 ? 2000000000 : (int)o[11];
    P.analytic = o[12] > 0; P.cap = cap;
    P.Rmin = L / tan(P.smax * (o[12] > 0 ? (o[12] < 1.0 ? o[12] : 1.0) : 1.0)); P.RminH = L / tan(P.smax);
    P.bw = bucket_width > 0 ? bucket_width : OBCA_HYBRID_DEFAULT_WIDTH;
    if (P.bw < 1e-6) return "need bucket_width >= 1e-6 (or <= 0 for the default)";
    const double fx = ceil((P.xmax - P.xmin) / P.res) + 1, fy = ceil((P.ymax - P.ymin) / P.res) + 1, fa = ceil(2 * HY_PI / P.yres);
    if (fx * fy > (double)OBCA_HYBRID_MAXMAP) return "the xy grid has more than OBCA_HYBRID_MAXMAP cells: its map does not fit the LDS of one workgroup";
    if ((fx + 1) * (fy + 1) * fa > (double)OBCA_HYBRID_MAXCELLS) return "the search grid has more than OBCA_HYBRID_MAXCELLS cells";
    P.nx = (int)fx; P.ny = (int)fy; P.nyaw = (int)fa; P.nmap = P.nx * P.ny; P.ncell = (P.nx + 1) * (P.ny + 1) * P.nyaw;
    P.sub = (int)ceil(P.step / 0.2); if (P.sub < 1) P.sub = 1;
    P.dsub = P.step / P.sub;
    P.maxnodes = maxnodes; P.maxchunks = maxchunks;
    { const double nodes = 1.0 + (double)P.maxexp * P.nprim, r = 2.0 * (nodes < maxnodes ? nodes : (double)maxnodes) + 4.0; P.maxrounds = r > 2e9 ? 2000000000 : (int)r; }
    for (int i = 0; i < 4; i++) P.ego[i] = ego[i];
    P.w1 = (float)(P.res * hypot(1.0, 0.0)); P.w2 = (float)(P.res * hypot(1.0, 1.0));
    for (int si = -P.nst; si <= P.nst; si++) {
        const int k = si + P.nst; P.steer[k] = P.smax * si / P.nst; P.kap[k] = tan(P.smax * si / P.nst) / L;
        P.sd[k] = sin(P.dsub * P.kap[k]); P.cd[k] = cos(P.dsub * P.kap[k]);
    }
    // the obstacle field: rows, their norms, the obstacles as polygons
    W.v.assign(vOb, vOb + nOb); W.off.assign(nOb + 1, 0);
    for (int j = 0; j < nOb; j++) { if (vOb[j] < 1 || vOb[j] > OBCA_HYBRID_MAXROWS) return "need 1 .. OBCA_HYBRID_MAXROWS rows per obstacle"; W.off[j + 1] = W.off[j] + vOb[j]; }
    const int M_ = W.off[nOb];
    W.A.assign(A, A + 2 * M_); W.b.assign(b, b + M_); W.rn.resize(M_); W.nrm.resize(M_);
    for (int r = 0; r < M_; r++) {
        if (!finite_(A[2 * r]) || !finite_(A[2 * r + 1]) || !finite_(b[r])) return "an obstacle row is not finite";
        const double n = hypot(A[2 * r], A[2 * r + 1]); W.rn[r] = n > 0 ? 1.0 / n : 0.0; W.nrm[r] = n;
    }
    const double far_ = host_far(XYbounds);
    W.voff.assign(nOb + 1, 0); W.vert.clear();
    for (int j = 0; j < nOb; j++) {
        host_polygon(W.A.data() + 2 * (size_t)W.off[j], W.b.data() + W.off[j], W.v[j], far_, W.vert);
        W.voff[j + 1] = (int)W.vert.size() / 2;
    }
    P.nOb = nOb; P.nrows = M_; P.nvert = (int)W.vert.size() / 2;
    // the cells a disc of the car's half width cannot stand on (the holonomic map's obstacles): a property of the field, not of the goal
    P.rad = min2(min2(ego[1], ego[3]), 0.5 * (ego[0] + ego[2])) * 0.9;
    blocked.assign((size_t)P.nmap, 0);
    const Field F = view(W, nOb);
    for (int iy = 0; iy < P.ny; iy++) for (int ix = 0; ix < P.nx; ix++) blocked[(size_t)iy * P.nx + ix] = cell_blocked(P, F, ix, iy);
    inst.resize((size_t)B * 10);
    for (int i = 0; i < B; i++) for (int e = 0; e < 2; e++) {
        const double *p = (e ? goals : starts) + 3 * (size_t)i; double *q = &inst[(size_t)i * 10 + 5 * e];
        q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = sin(p[2]); q[4] = cos(p[2]);
    }
    return nullptr;
}
// The fields of B instances, packed for `Fields`: nOb[i] obstacles per instance, their row counts in vOb, rows in A (x 2) and b, instance after instance.  Per instance
// what make_params does for its one field: rows, 1 / norm, norm, the obstacles as clipped polygons; and the record of its offsets.  Empty if the fields are good, else
// what is wrong with the FIRST instance that has something wrong.
static inline std::string make_fields(int B, const int *nOb, const int *vOb, const double *A, const double *b, const double *XYbounds, HostFields &W) {
    if (B < 1 || !nOb || !XYbounds) return "need B >= 1 and non-NULL nOb, XYbounds";
    const double far_ = host_far(XYbounds);
    W = HostFields();
    long long ob = 0, row = 0;
    for (int i = 0; i < B; i++) {
        const std::string who = "instance " + std::to_string(i) + ": ";
        if (nOb[i] < 0) return who + "a negative obstacle count";
        if (nOb[i] > OBCA_HYBRID_MAXOB) return who + "more than OBCA_HYBRID_MAXOB obstacles";
        if (nOb[i] > 0 && (!vOb || !A || !b)) return who + "obstacles, but vOb, A or b is NULL";
        W.rec.push_back((int)ob); W.rec.push_back((int)row); W.rec.push_back((int)(W.vert.size() / 2)); W.rec.push_back(nOb[i]);
        const long long row0 = row; const size_t vert0 = W.vert.size() / 2;
        for (int j = 0; j < nOb[i]; j++) {
            const int v = vOb[ob + j];
            if (v < 1 || v > OBCA_HYBRID_MAXROWS) return who + "need 1 .. OBCA_HYBRID_MAXROWS rows per obstacle";
            for (long long r = row; r < row + v; r++) {
                if (!finite_(A[2 * r]) || !finite_(A[2 * r + 1]) || !finite_(b[r])) return who + "an obstacle row is not finite";
                const double n = hypot(A[2 * r], A[2 * r + 1]);
                W.A.push_back(A[2 * r]); W.A.push_back(A[2 * r + 1]); W.b.push_back(b[r]); W.rn.push_back(n > 0 ? 1.0 / n : 0.0); W.nrm.push_back(n);
            }
            W.v.push_back(v); W.off.push_back((int)(row - row0)); W.voff.push_back((int)(W.vert.size() / 2 - vert0));
            host_polygon(A + 2 * row, b + row, v, far_, W.vert);
            row += v;
        }
        W.off.push_back((int)(row - row0)); W.voff.push_back((int)(W.vert.size() / 2 - vert0));
        ob += nOb[i];
    }
    return std::string();
}
// obca_scene_astar_batch's arguments: make_params for everything but the fields (P, inst; P.nOb, nrows, nvert stay zero: a search reads its field through F), then
// make_fields.  Empty if the call is good.
static inline std::string make_scenes(int B, const double *starts, const double *goals, const int *nOb, const int *vOb, const double *A, const double *b, const double *ego, double L,
                                      const double *XYbounds, const double *opts_in, int nopts, double bucket_width, int cap, int maxnodes, int maxchunks,
                                      Params &P, HostFields &W, std::vector<double> &inst) {
    HostField none; std::vector<unsigned char> free_map;
    if (const char *bad = make_params(B, starts, goals, 0, nullptr, nullptr, nullptr, ego, L, XYbounds, opts_in, nopts, bucket_width, cap, maxnodes, maxchunks, P, none, free_map, inst)) return bad;
    return make_fields(B, nOb, vOb, A, b, XYbounds, W);
}
// Chunks of a slot by default.  A bucket takes a chunk whenever it goes from empty to not empty (at most once per round and per bucket of a window) and one per
// HY_CE entries beyond that, so a search of R rounds and n nodes needs at most n / HY_CE + R + HY_W per window: a quarter of the nodes covers what was measured.
static inline int default_chunks(int maxnodes) { return maxnodes / 4 + 4 * HY_W; }
static inline size_t slot_bytes(int ncell, int maxnodes, int maxchunks) {
    const size_t b = (size_t)ncell * 16 + (size_t)maxnodes * sizeof(Node) + ((size_t)3 * maxnodes + 2 + (size_t)maxchunks * (HY_CH + 1)) * 4;
    return (b + 255) / 256 * 256;
}
// a slot's arrays in its block of slot_bytes bytes (256-byte aligned)
HY_HD SlotMem carve(void *block, int ncell, int maxnodes, int maxchunks) {
    SlotMem M; char *p = (char *)block;
    M.claim = (u64 *)p; p += (size_t)ncell * 8;
    M.cell_g = (unsigned *)p; p += (size_t)ncell * 4;
    M.cell_node = (int *)p; p += (size_t)ncell * 4;
    M.nodes = (Node *)p; p += (size_t)maxnodes * sizeof(Node);
    M.touched = (int *)p; p += ((size_t)maxnodes + 2) * 4;
    M.far = (int *)p; p += (size_t)2 * maxnodes * 4;
    M.chunks = (int *)p; p += (size_t)maxchunks * HY_CH * 4;
    M.chunklist = (int *)p;
    return M;
}
// bytes at the head of a slot's block that a search expects as all ones before the first search (claim words, cell table); the rest is written before it is read
static inline size_t slot_init_bytes(int ncell) { return (size_t)ncell * 16; }

}  // namespace hy
}  // namespace obca
