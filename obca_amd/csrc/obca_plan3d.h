// obca_plan3d.h -- the quadcopter's 3-D grid planner on the device: ONE WORKGROUP PER SEARCH, the whole grid in that workgroup's LDS (include/obca_plan3d.h is the ABI).
//
// The host search (obca_plan_astar3d, obca_planner.cpp) is an A* with a priority queue, which does not map onto a wavefront.  The grid of the shipped
// room is 41 x 41 x 21 = 35 301 nodes, 141 KB of fp32: it fits the 160 KiB of LDS one workgroup may use on gfx950, and a cost-to-go field needs no queue:
//   1. occupancy : every node gets +inf, or PL3_BLOCKED where the host planner's `blocked` holds (fp64, the same inclusive comparisons); the goal node gets 0.
//                  One array is all the LDS the grid takes.
//   2. relaxation: g[c] = min(g[c], g[nb] + w) over the 26 neighbours nb that are not blocked, w = (float)(res sqrt(dx^2 + dy^2 + dz^2)) -- the host's rule: only the
//                  neighbour node is tested.  Every thread PULLS into the nodes it owns, so a word has one writer; the update is in place, in whatever order the
//                  waves run.  The operator is monotone and the field only falls, so every fair order ends in the same fp32 field: the largest fixed point below the
//                  initial one (tests/test_gpu_plan3d.py compares the device's paths with a sequential host run bit for bit).  One barrier per sweep and a
//                  workgroup-wide "a node was lowered" vote through three rotating LDS words; a sweep that lowers nothing ends the phase, and a sweep that lowers
//                  nothing has written nothing, so all its reads saw the final field.  The sweep count is bounded by the node count.
//   3. descent   : wave 0 walks from the start node: 26 lanes evaluate g[nb] + w, the smallest wins, ties go to the lowest neighbour in the host's dz, dy, dx loop
//                  order.  At the fixed point every step lowers g by w > 0, so the walk ends on the goal node; it is bounded by the node count all the same.
//                  Way-points as the host writes them: start point, the chain of nodes (start node .. goal node), goal point.
//                  The way-points beyond the count are written as zeros: the output does not depend on what the buffer held.
//   4. resampling: fp64, one thread per stage: the way-points as the polyline of scenarios.quad_warm_start, sampled at N + 1 uniform arc lengths.
// The start node may itself be blocked (the host only tests the start POINT and the neighbours it moves to): the descent never reads g of the start node.
// Cell-to-thread map (PL3_MAP 0): node c belongs to thread c mod PL3_NT -- the 32 lanes of a bank group read 32 consecutive words for each of the 26 neighbours, which is
// conflict-free except where a run crosses a row end.  PL3_MAP 1 (each thread a contiguous run) and smaller workgroups exist for the A/B of tools/plan3d_rate.py.
// No contraction of a * b + c into an fma anywhere in this file: the host build (tests/emu/plan3d_emu.cpp, -DOBCA_EMU, every loop sequential) must return the same bits.
#pragma once
#include <math.h>
#include "../../include/obca_plan3d.h"

#ifdef OBCA_EMU
#define PL3_FN static inline
#else
#define PL3_FN __device__ __forceinline__
#pragma clang fp contract(off)
#endif
#ifndef PL3_NT
#define PL3_NT 1024      // threads per workgroup = per search: 16 waves, four per SIMD
#endif
#ifndef PL3_MAP
#define PL3_MAP 0
#endif

namespace obca {
namespace pl3 {

#define PL3_BLOCKED (-1.0f)      // sentinel of a blocked node in the cost-to-go array (costs are >= 0)
#define PL3_ST_SWEEPS (-3)       // status: the relaxation hit its sweep bound
#define PL3_IN_STRIDE(nBox) (6 + 6 * (nBox))      // doubles per instance of the input record: start, goal, boxes

struct Grid { int nx, ny, nz, ncell, nBox; double res, clear, room[3]; const double *boxes; };

// ---------------------------------------------------------------- argument checks of both entry points (host code; the library and the emulation share them)
// NULL if the arguments are good (then nx, ny, nz are set), else what is wrong.  pts: B x pstride doubles whose first three are a position.
static inline const char *check_args(int B, const double *starts, const double *goals, int pstride, int nBox, const double *boxes, double clear, const double *room,
                                     double res, int cap, int N, int with_N, int dims[3]) {
    if (B < 1 || !starts || !goals || !room || (nBox > 0 && !boxes)) return "need B >= 1 and non-NULL starts, goals, room (and boxes if nBox > 0)";
    if (cap < 2) return "need cap >= 2";
    if (nBox < 0 || nBox > OBCA_PLAN3D_MAXBOX) return "need 0 <= nBox <= OBCA_PLAN3D_MAXBOX (8)";
    if (with_N && (N < 1 || N > OBCA_PLAN3D_NMAX)) return "need 1 <= N <= OBCA_PLAN3D_NMAX (128 = OBCA_QUAD_NMAX)";
    if (!(res > 0) || !(res - res == 0.0) || !(clear - clear == 0.0)) return "need res > 0, res and clear finite";
    double cells = 1.0;
    for (int i = 0; i < 3; i++) {
        if (!(room[i] > 0) || !(room[i] - room[i] == 0.0) || room[i] / res > 1e6) return "need 0 < room[i] < 1e6 res";
        dims[i] = (int)floor(room[i] / res) + 1; cells *= dims[i];
    }
    if (cells > (double)OBCA_PLAN3D_MAXCELLS) return "the grid has more than OBCA_PLAN3D_MAXCELLS (40000) nodes: it does not fit the LDS of one workgroup";
    for (long long i = 0; i < (long long)B; i++) for (int k = 0; k < 3; k++) {
        const double s = starts[i * pstride + k], g = goals[i * pstride + k];
        if (!(s - s == 0.0) || !(g - g == 0.0)) return "a start or goal coordinate is not finite";
    }
    for (long long i = 0; i < (long long)B * nBox * 6; i++) if (!(boxes[i] - boxes[i] == 0.0)) return "a box coordinate is not finite";
    return nullptr;
}

// ---------------------------------------------------------------- the grid
// obca_plan_astar3d's `blocked`, comparison by comparison
PL3_FN bool blocked(const Grid &G, double x, double y, double z) {
    if (x < 0 || y < 0 || z < 0 || x > G.room[0] || y > G.room[1] || z > G.room[2]) return true;
    for (int j = 0; j < G.nBox; j++) {
        const double *b = G.boxes + 6 * j;
        if (x <= b[0] + G.clear && y <= b[1] + G.clear && z <= b[2] + G.clear && x >= -b[3] - G.clear && y >= -b[4] - G.clear && z >= -b[5] - G.clear) return true;
    }
    return false;
}
// its `cell`: the node nearest to a point (lround, cut to the grid; an unblocked point has no negative coordinate)
PL3_FN int node_of(double p, double res, int n) { const long v = lround(p / res); return v < 0 ? 0 : (v > n - 1 ? n - 1 : (int)v); }
PL3_FN float edge_w(double res, int d2) { return (float)(res * sqrt((double)d2)); }
PL3_FN float inf_f() { return HUGE_VALF; }

// one node pulls from its 26 neighbours; true if it was lowered.  w[d2]: edge weight by squared offset length (1, 2, 3)
PL3_FN bool relax_node(float *g, const Grid &G, int c, int x, int y, int z, const float *w) {
    const float g0 = g[c];
    if (g0 < 0.f) return false;
    float best = g0;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++) {
        if ((dz < 0 && z == 0) || (dz > 0 && z == G.nz - 1)) continue;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            if ((dy < 0 && y == 0) || (dy > 0 && y == G.ny - 1)) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if ((!dx && !dy && !dz) || (dx < 0 && x == 0) || (dx > 0 && x == G.nx - 1)) continue;
                const float v = g[c + (dz * G.ny + dy) * G.nx + dx], cand = v + w[dx * dx + dy * dy + dz * dz];
                if (v >= 0.f && cand < best) best = cand;
            }
        }
    }
    if (best < g0) { g[c] = best; return true; }
    return false;
}

// neighbour k = 0 .. 25 of the host's dz, dy, dx loop (the centre skipped): its offsets, and what a step to it would cost in all (+inf: outside, blocked or unreached)
PL3_FN void nb_offset(int k, int &dx, int &dy, int &dz) { const int i = k < 13 ? k : k + 1; dz = i / 9 - 1; dy = (i / 3) % 3 - 1; dx = i % 3 - 1; }
PL3_FN float step_cost(const float *g, const Grid &G, int x, int y, int z, int k, const float *w) {
    int dx, dy, dz; nb_offset(k, dx, dy, dz);
    const int qx = x + dx, qy = y + dy, qz = z + dz;
    if (qx < 0 || qy < 0 || qz < 0 || qx >= G.nx || qy >= G.ny || qz >= G.nz) return inf_f();
    const float v = g[(qz * G.ny + qy) * G.nx + qx];
    return v >= 0.f ? v + w[dx * dx + dy * dy + dz * dz] : inf_f();
}
// the cheapest step from node (x, y, z), ties to the lowest k; -1 if there is none.  On the device: called by the 64 lanes of one wavefront, the same answer in all.
PL3_FN int best_step(const float *g, const Grid &G, int x, int y, int z, const float *w) {
#ifdef OBCA_EMU
    int kb = -1; float m = inf_f();
    for (int k = 0; k < 26; k++) { const float c = step_cost(g, G, x, y, z, k, w); if (c < m) { m = c; kb = k; } }
    return kb;
#else
    const int lane = (int)(threadIdx.x & 63);
    const float c = lane < 26 ? step_cost(g, G, x, y, z, lane, w) : inf_f();
    float m = c;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
    if (!(m < inf_f())) return -1;
    return __ffsll((unsigned long long)__ballot(c == m)) - 1;
#endif
}

// ---------------------------------------------------------------- resampling (scenarios.quad_warm_start)
PL3_FN double seg_len(const double *wp, int j) {
    const double dx = wp[3 * j + 3] - wp[3 * j], dy = wp[3 * j + 4] - wp[3 * j + 1], dz = wp[3 * j + 5] - wp[3 * j + 2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}
// stage k of N + 1 on the polyline of K >= 2 way-points: arc length s = k (total / N) (np.linspace: the last one is the total itself), the segment i is the last one
// whose start lies at or before s (np.searchsorted(cum, s, "right") - 1, cut to the last segment), a segment of length 0 gives its first point
PL3_FN void resample_stage(const double *wp, int K, int N, int k, double out[3]) {
    double tot = 0.0;
    for (int j = 0; j < K - 1; j++) tot += seg_len(wp, j);
    const double s = k == N ? tot : k * (tot / N);
    double cum = 0.0, ci = 0.0; int i = 0;
    for (int j = 0; j < K - 1; j++) { if (cum <= s) { i = j; ci = cum; } cum += seg_len(wp, j); }
    const double L = seg_len(wp, i), a = L > 0 ? (s - ci) / L : 0.0;
    for (int q = 0; q < 3; q++) out[q] = wp[3 * i + q] + a * (wp[3 * i + 3 + q] - wp[3 * i + q]);
}

// ---------------------------------------------------------------- one search
#ifdef OBCA_EMU
static int emu_reverse = 0;      // the host build visits the nodes of a sweep in ascending (0) or descending (1) order: tests/test_plan3d_cpu.py wants the same field bits
#define PL3_TID0 1
#define PL3_WAVE0 1
#define PL3_LANE0 1
#define PL3_BARRIER() ((void)0)
#else
#define PL3_TID0 (threadIdx.x == 0)
#define PL3_WAVE0 (threadIdx.x < 64)
#define PL3_LANE0 (threadIdx.x == 0)
#define PL3_BARRIER() __syncthreads()
#endif

// start, goal: 3 doubles each; boxes: 6 G.nBox doubles (obca_quad_plan_resident.h reads the three where a problem record holds them); lds: 4 control words (three vote
// words, the instance's count), then the field (G.ncell floats).  The instance's count stays in the fourth control word for the caller.
// path: cap x 3; count, sweeps: this instance's; N > 0 and xws != NULL: also the warm start, (N + 1) x 12.
PL3_FN void plan_instance(const double *start, const double *goal, const double *boxes, Grid G, float *lds, double *path, int cap, int *count, int *sweeps, int N, double *xws) {
    int *ctl = (int *)lds; float *g = lds + 4;
    G.boxes = boxes;
    float w[4]; w[0] = 0.f; w[1] = edge_w(G.res, 1); w[2] = edge_w(G.res, 2); w[3] = edge_w(G.res, 3);
    int status = 1, nsweep = 0;
    if (blocked(G, start[0], start[1], start[2]) || blocked(G, goal[0], goal[1], goal[2])) status = -2;      // (every thread decides the same from the same numbers)
    const int sx = node_of(start[0], G.res, G.nx), sy = node_of(start[1], G.res, G.ny), sz = node_of(start[2], G.res, G.nz);
    const int gx = node_of(goal[0], G.res, G.nx), gy = node_of(goal[1], G.res, G.ny), gz = node_of(goal[2], G.res, G.nz);
    const int sid = (sz * G.ny + sy) * G.nx + sx, gid = (gz * G.ny + gy) * G.nx + gx;
#ifndef OBCA_EMU
    // this thread's nodes: c0, c0 + cstep, ... < cend, with the coordinates carried along (no division in the sweeps)
#if PL3_MAP == 0
    const int cstep = PL3_NT, c0 = (int)threadIdx.x, cend = G.ncell;
#else
    const int chunk = (G.ncell + PL3_NT - 1) / PL3_NT, cstep = 1, c0 = (int)threadIdx.x * chunk, cend = c0 + chunk < G.ncell ? c0 + chunk : G.ncell;
#endif
    const int x0 = c0 % G.nx, y0 = (c0 / G.nx) % G.ny, z0 = c0 / (G.nx * G.ny);
    const int stx = cstep % G.nx, sty = (cstep / G.nx) % G.ny, stz = cstep / (G.nx * G.ny);
#define PL3_FOR_NODES for (int c = c0, x = x0, y = y0, z = z0; c < cend; c += cstep, x += stx, y += (x >= G.nx), x -= (x >= G.nx) ? G.nx : 0, y += sty, z += (y >= G.ny), y -= (y >= G.ny) ? G.ny : 0, z += stz)
#else
#define PL3_FOR_NODES for (int i_ = 0, c = 0, x = 0, y = 0, z = 0; i_ < G.ncell && (c = emu_reverse ? G.ncell - 1 - i_ : i_, x = c % G.nx, y = (c / G.nx) % G.ny, z = c / (G.nx * G.ny), true); i_++)
#endif
    if (status > 0) {
        // 1. occupancy: every word of the field is written here, the control words too
        PL3_FOR_NODES g[c] = blocked(G, x * G.res, y * G.res, z * G.res) ? PL3_BLOCKED : (c == gid ? 0.f : inf_f());
        if (PL3_TID0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; ctl[3] = 0; }
        PL3_BARRIER();
        // 2. relaxation
        bool settled = sid == gid;      // (the host search ends on its first node then)
        for (int s = 0; !settled && s < G.ncell; s++) {
            bool low = false;
            PL3_FOR_NODES low |= relax_node(g, G, c, x, y, z, w);
            if (low) ctl[s % 3] = 1;
            PL3_BARRIER();
            settled = ctl[s % 3] == 0;
            if (PL3_TID0) ctl[(s + 2) % 3] = 0;      // the word of sweep s + 2: last read after the barrier of sweep s - 1, next written after that of sweep s + 1
            nsweep = s + 1;
        }
        if (!settled) status = PL3_ST_SWEEPS;
    }
    // 3. descent, on one wavefront
    if (PL3_WAVE0) {
        int cnt = status;      // -2 / -3 as they are
        if (status > 0) {
            int x = sx, y = sy, z = sz, c = sid, k = 1;      // k: way-points written so far (the start point)
            if (PL3_LANE0) { path[0] = start[0]; path[1] = start[1]; path[2] = start[2]; }
            cnt = 0;
            for (int step = 0; step <= G.ncell; step++) {
                if (k + 1 >= cap) { cnt = -1; break; }      // this node and the goal point no longer fit
                if (PL3_LANE0) { path[3 * k] = x * G.res; path[3 * k + 1] = y * G.res; path[3 * k + 2] = z * G.res; }
                k++;
                if (c == gid) { if (PL3_LANE0) { path[3 * k] = goal[0]; path[3 * k + 1] = goal[1]; path[3 * k + 2] = goal[2]; } cnt = k + 1; break; }
                const int kb = best_step(g, G, x, y, z, w);
                if (kb < 0) { cnt = 0; break; }      // (first step only: every node behind it has a finite cost)
                int dx, dy, dz; nb_offset(kb, dx, dy, dz);
                x += dx; y += dy; z += dz; c = (z * G.ny + y) * G.nx + x;
            }
        }
        if (PL3_LANE0) { *count = cnt; if (sweeps) *sweeps = nsweep; ctl[3] = cnt; }
    }
    // 4. the warm start
    PL3_BARRIER();      // (wave 0's way-points and count, for the other waves; every thread reaches it: status is the same in all)
    const int K = ctl[3] > 0 ? ctl[3] : 0;
    // the rest of the caller's array: every word of the output is written, whatever the buffer held
#ifdef OBCA_EMU
    for (int q = 3 * K; q < 3 * cap; q++) path[q] = 0.0;
#else
    for (int q = 3 * K + (int)threadIdx.x; q < 3 * cap; q += PL3_NT) path[q] = 0.0;
#endif
    if (N > 0 && xws) {
#ifdef OBCA_EMU
        for (int k = 0; k <= N; k++) {
#else
        for (int k = (int)threadIdx.x; k <= N; k += PL3_NT) {
#endif
            double p[3] = {0.0, 0.0, 0.0};
            if (K >= 2) resample_stage(path, K, N, k, p);
            for (int r = 0; r < 12; r++) xws[12 * k + r] = r < 3 ? p[r] : 0.0;
        }
    }
#undef PL3_FOR_NODES
}
// in: the instance's record (start, goal, boxes) in one piece
PL3_FN void plan_instance(const double *in, Grid G, float *lds, double *path, int cap, int *count, int *sweeps, int N, double *xws) {
    plan_instance(in, in + 3, in + 6, G, lds, path, cap, count, sweeps, N, xws);
}

}  // namespace pl3
}  // namespace obca
