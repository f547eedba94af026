// obca_plan_resident.h -- the resident route of the parking planner (include/obca_plan_resident.h is the ABI): the obstacle field and the poses of every search are put
// together ON THE DEVICE from the problem record an uploaded batch holds, so that the per-instance search (the planner's kernel text, its `Fields` route) runs in exactly
// the field the solve will solve in and nothing but status words crosses the bus.
//
// plan_pack_instance: one wavefront per instance.  It reads instance i's record (PH_* of obca_solver.h, as batch_upload_range packs it) and writes what the search reads:
//   the search's instance record, 10 doubles: x0[0..2], sin, cos of the heading, xF[0..2], sin, cos -- the only two libm calls per pose, and of this text;
//   the instance's part of hy::Fields: A, b = the record's UNIT rows as they stand, rn = nrm = 1.0 (the norm is 1 by construction: no hypot), per obstacle its row count,
//   row offset, vertex offset and its polygon -- the rows cut from the square of half side far_ by the polygon() the planner's host code calls --, and the four-int
//   record rec.
// Strides are FIXED per instance, so no prefix sum runs over the batch: nObMax obstacles, MMax rows, nObMax + 1 entries of off / voff, PLR_NV vertices per obstacle (a
// convex polygon gains at most one vertex per half-plane: 4 + OB_VMAX).  field_of computes F.v = S.v + rec[0], F.off = S.off + rec[0] + i, so rec = { i nObMax, i MMax,
// i nObMax PLR_NV, nOb } lands instance i on its own block of nObMax counts and of nObMax + 1 offsets; inside the block the polygons lie one behind the other, as the
// search's bounding test reads them (voff[j] .. voff[j + 1]).
// Obstacles run one per lane.  A polygon's vertices depend on its own rows only and every word has one writer, so the block is the same whatever the lane order; where a
// polygon STARTS depends on the counts of the obstacles before it: those go through LDS between two passes, the second clips again (at most OB_VMAX cuts) and writes.
// A record whose counts are outside the planner's limits cannot exist: park_prefix refuses an upload with other than 1 .. OB_NOBMAX obstacles, 1 .. OB_VMAX rows each or
// more than OB_MMAX rows, all within OBCA_HYBRID_MAXOB / OBCA_HYBRID_MAXROWS.  Every loop is bounded by those limits anyway, every index cut to its block.
// fp contraction is off: this header comes behind the planner's kernel text in the translation unit (which switches it off to the end) and needs its hy:: names.
#pragma once
#include "obca_solver.h"
#ifndef HY_CLIP
#error "include the planner's kernel text (hy::, HY_FN, HY_HD, HY_CLIP) before this header: it is compiled behind it, under its fp-contraction rule"
#endif

namespace obca {
namespace plr {

#define PLR_NT 64                   // threads per instance: one wavefront
#define PLR_NV (4 + OB_VMAX)        // vertices of an obstacle's block
static_assert(OB_NOBMAX <= OBCA_HYBRID_MAXOB && OB_VMAX <= OBCA_HYBRID_MAXROWS && PLR_NV <= HY_CLIP && OB_NOBMAX <= PLR_NT, "a batch's record must fit the planner's limits, an obstacle a lane");

#ifdef OBCA_EMU
#define PLR_FOR(i, n) for (int i##_ = 0, i##n_ = (n), i = 0; i##_ < i##n_ && ((i = hy::emu_perm(i##_, i##n_)), true); i##_++)      // HY_FOR: ascending, descending or shuffled (hy::emu_order)
#define PLR_SYNC() ((void)0)
#define PLR_LANE0 1
#define PLR_LDS
#else
#define PLR_FOR(i, n) for (int i = (int)threadIdx.x, i##n_ = (n); i < i##n_; i += PLR_NT)
#define PLR_SYNC() __syncthreads()
#define PLR_LANE0 (threadIdx.x == 0)
#define PLR_LDS __shared__
#endif

// What the packing writes and the search reads, for B instances: byte offsets of the arrays from the start of the block, [ inst B x 10 | A | b | rn | nrm | vert | rec
// v off voff (ints) ]; `bytes` is a multiple of 8.
struct Layout { size_t inst, A, b, rn, nrm, vert, rec, v, off, voff, bytes; };
HY_HD Layout layout(int B, int nObMax, int MMax) {
    const size_t n = (size_t)B, rows = n * MMax, obs = n * nObMax;
    Layout l; l.inst = 0; l.A = n * 80; l.b = l.A + rows * 16; l.rn = l.b + rows * 8; l.nrm = l.rn + rows * 8; l.vert = l.nrm + rows * 8;
    l.rec = l.vert + obs * PLR_NV * 16; l.v = l.rec + n * 16; l.off = l.v + obs * 4; l.voff = l.off + (obs + n) * 4;
    l.bytes = (l.voff + (obs + n) * 4 + 7) / 8 * 8;
    return l;
}
struct Block { double *inst; int *rec, *v, *off, *voff; double *A, *b, *rn, *nrm, *vert; };
HY_HD Block block_at(char *d, const Layout &l) {
    Block o; o.inst = (double *)(d + l.inst); o.A = (double *)(d + l.A); o.b = (double *)(d + l.b); o.rn = (double *)(d + l.rn); o.nrm = (double *)(d + l.nrm);
    o.vert = (double *)(d + l.vert); o.rec = (int *)(d + l.rec); o.v = (int *)(d + l.v); o.off = (int *)(d + l.off); o.voff = (int *)(d + l.voff);
    return o;
}
HY_HD hy::Fields fields_of(const Block &o) {
    hy::Fields S; S.rec = o.rec; S.v = o.v; S.off = o.off; S.voff = o.voff; S.A = o.A; S.b = o.b; S.rn = o.rn; S.nrm = o.nrm; S.vert = o.vert;
    return S;
}

HY_FN int cut(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// obstacle j of the record as a polygon: its rows cut from the square of half side far_ (the planners' one polygon()).  The vertices are in the buffer returned, n of them.
HY_FN const hy::P2 *polygon(const double *p, int j, double far_, hy::P2 *pa, hy::P2 *pb, int &n) {
    const int rows = cut((int)p[PH_VOB + j], 0, OB_VMAX), r0 = cut((int)p[PH_ROFF + j], 0, OB_MMAX - rows);
    return hy::polygon(p + PH_A + 2 * r0, p + PH_B + r0, rows, far_, pa, pb, n);
}

// instance i of a batch whose blocks hold nObMax obstacles and MMax rows; p: its problem record; far_ = host_far(XYbounds)
HY_FN void plan_pack_instance(int i, int nObMax, int MMax, double far_, const double *p, const Block &o) {
    PLR_LDS int nvx[OB_NOBMAX];      // vertices of every obstacle's polygon
    const int nob = cut(nObMax, 0, OB_NOBMAX), mm = cut(MMax, 0, OB_MMAX);
    const int nOb = cut((int)p[PH_NOB], 0, nob), M = cut((int)p[PH_M], 0, mm);
    const size_t ob0 = (size_t)i * nObMax, row0 = (size_t)i * MMax, vx0 = ob0 * PLR_NV, of0 = ob0 + i;
    if (PLR_LANE0) {
        double *q = o.inst + (size_t)i * 10;
        for (int e = 0; e < 2; e++) {
            const double *s = p + (e ? PH_XF : PH_X0);
            q[5 * e] = s[0]; q[5 * e + 1] = s[1]; q[5 * e + 2] = s[2]; q[5 * e + 3] = sin(s[2]); q[5 * e + 4] = cos(s[2]);
        }
        int *rec = o.rec + 4 * (size_t)i;
        rec[0] = (int)ob0; rec[1] = (int)row0; rec[2] = (int)vx0; rec[3] = nOb;
    }
    PLR_FOR(r, mm) {      // (the rows behind the instance's own are the zeros of the upload: no search reads them)
        o.A[2 * (row0 + r)] = p[PH_A + 2 * r]; o.A[2 * (row0 + r) + 1] = p[PH_A + 2 * r + 1]; o.b[row0 + r] = p[PH_B + r];
        o.rn[row0 + r] = 1.0; o.nrm[row0 + r] = 1.0;
    }
    PLR_FOR(j, nOb) {
        hy::P2 pa[HY_CLIP], pb[HY_CLIP]; int n;
        (void)polygon(p, j, far_, pa, pb, n);
        nvx[j] = cut(n, 0, PLR_NV);
    }
    PLR_SYNC();
    PLR_FOR(j, nOb) {
        hy::P2 pa[HY_CLIP], pb[HY_CLIP]; int n;
        const hy::P2 *poly = polygon(p, j, far_, pa, pb, n);
        n = cut(n, 0, PLR_NV);
        int v0 = 0; for (int k = 0; k < j; k++) v0 += nvx[k];
        o.v[ob0 + j] = cut((int)p[PH_VOB + j], 0, OB_VMAX); o.off[of0 + j] = cut((int)p[PH_ROFF + j], 0, M); o.voff[of0 + j] = v0;
        for (int k = 0; k < n; k++) { o.vert[2 * (vx0 + v0 + k)] = poly[k].x; o.vert[2 * (vx0 + v0 + k) + 1] = poly[k].y; }
        if (j == nOb - 1) { o.off[of0 + nOb] = M; o.voff[of0 + nOb] = v0 + n; }
    }
    if (PLR_LANE0 && nOb == 0) { o.off[of0] = 0; o.voff[of0] = 0; }
}

#ifndef OBCA_EMU
__global__ __launch_bounds__(PLR_NT) void obca_plan_pack_kernel(int B, int nObMax, int MMax, double far_, const double *prob, size_t s_prob, Block o) {
    const int i = blockIdx.x;
    if (i >= B) return;
    plan_pack_instance(i, nObMax, MMax, far_, prob + (size_t)i * s_prob, o);
}
#endif

}  // namespace plr
}  // namespace obca
