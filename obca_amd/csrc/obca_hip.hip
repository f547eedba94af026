// obca_hip.hip -- HIP kernels and the C ABI of libobca_hip.so (gfx950 only; see include/obca_hip.h).
//
// Kernels
//   obca_parking_ipm_kernel : one wavefront (64-thread workgroup) per problem instance, persistent over the whole
//                             interior-point solve (obca_solver.h).  grid = B, block = 64; four instances per CU.
//   obca_quad_ipm_kernel    : the same for the quadcopter NLP (obca_quad_solver.h).
//   obca_dualws_kernel      : one lane per (instance, stage, obstacle) convex sub-problem of DualMultWS (obca_model.h).
//   obca_validate_*_kernel  : one wavefront per instance, the a-posteriori feasibility classes of a solution or of a caller's trajectory (obca_validate.h).
//   obca_clearance_*_kernel : one wavefront per instance, the clearance of a solution or of a caller's trajectory between its nodes (obca_clearance.h).
//   obca_rollout_*_kernel   : one wavefront per instance, a solution or a caller's trajectory applied to the continuous vehicle model: deviations, clearance of the rolled samples (obca_rollout.h).
//   obca_track_*_kernel     : one wavefront per instance, TVLQR gains about a solution or a caller's trajectory and the closed loop rolled on the continuous model (obca_track.h).
//   obca_ensemble_*_kernel  : one wavefront per instance, one member per lane: up to 64 disturbed closed loops about a solution or a caller's trajectory, the gains computed once (obca_ensemble.h).
//   obca_advance_*_kernel   : one wavefront per instance, one step of the closed receding-horizon loop: the plant over the first `shift` intervals of the solution, the restart from the state it reached (obca_advance.h).
//   obca_move_*_kernel      : one wavefront per instance, the obstacle words of the problem records moved and inflated in place, all or nothing per instance (obca_scene_edit.h).
//   obca_predict_*_kernel   : one wavefront per instance, the clearance of a solution or of a caller's trajectory against obstacles that move at given rates while it is executed (obca_predict.h).
//   obca_certify_*_kernel   : one wavefront per instance, the clearance of a solution or of a caller's trajectory certified along its whole path by conservative advancement (obca_certify.h).
//   obca_refine_*_kernel    : one wavefront per destination instance, a solved parking instance on a finer horizon (obca_refine.h): into a second resident batch or host-bound arrays.
//   obca_quad_subdivide_*_kernel : the same for a solved quadcopter instance (obca_quad_subdivide.h): it rewrites a problem record.
//   obca_path_ws_*_kernel   : one wavefront per instance, the parking warm start from a planner path (obca_path_ws.h): into host-bound arrays or into a resident batch.
//   obca_plan_pack_kernel   : one wavefront per instance, the planner's obstacle field and poses from the problem record of a resident batch (obca_plan_resident.h).
//   obca_quad_plan_resident_kernel : one workgroup per selected instance, the quadcopter's 3-D grid search from the problem record of a resident batch, the resampled path
//                             written into the record's warm start (obca_quad_plan_resident.h over obca_plan3d.h).
//   obca_shift_kernel, obca_quad_shift_kernel : receding-horizon restarts, one workgroup per instance: the warm start of the next solve from the last solution
//                             (parking: obca_shift.h; quadcopter: obca_quad_shift.h).
// Host helpers the entry points are built from (below "host side"): EventPair, KernelStage (staging types); run_validate, launch_timed (a kernel between two events, results down);
//   run_chunks with parking_chunks / quad_chunks (host-pointer calls over the slots); into_call (refine / subdivide into a second batch); hybrid_call (both planner entry points) over hybrid_reserve / hybrid_launch (shared with the resident route).
// Memory (per instance, fp64, all in HBM; sizes for N=80, 3 obstacles / 5 rows in brackets):
//   prob  header+rx,ry,ryaw   [495]      z, zn  primal-dual iterate and the line search's
//   trial point (they swap) [6797 each]      d  stage part of the search direction [~650 used]
//   as    assembled stage records (N+1) x 60 [4860]     rs  Riccati records N x 74 [5920]      slice  state of a parked solve [480]
//   (the condensed obstacle sums, the forward-sweep trajectory and the composed stage-pair maps live in LDS; `oc` is used by the quadcopter kernel only)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <string>
#include <thread>
#include <atomic>
#include <algorithm>
#include "obca_solver.h"
#include "obca_quad_solver.h"
#include "obca_validate.h"
#include "obca_shift.h"
#include "obca_quad_shift.h"
#include "obca_path_ws.h"
#include "obca_clearance.h"
#include "obca_refine.h"
#include "obca_quad_subdivide.h"
#include "obca_rollout.h"
#include "obca_track.h"
#include "obca_ensemble.h"
#include "obca_advance.h"
#include "obca_scene_edit.h"
#include "obca_certify.h"
#include "obca_predict.h"
#include "../../include/obca_hip.h"
#include "../../include/obca_path_ws.h"
#include "../../include/obca_clearance.h"
#include "../../include/obca_refine.h"
#include "../../include/obca_quad_subdivide.h"
#include "../../include/obca_rollout.h"
#include "../../include/obca_track.h"
#include "../../include/obca_ensemble.h"
#include "../../include/obca_advance.h"
#include "../../include/obca_scene_edit.h"
#include "../../include/obca_certify.h"
#include "../../include/obca_predict.h"

using namespace obca;
#ifdef OBCA_POISON
#ifndef OBCA_LDS_GUARD
#define OBCA_LDS_GUARD 1024      // doubles (8 KB) of NaN guard behind the dynamic LDS block of the poisoned build
#endif
#endif

static_assert(sizeof(obca_opts) == sizeof(OptsAbi) && offsetof(obca_opts, max_soc) == offsetof(OptsAbi, max_soc), "obca_opts must mirror obca::OptsAbi");
static_assert(OBCA_QUAD_NMAX == QNMAX, "ABI limits must match the kernels");
static_assert(OBCA_PATH_WS_MAXNODES == PW_MAXNODES, "ABI limits must match the kernels");
static_assert(OBCA_CLR_OUT == CL_OUT && OBCA_CLR_MAXSUB == CL_SMAX && OBCA_CLR_TOUCH == CL_TOUCH, "ABI limits must match the kernels");
static_assert(OBCA_REFINE_MAXFACTOR == RF_MAXFACTOR, "ABI limits must match the kernels");
static_assert(OBCA_ROLL_OUT == RO_OUT && OBCA_ROLL_CLR == RO_CLR && OBCA_ROLL_MAXSUB == CL_SMAX, "ABI limits must match the kernels");
static_assert(OBCA_TRK_OUT == TK_OUT, "ABI limits must match the kernels");
static_assert(OBCA_ADV_OUT == AV_OUT, "ABI limits must match the kernels");
static_assert(OBCA_CERT_OUT == CT_OUT && OBCA_CERT_TICKS == CT_TICKS, "ABI limits must match the kernels");
static_assert(OBCA_VMAX == OB_VMAX && OBCA_NOBMAX == OB_NOBMAX && OBCA_NMAX == OB_NMAX && OBCA_MMAX == OB_MMAX, "ABI limits must match the kernels");

struct DevBufs {
    double *prob, *z0, *z, *zn, *d, *as, *rs, *oc, *info, *dws, *prof;     // zn: the second iterate buffer of the fused line search (obca_solver.h)
    double *slice;                                   // slice records (SL_SIZE doubles per instance) of the two-launch schedule
    // second-order correction (opts.max_soc > 0): the corrected right-hand-side rows of every instance; allocated at the first such solve
    double *csoc; size_t s_csoc, o_csoc;      // per instance: [ direction of a correction, o_csoc doubles (indexed like d: the layout's offsets below zxL) | the rows c_soc ]
    int *order;                                      // B instance indices in dispatch order (-1: nothing left to do), then the class counters
    size_t s_prob, s_z, s_as, s_rs, s_oc;   // strides in doubles
};

// One wavefront per SIMD (four one-wavefront instances per CU): each wave may then use 256 VGPRs + 256 AGPRs, and the register-hungry per-lane phases
// keep their spills (and most callee-saved registers) in AGPRs instead of scratch.  Against two waves per SIMD with 256 registers each this
// is faster at every batch size measured: a lone instance is ~10 % quicker per pass, and a full machine no longer streams the scratch
// save areas through HBM.
#ifndef OBCA_IPM_WAVES_PER_EU
#define OBCA_IPM_WAVES_PER_EU 1
#endif
#define OBCA_RESIDENT_PER_CU (4 * OBCA_IPM_WAVES_PER_EU)   // parking instances (one wavefront each) resident per CU
__global__ __launch_bounds__(OB_NT, OBCA_IPM_WAVES_PER_EU) void obca_parking_ipm_kernel(int B, int N, DevBufs b, Opts o, int mode, int budget, int max_soc, int recalc_y, int lsq_init, int restoration) {
    // mode 0: fresh solve of instance blockIdx.x (at most `budget` factorisation passes if budget > 0); mode 1: continue the parked solves in
    // the order the ordering kernel chose (workgroups are dispatched in blockIdx order, so the expected stragglers start first)
    const int inst = mode == 1 ? b.order[blockIdx.x] : (int)blockIdx.x;
    if (inst < 0 || inst >= B) return;
#ifdef OBCA_POISON      // diagnostic build: whatever the previous workgroup on this CU left in LDS is replaced by NaNs before anything is initialised
    {
#ifndef OBCA_POISON_VALUE      // (NaN hides behind fmax / fmin and every comparison: build with -DOBCA_POISON_VALUE=1e30 as well)
#define OBCA_POISON_VALUE __longlong_as_double(-1LL)
#endif
        const double nan_ = OBCA_POISON_VALUE;
        double *w = (double *)&g_sh;
#ifndef OBCA_POISON_PARTS
#define OBCA_POISON_PARTS 15      // bit 0: HBM work buffers, 1: the static LDS block, 2: the dynamic LDS block, 3: the guard behind it (bisecting builds set a subset)
#endif
        if (OBCA_POISON_PARTS & 2) for (int i = threadIdx.x; i < (int)(sizeof(Shared) / sizeof(double)); i += OB_NT) w[i] = nan_;
        if (OBCA_POISON_PARTS & 4) for (int i = threadIdx.x; i < (int)OB_DYN_LDS_DOUBLES(N); i += OB_NT) g_traj[i] = nan_;
        if (OBCA_POISON_PARTS & 8) for (int i = (int)OB_DYN_LDS_DOUBLES(N) + threadIdx.x; i < (int)OB_DYN_LDS_DOUBLES(N) + OBCA_LDS_GUARD; i += OB_NT) g_traj[i] = nan_;
        __syncthreads();
    }
#endif
    if (threadIdx.x == 0) {
        Inst &I = g_sh.inst;
        I.prob = (const gdbl *)(b.prob + (size_t)inst * b.s_prob);
        I.z = (gdbl *)(b.z + (size_t)inst * b.s_z); I.zn = (gdbl *)(b.zn + (size_t)inst * b.s_z); I.d = (gdbl *)(b.d + (size_t)inst * b.s_z);
        I.as = (gdbl *)(b.as + (size_t)inst * b.s_as); I.rs = (gdbl *)(b.rs + (size_t)inst * b.s_rs);
        I.oc = nullptr;
        g_sh.soc.dsoc = b.csoc ? (gdbl *)(b.csoc + (size_t)inst * b.s_csoc) : nullptr;
        g_sh.soc.csoc = b.csoc ? (gdbl *)(b.csoc + (size_t)inst * b.s_csoc + b.o_csoc) : nullptr;
#ifdef OBCA_PROFILE
        I.tlast = clock64();
#endif
    }
#ifdef OBCA_PROFILE
    if (threadIdx.x < 16) g_sh.prof[threadIdx.x] = mode ? b.prof[(size_t)inst * 16 + threadIdx.x] : 0.0;   // counters add up over the slices
#endif
    __syncthreads();
#if defined(OBCA_PROFILE) && !defined(OBCA_PROFILE_FINE)      // slots 11, 12 (the per-stage counters of the FINE build): when the workgroup started and ended on the constant 100 MHz clock (tools/load_profile.py: residency, shader clock rate)
    if (threadIdx.x == 0 && mode == 0) g_sh.prof[11] = (double)wall_clock64();
#endif
    solve_instance(N, o, b.info + (size_t)inst * 8, (gdbl *)(b.slice + (size_t)inst * SL_SIZE), mode, budget, max_soc, recalc_y, lsq_init, restoration);
#ifdef OBCA_PROFILE
    __syncthreads();
#ifndef OBCA_PROFILE_FINE
    if (threadIdx.x == 0 && mode == 0) {      // slot 12: resident time + (which SIMD of which CU of which XCD: XCC_ID << 12 | HW_ID[15:4]) / 65536 in the fraction
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        g_sh.prof[12] = ((double)wall_clock64() - g_sh.prof[11]) + (double)(((xcc & 15u) << 12) | ((hw >> 4) & 0xfffu)) / 65536.0;
    }
    __syncthreads();
#endif
    if (threadIdx.x < 16) b.prof[(size_t)inst * 16 + threadIdx.x] = g_sh.prof[threadIdx.x];
#endif
}

// instances resident per CU: registers allow 4 x OBCA_IPM_WAVES_PER_EU, LDS (static Shared + the horizon-sized dynamic part) may allow fewer -- ask the runtime
static int parking_resident_per_cu(int N) {
    // 0 = not asked yet.  Worker lanes of several devices call this concurrently: atomics (the answer depends on the
    static std::atomic<int> cache[OB_NMAX + 1];
                                                         // code object and the horizon only -- every device of a context is
                                                         // a gfx950 with 160 KB of LDS per CU, obca_create_multi checks)
    if (N < 0 || N > OB_NMAX) return OBCA_RESIDENT_PER_CU;
    int n = cache[N].load(std::memory_order_relaxed);
    if (!n) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, obca_parking_ipm_kernel, OB_NT, OB_DYN_LDS_DOUBLES(N) * sizeof(double)) != hipSuccess || n < 1) n = OBCA_RESIDENT_PER_CU;
        cache[N].store(n, std::memory_order_relaxed);
    }
    return n;
}

// difficulty class of a parked instance (0..63, higher = dispatched earlier)
__device__ inline int obca_slice_class(const double *st) {
    // inertia rungs so far + the correction / re-estimate passes of the IPOPT switches
    const int nreg = (int)st[SL_NREG] + (int)st[SL_NREGPREV] + (int)st[SL_XPASS];
    const double pinf = st[SL_PINF];
    int c = 8 * (nreg < 7 ? nreg : 7);
    // within the same retry count: the constraint violation that is left, one class per decade from 1e-6 up
    int e = (pinf > 1e-30 && pinf < 1e30) ? (int)floor(log10(pinf)) + 7 : (pinf >= 1e30 ? 7 : 0);
    e = e < 0 ? 0 : (e > 7 ? 7 : e);
    return c + e;
}

// Dispatch order of the second launch: parked instances sorted by a difficulty class (descending), finished ones dropped.  The class is what
// the first slice revealed about the instance: every inertia retry so far counts, then the constraint violation still left -- the instances
// that go on to need two or three times the median number of passes are almost all among those that already needed retries (DESIGN.md
// section 3 has the measured ranking quality).  One workgroup, counting sort on 64 classes; the order inside a class is whatever the LDS
// atomics give, which changes timing only, never results.
__global__ __launch_bounds__(1024) void obca_order_kernel(int B, const double *info, const double *slice, int *order) {
    __shared__ int cnt[64], base[64];
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        if ((int)info[(size_t)i * 8] != ST_SUSPENDED) continue;
        const double *st = slice + (size_t)i * SL_SIZE;
        atomicAdd(&cnt[obca_slice_class(st)], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) { int acc = 0; for (int c = 63; c >= 0; c--) { base[c] = acc; acc += cnt[c]; cnt[c] = 0; } base[0] = base[0]; order[B] = acc; }
    __syncthreads();
    const int total = order[B];
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        if ((int)info[(size_t)i * 8] != ST_SUSPENDED) continue;
        const double *st = slice + (size_t)i * SL_SIZE;
        const int c = obca_slice_class(st);
        order[base[c] + atomicAdd(&cnt[c], 1)] = i;
    }
    for (int i = total + threadIdx.x; i < B; i += blockDim.x) order[i] = -1;
}

// one lane per (instance, stage, obstacle); writes lam/mu into the iterate buffer `z` (instance layout) and d into dws
// (four wavefronts per SIMD for the 2-row class -- 128 registers, 35 spilled -- was measured
// in round 4: 0.29 ms against 0.25 ms at three wavefronts with 158 registers: not kept)
template <int VM>
__global__ __launch_bounds__(256) void obca_dualws_kernel(int B, int N, int nObMax, DevBufs b, double *zdst, size_t s_zdst) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)(N + 1) * nObMax;
    if (gid >= (long long)B * per) return;
    const int inst = (int)(gid / per); const int rem = (int)(gid % per);
    const int k = rem / nObMax, j = rem % nObMax;
    const double *p = b.prob + (size_t)inst * b.s_prob;
    const int nOb = (int)p[PH_NOB], M = (int)p[PH_M];
    if (j >= nOb) return;
    const int v = (int)p[PH_VOB + j], r0 = (int)p[PH_ROFF + j];
    double a1[VM], a2[VM], bj[VM], g[4];
#pragma unroll
    for (int i = 0; i < VM; i++) { bool on = i < v; a1[i] = on ? p[PH_A + 2 * (r0 + i)] : 0.0; a2[i] = on ? p[PH_A + 2 * (r0 + i) + 1] : 0.0; bj[i] = on ? p[PH_B + r0 + i] : 0.0; }
#pragma unroll
    for (int i = 0; i < 4; i++) g[i] = p[PH_G + i];
    const double rx = p[OB_HDR + k], ry = p[OB_HDR + (N + 1) + k], ryaw = p[OB_HDR + 2 * (N + 1) + k], off = p[PH_OFF];
    double sn, cs; sincos(ryaw, &sn, &cs);
    double lam[VM], mu[4], dv;
    dualws_one<VM>(v, a1, a2, bj, g, rx + cs * off, ry + sn * off, cs, sn, lam, mu, &dv);
    Lay l; make_layout(N, nOb, M, l);
    double *z = zdst + (size_t)inst * s_zdst;
#pragma unroll
    for (int i = 0; i < VM; i++) if (i < v) z[l.lam + k * M + r0 + i] = lam[i];
#pragma unroll
    for (int i = 0; i < 4; i++) z[l.mu + 4 * (k * nOb + j) + i] = mu[i];
    if (b.dws) b.dws[(size_t)inst * per + rem] = dv;
}

// receding-horizon restart of the parking batch (obca_shift.h): one wavefront per instance writes the start iterate of the next solve from the resident solution and advances
// X0 and the tracking reference of its problem record; the direction buffer (free between solves) is the scratch of the in-place move; x0_new: 4 x B on the device, or NULL
__global__ __launch_bounds__(OB_NT) void obca_shift_kernel(int B, int N, int shift, DevBufs b, const double *x0_new) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    shf::shift_instance(N, shift, b.prob + (size_t)inst * b.s_prob, b.z + (size_t)inst * b.s_z, b.z0 + (size_t)inst * b.s_z, b.d + (size_t)inst * b.s_z,
                        x0_new ? x0_new + (size_t)inst * 4 : nullptr, 0);
}

// quadcopter path: one 128-thread workgroup per instance, persistent over the interior-point solve (obca_quad_solver.h)
struct QDevBufs {
    double *prob, *z, *d, *as, *rs, *oc, *info, *prof;
    size_t s_prob, s_z, s_d, s_as, s_rs, s_oc;
};
#ifndef OBCA_QUAD_WAVES_PER_EU
#define OBCA_QUAD_WAVES_PER_EU 1      // as for the parking kernel
#endif
__global__ __launch_bounds__(QNT, OBCA_QUAD_WAVES_PER_EU) void obca_quad_ipm_kernel(int B, int N, QDevBufs b, Opts o, int max_soc, int lsq_init, int obj_scaling) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
#ifdef OBCA_POISON
    {
        const double nan_ = OBCA_POISON_VALUE;
        double *w = (double *)&quad::gq_sh;
        for (int i = threadIdx.x; i < (int)(sizeof(quad::QShared) / sizeof(double)); i += QNT) w[i] = nan_;
        for (int i = threadIdx.x; i < (N + 2) * (QS + QU); i += QNT) quad::gq_traj[i] = nan_;
        __syncthreads();
    }
#endif
    if (threadIdx.x == 0) {
        quad::QInst &I = quad::gq_sh.inst;
        I.prob = (const gdbl *)(b.prob + (size_t)inst * b.s_prob);
        I.z = (gdbl *)(b.z + (size_t)inst * b.s_z); I.d = (gdbl *)(b.d + (size_t)inst * b.s_d);
        I.as = (gdbl *)(b.as + (size_t)inst * b.s_as); I.rs = (gdbl *)(b.rs + (size_t)inst * b.s_rs);
        I.oc = (gdbl *)(b.oc + (size_t)inst * b.s_oc);
#ifdef OBCA_PROFILE
        quad::gq_sh.tlast = clock64();
#endif
    }
#ifdef OBCA_PROFILE
    if (threadIdx.x < 16) quad::gq_sh.prof[threadIdx.x] = 0;
#endif
    __syncthreads();
    quad::q_solve_instance(N, o, b.info + (size_t)inst * 8, max_soc, lsq_init, obj_scaling);
#ifdef OBCA_PROFILE
    __syncthreads();
    if (threadIdx.x < 16) b.prof[(size_t)inst * 16 + threadIdx.x] = quad::gq_sh.prof[threadIdx.x];
#endif
}

// receding-horizon restart of the quadcopter batch (obca_quad_shift.h): one wavefront per instance rewrites the warm start, TWS, DWS, X0 (and XF) words of its problem
// record from the resident solution; x0_new / xF_new: 12 x B on the device, or NULL
__global__ __launch_bounds__(QNT) void obca_quad_shift_kernel(int B, int N, int shift, QDevBufs b, const double *x0_new, const double *xF_new) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    quad::quad_shift_instance(N, shift, b.prob + (size_t)inst * b.s_prob, b.z + (size_t)inst * b.s_z, b.info + (size_t)inst * 8,
                              x0_new ? x0_new + (size_t)inst * QX : nullptr, xF_new ? xF_new + (size_t)inst * QX : nullptr);
}

// a-posteriori checks (obca_validate.h): one wavefront per instance; the point is read in the solver's layout (resident: the last solution; host-pointer
// entries: the packed trajectory), `aux` holds per instance [ |a_r| of the MMax rows | timeScale (N + 1) | slack nObMax x (N + 1) ] (the last two for host-pointer calls only)
__global__ __launch_bounds__(OB_NT) void obca_validate_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *aux, size_t s_aux,
                                                                      int MMax, int use_ts, int use_sl, double tol, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = aux + (size_t)inst * s_aux;
    val::validate_parking_instance(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, a, use_ts ? a + MMax : nullptr, use_sl ? a + MMax + N + 1 : nullptr, tol, out + (size_t)inst * PV_OUT);
}
__global__ __launch_bounds__(QNT) void obca_validate_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *base, size_t s_base, int ox, int ou, int ot, int tstride, int olam,
                                                                 double tol, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *v = base + (size_t)inst * s_base;
    val::validate_quad_instance(N, prob + (size_t)inst * s_prob, v + ox, v + ou, v + ot, tstride, v + olam, tol, out + (size_t)inst * QV_OUT);
}

// clearance between the nodes (obca_clearance.h): one wavefront per instance; z: points in the solver's layout (resident: the last solution; host-pointer entry: the packed
// trajectory), ts: (N + 1) timeScale values per instance or NULL (the point's own t); VM: the row class of the batch's widest obstacle, as for obca_dualws_kernel
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_clearance_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *ts, int S, double need, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    clr::clearance_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, ts ? ts + (size_t)inst * (N + 1) : nullptr, S, need, 0, out + (size_t)inst * CL_OUT);
}
// x: 12 x (N + 1) per instance at stride s_x, ts[k * tstride] at stride s_ts (resident: both inside the iterate, one t; host-pointer entry: x in the problem record, timeScale beside it)
__global__ __launch_bounds__(QNT) void obca_clearance_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *ts, size_t s_ts, int tstride,
                                                                  int S, double need, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    clr::clearance_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, ts + (size_t)inst * s_ts, tstride, S, need, 0, out + (size_t)inst * CL_OUT);
}

// rollout on the continuous models (obca_rollout.h): one wavefront per instance; the arguments of the clearance kernels, then the two regions of the work buffer: the sample
// poses (s_pose doubles per instance) and the node states (s_X)
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_rollout_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *ts, int S, int restart, double need,
                                                                     double *pose, size_t s_pose, double *X, size_t s_X, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    roll::rollout_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, ts ? ts + (size_t)inst * (N + 1) : nullptr, S, restart, need, 0,
                                       pose + (size_t)inst * s_pose, X + (size_t)inst * s_X, out + (size_t)inst * RO_OUT);
}
__global__ __launch_bounds__(QNT) void obca_rollout_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *u, size_t s_u, const double *ts, size_t s_ts, int tstride,
                                                                int S, int restart, double need, double *pose, size_t s_pose, double *X, size_t s_X, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    roll::rollout_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, u + (size_t)inst * s_u, ts + (size_t)inst * s_ts, tstride, S, restart, need, 0,
                                pose + (size_t)inst * s_pose, X + (size_t)inst * s_X, out + (size_t)inst * RO_OUT);
}

// closed-loop rollout (obca_track.h): one wavefront per instance; the arguments of the rollout kernels with the two modes and the weights, `aux` (s_aux doubles per
// instance, dx0 first; has_dx0 0: none), then the regions of the work buffer -- [A|B] with the applied inputs behind it (s_AB doubles per instance), the sample poses, the
// node states -- and the gains (s_K)
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_track_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *aux, size_t s_aux, int has_dx0, int has_ts,
                                                                   int S, int feedback, int clamp, trk::Weights w, double need, double *AB, size_t s_AB, double *pose, size_t s_pose,
                                                                   double *X, size_t s_X, double *K, size_t s_K, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = aux + (size_t)inst * s_aux;
    trk::track_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, has_ts ? a + 4 : nullptr, S, feedback, clamp, w, has_dx0 ? a : nullptr, need, 0,
                                    AB + (size_t)inst * s_AB, AB + (size_t)inst * s_AB + (size_t)N * 4 * 6, pose + (size_t)inst * s_pose, X + (size_t)inst * s_X, K + (size_t)inst * s_K, out + (size_t)inst * TK_OUT);
}
__global__ __launch_bounds__(QNT) void obca_track_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *u, size_t s_u, const double *ts, size_t s_ts, int tstride,
                                                              const double *aux, size_t s_aux, int has_dx0, int S, int feedback, int clamp, trk::Weights w, double need,
                                                              double *AB, size_t s_AB, double *pose, size_t s_pose, double *X, size_t s_X, double *K, size_t s_K, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    trk::track_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, u + (size_t)inst * s_u, ts + (size_t)inst * s_ts, tstride, S, feedback, clamp, w,
                             has_dx0 ? aux + (size_t)inst * s_aux : nullptr, need, 0, AB + (size_t)inst * s_AB, AB + (size_t)inst * s_AB + (size_t)N * QX * (QX + QU), pose + (size_t)inst * s_pose, X + (size_t)inst * s_X,
                             K + (size_t)inst * s_K, out + (size_t)inst * TK_OUT);
}

// closed-loop ensemble (obca_ensemble.h): one wavefront per instance, one member per lane; the arguments of the track kernels with the number of members M; `aux` (s_aux
// doubles per instance) holds [ dx0 nx x M | dub nu x M | what a host-pointer call adds ]; AB and K as the track kernels take them, then the member records (M x EN_MEM per
// instance) and the final states (M x nx)
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_ensemble_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *aux, size_t s_aux, int has_ts,
                                                                      int S, int M, int feedback, int clamp, trk::Weights w, double need, double *AB, size_t s_AB, double *K, size_t s_K,
                                                                      double *mem, double *fin, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = aux + (size_t)inst * s_aux;
    ens::ensemble_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, has_ts ? a + 6 * M : nullptr, S, M, feedback, clamp, w, a, a + 4 * M, need, 0,
                                       AB + (size_t)inst * s_AB, K + (size_t)inst * s_K, mem + (size_t)inst * ens::ensemble_mem_len(M), fin + (size_t)inst * ens::ensemble_fin_len(M, 4),
                                       out + (size_t)inst * EN_OUT);
}
__global__ __launch_bounds__(QNT) void obca_ensemble_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *u, size_t s_u, const double *ts, size_t s_ts,
                                                                 int tstride, const double *aux, size_t s_aux, int S, int M, int feedback, int clamp, trk::Weights w, double need,
                                                                 double *AB, size_t s_AB, double *K, size_t s_K, double *mem, double *fin, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = aux + (size_t)inst * s_aux;
    ens::ensemble_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, u + (size_t)inst * s_u, ts + (size_t)inst * s_ts, tstride, S, M, feedback, clamp, w, a, a + QX * M,
                                need, 0, AB + (size_t)inst * s_AB, K + (size_t)inst * s_K, mem + (size_t)inst * ens::ensemble_mem_len(M), fin + (size_t)inst * ens::ensemble_fin_len(M, QX),
                                out + (size_t)inst * EN_OUT);
}

// one closed-loop step (obca_advance.h): one wavefront per instance; the batch's buffers (the restart rewrites prob and z0; b.d is its scratch), the sub-steps, `aux` (s_aux
// doubles per instance: the kick, for the quadcopter xF_new behind it; has_* 0: none), the two regions of the work buffer, the plant states (nx per instance), the log (s_log
// doubles per instance, this step's rows at `log_at`; NULL: none) and field [15] of the record
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_advance_parking_kernel(int B, int N, int shift, DevBufs b, int S, const double *aux, int has_kick, double need, double *pose, size_t s_pose,
                                                                     double *X, size_t s_X, double *st, double *log, size_t s_log, size_t log_at, double logged, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    adv::advance_parking_instance<VM>(N, shift, b.prob + (size_t)inst * b.s_prob, b.z + (size_t)inst * b.s_z, b.z0 + (size_t)inst * b.s_z, b.d + (size_t)inst * b.s_z, S,
                                      has_kick ? aux + (size_t)inst * 4 : nullptr, need, 0, pose + (size_t)inst * s_pose, X + (size_t)inst * s_X, st + (size_t)inst * 4,
                                      log ? log + (size_t)inst * s_log + log_at : nullptr, logged, out + (size_t)inst * AV_OUT);
}
__global__ __launch_bounds__(QNT) void obca_advance_quad_kernel(int B, int N, int shift, QDevBufs b, int S, const double *aux, int has_kick, int has_xF, double need, double *pose, size_t s_pose,
                                                                double *X, size_t s_X, double *st, double *log, size_t s_log, size_t log_at, double logged, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = aux + (size_t)inst * 2 * QX;
    adv::advance_quad_instance(N, shift, b.prob + (size_t)inst * b.s_prob, b.z + (size_t)inst * b.s_z, b.info + (size_t)inst * 8, S, has_kick ? a : nullptr, has_xF ? a + QX : nullptr,
                               need, 0, pose + (size_t)inst * s_pose, X + (size_t)inst * s_X, st + (size_t)inst * QX, log ? log + (size_t)inst * s_log + log_at : nullptr, logged,
                               out + (size_t)inst * AV_OUT);
}

// the obstacles of the records moved and inflated in place (obca_scene_edit.h): one wavefront per instance; `in`: s_in doubles per instance (SE_PIN per obstacle / SE_QIN per
// box), `out`: the status, one double per instance
__global__ __launch_bounds__(OB_NT) void obca_move_parking_kernel(int B, double *prob, size_t s_prob, const double *in, size_t s_in, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    sed::move_parking_instance(prob + (size_t)inst * s_prob, in + (size_t)inst * s_in, 0, out + inst);
}
__global__ __launch_bounds__(QNT) void obca_move_quad_kernel(int B, double *prob, size_t s_prob, const double *in, double *out) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    sed::move_quad_instance(prob + (size_t)inst * s_prob, in + (size_t)inst * QOB * SE_QIN, 0, out + inst);
}

// clearance against obstacles that move (obca_predict.h): one wavefront per instance; the arguments of the clearance kernels, with `in` holding per instance s_in doubles,
// [ the rates, s_rt doubles (PR_PIN per obstacle / PR_QIN per box) | timeScale (N + 1) of a host-pointer call ], and the profile rows (s_prof doubles each) or nullptr
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_predict_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *in, size_t s_in, size_t s_rt, int has_ts,
                                                                     int S, double need, double *out, double *prof, size_t s_prof) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const double *a = in + (size_t)inst * s_in;
    prd::predict_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, has_ts ? a + s_rt : nullptr, a, S, need, 0, out + (size_t)inst * PR_OUT,
                                      prof ? prof + (size_t)inst * s_prof : nullptr);
}
__global__ __launch_bounds__(QNT) void obca_predict_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *ts, size_t s_ts, int tstride,
                                                                const double *in, size_t s_in, int S, double need, double *out, double *prof, size_t s_prof) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    prd::predict_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, ts + (size_t)inst * s_ts, tstride, in + (size_t)inst * s_in, S, need, 0,
                               out + (size_t)inst * PR_OUT, prof ? prof + (size_t)inst * s_prof : nullptr);
}

// clearance certificate (obca_certify.h): one wavefront per instance; the arguments of the clearance kernels with need, slack and max_steps in place of the sub-steps, then
// the interval array (2 (N + 1) per instance).  The item table is the launch's dynamic LDS: cert::certify_work_len(N, the batch's most obstacles) doubles
template <int VM>
__global__ __launch_bounds__(OB_NT) void obca_certify_parking_kernel(int B, int N, const double *prob, size_t s_prob, const double *z, size_t s_z, const double *ts, double need, double slack, int max_steps,
                                                                     double *iv, double *out) {
    extern __shared__ double cert_work[];
    const int inst = blockIdx.x;
    if (inst >= B) return;
    cert::certify_parking_instance<VM>(N, prob + (size_t)inst * s_prob, z + (size_t)inst * s_z, ts ? ts + (size_t)inst * (N + 1) : nullptr, need, slack, max_steps, 0, cert_work,
                                       iv + (size_t)inst * cert::certify_iv_len(N), out + (size_t)inst * CT_OUT);
}
__global__ __launch_bounds__(QNT) void obca_certify_quad_kernel(int B, int N, const double *prob, size_t s_prob, const double *x, size_t s_x, const double *ts, size_t s_ts, int tstride,
                                                                double need, double slack, int max_steps, double *iv, double *out) {
    extern __shared__ double cert_work[];
    const int inst = blockIdx.x;
    if (inst >= B) return;
    cert::certify_quad_instance(N, prob + (size_t)inst * s_prob, x + (size_t)inst * s_x, ts + (size_t)inst * s_ts, tstride, need, slack, max_steps, 0, cert_work,
                                iv + (size_t)inst * cert::certify_iv_len(N), out + (size_t)inst * CT_OUT);
}

// warm starts from planner paths (obca_path_ws.h): one wavefront per instance.  paths / dirs: B x rows (x 3) dense on the device -- the rows below the longest count of the
// call --, `cap` the rows of the caller's arrays (what a count is checked against).  Host-pointer call: outputs per instance, zeros where the status is negative.
__global__ __launch_bounds__(OB_NT) void obca_path_ws_host_kernel(int B, int N, const double *paths, const int *dirs, const int *counts, int rows, int cap, const double *xF /* 4 x B or NULL */,
                                                                  double v_nom, double L, double a_max, double *Ts, double *xWS, double *uWS, int *status) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    double *ts = Ts + inst, *x = xWS + (size_t)inst * 4 * (N + 1), *u = uWS + (size_t)inst * 2 * N;
    int st = pw::path_ws_count_status(counts[inst], cap);
    if (!st) st = pw::path_ws_instance(N, counts[inst], paths + (size_t)inst * rows * 3, dirs + (size_t)inst * rows, xF ? xF + (size_t)inst * 4 : nullptr, v_nom, L, a_max, ts, x, u);
    if (st) pw::path_ws_zero(N, ts, x, u);
    if (threadIdx.x == 0) status[inst] = st;
}
// resident call: into the problem record and the start iterate of the batch's instances
__global__ __launch_bounds__(OB_NT) void obca_path_ws_batch_kernel(int B, int N, const double *paths, const int *dirs, const int *counts, int rows, int cap, int use_xF, double v_nom, double a_max,
                                                                   DevBufs b, int *status) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const int st = pw::path_ws_record(N, counts[inst], cap, paths + (size_t)inst * rows * 3, dirs + (size_t)inst * rows, use_xF, v_nom, a_max,
                                      b.prob + (size_t)inst * b.s_prob, b.z0 + (size_t)inst * b.s_z, (int)b.s_z);
    if (threadIdx.x == 0) status[inst] = st;
}

// a solved instance on a finer horizon (obca_refine.h): one wavefront per DESTINATION instance.  Resident call: instance sel[j] of the source batch `s` (horizon N: record, last
// iterate, start iterate, info) becomes instance j of the batch `d` (horizon r N: record and start iterate, every word of both)
__global__ __launch_bounds__(OB_NT) void obca_refine_batch_kernel(int n, int N, int r, int duals, const int *sel, DevBufs s, DevBufs d, int *status) {
    const int j = blockIdx.x;
    if (j >= n) return;
    const size_t i = (size_t)sel[j];
    const int st = rfn::refine_record(N, r, duals, s.prob + i * s.s_prob, s.z + i * s.s_z, s.z0 + i * s.s_z, s.info + i * 8, 0, d.prob + (size_t)j * d.s_prob, d.z0 + (size_t)j * d.s_z, (int)d.s_z);
    if (threadIdx.x == 0) status[j] = st;
}
// host-pointer call: dense arrays per instance, ts: (N + 1) per instance or NULL
__global__ __launch_bounds__(OB_NT) void obca_refine_host_kernel(int B, int N, int r, const double *Ts, double L, const double *x, const double *u, const double *ts, double *Tsf, double *xf, double *uf) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const size_t i = inst, Nf = (size_t)N * r;
    (void)rfn::refine_host_instance(N, r, Ts[i], L, x + i * 4 * (N + 1), u + i * 2 * N, ts ? ts + i * (N + 1) : nullptr, 0, Tsf + i, xf + i * 4 * (Nf + 1), uf + i * 2 * Nf);
}

// a solved quadcopter instance on a finer horizon (obca_quad_subdivide.h): one wavefront per DESTINATION instance.  Resident call: instance sel[j] of the source batch `s`
// (horizon N: record, last iterate, info) becomes instance j of the batch `d` (horizon r N: every word of its problem record)
__global__ __launch_bounds__(QNT) void obca_quad_subdivide_batch_kernel(int n, int N, int r, double margin, const int *sel, QDevBufs s, QDevBufs d, int *status) {
    const int j = blockIdx.x;
    if (j >= n) return;
    const size_t i = (size_t)sel[j];
    const int st = qsd::subdivide_record(N, r, margin, s.prob + i * s.s_prob, s.z + i * s.s_z, s.info + i * 8, 0, d.prob + (size_t)j * d.s_prob);
    if (threadIdx.x == 0) status[j] = st;
}
// host-pointer call: dense arrays per instance, ts: (N + 1) per instance or NULL
__global__ __launch_bounds__(QNT) void obca_quad_subdivide_host_kernel(int B, int N, int r, const double *Ts, const double *x, const double *ts, double *Tsf, double *xf) {
    const int inst = blockIdx.x;
    if (inst >= B) return;
    const size_t i = inst;
    (void)qsd::subdivide_host_instance(N, r, Ts[i], x + i * QX * (N + 1), ts ? ts + i * (N + 1) : nullptr, 0, Tsf + i, xf + i * QX * ((size_t)N * r + 1));
}

// rows of a strided device array <-> a dense staging array (one contiguous PCIe transfer per direction instead of a 2-D copy):
//   scatter: dst[i * ds + j] = j < W ? src[i * W + j] : 0   for j < zero_to   (upload: primal prefix of the iterate, rest of the row cleared)
//   gather : dst[i * W + j] = src[i * ss + j]                                   (download: the output prefix of the iterate)
__global__ __launch_bounds__(256) void obca_scatter_rows_kernel(double *dst, size_t ds, const double *src, size_t W, size_t zero_to) {
    const size_t i = blockIdx.x;                     // row (instance) in grid.x: no 65 535 limit on the batch size
    for (size_t j = (size_t)blockIdx.y * blockDim.x + threadIdx.x; j < zero_to; j += (size_t)gridDim.y * blockDim.x)
        dst[i * ds + j] = j < W ? src[i * W + j] : 0.0;
}
__global__ __launch_bounds__(256) void obca_gather_rows_kernel(double *dst, size_t W, const double *src, size_t ss) {
    const size_t i = blockIdx.x;
    for (size_t j = (size_t)blockIdx.y * blockDim.x + threadIdx.x; j < W; j += (size_t)gridDim.y * blockDim.x)
        dst[i * W + j] = src[i * ss + j];
}


// ------------------------------------------------------------------------------------------------ host side
// A context drives one or several devices.  Every device has OBCA_SLOTS worker lanes ("slots": a HIP stream, a cached chunk-sized batch
// with pinned staging buffers); the host-pointer entry points cut a call's batch into chunks and a host thread per slot pulls chunks from a
// shared counter (work queue, SURVEY 8e: solve times are heavy-tailed, a static slice per device would wait for the unluckiest one):
// pack into pinned memory -> H2D -> DualMultWS + interior point -> D2H of the outputs only -> unpack into the caller's arrays.  With several
// slots per device the transfers and the host-side (un)packing of one chunk overlap the solves of the others, and the few hard instances
// at the end of one chunk overlap the bulk of the next.  Instances are independent: no collective touches the data path.
struct obca_batch;
struct obca_quad_batch;
struct Slot { int device; hipStream_t stream; obca_batch *pb; obca_quad_batch *qb; int cus; };

// Device work buffers never carry what a previous owner of the memory left in them:
// every allocation is filled once, on the stream of the batch it belongs to (the
// lanes' streams do not synchronise with the null stream).  The product build clears
// them; -DOBCA_POISON (diagnostic build, tools/determinism_ragged.py) fills them with
// the all-ones NaN pattern instead -- and the kernels then also poison their LDS at entry
// -- so that any read of a value nothing has written yet shows up as NaN in the results.
#if defined(OBCA_POISON) && (!defined(OBCA_POISON_PARTS) || (OBCA_POISON_PARTS & 1))
#define OBCA_FILL_BYTE 0xFF
#else
#define OBCA_FILL_BYTE 0
#endif
static hipError_t dev_alloc(void **p, size_t bytes, hipStream_t stream) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    return hipMemsetAsync(*p, OBCA_FILL_BYTE, bytes, stream);
}

// Staging memory that only grows: `cap` doubles at `p` (read like the plain pointer); reserve() keeps a block that is large enough, else frees it
// and allocates `need` doubles (the contents are not carried over); release() frees.  PinnedBuf: page-locked host memory; DevBuf: device memory from dev_alloc.
namespace {      // (their member functions are no symbols of the library)
struct PinnedBuf {
    double *p = nullptr; size_t cap = 0;
    operator double *() const { return p; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    int reserve(std::string &err, size_t need) {
        if (cap >= need) return 0;
        release();
        if (hipHostMalloc((void **)&p, need * sizeof(double), hipHostMallocDefault) != hipSuccess) { err = "hipHostMalloc failed"; return -2; }
        cap = need;
        return 0;
    }
};
struct DevBuf {
    double *p = nullptr; size_t cap = 0;
    operator double *() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t need, hipStream_t stream) {
        if (cap >= need) return hipSuccess;
        release();
        const hipError_t e = dev_alloc((void **)&p, need * sizeof(double), stream);
        if (e == hipSuccess) cap = need;
        return e;
    }
};
// two events around a kernel, created by the first ensure(); `timed`: an interval has been recorded between them, elapsed() refuses before
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr; int have = 0, timed = 0;
    int ensure(std::string &err) {
        if (have) return 0;
        if (hipEventCreate(&e0) != hipSuccess) { err = "hipEventCreate failed"; return -2; }
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); err = "hipEventCreate failed"; return -2; }
        have = 1;
        return 0;
    }
    hipError_t begin(hipStream_t stream) { return hipEventRecord(e0, stream); }
    hipError_t end(hipStream_t stream) { return hipEventRecord(e1, stream); }
    bool elapsed(float *ms) const { return timed && hipEventElapsedTime(ms, e0, e1) == hipSuccess; }
    void release() { if (have) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); } have = timed = 0; }
};
// staging of one kernel call (path warm start, refine, subdivide): a device block, its pinned mirror, the events around the kernel.  Allocates nothing until first used.
struct KernelStage {
    DevBuf dev; PinnedBuf host; EventPair ev;
    void release() { dev.release(); host.release(); ev.release(); }
};
// the planner (obca_hybrid.h): the configuration, the slots' memory (kept while the next call fits it), the staging block of a call; per entry point (shared field, per-instance
// fields) the events around the kernel and the LDS attribute its instantiation has been given
struct HybridBufs {
    int slots = 0, max_nodes = 0, max_chunks = 0;      // as configured (0 = default)
    char *slotmem = nullptr; size_t slot_bytes = 0; int nslots = 0, ncell = 0, nodes = 0, chunks = 0;
    char *io = nullptr; size_t io_bytes = 0;
    EventPair ev[2]; int lds_set[2] = {0, 0};      // [0]: obca_hybrid_astar_batch, [1]: obca_scene_astar_batch (obca_batch_plan_warm_start launches [1]'s kernel between events of its batch)
    unsigned long long serial = 0;                 // counts the calls that have taken the staging block: what a call left in it is there while the number stands
    int slot_allocs = 0, io_allocs = 0;            // how often the slots / the staging block have been allocated (obca_batch_packed_block reports them: a call that fits reuses both)
    void release() {
        if (slotmem) (void)hipFree(slotmem);
        if (io) (void)hipFree(io);
        ev[0].release(); ev[1].release();
        slotmem = io = nullptr; slot_bytes = io_bytes = 0; nslots = 0; serial++;
    }
};
// obca_batch_plan_warm_start on a batch (include/obca_plan_resident.h): the events around its three kernels -- packing, search, warm start -- and where the call left its
// instance records and paths in the planner's staging block (`serial`: HybridBufs' when the call took the block; 0: no call yet)
struct PlanRun {
    EventPair ev[3]; unsigned long long serial = 0; int cap = 0, B = 0, nObMax = 0, MMax = 0; size_t o_inst = 0, o_paths = 0, o_dirs = 0;      // nObMax, MMax: the strides of the packed block at o_inst
    void release() { for (EventPair &e : ev) e.release(); serial = 0; }
};
}  // namespace

struct obca_ctx {
    int device; hipStream_t stream;         // primary device / stream (= slots[0]): the device-resident obca_batch_* API runs here
    std::vector<int> devices; std::vector<Slot> slots;
    std::string err; std::string name; int cus;
    KernelStage pw;                         // staging of obca_parking_path_warm_start_batch (primary device)
    KernelStage rf;                         // the same set for obca_parking_refine_batch
    KernelStage qsd;                        // and for obca_quadcopter_subdivide_batch
    HybridBufs hyb;                         // the planner's slots and staging (obca_hybrid_astar_batch, obca_scene_astar_batch) and its configuration (obca_hybrid_configure)
    int gp_lds = 0;                         // the dynamic LDS obca_quad_plan_resident_kernel has been given on the primary device (obca_quad_batch_grid_plan_warm_start)
};
static std::string g_create_err;

// buffers of the validate calls of a batch: device input (row lengths; a host-pointer call's trajectory extras) and output, their pinned mirrors, the events around the kernel
struct ValBufs { DevBuf d_in, d_out; PinnedBuf h_in, h_out; EventPair ev; };
// what a parking and a quadcopter batch have in common
struct BatchCore {
    obca_ctx *ctx; int device; hipStream_t stream; std::string err;
    int B, cap, N;
    int uploaded = 0;
    int solved = 0;      // a solve has been queued since the last upload / shift: d.z holds a solution the validate entry points may check
    long long bytes = 0;
    DevBuf stage;                                           // dense device staging of the PCIe transfers
    PinnedBuf h_prob, h_info;                               // pinned host staging
    hipEvent_t e0 = nullptr, e1 = nullptr;                  // around the kernels of the last solve
    ValBufs val;
    ValBufs clr;                                            // the same set for the clearance calls (obca_clearance.h): a clearance call leaves validate's row lengths and events alone
    ValBufs rol;                                            // ... and for the rollout calls (obca_rollout.h)
    DevBuf rol_w;                                           // their work buffer: [ sample poses 3 x (N S + 1) | node states nx x (N + 1) ] x B, allocated by the first call, grown on demand
    int rol_B = 0, rol_N = 0, rol_S = 0;                    // the instances, horizon and sub-steps of the last rollout (0: none yet): where its node states lie in rol_w
    ValBufs trk;                                            // ... and for the track calls (obca_track.h), with a work buffer of their own: a rollout's node states stay valid
    DevBuf trk_w, trk_K;                                    // [ [A|B] N nx (nx + nu) + applied inputs N nu | sample poses | node states ] x B; the gains N nu nx x B
    int trk_B = 0, trk_N = 0, trk_S = 0;                    // as rol_B, rol_N, rol_S
    ValBufs ens;                                            // ... and for the ensemble calls (obca_ensemble.h), again with buffers of their own
    DevBuf ens_w, ens_K, ens_mem, ens_fin;                  // [A|B] N nx (nx + nu) x B; the gains; the member records M x EN_MEM x B; the final states M x nx x B
    int ens_B = 0, ens_N = 0, ens_M = 0;                    // the instances, horizon and members of the last ensemble call (0: none yet)
    ValBufs adv;                                            // ... and for the advance calls (obca_advance.h): a previous rollout's states stay valid
    DevBuf adv_w, adv_st, adv_log;                          // [ sample poses 3 x (shift S + 1) | node states nx x (shift + 1) ] x B; the plant states nx x B; the log B x adv_cap x nx
    int adv_B = 0, adv_N = 0;                               // the instances and horizon of the last advance (0: none yet): adv_st holds its plant states
    int adv_cap = 0, adv_n = 0;                             // the log's rows per instance (0: no log) and the nodes in it
    ValBufs mov;                                            // ... and for the move calls (obca_scene_edit.h): the motions go up, a status per instance comes down
    ValBufs cer;                                            // ... and for the certify calls (obca_certify.h)
    DevBuf cer_iv;                                          // their interval arrays, 2 (N + 1) x B
    int cer_B = 0, cer_N = 0;                               // the instances and horizon of the last certify call (0: none yet)
    ValBufs prd;                                            // ... and for the predict calls (obca_predict.h): the rates go up in a buffer set of the call's own, PR_OUT doubles per instance come down
    DevBuf prd_w;                                           // their profile, (N S + 1) x B: allocated by the first call that keeps one, sized for that call, grown on demand
    int prd_B = 0, prd_N = 0, prd_S = 0;                    // the instances, horizon and sub-steps of the last call that kept a profile (0: none yet)
    BatchCore(obca_ctx *c, int dev, hipStream_t s, int B_, int N_) : ctx(c), device(dev), stream(s), B(B_), cap(B_), N(N_) {}
};
struct obca_quad_batch : BatchCore {
    using BatchCore::BatchCore;
    QDevBufs d = {};
    PinnedBuf h_z;
    KernelStage sd;       // obca_quad_batch_subdivide_into, this batch the destination: selection and status on the device, the events around the kernel
    KernelStage gp;       // obca_quad_batch_grid_plan_warm_start: selection, counts and sweeps on the device, the events around the kernel
    DevBuf gp_paths; int gp_cap = 0;      // ... and its way-points, B x gp_cap x 3, allocated at the first call and kept with the batch (gp_cap: the last call's cap, 0 before)
};
struct obca_batch : BatchCore {
    using BatchCore::BatchCore;
    int nObMax = 0, MMax = 0, zlen = 0, have_duals = 0, dist = 0, vmax = 0;   // vmax: most rows of one obstacle in the uploaded instances
    DevBufs d = {};
    PinnedBuf h_zin, h_zout;
    std::vector<int> nOb, M, obOff, rowOff;                 // per instance; offsets into the caller's packed obstacle arrays
    // |a_r| of every half-space row of the uploaded instances (index: row offset - rowOff[0]), see batch_upload_range
    std::vector<double> rowLen;
    int fixTime = 0;
    hipEvent_t e2 = nullptr;      // e0 .. e1: DualMultWS, e1 .. e2: interior point
    int sliced = 0;      // slice length (passes) of the last solve if it used the two-launch schedule, else 0
    int val_rl = 0;      // the row lengths of the uploaded instances are in val.d_in (resident validate)
    KernelStage pw;       // obca_batch_set_path_warm_start
    KernelStage rf;       // obca_batch_refine_into, this batch the destination: selection and status on the device, the events around the kernel
    std::vector<int> vmx;                                   // per instance: most rows of one of its obstacles (a refined selection takes its own row class along)
    // ego, L and XYbounds as obca_batch_upload was given them (the record holds what the solve derives from them): the planner's parameter block is made from these
    // (obca_batch_plan_warm_start).  have_geo: an upload has set them -- a batch that obca_batch_refine_into filled has none
    double ego[4] = {0, 0, 0, 0}, XYb[4] = {0, 0, 0, 0}, L = 0; int have_geo = 0;
    PlanRun plan;         // obca_batch_plan_warm_start
};

#define HIPCHK(bt, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (bt)->err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } } while (0)
// The device index of a context / batch was validated when the context was created (obca_create: hipSetDevice checked there); later calls only select it again,
// and whatever they then launch or copy reports its own error.  Release paths ignore the status of hipFree & co. on purpose -- `(void)` says so at each site
// (the library builds with -Wall -Wextra -Werror: an ignored status is a compile error).
static inline void use_device(int device) { (void)hipSetDevice(device); }
static inline int fin(BatchCore *bt, int rc) { if (rc) bt->ctx->err = bt->err; return rc; }

// the bodies of the obca_batch_* / obca_quad_batch_* entry points that differ in nothing but the text of their error (`what`)
static int core_sync(BatchCore *bt, const char *what) {
    if (!bt) return -1;
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess) { bt->ctx->err = what; return -2; }
    return 0;
}
// every *_ms entry point of an event pair: refuses with `what` until the pair has timed a call
static int core_elapsed_ms(obca_ctx *ctx, const EventPair &ev, float *ms, const char *what) {
    if (!ev.elapsed(ms)) { ctx->err = what; return -2; }
    return 0;
}
static int core_scratch_bytes(const BatchCore *bt, long long *bytes) { if (!bt || !bytes) return -1; *bytes = bt->bytes; return 0; }
#ifdef OBCA_PROFILE      /* the per-phase clocks exist in the profiling build only (libobca_hip_prof.so, tools/phase_profile.py): not an entry point of the product */
static int core_phase_cycles(BatchCore *bt, const double *prof, double *out /* B x 16 */, const char *what) {
    if (!out) return -1;
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess || hipMemcpy(out, prof, (size_t)bt->B * 16 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { bt->ctx->err = what; return -2; }
    return 0;
}
#endif
// everything of the core that a batch's destroy releases, except `stage` (it goes with the family's device buffers); the batch's device is selected
static void core_release(BatchCore *bt) {
    bt->rol_w.release(); bt->trk_w.release(); bt->trk_K.release();
    bt->ens_w.release(); bt->ens_K.release(); bt->ens_mem.release(); bt->ens_fin.release(); bt->cer_iv.release(); bt->prd_w.release();
    bt->adv_w.release(); bt->adv_st.release(); bt->adv_log.release();
    for (ValBufs *pv : {&bt->val, &bt->clr, &bt->rol, &bt->trk, &bt->ens, &bt->cer, &bt->adv, &bt->mov, &bt->prd}) {
        ValBufs &v = *pv;
        v.d_in.release(); v.d_out.release(); v.h_in.release(); v.h_out.release(); v.ev.release();
    }
    bt->h_prob.release(); bt->h_info.release();
    (void)hipEventDestroy(bt->e0); (void)hipEventDestroy(bt->e1);
}

extern "C" {

int obca_default_opts(obca_opts *o) {
    if (!o) return -1;
    o->tol = 1e-5; o->max_iter = 200;                 /* ParkingSignedDist.jl:42 */
    o->mu_init = 0.1; o->kappa_eps = 10; o->kappa_mu = 0.2; o->theta_mu = 1.5; o->tau_min = 0.99;
    o->bound_push = 1e-2; o->bound_frac = 1e-2;
    o->dw_min = 1e-12;                                 /* min_hessian_perturbation, :43 */
    o->dw0 = 1e-4; o->dw_max = 1e40; o->kw_inc0 = 100; o->kw_inc = 8; o->kw_dec = 1.0 / 3;
    o->dc_bar = 1e-7;                                  /* jacobian_regularization_value, :43 */
    o->kappa_c = 0.25;
    o->gamma_theta = 1e-5; o->gamma_phi = 1e-8; o->delta = 1; o->s_theta = 1.1; o->s_phi = 2.3;
    o->eta_phi = 1e-8; o->gamma_alpha = 0.05; o->s_max = 100; o->kappa_sigma = 1e10;
    o->constr_viol_tol = 1e-4; o->dual_inf_tol = 1; o->compl_inf_tol = 1e-4; o->rho_term = 1e3;
    o->max_soc = 0; o->recalc_y = 0; o->lsq_init = 0; o->obj_scaling = 0; o->restoration = 0;
                     /* throughput defaults: the three IPOPT switches off (obca_reference_opts switches them on; obca_hip.h has the numbers behind the choice) */
    return 0;
}

int obca_reference_opts(obca_opts *o) {            /* the reference's IPOPT configuration as far as the kernels carry it */
    if (obca_default_opts(o)) return -1;
    o->max_soc = 4;                                    /* IPOPT default max_soc */
    o->recalc_y = 1;                                   /* recalc_y = "yes", ParkingSignedDist.jl:41 / ParkingDist.jl:41 */
    o->lsq_init = 1;                                   /* IPOPT default: least-squares initial multipliers, constr_mult_init_max = 1e3 */
    o->restoration = 1;                                /* IPOPT has a restoration phase; the kernels carry a block feasibility restoration in its place (obca_hip.h) */
    return 0;
}

int obca_visible_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

/* devices == NULL or ndev <= 0: every visible device */
int obca_create_multi(obca_ctx **out, const int *devices, int ndev) {
    if (!out) return -1;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_create_err = "no HIP device available (libobca_hip has no CPU fallback)"; return -2; }
    std::vector<int> devs;
    if (!devices || ndev <= 0) { for (int i = 0; i < n; i++) devs.push_back(i); }
    else devs.assign(devices, devices + ndev);
    int nslot = 8;                                       // worker lanes per device (OBCA_SLOTS; 4 until round 6: with 16 hardware queues 8 lanes give +2.6 % on the host-pointer call)
    if (const char *ev = getenv("OBCA_SLOTS")) { nslot = atoi(ev); if (nslot < 1) nslot = 1; if (nslot > 16) nslot = 16; }
    // every device is validated before anything is created, so that a bad index cannot leave a half-built context (or a leaked stream) behind
    std::vector<hipDeviceProp_t> props(devs.size());
    for (size_t di = 0; di < devs.size(); di++) {
        const int dv = devs[di];
        if (dv < 0 || dv >= n) { g_create_err = "device index out of range"; return -1; }
        if (hipGetDeviceProperties(&props[di], dv) != hipSuccess) { g_create_err = "hipGetDeviceProperties failed"; return -2; }
        if (std::string(props[di].gcnArchName).find("gfx950") == std::string::npos) {
            g_create_err = std::string("device is ") + props[di].gcnArchName + ", libobca_hip is built for gfx950 only"; return -2;
        }
    }
    obca_ctx *c = new obca_ctx();
    c->devices = devs;
    c->name = std::string(props[0].name) + " (" + props[0].gcnArchName + ")"; c->cus = props[0].multiProcessorCount;
    for (int s = 0; s < nslot; s++) for (size_t di = 0; di < devs.size(); di++) {       // slot order interleaves the devices
        Slot sl; sl.device = devs[di]; sl.pb = nullptr; sl.qb = nullptr; sl.cus = props[di].multiProcessorCount; sl.stream = nullptr;
        // Non-blocking: the streams never synchronise implicitly with the legacy default stream, which other libraries in the process may use.
        // Only the primary lane gets its stream now; the others are created when a call first needs them: HIP spreads streams over a handful of
        // hardware queues in creation order, and a process that keeps several single-lane contexts busy at once (bench.py) would otherwise find
        // its four primary streams on ONE queue, serialised (measured: 103 k instead of 132 k solves/s).
        if (s == 0 && di == 0 && (hipSetDevice(sl.device) != hipSuccess || hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess)) {
            g_create_err = "hipStreamCreate failed"; delete c; return -2;
        }
        c->slots.push_back(sl);
    }
    c->device = c->slots[0].device; c->stream = c->slots[0].stream;
    use_device(c->device);
    *out = c;
    return 0;
}
int obca_create(obca_ctx **out, int device) { return obca_create_multi(out, &device, 1); }
int obca_device_count(const obca_ctx *c) { return c ? (int)c->devices.size() : -1; }
int obca_batch_destroy(obca_batch *bt);
int obca_quad_batch_destroy(obca_quad_batch *bt);
int obca_destroy(obca_ctx *c) {
    if (!c) return -1;
    for (auto &s : c->slots) {
        if (s.pb) obca_batch_destroy(s.pb);
        if (s.qb) obca_quad_batch_destroy(s.qb);
        if (s.stream) { use_device(s.device); (void)hipStreamDestroy(s.stream); }
    }
    use_device(c->device);
    c->pw.release(); c->rf.release(); c->qsd.release(); c->hyb.release();
    delete c; return 0;
}
const char *obca_last_error(const obca_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }
int obca_device_name(const obca_ctx *c, char *buf, int n) { if (!c || !buf || n <= 0) return -1; snprintf(buf, n, "%s", c->name.c_str()); return 0; }

}  // extern "C"

static int batch_create_on(obca_ctx *ctx, int device, hipStream_t stream, int B, int N, obca_batch **out, std::string &err) {
    if (B < 1 || N < 0 || N > OBCA_NMAX) { err = "obca_batch_create: need B>=1, 0<=N<=OBCA_NMAX"; return -1; }
    obca_batch *bt = new obca_batch(ctx, device, stream, B, N);
    use_device(device);
    if (hipEventCreate(&bt->e0) != hipSuccess || hipEventCreate(&bt->e1) != hipSuccess || hipEventCreate(&bt->e2) != hipSuccess) { err = "hipEventCreate failed"; delete bt; return -2; }
    *out = bt;
    return 0;
}
static void free_dev(obca_batch *bt) {
    double **ps[] = {&bt->d.prob, &bt->d.z0, &bt->d.z, &bt->d.zn, &bt->d.d, &bt->d.as, &bt->d.rs, &bt->d.oc, &bt->d.info, &bt->d.dws, &bt->d.prof, &bt->d.slice, &bt->d.csoc};
    for (auto p : ps) { if (*p) (void)hipFree(*p); *p = nullptr; }
    if (bt->d.order) (void)hipFree(bt->d.order); bt->d.order = nullptr;
    bt->stage.release();
}

// everything a parking call hands over (host pointers of the whole call; a chunk is instances lo .. lo+n-1 of it)
struct ParkIn {
    const double *Ts; double L; const double *ego, *XYb; int fixTime;
    const double *x0, *xF; const int *nOb, *vOb; const double *A, *b, *rx, *ry, *ryaw, *xWS, *uWS, *lWS, *nWS;
    std::vector<int> obOff, rowOff;                    // running sums over the call's instances
};
struct ParkOut { double *xp, *up, *ts; int *exitflag; double *lp, *np, *slp, *info; double *lWS, *nWS, *dd; };

static int park_prefix(std::string &err, int B, const int *nOb, const int *vOb, ParkIn &in) {
    in.obOff.assign(B + 1, 0); in.rowOff.assign(B + 1, 0);
    for (int i = 0; i < B; i++) {
        const int n = nOb[i];
        if (n < 1 || n > OBCA_NOBMAX) { err = "nOb out of range 1..OBCA_NOBMAX"; return -1; }
        int m = 0;
        for (int j = 0; j < n; j++) { const int v = vOb[in.obOff[i] + j]; if (v < 1 || v > OBCA_VMAX) { err = "vOb out of range 1..OBCA_VMAX"; return -1; } m += v; }
        if (m > OBCA_MMAX) { err = "more than OBCA_MMAX half-space rows in one instance"; return -1; }
        in.obOff[i + 1] = in.obOff[i] + n; in.rowOff[i + 1] = in.rowOff[i] + m;
    }
    return 0;
}

// device buffers of the batch for instances of up to nObMax obstacles and MMax rows (a cached batch keeps the largest shape it has seen); the batch's device is selected
static int batch_reserve_shape(obca_batch *bt, int nObMax, int MMax) {
    const int N = bt->N, N1 = N + 1;
    const size_t B = bt->cap;
    if (!bt->uploaded || nObMax > bt->nObMax || MMax > bt->MMax) {       // (a cached batch keeps the largest shape it has seen)
        // (re)allocation: the batch counts as empty until every buffer exists -- a failed hipMalloc must leave a state the next call can recover from,
        // not a batch that still claims to be uploaded with null device pointers
        free_dev(bt);
        bt->uploaded = 0; bt->bytes = 0;
        bt->nObMax = std::max(nObMax, bt->nObMax); bt->MMax = std::max(MMax, bt->MMax);
        Lay lmax; make_layout(N, bt->nObMax, bt->MMax, lmax);
        bt->zlen = lmax.len;
        DevBufs &d = bt->d;
        d.s_prob = OB_HDR + 3 * (size_t)N1; d.s_z = lmax.len; d.s_as = (size_t)N1 * OB_AS; d.s_rs = (size_t)N1 * OB_RS;
        d.s_oc = (size_t)N1 * bt->nObMax * OB_OC; d.o_csoc = (size_t)lmax.zxL; d.s_csoc = d.o_csoc + (size_t)(lmax.zxL - lmax.pi);
        size_t tot = 0;
#define ALLOC(ptr, cnt) do { size_t by_ = (size_t)(cnt) * sizeof(double); hipError_t e_ = dev_alloc((void **)&(ptr), by_, bt->stream); if (e_ != hipSuccess) { bt->err = std::string("hipMalloc(" #ptr "): ") + hipGetErrorString(e_); free_dev(bt); return -2; } tot += by_; } while (0)
        ALLOC(d.prob, B * d.s_prob); ALLOC(d.z0, B * d.s_z); ALLOC(d.z, B * d.s_z); ALLOC(d.zn, B * d.s_z); ALLOC(d.d, B * d.s_z);
        ALLOC(d.as, B * d.s_as); ALLOC(d.rs, B * d.s_rs);      // (d.oc stays null: the condensed obstacle sums of the parking kernel live in LDS since round 4)
        ALLOC(d.info, B * 8); ALLOC(d.dws, B * N1 * bt->nObMax); ALLOC(d.prof, B * 16);
        ALLOC(d.slice, B * SL_SIZE);
        ALLOC(d.csoc, B * d.s_csoc);      // (rows + direction of a second-order correction: with the other buffers since round 6 -- allocated by the first solve that asked for corrections, it put a 60 MB hipMalloc into that solve: profiles/r06_first_solve_costs.txt)
        if (hipError_t e_ = bt->stage.reserve(B * (size_t)lmax.nprimal, bt->stream)) { bt->err = std::string("hipMalloc(bt->stage): ") + hipGetErrorString(e_); free_dev(bt); return -2; }
        tot += bt->stage.cap * sizeof(double);                           // nprimal >= the output prefix
        if (dev_alloc((void **)&d.order, (B + 1) * sizeof(int), bt->stream) != hipSuccess) { bt->err = "hipMalloc(order) failed"; free_dev(bt); return -2; }
        tot += (B + 1) * sizeof(int);
#undef ALLOC
        bt->bytes = (long long)tot;
    }
    return 0;
}

// instances lo .. lo+n-1 of the call become instances 0 .. n-1 of the batch (n <= capacity)
static int batch_upload_range(obca_batch *bt, const ParkIn &in, int lo, int n) {
    const int N = bt->N, N1 = N + 1;
    if (n < 1 || n > bt->cap) { bt->err = "obca_batch_upload: more instances than the batch was created for"; return -1; }
    bt->B = n; bt->solved = 0; bt->val_rl = 0; bt->adv_n = 0;      // (an upload empties the log of obca_advance.h)
    bt->nOb.assign(n, 0); bt->M.assign(n, 0); bt->obOff.assign(n + 1, 0); bt->rowOff.assign(n + 1, 0); bt->vmx.assign(n, 0);
    int nObMax = 0, MMax = 0; bt->vmax = 0;
    for (int i = 0; i < n; i++) {
        const int g = lo + i;
        for (int j = in.obOff[g]; j < in.obOff[g + 1]; j++) bt->vmx[i] = std::max(bt->vmx[i], in.vOb[j]);
        bt->vmax = std::max(bt->vmax, bt->vmx[i]);
        bt->nOb[i] = in.obOff[g + 1] - in.obOff[g]; bt->M[i] = in.rowOff[g + 1] - in.rowOff[g];
        bt->obOff[i] = in.obOff[g]; bt->rowOff[i] = in.rowOff[g];
        nObMax = std::max(nObMax, bt->nOb[i]); MMax = std::max(MMax, bt->M[i]);
    }
    bt->obOff[n] = in.obOff[lo + n]; bt->rowOff[n] = in.rowOff[lo + n];
    bt->rowLen.assign((size_t)(bt->rowOff[n] - bt->rowOff[0]), 1.0);
    use_device(bt->device);
    const size_t B = bt->cap;
    if (int rc = batch_reserve_shape(bt, nObMax, MMax)) return rc;
    const DevBufs &d = bt->d;
    Lay lmax; make_layout(N, bt->nObMax, bt->MMax, lmax);
    const bool duals = in.lWS && in.nWS;
    // only what the caller provides travels over PCIe: x, u, t (the same offsets in every instance's layout) and, with a dual warm start, lam and mu;
    // the scatter kernel clears the rest of each row
    const size_t W = duals ? (size_t)lmax.sl : (size_t)lmax.lam;
    if (bt->h_prob.reserve(bt->err, B * d.s_prob) || bt->h_zin.reserve(bt->err, B * W)) return -2;
    const double *ego = in.ego, *XYb = in.XYb;
    const double W_ev = ego[1] + ego[3], L_ev = ego[0] + ego[2];     /* ParkingSignedDist.jl:182-188 */
    for (int i = 0; i < n; i++) {
        const int g = lo + i;
        double *p = bt->h_prob + (size_t)i * d.s_prob;
        memset(p, 0, sizeof(double) * OB_HDR);
        const int no = bt->nOb[i], m = bt->M[i];
        p[PH_TS] = in.Ts[g]; p[PH_L] = in.L; p[PH_DIST] = bt->dist ? 1.0 : 0.0;
        p[PH_G] = L_ev / 2; p[PH_G + 1] = W_ev / 2; p[PH_G + 2] = L_ev / 2; p[PH_G + 3] = W_ev / 2;
        p[PH_OFF] = (ego[0] + ego[2]) / 2 - ego[2];
        p[PH_XL] = XYb[0]; p[PH_XL + 1] = XYb[2]; p[PH_XL + 2] = -1e300; p[PH_XL + 3] = -1.0;     /* :104-106 */
        p[PH_XU] = XYb[1]; p[PH_XU + 1] = XYb[3]; p[PH_XU + 2] = 1e300; p[PH_XU + 3] = 2.0;
        for (int q = 0; q < 4; q++) { p[PH_X0 + q] = in.x0 ? in.x0[4 * (size_t)g + q] : 0.0; p[PH_XF + q] = in.xF ? in.xF[4 * (size_t)g + q] : 0.0; }
        p[PH_FIX] = in.fixTime ? 1 : 0; p[PH_NOB] = no; p[PH_M] = m;
        int ro = 0;
        for (int j = 0; j < no; j++) { const int v = in.vOb[bt->obOff[i] + j]; p[PH_VOB + j] = v; p[PH_ROFF + j] = ro; ro += v; }
        p[PH_ROFF + no] = ro;
        const size_t r0 = bt->rowOff[i];
        // The solve runs on unit-length half-space rows a_r / |a_r|, b_r / |a_r| (the
        // same obstacle; lambda_r scales with |a_r|, A'lam and b'lam do not change) and
        // hands lambda back in the caller's scaling.  obstHrep.jl:57-86 leaves the rows of a sloped edge unnormalised ([-s 1]: |a| up to 1e3 for a steep edge);
        // IPOPT's default gradient-based NLP scaling stands between such rows and the
        // reference's solves.  Without either 1.2-1.9 % of the config-5 instances -- all of
        // them with a row of |a| > 100 -- failed and the iteration counts had a tail up
        // to 400; with unit rows all solve in at most 80.  The
        // reference's own scenarios have rows of length 1: nothing changes for them, bit for bit.
        double *rl = bt->rowLen.data() + (r0 - (size_t)bt->rowOff[0]);
        for (int r = 0; r < m; r++) {
            const double a1 = in.A[2 * (r0 + r)], a2 = in.A[2 * (r0 + r) + 1]; double nr = hypot(a1, a2);
            if (!(nr > 0)) nr = 1.0;
            rl[r] = nr; p[PH_A + 2 * r] = a1 / nr; p[PH_A + 2 * r + 1] = a2 / nr; p[PH_B + r] = in.b[r0 + r] / nr;
        }
        memcpy(p + OB_HDR, in.rx + (size_t)g * N1, sizeof(double) * N1);
        memcpy(p + OB_HDR + N1, in.ry + (size_t)g * N1, sizeof(double) * N1);
        memcpy(p + OB_HDR + 2 * N1, in.ryaw + (size_t)g * N1, sizeof(double) * N1);
        Lay l; make_layout(N, no, m, l);
        double *z = bt->h_zin + (size_t)i * W;
        if (in.xWS) memcpy(z + l.x, in.xWS + (size_t)g * 4 * N1, sizeof(double) * 4 * N1); else memset(z + l.x, 0, sizeof(double) * 4 * N1);
        if (in.uWS) memcpy(z + l.u, in.uWS + (size_t)g * 2 * N, sizeof(double) * 2 * N); else memset(z + l.u, 0, sizeof(double) * 2 * N);
        z[l.t] = 1.0;                                                 /* ParkingSignedDist.jl:214 */
        if (duals) {
            // caller's row scaling -> unit rows
            for (int k = 0; k < N1; k++) for (int r = 0; r < m; r++) z[l.lam + k * m + r] = in.lWS[r0 * N1 + (size_t)k * m + r] * rl[r];
            memcpy(z + l.mu, in.nWS + (size_t)bt->obOff[i] * 4 * N1, sizeof(double) * 4 * no * N1);
            if ((size_t)l.sl < W) memset(z + l.sl, 0, sizeof(double) * (W - l.sl));      // a smaller instance's layout ends before the widest one's
        }
    }
    bt->have_duals = duals ? 1 : 0; bt->fixTime = in.fixTime ? 1 : 0;
    for (int q = 0; q < 4; q++) { bt->ego[q] = ego[q]; bt->XYb[q] = XYb[q]; }
    bt->L = in.L; bt->have_geo = 1;
    HIPCHK(bt, hipMemcpyAsync(d.prob, bt->h_prob, (size_t)n * d.s_prob * sizeof(double), hipMemcpyHostToDevice, bt->stream));
    HIPCHK(bt, hipMemcpyAsync(bt->stage, bt->h_zin, (size_t)n * W * sizeof(double), hipMemcpyHostToDevice, bt->stream));
    hipLaunchKernelGGL(obca_scatter_rows_kernel, dim3(n, (unsigned)((d.s_z + 1023) / 1024)), dim3(256), 0, bt->stream, d.z0, d.s_z, (const double *)bt->stage, W, d.s_z);
    HIPCHK(bt, hipGetLastError());
    bt->uploaded = 1;
    return 0;
}

static int launch_dualws(obca_batch *bt, double *zdst) {
    long long tot = (long long)bt->B * (bt->N + 1) * bt->nObMax;
    int blocks = (int)((tot + 255) / 256);
    // (the sub-problem is sized by the template: the reference's scenarios have <= 2 rows per obstacle)
    if (bt->vmax <= 2) hipLaunchKernelGGL(obca_dualws_kernel<2>, dim3(blocks), dim3(256), 0, bt->stream, bt->B, bt->N, bt->nObMax, bt->d, zdst, bt->d.s_z);
    else if (bt->vmax <= OB_VMID) hipLaunchKernelGGL(obca_dualws_kernel<OB_VMID>, dim3(blocks), dim3(256), 0, bt->stream, bt->B, bt->N, bt->nObMax, bt->d, zdst, bt->d.s_z);
    else hipLaunchKernelGGL(obca_dualws_kernel<OB_VMAX>, dim3(blocks), dim3(256), 0, bt->stream, bt->B, bt->N, bt->nObMax, bt->d, zdst, bt->d.s_z);
    HIPCHK(bt, hipGetLastError());
    return 0;
}

// asynchronous on the batch's stream: warm start -> (DualMultWS) -> interior point; dualws_only: stop after DualMultWS
static int batch_solve(obca_batch *bt, const obca_opts *opts, int dualws_only) {
    if (!bt->uploaded) { bt->err = "obca_batch_solve: nothing uploaded"; return -1; }
    if (!dualws_only && bt->N < 2) { bt->err = "obca_batch_solve: the NLP needs a horizon N>=2"; return -1; }
    obca_opts o; if (opts) o = *opts; else obca_default_opts(&o);
    Opts ko; memcpy(&ko, &o, sizeof ko);
    use_device(bt->device);
    if (o.max_soc < 0 || o.max_soc > 16) { bt->err = "opts.max_soc must be in 0 .. 16"; return -1; }
    if (o.restoration < 0 || o.restoration > 2) { bt->err = "opts.restoration must be 0, 1 or 2"; return -1; }
    // IPOPT's objective scaling is 1 on the parking NLP only at the reference's own start
    // (gradient = the slack penalty 1e2); a caller's start with a larger gradient would
    // be scaled by IPOPT and is not by these kernels: the switch is refused here rather
    // than silently ignored (the quadcopter entry points refuse recalc_y the same way)
    if (o.obj_scaling != 0) { bt->err = "opts.obj_scaling is carried by the quadcopter kernel only (obca_quadcopter_reference_opts); the parking entry points take 0"; return -1; }
    if (o.max_soc > 0 && !bt->d.csoc) {      // the second-order correction keeps its right-hand-side rows per instance
        hipError_t e_ = dev_alloc((void **)&bt->d.csoc, (size_t)bt->cap * bt->d.s_csoc * sizeof(double), bt->stream);
        if (e_ != hipSuccess) { bt->d.csoc = nullptr; bt->err = std::string("hipMalloc(csoc): ") + hipGetErrorString(e_); return -2; }
        bt->bytes += (long long)((size_t)bt->cap * bt->d.s_csoc * sizeof(double));
    }
    const DevBufs &d = bt->d;
    // a solve starts from the uploaded iterate: reset z <- z0 (device-to-device), DualMultWS writes its multipliers into z
    HIPCHK(bt, hipMemcpyAsync(d.z, d.z0, (size_t)bt->B * d.s_z * sizeof(double), hipMemcpyDeviceToDevice, bt->stream));
    HIPCHK(bt, hipEventRecord(bt->e0, bt->stream));
    if (!bt->have_duals || dualws_only) { int rc = launch_dualws(bt, d.z); if (rc) return rc; }
    HIPCHK(bt, hipEventRecord(bt->e1, bt->stream));
    if (dualws_only) { HIPCHK(bt, hipEventRecord(bt->e2, bt->stream)); return 0; }
    // Two-launch schedule.  The kernel keeps a fixed number of instances resident; a larger batch is dispatched in blockIdx
    // order as workgroups retire, so an instance that needs three times the median number of passes and happens to sit late in the batch
    // would start late and finish alone.  Instead every instance first runs a short slice (OBCA_SLICE_PASSES factorisation passes, default
    // 6), the parked solves are ranked by what the slice revealed, and a second launch finishes them hardest-first.  No work is repeated
    // and every instance walks through the same iterates as in a single launch.  OBCA_SLICE_PASSES=0 turns it off; OBCA_SLICE_ONLY=1
    // (diagnostic) stops after the first slice.
    int budget = 6;
    if (const char *e = getenv("OBCA_SLICE_PASSES")) budget = atoi(e);
    const bool slice_only = getenv("OBCA_SLICE_ONLY") && atoi(getenv("OBCA_SLICE_ONLY"));
    // forward-sweep trajectory + stage buffers / pair maps, sized for the horizon (obca_solver.h)
#ifdef OBCA_POISON      // the poisoned build adds a guard of OBCA_LDS_GUARD doubles behind the dynamic block (NaNs, written at entry, never again): a read beyond the block finds it
    const size_t dyn_lds = (OB_DYN_LDS_DOUBLES(bt->N) + OBCA_LDS_GUARD) * sizeof(double);
#else
    const size_t dyn_lds = OB_DYN_LDS_DOUBLES(bt->N) * sizeof(double);
#endif
    const int slots = parking_resident_per_cu(bt->N) * (bt->ctx->cus > 0 ? bt->ctx->cus : 256);
    // OBCA_SLICE_ALWAYS=1 (tuning knob): the two-launch schedule also for a batch that fits the machine -- with several batches in flight the workgroups of a launch start as
    // slots free up, in blockIdx order, and the ranking lets the long solves of a batch start first
    const bool slice_always = getenv("OBCA_SLICE_ALWAYS") && atoi(getenv("OBCA_SLICE_ALWAYS"));
    bt->sliced = (budget > 0 && (bt->B > slots || slice_only || slice_always)) ? budget : 0;   // 0: single launch, else the slice length
    if (!bt->sliced) {
        hipLaunchKernelGGL(obca_parking_ipm_kernel, dim3(bt->B), dim3(OB_NT), dyn_lds, bt->stream, bt->B, bt->N, bt->d, ko, 0, 0, o.max_soc, o.recalc_y != 0, o.lsq_init != 0, o.restoration);
        HIPCHK(bt, hipGetLastError());
    } else {
        hipLaunchKernelGGL(obca_parking_ipm_kernel, dim3(bt->B), dim3(OB_NT), dyn_lds, bt->stream, bt->B, bt->N, bt->d, ko, 0, budget, o.max_soc, o.recalc_y != 0, o.lsq_init != 0, o.restoration);
        HIPCHK(bt, hipGetLastError());
        if (!slice_only) {
            hipLaunchKernelGGL(obca_order_kernel, dim3(1), dim3(1024), 0, bt->stream, bt->B, (const double *)d.info, (const double *)d.slice, d.order);
            HIPCHK(bt, hipGetLastError());
            hipLaunchKernelGGL(obca_parking_ipm_kernel, dim3(bt->B), dim3(OB_NT), dyn_lds, bt->stream, bt->B, bt->N, bt->d, ko, 1, 0, o.max_soc, o.recalc_y != 0, o.lsq_init != 0, o.restoration);
            HIPCHK(bt, hipGetLastError());
        }
    }
    HIPCHK(bt, hipEventRecord(bt->e2, bt->stream));
    bt->solved = 1;
    return 0;
}

// outputs of the batch's instances into the caller's arrays (instance i of the batch = instance lo + i of the call; packed obstacle outputs
// go to the offsets recorded at upload).  Synchronises the batch's stream.
static int batch_download_range(obca_batch *bt, const ParkOut &o, int lo) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    const DevBufs &d = bt->d;
    use_device(bt->device);
    Lay lmax; make_layout(N, bt->nObMax, bt->MMax, lmax);
    const size_t W = (size_t)lmax.so;                       // outputs are a prefix of the iterate: x, u, t, lam, mu, sl
    const bool want_z = o.xp || o.up || o.ts || o.lp || o.np || o.slp || o.lWS || o.nWS;
    if (bt->h_zout.reserve(bt->err, (size_t)bt->cap * std::max(W, (size_t)N1 * bt->nObMax)) || bt->h_info.reserve(bt->err, (size_t)bt->cap * 8)) return -2;
    if (want_z) {
        hipLaunchKernelGGL(obca_gather_rows_kernel, dim3(B, (unsigned)((W + 1023) / 1024)), dim3(256), 0, bt->stream, bt->stage, W, (const double *)d.z, d.s_z);
        HIPCHK(bt, hipGetLastError());
        HIPCHK(bt, hipMemcpyAsync(bt->h_zout, bt->stage, (size_t)B * W * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
    }
    HIPCHK(bt, hipMemcpyAsync(bt->h_info, d.info, (size_t)B * 8 * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
    HIPCHK(bt, hipStreamSynchronize(bt->stream));
    for (int i = 0; i < B; i++) {
        const size_t g = (size_t)lo + i;
        Lay l; make_layout(N, bt->nOb[i], bt->M[i], l);
        const double *z = bt->h_zout + (size_t)i * W;
        if (o.xp) memcpy(o.xp + g * 4 * N1, z + l.x, sizeof(double) * 4 * N1);
        if (o.up) memcpy(o.up + g * 2 * N, z + l.u, sizeof(double) * 2 * N);
        if (o.ts) for (int k = 0; k < N1; k++) o.ts[g * N1 + k] = bt->fixTime ? 1.0 : z[l.t];   /* ParkingSignedDist.jl:304-308 */
        const double *rl = bt->rowLen.data() + (bt->rowOff[i] - bt->rowOff[0]); const int m = bt->M[i];      // lambda back in the caller's row scaling
        if (o.lp) for (int k = 0; k < N1; k++) for (int r = 0; r < m; r++) o.lp[(size_t)bt->rowOff[i] * N1 + (size_t)k * m + r] = z[l.lam + k * m + r] / rl[r];
        if (o.np) memcpy(o.np + (size_t)bt->obOff[i] * 4 * N1, z + l.mu, sizeof(double) * 4 * bt->nOb[i] * N1);
        if (o.slp) memcpy(o.slp + (size_t)bt->obOff[i] * N1, z + l.sl, sizeof(double) * bt->nOb[i] * N1);
        if (o.lWS) for (int k = 0; k < N1; k++) for (int r = 0; r < m; r++) o.lWS[(size_t)bt->rowOff[i] * N1 + (size_t)k * m + r] = z[l.lam + k * m + r] / rl[r];
        if (o.nWS) memcpy(o.nWS + (size_t)bt->obOff[i] * 4 * N1, z + l.mu, sizeof(double) * 4 * bt->nOb[i] * N1);
        if (o.exitflag) o.exitflag[g] = (int)bt->h_info[(size_t)i * 8 + 7];
        if (o.info) memcpy(o.info + g * 8, bt->h_info + (size_t)i * 8, sizeof(double) * 8);
    }
    if (o.dd) {   // DualMultWS distances: nOb_i x (N+1) packed
        HIPCHK(bt, hipMemcpyAsync(bt->h_zout, d.dws, (size_t)B * N1 * bt->nObMax * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
        HIPCHK(bt, hipStreamSynchronize(bt->stream));
        for (int i = 0; i < B; i++) for (int k = 0; k < N1; k++) for (int j = 0; j < bt->nOb[i]; j++)
            o.dd[(size_t)bt->obOff[i] * N1 + (size_t)k * bt->nOb[i] + j] = bt->h_zout[(size_t)i * N1 * bt->nObMax + (size_t)k * bt->nObMax + j];
    }
    return 0;
}

// ---- a-posteriori validation (obca_validate.h)
static int val_reserve(std::string &err, ValBufs &v, size_t in_doubles, size_t out_doubles, hipStream_t stream) {
    if (int rc = v.ev.ensure(err)) return rc;
    if (v.d_in.reserve(in_doubles, stream) != hipSuccess) { err = "hipMalloc(validate input) failed"; return -2; }
    if (v.d_out.reserve(out_doubles, stream) != hipSuccess) { err = "hipMalloc(validate output) failed"; return -2; }
    if (v.h_in.reserve(err, in_doubles) || v.h_out.reserve(err, out_doubles)) return -2;
    return 0;
}
// One validate (v = bt->val) or clearance (v = bt->clr) call over the batch's instances, on its stream: reserve the buffers -> if `upload`, pack(i, row) fills instance i's `s_in` doubles of v.h_in
// and they travel up to v.d_in (else v.d_in is left as it is) -> launch() between the two events -> the `s_out` result doubles per instance come down -> unpack(i, row) reads instance i's.
// Synchronises the batch's stream.
template <typename Pack, typename Launch, typename Unpack>
static int run_validate(BatchCore *bt, ValBufs &v, size_t s_in, bool upload, size_t s_out, Pack &&pack, Launch &&launch, Unpack &&unpack) {
    const int B = bt->B;
    use_device(bt->device);
    if (int rc = val_reserve(bt->err, v, std::max<size_t>(1, (size_t)bt->cap * s_in), (size_t)bt->cap * s_out, bt->stream)) return rc;
    if (upload) {
        for (int i = 0; i < B; i++) pack(i, v.h_in + (size_t)i * s_in);
        HIPCHK(bt, hipMemcpyAsync(v.d_in, v.h_in, (size_t)B * s_in * sizeof(double), hipMemcpyHostToDevice, bt->stream));
    }
    HIPCHK(bt, v.ev.begin(bt->stream));
    launch();
    HIPCHK(bt, hipGetLastError());
    HIPCHK(bt, v.ev.end(bt->stream));
    v.ev.timed = 1;
    HIPCHK(bt, hipMemcpyAsync(v.h_out, v.d_out, (size_t)B * s_out * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
    HIPCHK(bt, hipStreamSynchronize(bt->stream));
    for (int i = 0; i < B; i++) unpack(i, (const double *)v.h_out + (size_t)i * s_out);
    return 0;
}

// Checks the batch's instances: resident (ts == nullptr: the last solution in d.z, only the row lengths travel up) or a caller's trajectory that
// batch_upload_range has just packed into d.z0 (ts: (N + 1) per instance of the call, sl: the caller's packed slack or nullptr = the zeros of the upload).
// Instance i of the batch is instance lo + i of the call.  Only PV_OUT doubles per instance come back.
static int batch_validate_range(obca_batch *bt, const double *ts, const double *sl, double tol, int lo, int *ok, int *ref_ok, double *viol) {
    const int B = bt->B, N = bt->N, N1 = N + 1, MMax = bt->MMax;
    const bool host = ts != nullptr;
    const size_t s_aux = (size_t)MMax + (host ? (size_t)N1 + (size_t)bt->nObMax * N1 : 0);
    const int rc = run_validate(bt, bt->val, s_aux, host || !bt->val_rl, PV_OUT, [&](int i, double *a) {
        const double *rl = bt->rowLen.data() + (bt->rowOff[i] - bt->rowOff[0]);
        for (int r = 0; r < MMax; r++) a[r] = r < bt->M[i] ? rl[r] : 1.0;
        if (host) {
            memcpy(a + MMax, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
            double *as = a + MMax + N1; const size_t ns = (size_t)bt->nOb[i] * N1;
            if (sl) memcpy(as, sl + (size_t)bt->obOff[i] * N1, sizeof(double) * ns); else memset(as, 0, sizeof(double) * ns);
        }
    }, [&] {
        hipLaunchKernelGGL(obca_validate_parking_kernel, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, (const double *)(host ? bt->d.z0 : bt->d.z), bt->d.s_z,
                           (const double *)bt->val.d_in, s_aux, MMax, host ? 1 : 0, (host && sl) ? 1 : 0, tol, bt->val.d_out);
    }, [&](int i, const double *o) {
        const size_t g = (size_t)lo + i;
        if (viol) memcpy(viol + g * PV_NCLS, o, sizeof(double) * PV_NCLS);
        if (ok) ok[g] = o[PV_NCLS] != 0.0;
        if (ref_ok) ref_ok[g] = o[PV_NCLS + 1] != 0.0;
    });
    if (!rc && !host) bt->val_rl = 1;      // the row lengths stay in val.d_in until the next upload: the next resident validate skips its H2D
    return rc;
}

// Clearance between the nodes of the batch's instances (obca_clearance.h): resident (`host` false: the last solution in d.z) or a caller's trajectory that batch_upload_range
// has just packed into d.z0 (ts: (N + 1) per instance of the call, or nullptr = 1: the t of the packed point).  Instance i of the batch is instance lo + i of the call.
// Only CL_OUT doubles per instance come back.
static int batch_clearance_range(obca_batch *bt, bool host, const double *ts, int S, double need, int lo, double *out) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    return run_validate(bt, bt->clr, ts ? (size_t)N1 : 0, ts != nullptr, CL_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z, *dts = ts ? (const double *)bt->clr.d_in : nullptr;
#define CLR_LAUNCH(VM) hipLaunchKernelGGL(obca_clearance_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, dts, S, need, bt->clr.d_out)
        if (bt->vmax <= 2) CLR_LAUNCH(2); else if (bt->vmax <= OB_VMID) CLR_LAUNCH(OB_VMID); else CLR_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef CLR_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * CL_OUT, o, sizeof(double) * CL_OUT); });
}

// What the two rollout routes share (obca_rollout.h).  Before the kernel: the work buffer for B instances of horizon N at S sub-steps (grown on demand).  After it: the
// bookkeeping of the *_states calls and, for a host-pointer call, the node states of the chunk into the caller's X (nx x (N + 1) per instance, instance lo + i of the call).
static int rollout_reserve(BatchCore *bt, int nx, int S) {
    use_device(bt->device);
    if (bt->rol_w.reserve((size_t)bt->B * (roll::rollout_pose_len(bt->N, S) + roll::rollout_state_len(bt->N, nx)), bt->stream) != hipSuccess) { bt->err = "hipMalloc(rollout work buffer) failed"; return -2; }
    return 0;
}
static inline double *rollout_states_at(BatchCore *bt, int S) { return bt->rol_w + (size_t)bt->B * roll::rollout_pose_len(bt->N, S); }
static int rollout_finish(BatchCore *bt, int rc, int nx, int S, int lo, double *X) {
    bt->rol_B = bt->rol_N = bt->rol_S = 0;
    if (rc) return rc;
    bt->rol_B = bt->B; bt->rol_N = bt->N; bt->rol_S = S;
    const size_t n = (size_t)bt->B * roll::rollout_state_len(bt->N, nx);
    if (X) HIPCHK(bt, hipMemcpy(X + (size_t)lo * roll::rollout_state_len(bt->N, nx), rollout_states_at(bt, S), n * sizeof(double), hipMemcpyDeviceToHost));      // (run_validate has synchronised the stream)
    return 0;
}
static int rollout_states(BatchCore *bt, int nx, double *X, const char *entry) {
    if (!X) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->rol_B || bt->rol_B != bt->B || bt->rol_N != bt->N) { bt->ctx->err = std::string(entry) + ": no rollout has run on this batch since it was last filled"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess || hipMemcpy(X, rollout_states_at(bt, bt->rol_S), (size_t)bt->B * roll::rollout_state_len(bt->N, nx) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// Rollout of the batch's parking instances: the arguments of batch_clearance_range, then the mode and the caller's X (host-pointer calls; nullptr: the states stay on the device)
static int batch_rollout_range(obca_batch *bt, bool host, const double *ts, int S, int restart, double need, int lo, double *out, double *X) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    if (int rc = rollout_reserve(bt, 4, S)) return rc;
    const int rc = run_validate(bt, bt->rol, ts ? (size_t)N1 : 0, ts != nullptr, RO_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z, *dts = ts ? (const double *)bt->rol.d_in : nullptr;
#define ROL_LAUNCH(VM) hipLaunchKernelGGL(obca_rollout_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, dts, S, restart, need, \
                                          (double *)bt->rol_w, roll::rollout_pose_len(N, S), rollout_states_at(bt, S), roll::rollout_state_len(N, 4), (double *)bt->rol.d_out)
        if (bt->vmax <= 2) ROL_LAUNCH(2); else if (bt->vmax <= OB_VMID) ROL_LAUNCH(OB_VMID); else ROL_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef ROL_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * RO_OUT, o, sizeof(double) * RO_OUT); });
    return rollout_finish(bt, rc, 4, S, lo, X);
}

// What the two track routes share (obca_track.h), as the rollout's: the work buffer and the gains for B instances before the kernel; after it the bookkeeping of the
// *_states / *_gains calls and, for a host-pointer call, the chunk's node states and gains into the caller's X and K.
struct TrackDims { int nx, nu; size_t ab, pose, st, gain; };
static TrackDims track_dims(const BatchCore *bt, int nx, int nu, int S) {
    return {nx, nu, trk::track_ab_len(bt->N, nx, nu), roll::rollout_pose_len(bt->N, S), roll::rollout_state_len(bt->N, nx), trk::track_gain_len(bt->N, nx, nu)};
}
static int track_reserve(BatchCore *bt, const TrackDims &d) {
    use_device(bt->device);
    if (bt->trk_w.reserve((size_t)bt->B * (d.ab + d.pose + d.st), bt->stream) != hipSuccess || bt->trk_K.reserve((size_t)bt->B * d.gain, bt->stream) != hipSuccess) {
        bt->err = "hipMalloc(track work buffer) failed"; return -2;
    }
    return 0;
}
static inline double *track_poses_at(BatchCore *bt, const TrackDims &d) { return bt->trk_w + (size_t)bt->B * d.ab; }
static inline double *track_states_at(BatchCore *bt, const TrackDims &d) { return bt->trk_w + (size_t)bt->B * (d.ab + d.pose); }
static int track_finish(BatchCore *bt, int rc, const TrackDims &d, int S, int lo, double *X, double *K) {
    bt->trk_B = bt->trk_N = bt->trk_S = 0;
    if (rc) return rc;
    bt->trk_B = bt->B; bt->trk_N = bt->N; bt->trk_S = S;
    if (X) HIPCHK(bt, hipMemcpy(X + (size_t)lo * d.st, track_states_at(bt, d), (size_t)bt->B * d.st * sizeof(double), hipMemcpyDeviceToHost));      // (run_validate has synchronised the stream)
    if (K) HIPCHK(bt, hipMemcpy(K + (size_t)lo * d.gain, (const double *)bt->trk_K, (size_t)bt->B * d.gain * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
static int track_fetch(BatchCore *bt, int nx, int nu, bool gains, double *dst, const char *entry) {
    if (!dst) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->trk_B || bt->trk_B != bt->B || bt->trk_N != bt->N) { bt->ctx->err = std::string(entry) + ": no track call has run on this batch since it was last filled"; return -1; }
    const TrackDims d = track_dims(bt, nx, nu, bt->trk_S);
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess ||
        hipMemcpy(dst, gains ? (const double *)bt->trk_K : track_states_at(bt, d), (size_t)bt->B * (gains ? d.gain : d.st) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// The closed-loop rollout of the batch's parking instances: the arguments of batch_rollout_range with the modes, the weights and dx0 (4 per instance of the call, or nullptr);
// per instance [ dx0 4 | timeScale N + 1 (host-pointer calls) ] travels up
static int batch_track_range(obca_batch *bt, bool host, const double *ts, int S, int feedback, int clamp, const trk::Weights &w, const double *dx0, double need, int lo, double *out, double *X, double *K) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    const TrackDims d = track_dims(bt, 4, 2, S);
    if (int rc = track_reserve(bt, d)) return rc;
    const size_t W = 4 + (ts ? (size_t)N1 : 0);
    const int rc = run_validate(bt, bt->trk, W, true, TK_OUT, [&](int i, double *a) {
        if (dx0) memcpy(a, dx0 + ((size_t)lo + i) * 4, sizeof(double) * 4); else memset(a, 0, sizeof(double) * 4);
        if (ts) memcpy(a + 4, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z;
#define TRK_LAUNCH(VM) hipLaunchKernelGGL(obca_track_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, (const double *)bt->trk.d_in, W, \
                                          dx0 ? 1 : 0, ts ? 1 : 0, S, feedback, clamp, w, need, (double *)bt->trk_w, d.ab, track_poses_at(bt, d), d.pose, track_states_at(bt, d), d.st, \
                                          (double *)bt->trk_K, d.gain, (double *)bt->trk.d_out)
        if (bt->vmax <= 2) TRK_LAUNCH(2); else if (bt->vmax <= OB_VMID) TRK_LAUNCH(OB_VMID); else TRK_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef TRK_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * TK_OUT, o, sizeof(double) * TK_OUT); });
    return track_finish(bt, rc, d, S, lo, X, K);
}

// What the two ensemble routes share (obca_ensemble.h), as the track routes': the buffers for B instances of M members before the kernel; after it the bookkeeping of the
// *_members / *_final calls and, for a host-pointer call, the chunk's member records and final states into the caller's mem and fin.
struct EnsDims { int nx, nu, M; size_t ab, gain, mem, fin; };
static EnsDims ensemble_dims(const BatchCore *bt, int nx, int nu, int M) {
    return {nx, nu, M, ens::ensemble_ab_len(bt->N, nx, nu), trk::track_gain_len(bt->N, nx, nu), ens::ensemble_mem_len(M), ens::ensemble_fin_len(M, nx)};
}
static int ensemble_reserve(BatchCore *bt, const EnsDims &d) {
    use_device(bt->device);
    if (bt->ens_w.reserve((size_t)bt->B * d.ab, bt->stream) != hipSuccess || bt->ens_K.reserve((size_t)bt->B * d.gain, bt->stream) != hipSuccess ||
        bt->ens_mem.reserve((size_t)bt->B * d.mem, bt->stream) != hipSuccess || bt->ens_fin.reserve((size_t)bt->B * d.fin, bt->stream) != hipSuccess) {
        bt->err = "hipMalloc(ensemble work buffer) failed"; return -2;
    }
    return 0;
}
// per instance [ dx0 nx x M | dub nu x M ] of a call's arrays (nullptr: zeros), instance g of the call
static void ensemble_pack(const EnsDims &d, const double *dx0, const double *dub, size_t g, double *a) {
    const size_t nd = (size_t)d.nx * d.M, nb = (size_t)d.nu * d.M;
    if (dx0) memcpy(a, dx0 + g * nd, sizeof(double) * nd); else memset(a, 0, sizeof(double) * nd);
    if (dub) memcpy(a + nd, dub + g * nb, sizeof(double) * nb); else memset(a + nd, 0, sizeof(double) * nb);
}
static int ensemble_finish(BatchCore *bt, int rc, const EnsDims &d, int lo, double *mem, double *fin) {
    bt->ens_B = bt->ens_N = bt->ens_M = 0;
    if (rc) return rc;
    bt->ens_B = bt->B; bt->ens_N = bt->N; bt->ens_M = d.M;
    if (mem) HIPCHK(bt, hipMemcpy(mem + (size_t)lo * d.mem, (const double *)bt->ens_mem, (size_t)bt->B * d.mem * sizeof(double), hipMemcpyDeviceToHost));      // (run_validate has synchronised the stream)
    if (fin) HIPCHK(bt, hipMemcpy(fin + (size_t)lo * d.fin, (const double *)bt->ens_fin, (size_t)bt->B * d.fin * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
static int ensemble_fetch(BatchCore *bt, int nx, bool final_states, double *dst, const char *entry) {
    if (!dst) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->ens_B || bt->ens_B != bt->B || bt->ens_N != bt->N) { bt->ctx->err = std::string(entry) + ": no ensemble call has run on this batch since it was last filled"; return -1; }
    const size_t n = (size_t)bt->B * (final_states ? ens::ensemble_fin_len(bt->ens_M, nx) : ens::ensemble_mem_len(bt->ens_M));
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess ||
        hipMemcpy(dst, final_states ? (const double *)bt->ens_fin : (const double *)bt->ens_mem, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// The ensemble about the batch's parking instances: the arguments of batch_track_range with the members, dx0 (4 x M per instance of the call, or nullptr) and dub (2 x M);
// per instance [ dx0 4 M | dub 2 M | timeScale N + 1 (host-pointer calls) ] travels up
static int batch_ensemble_range(obca_batch *bt, bool host, const double *ts, int S, int M, int feedback, int clamp, const trk::Weights &w, const double *dx0, const double *dub, double need, int lo,
                                double *out, double *mem, double *fin) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    const EnsDims d = ensemble_dims(bt, 4, 2, M);
    if (int rc = ensemble_reserve(bt, d)) return rc;
    const size_t W = (size_t)6 * M + (ts ? (size_t)N1 : 0);
    const int rc = run_validate(bt, bt->ens, W, true, EN_OUT, [&](int i, double *a) {
        ensemble_pack(d, dx0, dub, (size_t)lo + i, a);
        if (ts) memcpy(a + 6 * M, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z;
#define ENS_LAUNCH(VM) hipLaunchKernelGGL(obca_ensemble_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, (const double *)bt->ens.d_in, W, \
                                          ts ? 1 : 0, S, M, feedback, clamp, w, need, (double *)bt->ens_w, d.ab, (double *)bt->ens_K, d.gain, (double *)bt->ens_mem, (double *)bt->ens_fin, \
                                          (double *)bt->ens.d_out)
        if (bt->vmax <= 2) ENS_LAUNCH(2); else if (bt->vmax <= OB_VMID) ENS_LAUNCH(OB_VMID); else ENS_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef ENS_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * EN_OUT, o, sizeof(double) * EN_OUT); });
    return ensemble_finish(bt, rc, d, lo, mem, fin);
}

// What the two advance calls share (obca_advance.h).  advance_refuse: the refusals, before anything is launched or written.  advance_reserve: the work buffer and the plant
// states for B instances.  advance_finish: the bookkeeping after the kernel -- the batch counts as unsolved, as after a shift; the log has grown.
static int advance_refuse(BatchCore *bt, const char *entry, int shift, int substeps, double need, const double *out) {
    std::string &err = bt->ctx->err;
    if (!out) { err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->uploaded || !bt->solved) { err = std::string(entry) + ": nothing has been solved since the last upload, shift or advance"; return -1; }
    if (const char *bad = adv::advance_check_args(bt->N, shift, substeps, need)) { err = std::string(entry) + ": " + bad; return -1; }
    if (bt->adv_cap && bt->adv_n + shift > bt->adv_cap) { err = std::string(entry) + ": the log is full (obca_batch_advance_log sets its capacity)"; return -1; }
    return 0;
}
static int advance_reserve(BatchCore *bt, int nx, int shift, int S) {
    use_device(bt->device);
    if (bt->adv_w.reserve((size_t)bt->B * (adv::advance_pose_len(shift, S) + adv::advance_state_len(shift, nx)), bt->stream) != hipSuccess ||
        bt->adv_st.reserve((size_t)bt->cap * nx, bt->stream) != hipSuccess) { bt->err = "hipMalloc(advance work buffer) failed"; return -2; }
    return 0;
}
static int advance_finish(BatchCore *bt, int rc, int shift) {
    bt->adv_B = bt->adv_N = 0;
    if (rc) return rc;
    bt->adv_B = bt->B; bt->adv_N = bt->N;
    if (bt->adv_cap) bt->adv_n += shift;
    bt->solved = 0;      // d.z still holds the previous solution, but the problem (x0, reference / warm start) has moved on
    return 0;
}
static int advance_state(BatchCore *bt, int nx, double *X, const char *entry) {
    if (!X) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->adv_B || bt->adv_B != bt->B || bt->adv_N != bt->N) { bt->ctx->err = std::string(entry) + ": no advance has run on this batch since it was last filled"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess || hipMemcpy(X, (const double *)bt->adv_st, (size_t)bt->B * nx * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
static int advance_log(BatchCore *bt, int nx, int capacity, const char *entry) {
    if (capacity < 0 || (size_t)capacity > ((size_t)1 << 31) / ((size_t)bt->cap * nx)) { bt->ctx->err = std::string(entry) + ": capacity out of range"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess) { bt->ctx->err = std::string(entry) + ": hipStreamSynchronize failed"; return -2; }
    bt->adv_log.release(); bt->adv_cap = bt->adv_n = 0;
    if (!capacity) return 0;
    if (bt->adv_log.reserve((size_t)bt->cap * capacity * nx, bt->stream) != hipSuccess) { bt->ctx->err = std::string(entry) + ": hipMalloc(log) failed"; return -2; }
    bt->adv_cap = capacity;
    return 0;
}
static int advance_log_states(BatchCore *bt, int nx, double *X, int *nodes, const char *entry) {
    if (!nodes) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->adv_cap) { bt->ctx->err = std::string(entry) + ": this batch has no log (obca_batch_advance_log allocates one)"; return -1; }
    *nodes = bt->adv_n;
    if (!X || !bt->adv_n) return 0;
    use_device(bt->device);
    const size_t row = (size_t)bt->adv_n * nx * sizeof(double);      // the filled rows of every instance, dense
    if (hipStreamSynchronize(bt->stream) != hipSuccess ||
        hipMemcpy2D(X, row, (const double *)bt->adv_log, (size_t)bt->adv_cap * nx * sizeof(double), row, (size_t)bt->B, hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// One step of the batch's parking instances: the kick (4 per instance, or nullptr) travels up
static int batch_advance_run(obca_batch *bt, int shift, int S, const double *kick, double need, double *out) {
    const int B = bt->B, N = bt->N;
    if (int rc = advance_reserve(bt, 4, shift, S)) return rc;
    const size_t sp = adv::advance_pose_len(shift, S), sx = adv::advance_state_len(shift, 4);
    const int rc = run_validate(bt, bt->adv, 4, kick != nullptr, AV_OUT, [&](int i, double *a) { memcpy(a, kick + (size_t)i * 4, sizeof(double) * 4); }, [&] {
        double *log = bt->adv_cap ? (double *)bt->adv_log : nullptr;
        const double logged = bt->adv_cap ? (double)(bt->adv_n + shift) : -1.0;
#define ADV_LAUNCH(VM) hipLaunchKernelGGL(obca_advance_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, shift, bt->d, S, (const double *)bt->adv.d_in, kick ? 1 : 0, need, \
                                          (double *)bt->adv_w, sp, bt->adv_w + (size_t)B * sp, sx, (double *)bt->adv_st, log, (size_t)bt->adv_cap * 4, (size_t)bt->adv_n * 4, logged, (double *)bt->adv.d_out)
        if (bt->vmax <= 2) ADV_LAUNCH(2); else if (bt->vmax <= OB_VMID) ADV_LAUNCH(OB_VMID); else ADV_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef ADV_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + (size_t)i * AV_OUT, o, sizeof(double) * AV_OUT); });
    return advance_finish(bt, rc, shift);
}

// What the two certify routes share (obca_certify.h): the interval arrays for B instances before the kernel; after it the bookkeeping of the *_intervals calls and, for a
// host-pointer call, the chunk's interval arrays into the caller's iv.
static int certify_reserve(BatchCore *bt) {
    use_device(bt->device);
    if (bt->cer_iv.reserve((size_t)bt->B * cert::certify_iv_len(bt->N), bt->stream) != hipSuccess) { bt->err = "hipMalloc(certify interval array) failed"; return -2; }
    return 0;
}
static int certify_finish(BatchCore *bt, int rc, int lo, double *iv) {
    bt->cer_B = bt->cer_N = 0;
    if (rc) return rc;
    bt->cer_B = bt->B; bt->cer_N = bt->N;
    const size_t n = cert::certify_iv_len(bt->N);
    if (iv) HIPCHK(bt, hipMemcpy(iv + (size_t)lo * n, (const double *)bt->cer_iv, (size_t)bt->B * n * sizeof(double), hipMemcpyDeviceToHost));      // (run_validate has synchronised the stream)
    return 0;
}
static int certify_fetch(BatchCore *bt, double *iv, const char *entry) {
    if (!iv) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->cer_B || bt->cer_B != bt->B || bt->cer_N != bt->N) { bt->ctx->err = std::string(entry) + ": no certify call has run on this batch since it was last filled"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess ||
        hipMemcpy(iv, (const double *)bt->cer_iv, (size_t)bt->B * cert::certify_iv_len(bt->N) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// The certificate of the batch's parking instances: the arguments of batch_clearance_range with need, slack and max_steps, then the caller's iv (host-pointer calls; nullptr:
// the interval arrays stay on the device)
static int batch_certify_range(obca_batch *bt, bool host, const double *ts, double need, double slack, int max_steps, int lo, double *out, double *iv) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    if (int rc = certify_reserve(bt)) return rc;
    const size_t lds = cert::certify_work_len(N, bt->nObMax) * sizeof(double);      // (at most 3 x 129 x 16 doubles = 49.5 KB: below the 64 KB a launch may ask for)
    const int rc = run_validate(bt, bt->cer, ts ? (size_t)N1 : 0, ts != nullptr, CT_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z, *dts = ts ? (const double *)bt->cer.d_in : nullptr;
#define CERT_LAUNCH(VM) hipLaunchKernelGGL(obca_certify_parking_kernel<VM>, dim3(B), dim3(OB_NT), lds, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, dts, need, slack, max_steps, \
                                           (double *)bt->cer_iv, (double *)bt->cer.d_out)
        if (bt->vmax <= 2) CERT_LAUNCH(2); else if (bt->vmax <= OB_VMID) CERT_LAUNCH(OB_VMID); else CERT_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef CERT_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * CT_OUT, o, sizeof(double) * CT_OUT); });
    return certify_finish(bt, rc, lo, iv);
}

// What the two predict routes share (obca_predict.h).  Before the kernel: the profile buffer for B instances of horizon N at S sub-steps if the call keeps one (grown on
// demand).  After it: the bookkeeping of the *_predict_profile calls and, for a host-pointer call, the chunk's profile rows into the caller's array.
static int predict_reserve(BatchCore *bt, int S, bool keep) {
    if (!keep) return 0;
    use_device(bt->device);
    if (bt->prd_w.reserve((size_t)bt->B * ((size_t)bt->N * S + 1), bt->stream) != hipSuccess) { bt->err = "hipMalloc(predict profile) failed"; return -2; }
    return 0;
}
static int predict_finish(BatchCore *bt, int rc, int S, bool keep, int lo, double *profile) {
    if (!keep) return rc;      // (a call without a profile leaves the last kept one as it is)
    bt->prd_B = bt->prd_N = bt->prd_S = 0;
    if (rc) return rc;
    bt->prd_B = bt->B; bt->prd_N = bt->N; bt->prd_S = S;
    const size_t n = (size_t)bt->N * S + 1;
    if (profile) HIPCHK(bt, hipMemcpy(profile + (size_t)lo * n, (const double *)bt->prd_w, (size_t)bt->B * n * sizeof(double), hipMemcpyDeviceToHost));      // (run_validate has synchronised the stream)
    return 0;
}
static int predict_fetch(BatchCore *bt, double *out, int capacity, const char *entry) {
    if (!out) { bt->ctx->err = std::string(entry) + ": NULL argument"; return -1; }
    if (!bt->prd_B || bt->prd_B != bt->B || bt->prd_N != bt->N) { bt->ctx->err = std::string(entry) + ": no predict call has kept a profile on this batch since it was last filled"; return -1; }
    const size_t n = (size_t)bt->B * ((size_t)bt->N * bt->prd_S + 1);
    if (capacity < 0 || (size_t)capacity < n) { bt->ctx->err = std::string(entry) + ": capacity is below B (N substeps + 1)"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess || hipMemcpy(out, (const double *)bt->prd_w, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = std::string(entry) + ": D2H failed"; return -2;
    }
    return 0;
}
// The prediction for the batch's parking instances: the arguments of batch_clearance_range, then the rates (PR_PIN per obstacle, packed over the obstacles of the call),
// whether a profile is kept and the caller's profile array (host-pointer calls; nullptr: the profile stays on the device).  The rates travel in rows of nObMax obstacles.
static int batch_predict_range(obca_batch *bt, bool host, const double *ts, const double *rates, int S, double need, bool keep, int lo, double *out, double *profile) {
    const int B = bt->B, N = bt->N, N1 = N + 1;
    if (int rc = predict_reserve(bt, S, keep)) return rc;
    const size_t s_rt = (size_t)PR_PIN * bt->nObMax, s_in = s_rt + (ts ? (size_t)N1 : 0);
    const int rc = run_validate(bt, bt->prd, s_in, true, PR_OUT, [&](int i, double *a) {
        memset(a, 0, sizeof(double) * s_rt);
        const size_t o = (size_t)(host ? bt->obOff[i] : bt->obOff[i] - bt->obOff[0]);
        memcpy(a, rates + (size_t)PR_PIN * o, sizeof(double) * PR_PIN * bt->nOb[i]);
        if (ts) memcpy(a + s_rt, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *z = host ? bt->d.z0 : bt->d.z;
#define PRD_LAUNCH(VM) hipLaunchKernelGGL(obca_predict_parking_kernel<VM>, dim3(B), dim3(OB_NT), 0, bt->stream, B, N, (const double *)bt->d.prob, bt->d.s_prob, z, bt->d.s_z, (const double *)bt->prd.d_in, s_in, s_rt, \
                                          ts ? 1 : 0, S, need, (double *)bt->prd.d_out, keep ? (double *)bt->prd_w : nullptr, (size_t)N * S + 1)
        if (bt->vmax <= 2) PRD_LAUNCH(2); else if (bt->vmax <= OB_VMID) PRD_LAUNCH(OB_VMID); else PRD_LAUNCH(OB_VMAX);      // (the row class of launch_dualws)
#undef PRD_LAUNCH
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * PR_OUT, o, sizeof(double) * PR_OUT); });
    return predict_finish(bt, rc, S, keep, lo, profile);
}

// ---- chunked execution of a host-pointer call over the slots of the context (work queue)
template <typename F>
static int run_chunks(obca_ctx *ctx, int B, int chunk, F &&fn /* int(Slot &, int lo, int n, std::string &err) */) {
    const int nchunks = (B + chunk - 1) / chunk;
    const int nw = std::min<int>(nchunks, (int)ctx->slots.size());
    std::atomic<int> next(0);
    // OBCA_CHUNK_PERM = s (diagnostic, tests/test_gpu_determinism.py): the t-th ticket of
    // the queue is chunk (t + s) mod nchunks for even s, the chunks in descending order
    // from there for odd s -- which lane (stream, cached batch, staging buffers) solves which chunk must not matter to a single bit of the results
    int perm = 0; if (const char *e = getenv("OBCA_CHUNK_PERM")) perm = atoi(e) > 0 ? atoi(e) : 0;
    std::vector<int> rcs(nw, 0); std::vector<std::string> errs(nw);
    for (int w = 0; w < nw; w++) {      // lanes get their stream on first use (see obca_create_multi)
        Slot &s = ctx->slots[w];
        if (!s.stream && (hipSetDevice(s.device) != hipSuccess || hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess)) { ctx->err = "hipStreamCreate failed"; return -2; }
    }
    auto work = [&](int w) {
        Slot &s = ctx->slots[w];
        use_device(s.device);
        for (;;) {
            const int t = next.fetch_add(1);
            if (t >= nchunks) break;
            const int c = !perm ? t : ((perm & 1) ? ((nchunks - 1 - t) + perm) % nchunks : (t + perm) % nchunks);
            const int lo = c * chunk, n = std::min(chunk, B - lo);
            const int rc = fn(s, lo, n, errs[w]);
            if (rc) { rcs[w] = rc; next.store(nchunks); break; }
        }
    };
    if (nw <= 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int w = 1; w < nw; w++) th.emplace_back(work, w);
        work(0);
        for (auto &t : th) t.join();
    }
    use_device(ctx->device);
    for (int w = 0; w < nw; w++) if (rcs[w]) { ctx->err = errs[w]; return rcs[w]; }
    return 0;
}
static int pick_chunk(const obca_ctx *ctx, int B, int resident_per_cu) {
    // twice the instances resident on one GPU per chunk: measured best on config-2 batches (PCIe-inclusive, 4 lanes: 92-98 k solves/s against 75 k
    // with 256-instance chunks) -- what counts is the number of instances in flight (lanes x chunk), which must cover the heavy tail of the
    // solve times several times over; chunks beyond the resident capacity use the two-launch schedule of batch_solve
    int chunk = (resident_per_cu >= 4 ? 1 : 2) * resident_per_cu * (ctx->cus > 0 ? ctx->cus : 256);      // 1024 on a 256-CU part for both paths
    if (const char *e = getenv("OBCA_CHUNK")) { const int v = atoi(e); if (v > 0) chunk = v; }
    // small calls: still give every slot something to do once there is enough work to hide a transfer behind
    const int ns = (int)ctx->slots.size();
    if (B < chunk * ns && B >= 64 * ns) chunk = (B + ns - 1) / ns;
    return std::max(1, std::min(chunk, B));
}
static int batch_create_on(obca_ctx *ctx, int device, hipStream_t stream, int B, int N, obca_quad_batch **out, std::string &err);
// the slot's cached batch (`cached` is s.pb or s.qb) if it holds `need` instances of horizon N, else a new one of capacity `cap` in its place
template <typename BT>
static int slot_batch(obca_ctx *ctx, Slot &s, BT *&cached, int (*destroy)(BT *), int need, int cap, int N, std::string &err) {
    if (cached && (cached->cap < need || cached->N != N)) { destroy(cached); cached = nullptr; }
    return cached ? 0 : batch_create_on(ctx, s.device, s.stream, cap, N, &cached, err);
}

// a parking host-pointer call over the slots: per chunk the slot's cached batch -> upload of the chunk's instances -> op(batch, lo) -> the batch's error text if one of them failed
template <typename Op>
static int parking_chunks(obca_ctx *ctx, int dist, int B, int N, const ParkIn &in, Op &&op /* int(obca_batch *, int lo) */) {
    const int chunk = pick_chunk(ctx, B, 4);
    return run_chunks(ctx, B, chunk, [&](Slot &s, int lo, int n, std::string &err) -> int {
        int rc = slot_batch(ctx, s, s.pb, obca_batch_destroy, std::min(chunk, B), std::min(chunk, B), N, err);
        if (rc) return rc;
        obca_batch *bt = s.pb; bt->dist = dist ? 1 : 0;
        rc = batch_upload_range(bt, in, lo, n);
        if (!rc) rc = op(bt, lo);
        if (rc) err = bt->err;
        return rc;
    });
}

static int parking_call(obca_ctx *ctx, int dist, int dualws_only, int B, int N, ParkIn &in, const obca_opts *opts, const ParkOut &out) {
    if (!ctx) return -1;
    if (B < 1 || N < 0 || N > OBCA_NMAX) { ctx->err = "need B>=1, 0<=N<=OBCA_NMAX"; return -1; }
    if (!in.Ts || !in.ego || !in.XYb || !in.nOb || !in.vOb || !in.A || !in.b || !in.rx || !in.ry || !in.ryaw) { ctx->err = "NULL argument"; return -1; }
    if (!dualws_only && N < 2) { ctx->err = "the NLP needs a horizon N>=2"; return -1; }
    if (int rc = park_prefix(ctx->err, B, in.nOb, in.vOb, in)) return rc;
    return parking_chunks(ctx, dist, B, N, in, [&](obca_batch *bt, int lo) -> int {
        const int rc = batch_solve(bt, opts, dualws_only);
        return rc ? rc : batch_download_range(bt, out, lo);
    });
}

extern "C" {

int obca_batch_create(obca_ctx *ctx, int B, int N, obca_batch **out) {
    if (!ctx || !out) return -1;
    return batch_create_on(ctx, ctx->device, ctx->stream, B, N, out, ctx->err);
}
int obca_batch_destroy(obca_batch *bt) {
    if (!bt) return -1;
    use_device(bt->device);
    free_dev(bt); core_release(bt); (void)hipEventDestroy(bt->e2); bt->h_zin.release(); bt->h_zout.release(); bt->pw.release(); bt->rf.release(); bt->plan.release();
    delete bt; return 0;
}
#ifdef OBCA_PROFILE
int obca_batch_debug_phase_cycles(obca_batch *bt, double *out) { return bt ? core_phase_cycles(bt, bt->d.prof, out, "obca_batch_debug_phase_cycles: copy failed") : -1; }
#endif
int obca_batch_set_formulation(obca_batch *bt, int dist) { if (!bt) return -1; bt->dist = dist ? 1 : 0; return 0; }   /* before obca_batch_upload */
int obca_batch_scratch_bytes(const obca_batch *bt, long long *bytes) { return core_scratch_bytes(bt, bytes); }

int obca_batch_upload(obca_batch *bt, const double *Ts, double L, const double ego[4], const double XYb[4], int fixTime,
                      const double *x0, const double *xF, const int *nOb, const int *vOb, const double *A, const double *b,
                      const double *rx, const double *ry, const double *ryaw, const double *xWS, const double *uWS,
                      const double *lWS, const double *nWS) {
    if (!bt) return -1;
    if (!Ts || !ego || !XYb || !nOb || !vOb || !A || !b || !rx || !ry || !ryaw) { bt->ctx->err = "obca_batch_upload: NULL argument"; return -1; }
    ParkIn in = {Ts, L, ego, XYb, fixTime, x0, xF, nOb, vOb, A, b, rx, ry, ryaw, xWS, uWS, lWS, nWS, {}, {}};
    if (int rc = park_prefix(bt->err, bt->cap, nOb, vOb, in)) { bt->ctx->err = "obca_batch_upload: " + bt->err; return rc; }
    int rc = batch_upload_range(bt, in, 0, bt->cap);
    if (!rc && hipStreamSynchronize(bt->stream) != hipSuccess) { bt->err = "obca_batch_upload: stream sync failed"; rc = -2; }
    return fin(bt, rc);
}
int obca_batch_solve(obca_batch *bt, const obca_opts *opts) { if (!bt) return -1; return fin(bt, batch_solve(bt, opts, 0)); }
int obca_batch_shift_warm_start(obca_batch *bt, int shift, const double *x0_new) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    if (!bt->uploaded) { ctx->err = "obca_batch_shift_warm_start: nothing uploaded"; return -1; }
    if (shift < 0 || shift > bt->N) { ctx->err = "obca_batch_shift_warm_start: shift out of range 0..N"; return -1; }
    if (!bt->solved) { ctx->err = "obca_batch_shift_warm_start: nothing has been solved since the last upload or shift"; return -1; }
    for (size_t i = 0; x0_new && i < (size_t)bt->B * 4; i++)
        if (!(x0_new[i] - x0_new[i] == 0.0)) { ctx->err = "obca_batch_shift_warm_start: non-finite entry in x0_new"; return -1; }
    use_device(bt->device);
    double *dx0 = nullptr;
    if (x0_new) {   // staged through the (idle) device staging buffer of the batch: nothing to free on the error paths
        if (bt->h_info.reserve(bt->err, (size_t)bt->cap * 8)) return fin(bt, -2);
        memcpy(bt->h_info, x0_new, (size_t)bt->B * 4 * sizeof(double));
        dx0 = bt->stage;
        if (hipMemcpyAsync(dx0, bt->h_info, (size_t)bt->B * 4 * sizeof(double), hipMemcpyHostToDevice, bt->stream) != hipSuccess) { ctx->err = "obca_batch_shift_warm_start: H2D failed"; return -2; }
    }
    hipLaunchKernelGGL(obca_shift_kernel, dim3(bt->B), dim3(OB_NT), 0, bt->stream, bt->B, bt->N, shift, bt->d, (const double *)dx0);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bt->stream) != hipSuccess) { ctx->err = "obca_batch_shift_warm_start: kernel failed"; return -2; }
    bt->solved = 0;                                     // d.z still holds the previous solution, but the problem (x0, reference) has moved on
    bt->have_duals = 1;                                 // the shifted multipliers are the dual warm start: DualMultWS is skipped
    return 0;
}
int obca_batch_sync(obca_batch *bt) { return core_sync(bt, "obca_batch_sync: hipStreamSynchronize failed"); }
int obca_batch_last_schedule(const obca_batch *bt, int *ipm_launches, int *slice_passes) {
    if (!bt) return -1;
    if (ipm_launches) *ipm_launches = bt->sliced ? 2 : 1;
    if (slice_passes) *slice_passes = bt->sliced;
    return 0;
}
int obca_batch_kernel_ms(obca_batch *bt, float *ipm_ms, float *dualws_ms) {
    if (!bt) return -1;
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, bt->e0, bt->e1) != hipSuccess || hipEventElapsedTime(&b, bt->e1, bt->e2) != hipSuccess) { bt->ctx->err = "obca_batch_kernel_ms: events not ready"; return -2; }
    if (dualws_ms) *dualws_ms = a; if (ipm_ms) *ipm_ms = b;
    return 0;
}
int obca_batch_download(obca_batch *bt, double *xp, double *up, double *ts, int *exitflag, double *lp, double *np, double *slp, double *info) {
    if (!bt) return -1;
    if (!bt->uploaded) { bt->ctx->err = "obca_batch_download: nothing uploaded"; return -1; }
    ParkOut o = {xp, up, ts, exitflag, lp, np, slp, info, nullptr, nullptr, nullptr};
    return fin(bt, batch_download_range(bt, o, 0));
}

int obca_batch_validate(obca_batch *bt, double tol, int *ok, int *ref_ok, double *viol) {
    if (!bt) return -1;
    if (!ok) { bt->ctx->err = "obca_batch_validate: NULL argument"; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_validate: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_validate: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_validate_range(bt, nullptr, nullptr, tol > 0 ? tol : PV_REF_TOL, 0, ok, ref_ok, viol));
}
int obca_batch_validate_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->val.ev, ms, "obca_batch_validate_ms: no validate call has run on this batch") : -1; }
int obca_parking_constraints_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const double XYb[4], int fixTime,
                                   const double *x0, const double *xF, const int *nOb, const int *vOb, const double *A, const double *b, int dist,
                                   const double *x, const double *u, const double *timeScale, const double *l, const double *n, const double *sl,
                                   double tol, int *ok, int *ref_ok, double *viol) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_constraints_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !XYb || !x0 || !xF || !nOb || !vOb || !A || !b || !x || !u || !timeScale || !l || !n || !ok) { ctx->err = "obca_parking_constraints_batch: NULL argument"; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: no check reads it
    ParkIn in = {Ts, L, ego, XYb, fixTime, x0, xF, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, l, n, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    const double tl = tol > 0 ? tol : PV_REF_TOL;
    return parking_chunks(ctx, dist, B, N, in, [&](obca_batch *bt, int lo) { return batch_validate_range(bt, timeScale, sl, tl, lo, ok, ref_ok, viol); });
}

int obca_batch_clearance(obca_batch *bt, int substeps, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_batch_clearance: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { bt->ctx->err = std::string("obca_batch_clearance: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_clearance: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_clearance: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_clearance_range(bt, false, nullptr, substeps, need, 0, out));
}
int obca_batch_clearance_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->clr.ev, ms, "obca_batch_clearance_ms: no clearance call has run on this batch") : -1; }
int obca_parking_clearance_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                                 const double *x, const double *u, const double *timeScale, int substeps, double need, double *out) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_clearance_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out) { ctx->err = "obca_parking_clearance_batch: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { ctx->err = std::string("obca_parking_clearance_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the check does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_clearance_range(bt, true, timeScale, substeps, need, lo, out); });
}

int obca_batch_predict_clearance(obca_batch *bt, const double *rates, int substeps, double need, int keep_profile, double *out) {
    if (!bt) return -1;
    if (!out || !rates) { bt->ctx->err = "obca_batch_predict_clearance: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { bt->ctx->err = std::string("obca_batch_predict_clearance: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_predict_clearance: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_predict_clearance: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_predict_range(bt, false, nullptr, rates, substeps, need, keep_profile != 0, 0, out, nullptr));
}
int obca_batch_predict_clearance_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->prd.ev, ms, "obca_batch_predict_clearance_ms: no predict call has run on this batch") : -1; }
int obca_batch_predict_profile(obca_batch *bt, double *out, int capacity) { return bt ? predict_fetch(bt, out, capacity, "obca_batch_predict_profile") : -1; }
int obca_parking_predict_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, int substeps, double need, double *out, const double *rates, double *profile) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_predict_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out || !rates) { ctx->err = "obca_parking_predict_batch: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { ctx->err = std::string("obca_parking_predict_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the check does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_predict_range(bt, true, timeScale, rates, substeps, need, profile != nullptr, lo, out, profile); });
}

int obca_batch_rollout(obca_batch *bt, int substeps, int restart, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_batch_rollout: NULL argument"; return -1; }
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { bt->ctx->err = std::string("obca_batch_rollout: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_rollout: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_rollout: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_rollout_range(bt, false, nullptr, substeps, restart, need, 0, out, nullptr));
}
int obca_batch_rollout_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->rol.ev, ms, "obca_batch_rollout_ms: no rollout has run on this batch") : -1; }
int obca_batch_rollout_states(obca_batch *bt, double *X) { return bt ? rollout_states(bt, 4, X, "obca_batch_rollout_states") : -1; }
int obca_parking_rollout_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, int substeps, int restart, double need, double *out, double *X) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_rollout_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out) { ctx->err = "obca_parking_rollout_batch: NULL argument"; return -1; }
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { ctx->err = std::string("obca_parking_rollout_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the call does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_rollout_range(bt, true, timeScale, substeps, restart, need, lo, out, X); });
}

int obca_batch_track(obca_batch *bt, int substeps, int feedback, int clamp, const double q[4], const double r[2], const double qf[4], const double *dx0, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_batch_track: NULL argument"; return -1; }
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, 4, 2, need)) { bt->ctx->err = std::string("obca_batch_track: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_track: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_track: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_track_range(bt, false, nullptr, substeps, feedback, clamp, trk::make_weights(q, r, qf, 4, 2), dx0, need, 0, out, nullptr, nullptr));
}
int obca_batch_track_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->trk.ev, ms, "obca_batch_track_ms: no track call has run on this batch") : -1; }
int obca_batch_track_states(obca_batch *bt, double *X) { return bt ? track_fetch(bt, 4, 2, false, X, "obca_batch_track_states") : -1; }
int obca_batch_track_gains(obca_batch *bt, double *K) { return bt ? track_fetch(bt, 4, 2, true, K, "obca_batch_track_gains") : -1; }
int obca_parking_track_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                             const double *x, const double *u, const double *timeScale, int substeps, int feedback, int clamp, const double q[4], const double r[2], const double qf[4],
                             const double *dx0, double need, double *out, double *X, double *K) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_track_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out) { ctx->err = "obca_parking_track_batch: NULL argument"; return -1; }
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, 4, 2, need)) { ctx->err = std::string("obca_parking_track_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the call does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    const trk::Weights w = trk::make_weights(q, r, qf, 4, 2);
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_track_range(bt, true, timeScale, substeps, feedback, clamp, w, dx0, need, lo, out, X, K); });
}

int obca_batch_ensemble(obca_batch *bt, int substeps, int members, int feedback, int clamp, const double q[4], const double r[2], const double qf[4], const double *dx0, const double *dub, double need,
                        double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_batch_ensemble: NULL argument"; return -1; }
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, 4, 2, need)) { bt->ctx->err = std::string("obca_batch_ensemble: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_ensemble: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_ensemble: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_ensemble_range(bt, false, nullptr, substeps, members, feedback, clamp, trk::make_weights(q, r, qf, 4, 2), dx0, dub, need, 0, out, nullptr, nullptr));
}
int obca_batch_ensemble_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->ens.ev, ms, "obca_batch_ensemble_ms: no ensemble call has run on this batch") : -1; }
int obca_batch_ensemble_members(obca_batch *bt, double *mem) { return bt ? ensemble_fetch(bt, 4, false, mem, "obca_batch_ensemble_members") : -1; }
int obca_batch_ensemble_final(obca_batch *bt, double *fin) { return bt ? ensemble_fetch(bt, 4, true, fin, "obca_batch_ensemble_final") : -1; }
int obca_parking_ensemble_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                                const double *x, const double *u, const double *timeScale, int substeps, int members, int feedback, int clamp, const double q[4], const double r[2], const double qf[4],
                                const double *dx0, const double *dub, double need, double *out, double *mem, double *fin) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_ensemble_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out) { ctx->err = "obca_parking_ensemble_batch: NULL argument"; return -1; }
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, 4, 2, need)) { ctx->err = std::string("obca_parking_ensemble_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the call does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    const trk::Weights w = trk::make_weights(q, r, qf, 4, 2);
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_ensemble_range(bt, true, timeScale, substeps, members, feedback, clamp, w, dx0, dub, need, lo, out, mem, fin); });
}

int obca_batch_advance(obca_batch *bt, int shift, int substeps, const double *kick, double need, double *out) {
    if (!bt) return -1;
    if (int rc = advance_refuse(bt, "obca_batch_advance", shift, substeps, need, out)) return rc;
    const int rc = batch_advance_run(bt, shift, substeps, kick, need, out);
    if (!rc) bt->have_duals = 1;                        // the shifted multipliers are the dual warm start: DualMultWS is skipped
    return fin(bt, rc);
}
int obca_batch_advance_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->adv.ev, ms, "obca_batch_advance_ms: no advance has run on this batch") : -1; }
int obca_batch_advance_state(obca_batch *bt, double *X) { return bt ? advance_state(bt, 4, X, "obca_batch_advance_state") : -1; }
int obca_batch_advance_log(obca_batch *bt, int capacity_nodes) { return bt ? advance_log(bt, 4, capacity_nodes, "obca_batch_advance_log") : -1; }
int obca_batch_advance_log_states(obca_batch *bt, double *X, int *nodes) { return bt ? advance_log_states(bt, 4, X, nodes, "obca_batch_advance_log_states") : -1; }

// obca_scene_edit.h.  The motions are staged through the call's own pinned and device buffers (bt->mov), SE_PIN doubles per obstacle in rows of nObMax obstacles; the
// kernel edits d.prob in place.  Nothing of the host's state describes the geometry: h_prob is staging, rowLen / vmx / vmax / nOb / M hold lengths and counts, which stand.
int obca_batch_move_obstacles(obca_batch *bt, const double *motion, const double *pivot, const double *inflate, int *status) {
    if (!bt) return -1;
    if (!status) { bt->ctx->err = "obca_batch_move_obstacles: NULL argument"; return -1; }
    if (!bt->uploaded) { bt->ctx->err = "obca_batch_move_obstacles: nothing uploaded"; return -1; }
    const int B = bt->B; const size_t s_in = (size_t)SE_PIN * bt->nObMax;
    return fin(bt, run_validate(bt, bt->mov, s_in, true, 1, [&](int i, double *a) {
        memset(a, 0, sizeof(double) * s_in);
        const size_t o = (size_t)(bt->obOff[i] - bt->obOff[0]);
        for (int j = 0; j < bt->nOb[i]; j++) {
            double *m = a + SE_PIN * j;
            if (motion) { m[0] = motion[3 * (o + j)]; m[1] = motion[3 * (o + j) + 1]; m[2] = motion[3 * (o + j) + 2]; }
            if (pivot) { m[3] = pivot[2 * (o + j)]; m[4] = pivot[2 * (o + j) + 1]; }
            if (inflate) m[5] = inflate[o + j];
        }
    }, [&] {
        hipLaunchKernelGGL(obca_move_parking_kernel, dim3(B), dim3(OB_NT), 0, bt->stream, B, bt->d.prob, bt->d.s_prob, (const double *)bt->mov.d_in, s_in, (double *)bt->mov.d_out);
    }, [&](int i, const double *o) { status[i] = o[0] != 0.0; }));
}
int obca_batch_move_obstacles_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->mov.ev, ms, "obca_batch_move_obstacles_ms: no move call has run on this batch") : -1; }
int obca_batch_obstacles_download(obca_batch *bt, double *A, double *b) {
    if (!bt) return -1;
    if (!A && !b) { bt->ctx->err = "obca_batch_obstacles_download: NULL arguments"; return -1; }
    if (!bt->uploaded) { bt->ctx->err = "obca_batch_obstacles_download: nothing uploaded"; return -1; }
    const DevBufs &d = bt->d; const size_t B = bt->B;
    use_device(bt->device);
    // through the pinned problem staging of the batch (an upload refills it): the records as they lie
    if (bt->h_prob.reserve(bt->err, (size_t)bt->cap * d.s_prob)) return fin(bt, -2);
    if (hipMemcpyAsync(bt->h_prob, d.prob, B * d.s_prob * sizeof(double), hipMemcpyDeviceToHost, bt->stream) != hipSuccess || hipStreamSynchronize(bt->stream) != hipSuccess) {
        bt->ctx->err = "obca_batch_obstacles_download: copy failed"; return -2;
    }
    for (size_t i = 0; i < B; i++) {
        const double *p = bt->h_prob + i * d.s_prob; const size_t r0 = (size_t)(bt->rowOff[i] - bt->rowOff[0]), m = (size_t)bt->M[i];
        if (A) memcpy(A + 2 * r0, p + PH_A, sizeof(double) * 2 * m);
        if (b) memcpy(b + r0, p + PH_B, sizeof(double) * m);
    }
    return 0;
}

int obca_batch_certify(obca_batch *bt, double need, double slack, int max_steps, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_batch_certify: NULL argument"; return -1; }
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { bt->ctx->err = std::string("obca_batch_certify: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_batch_certify: nothing has been solved since the last upload or shift"; return -1; }
    if (bt->N < 1) { bt->ctx->err = "obca_batch_certify: needs a horizon N>=1"; return -1; }
    return fin(bt, batch_certify_range(bt, false, nullptr, need, slack, max_steps, 0, out, nullptr));
}
int obca_batch_certify_ms(obca_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->cer.ev, ms, "obca_batch_certify_ms: no certify call has run on this batch") : -1; }
int obca_batch_certify_intervals(obca_batch *bt, double *iv) { return bt ? certify_fetch(bt, iv, "obca_batch_certify_intervals") : -1; }
int obca_parking_certify_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, double need, double slack, int max_steps, double *out, double *iv) {
    if (!ctx) return -1;
    if (B < 1 || N < 1 || N > OBCA_NMAX) { ctx->err = "obca_parking_certify_batch: need B>=1, 1<=N<=OBCA_NMAX"; return -1; }
    if (!Ts || !ego || !nOb || !vOb || !A || !b || !x || !u || !out) { ctx->err = "obca_parking_certify_batch: NULL argument"; return -1; }
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { ctx->err = std::string("obca_parking_certify_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * (N + 1), 0.0);      // the tracking reference of a solve: the call does not read it (nor the bounds, the start and the goal)
    const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts, L, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, zero.data(), zero.data(), zero.data(), x, u, nullptr, nullptr, {}, {}};
    if (int rc = park_prefix(ctx->err, B, nOb, vOb, in)) return rc;
    return parking_chunks(ctx, 0, B, N, in, [&](obca_batch *bt, int lo) { return batch_certify_range(bt, true, timeScale, need, slack, max_steps, lo, out, iv); });
}

int obca_parking_signed_dist_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const double XYb[4],
                                   int fixTime, const double *x0, const double *xF, const int *nOb, const int *vOb, const double *A,
                                   const double *b, const double *rx, const double *ry, const double *ryaw, const double *xWS,
                                   const double *uWS, const double *lWS, const double *nWS, const obca_opts *opts, double *xp,
                                   double *up, double *timeScale, int *exitflag, double *lp, double *np, double *slp, double *info) {
    if (!ctx) return -1;
    if (!x0 || !xF || !xWS || !uWS) { ctx->err = "obca_parking_signed_dist_batch: NULL argument"; return -1; }
    ParkIn in = {Ts, L, ego, XYb, fixTime, x0, xF, nOb, vOb, A, b, rx, ry, ryaw, xWS, uWS, lWS, nWS, {}, {}};
    ParkOut o = {xp, up, timeScale, exitflag, lp, np, slp, info, nullptr, nullptr, nullptr};
    return parking_call(ctx, 0, 0, B, N, in, opts, o);
}
int obca_parking_dist_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4], const double XYb[4],
                            int fixTime, const double *x0, const double *xF, const int *nOb, const int *vOb, const double *A,
                            const double *b, const double *rx, const double *ry, const double *ryaw, const double *xWS,
                            const double *uWS, const double *lWS, const double *nWS, const obca_opts *opts, double *xp,
                            double *up, double *timeScale, int *exitflag, double *lp, double *np, double *info) {
    if (!ctx) return -1;
    if (!x0 || !xF || !xWS || !uWS) { ctx->err = "obca_parking_dist_batch: NULL argument"; return -1; }
    ParkIn in = {Ts, L, ego, XYb, fixTime, x0, xF, nOb, vOb, A, b, rx, ry, ryaw, xWS, uWS, lWS, nWS, {}, {}};
    ParkOut o = {xp, up, timeScale, exitflag, lp, np, nullptr, info, nullptr, nullptr, nullptr};
    return parking_call(ctx, 1, 0, B, N, in, opts, o);
}

int obca_dualmult_ws_batch(obca_ctx *ctx, int B, int N, const double ego[4], const int *nOb, const int *vOb, const double *A,
                           const double *b, const double *rx, const double *ry, const double *ryaw, double *lWS, double *nWS, double *dd) {
    if (!ctx) return -1;
    if (!lWS || !nWS) { ctx->err = "obca_dualmult_ws_batch: NULL output"; return -1; }
    if (B < 1) { ctx->err = "obca_dualmult_ws_batch: need B>=1"; return -1; }
    std::vector<double> Ts(B, 1.0); const double XYb[4] = {0, 0, 0, 0};
    ParkIn in = {Ts.data(), 1.0, ego, XYb, 0, nullptr, nullptr, nOb, vOb, A, b, rx, ry, ryaw, nullptr, nullptr, nullptr, nullptr, {}, {}};
    ParkOut o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lWS, nWS, dd};
    return parking_call(ctx, 0, 1, B, N, in, nullptr, o);
}

}  // extern "C"

// ---- one kernel between the events of `ev`, then the copies of `down` to the host, then the stream is synchronised: the launch of every call that stages through a KernelStage
// and of the planner.  `ok`: what the caller queued before (its upload) went through -- nothing is launched behind a failed copy; `entry` names the entry point in the error.
struct Down { void *dst; const void *src; size_t bytes; };
template <typename Launch>
static int launch_timed(std::string &err, const char *entry, hipStream_t stream, EventPair &ev, bool ok, Launch &&launch, std::initializer_list<Down> down) {
    ok = ok && ev.begin(stream) == hipSuccess;
    if (ok) launch();
    ok = ok && hipGetLastError() == hipSuccess && ev.end(stream) == hipSuccess;
    for (const Down &c : down) ok = ok && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (hipStreamSynchronize(stream) != hipSuccess || !ok) { err = std::string(entry) + ": kernel or copy failed"; return -2; }
    ev.timed = 1;
    return 0;
}

// ---- warm starts from planner paths (obca_path_ws.h, include/obca_path_ws.h)
// What both calls send up, packed on the host into the pinned mirror so that ONE contiguous transfer carries it and only the rows below the longest usable count of the
// call cross the bus: doubles [ paths B x rows x 3 | xF 4 x B (host-pointer call) ], then ints [ dirs B x rows | counts B ]; behind them, device only, [ status B ] and
// `out_doubles` of output.  Device pointers in `d`.
struct PathWsDev { const double *paths, *xF; const int *dirs, *counts; int *status; double *out; int rows; };
static int path_ws_stage(std::string &err, KernelStage &w, hipStream_t stream, int B, const double *paths, const int *dirs, const int *counts, int cap, const double *xF,
                         size_t out_doubles, PathWsDev &d) {
    int rows = 0;
    for (int i = 0; i < B; i++) if (!pw::path_ws_count_status(counts[i], cap)) rows = std::max(rows, counts[i]);
    const size_t np = (size_t)B * rows * 3, nd = np + (xF ? (size_t)B * 4 : 0), ni = (size_t)B * rows + B, up = nd + (ni + 1) / 2, st = (ni + B + 1) / 2;
    if (int rc = w.ev.ensure(err)) return rc;
    if (w.dev.reserve(nd + st + out_doubles, stream) != hipSuccess) { err = "hipMalloc(path warm start) failed"; return -2; }
    if (w.host.reserve(err, up)) return -2;
    double *h = w.host; int *hi = (int *)(h + nd);
    for (int i = 0; i < B; i++) {
        const int c = pw::path_ws_count_status(counts[i], cap) ? 0 : counts[i];      // nothing of an instance without a usable path is read
        memcpy(h + (size_t)i * rows * 3, paths + (size_t)i * cap * 3, sizeof(double) * 3 * c);
        memset(h + (size_t)i * rows * 3 + 3 * (size_t)c, 0, sizeof(double) * 3 * (rows - c));
        memcpy(hi + (size_t)i * rows, dirs + (size_t)i * cap, sizeof(int) * c);
        memset(hi + (size_t)i * rows + c, 0, sizeof(int) * (rows - c));
    }
    if (xF) memcpy(h + np, xF, sizeof(double) * 4 * B);
    memcpy(hi + (size_t)B * rows, counts, sizeof(int) * B);
    if (hipMemcpyAsync(w.dev, w.host, nd * sizeof(double) + ni * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) { err = "path warm start: H2D failed"; return -2; }
    double *dv = w.dev; int *di = (int *)(dv + nd);
    d.paths = dv; d.xF = xF ? dv + np : nullptr; d.dirs = di; d.counts = di + (size_t)B * rows; d.status = di + ni; d.out = dv + nd + st; d.rows = rows;
    return 0;
}

extern "C" {

int obca_parking_path_warm_start_batch(obca_ctx *ctx, int B, int N, const double *paths, const int *dirs, const int *counts, int cap, const double *xF,
                                       double v_nom, double L, double a_max, double *Ts, double *xWS, double *uWS, int *status) {
    if (!ctx) return -1;
    if (const char *bad = pw::path_ws_check_args(B, N, cap, v_nom, L, a_max, paths && dirs && counts && Ts && xWS && uWS && status)) {
        ctx->err = std::string("obca_parking_path_warm_start_batch: ") + bad; return -1;
    }
    use_device(ctx->device);
    const size_t nx = (size_t)B * 4 * (N + 1), nu = (size_t)B * 2 * N;
    PathWsDev d;
    if (int rc = path_ws_stage(ctx->err, ctx->pw, ctx->stream, B, paths, dirs, counts, cap, xF, (size_t)B + nx + nu, d)) return rc;
    double *dTs = d.out, *dx = d.out + B, *du = d.out + B + nx;
    return launch_timed(ctx->err, "obca_parking_path_warm_start_batch", ctx->stream, ctx->pw.ev, true, [&] {
        hipLaunchKernelGGL(obca_path_ws_host_kernel, dim3(B), dim3(OB_NT), 0, ctx->stream, B, N, d.paths, d.dirs, d.counts, d.rows, cap, d.xF, v_nom, L, a_max, dTs, dx, du, d.status);
    }, {{Ts, dTs, (size_t)B * sizeof(double)}, {xWS, dx, nx * sizeof(double)}, {uWS, du, nu * sizeof(double)}, {status, d.status, (size_t)B * sizeof(int)}});
}

int obca_batch_set_path_warm_start(obca_batch *bt, const double *paths, const int *dirs, const int *counts, int cap, int use_xF, double v_nom, double a_max, int *status) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    if (!bt->uploaded) { ctx->err = "obca_batch_set_path_warm_start: nothing uploaded"; return -1; }
    if (const char *bad = pw::path_ws_check_args(bt->B, bt->N, cap, v_nom, 1.0, a_max, paths && dirs && counts && status)) {
        ctx->err = std::string("obca_batch_set_path_warm_start: ") + bad; return -1;
    }
    use_device(bt->device);
    PathWsDev d;
    if (int rc = path_ws_stage(bt->err, bt->pw, bt->stream, bt->B, paths, dirs, counts, cap, nullptr, 0, d)) return fin(bt, rc);
    // from here on the record and the start iterate may be rewritten, whatever becomes of the call: d.z no longer answers the problem, and the start's multipliers
    // count as cleared -- the next solve runs DualMultWS
    bt->solved = 0; bt->have_duals = 0;
    return launch_timed(ctx->err, "obca_batch_set_path_warm_start", bt->stream, bt->pw.ev, true, [&] {
        hipLaunchKernelGGL(obca_path_ws_batch_kernel, dim3(bt->B), dim3(OB_NT), 0, bt->stream, bt->B, bt->N, d.paths, d.dirs, d.counts, d.rows, cap, use_xF ? 1 : 0, v_nom, a_max, bt->d, d.status);
    }, {{status, d.status, (size_t)bt->B * sizeof(int)}});
}

int obca_batch_path_ws_ms(obca_batch *bt, float *ms) {
    return bt && ms ? core_elapsed_ms(bt->ctx, bt->pw.ev, ms, "obca_batch_path_ws_ms: no path warm start has run on this batch") : -1;
}

}  // extern "C"

// ---- solved batches on a finer horizon (obca_refine.h, include/obca_refine.h)
// What obca_batch_refine_into and obca_quad_batch_subdivide_into share: a selection of a solved batch, rewritten by a kernel into a second batch of the context.  Checks the two
// batches and the selection (`unsolved`: the family's text for a source without a solution, `bad_args`: what the family's check of (n, N, factor, ...) said), runs prepare()
// -- the host side of the destination --, stages the selection in `w` (dst->rf or dst->sd) as ints [ sel cap | status cap ], runs launch(sel, status) on the destination's
// stream and brings the status words back.  The destination counts as not uploaded until the kernel has written every record.
template <typename BT, typename Prepare, typename Launch>
static int into_call(const char *entry, BT *dst, BT *src, KernelStage &w, int factor, const char *unsolved, const char *bad_args, const int *sel, int n, int *status,
                     Prepare &&prepare /* int() */, Launch &&launch /* (const int *sel, int *status): device pointers */) {
    obca_ctx *ctx = dst->ctx;
    const char *bad = nullptr;
    if (!status) bad = "NULL argument";
    else if (dst == src || dst->ctx != src->ctx || dst->stream != src->stream) bad = "source and destination must be two batches of one context";
    else if (!src->uploaded || !src->solved) bad = unsolved;
    else if (bad_args) bad = bad_args;
    else if (dst->N != factor * src->N) bad = "the destination's horizon must be factor * the source's";
    else if (n > dst->cap) bad = "more instances than the destination was created for";
    for (int j = 0; !bad && sel && j < n; j++) if (sel[j] < 0 || sel[j] >= src->B) bad = "an index outside 0 .. B - 1 of the source";
    if (!bad && !sel && n > src->B) bad = "an index outside 0 .. B - 1 of the source";
    if (bad) { ctx->err = std::string(entry) + ": " + bad; return -1; }
    use_device(dst->device);
    if (int rc = prepare()) return fin(dst, rc);
    if (int rc = w.ev.ensure(dst->err)) return fin(dst, rc);
    if (w.dev.reserve((size_t)dst->cap + 1, dst->stream) != hipSuccess) { ctx->err = std::string(entry) + ": hipMalloc failed"; return -2; }
    if (w.host.reserve(dst->err, ((size_t)dst->cap + 1) / 2 + 1)) return fin(dst, -2);
    int *hs = (int *)w.host.p, *dsel = (int *)w.dev.p, *dst_st = dsel + dst->cap;
    dst->uploaded = 0;      // until the kernel has written every record (and, for a parking batch, every row)
    for (int j = 0; j < n; j++) hs[j] = sel ? sel[j] : j;
    const bool up = hipMemcpyAsync(dsel, hs, (size_t)n * sizeof(int), hipMemcpyHostToDevice, dst->stream) == hipSuccess;
    const int rc = launch_timed(ctx->err, entry, dst->stream, w.ev, up, [&] { launch((const int *)dsel, dst_st); }, {{status, dst_st, (size_t)n * sizeof(int)}});
    if (!rc) dst->uploaded = 1;
    return rc;
}

extern "C" {

int obca_batch_refine_into(obca_batch *dst, obca_batch *src, int factor, int duals, const int *sel, int n, int *status) {
    if (!dst || !src) return -1;
    return into_call("obca_batch_refine_into", dst, src, dst->rf, factor, "nothing has been solved on the source since its last upload, shift or path warm start",
                     rfn::refine_check_args(n, src->N, factor, duals), sel, n, status, [&] {
        // the host records of the selection, in its order: the packed outputs of a later download follow the running sums, lambda goes back through the source's row lengths
        dst->B = n; dst->solved = 0; dst->val_rl = 0;
        dst->nOb.assign(n, 0); dst->M.assign(n, 0); dst->obOff.assign(n + 1, 0); dst->rowOff.assign(n + 1, 0); dst->vmx.assign(n, 0); dst->rowLen.clear();
        int nObMax = 0, MMax = 0; dst->vmax = 0;
        for (int j = 0; j < n; j++) {
            const int i = sel ? sel[j] : j;
            dst->nOb[j] = src->nOb[i]; dst->M[j] = src->M[i]; dst->vmx[j] = src->vmx[i];
            dst->obOff[j + 1] = dst->obOff[j] + dst->nOb[j]; dst->rowOff[j + 1] = dst->rowOff[j] + dst->M[j];
            const double *rl = src->rowLen.data() + (src->rowOff[i] - src->rowOff[0]);
            dst->rowLen.insert(dst->rowLen.end(), rl, rl + src->M[i]);
            nObMax = std::max(nObMax, dst->nOb[j]); MMax = std::max(MMax, dst->M[j]); dst->vmax = std::max(dst->vmax, dst->vmx[j]);
        }
        dst->dist = src->dist; dst->fixTime = src->fixTime; dst->have_duals = duals; dst->have_geo = 0;
        return batch_reserve_shape(dst, nObMax, MMax);
    }, [&](const int *dsel, int *dstatus) {
        hipLaunchKernelGGL(obca_refine_batch_kernel, dim3(n), dim3(OB_NT), 0, dst->stream, n, src->N, factor, duals, dsel, src->d, dst->d, dstatus);
    });
}

int obca_batch_refine_ms(obca_batch *dst, float *ms) {
    return dst && ms ? core_elapsed_ms(dst->ctx, dst->rf.ev, ms, "obca_batch_refine_ms: no refine call has written into this batch") : -1;
}

int obca_parking_refine_batch(obca_ctx *ctx, int B, int N, int factor, const double *Ts, double L, const double *x, const double *u, const double *timeScale,
                              double *Ts_f, double *x_f, double *u_f) {
    if (!ctx) return -1;
    const char *bad = rfn::refine_check_args(B, N, factor, 0);
    if (!bad && !(Ts && x && u && Ts_f && x_f && u_f)) bad = "NULL argument";
    if (bad) { ctx->err = std::string("obca_parking_refine_batch: ") + bad; return -1; }
    use_device(ctx->device);
    KernelStage &w = ctx->rf;
    if (int rc = w.ev.ensure(ctx->err)) return rc;
    const size_t Nf = (size_t)N * factor, nx = (size_t)B * 4 * (N + 1), nu = (size_t)B * 2 * N, nt = timeScale ? (size_t)B * (N + 1) : 0, nin = B + nx + nu + nt;
    const size_t nxf = (size_t)B * 4 * (Nf + 1), nuf = (size_t)B * 2 * Nf;
    if (w.dev.reserve(nin + B + nxf + nuf, ctx->stream) != hipSuccess) { ctx->err = "obca_parking_refine_batch: hipMalloc failed"; return -2; }
    if (w.host.reserve(ctx->err, nin)) return -2;
    double *h = w.host, *d = w.dev;      // one contiguous transfer up: [ Ts B | x | u | timeScale ]
    memcpy(h, Ts, sizeof(double) * B); memcpy(h + B, x, sizeof(double) * nx); memcpy(h + B + nx, u, sizeof(double) * nu);
    if (nt) memcpy(h + B + nx + nu, timeScale, sizeof(double) * nt);
    double *dTsf = d + nin, *dxf = dTsf + B, *duf = dxf + nxf;
    const bool up = hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    return launch_timed(ctx->err, "obca_parking_refine_batch", ctx->stream, w.ev, up, [&] {
        hipLaunchKernelGGL(obca_refine_host_kernel, dim3(B), dim3(OB_NT), 0, ctx->stream, B, N, factor, (const double *)d, L, (const double *)(d + B), (const double *)(d + B + nx),
                           (const double *)(nt ? d + B + nx + nu : nullptr), dTsf, dxf, duf);
    }, {{Ts_f, dTsf, (size_t)B * sizeof(double)}, {x_f, dxf, nxf * sizeof(double)}, {u_f, duf, nuf * sizeof(double)}});
}

}  // extern "C"

/* ---------------------------------------------------------------- quadcopter path */
static void free_dev(obca_quad_batch *bt) {
    double **ps[] = {&bt->d.prob, &bt->d.z, &bt->d.d, &bt->d.as, &bt->d.rs, &bt->d.oc, &bt->d.info, &bt->d.prof};
    for (auto p : ps) { if (*p) (void)hipFree(*p); *p = nullptr; }
    bt->stage.release();
}
static int batch_create_on(obca_ctx *ctx, int device, hipStream_t stream, int B, int N, obca_quad_batch **out, std::string &err) {
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { err = "obca_quad_batch_create: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    obca_quad_batch *bt = new obca_quad_batch(ctx, device, stream, B, N);
    use_device(device);
    quad::QLay l; quad::q_make_layout(N, l);
    QDevBufs &d = bt->d; const size_t N1 = N + 1;
    d.s_prob = QPH_SIZE + QX * N1; d.s_z = l.len; d.s_d = QDIR_DOUBLES(l);
         /* two direction buffers (dv | dy) + the rows of a second-order correction, see QCS */ d.s_as = N1 * QSP; d.s_rs = N1 * QRR; d.s_oc = N1 * QOB * OB_OC;
    size_t tot = 0;
#define ALLOC(ptr, cnt) do { size_t by_ = (size_t)(cnt) * sizeof(double); if (dev_alloc((void **)&(ptr), by_, stream) != hipSuccess) { err = "obca_quad_batch_create: hipMalloc failed"; free_dev(bt); delete bt; return -2; } tot += by_; } while (0)
    ALLOC(d.prob, B * d.s_prob); ALLOC(d.z, B * d.s_z); ALLOC(d.d, B * d.s_d); ALLOC(d.as, B * d.s_as); ALLOC(d.rs, B * d.s_rs);
    ALLOC(d.oc, B * d.s_oc); ALLOC(d.info, (size_t)B * 8); ALLOC(d.prof, (size_t)B * 16);
#undef ALLOC
    if (bt->stage.reserve((size_t)B * l.so, stream) != hipSuccess) { err = "obca_quad_batch_create: hipMalloc failed"; free_dev(bt); delete bt; return -2; }
    bt->bytes = (long long)(tot + bt->stage.cap * sizeof(double));
    if (hipEventCreate(&bt->e0) != hipSuccess || hipEventCreate(&bt->e1) != hipSuccess) { err = "hipEventCreate failed"; free_dev(bt); delete bt; return -2; }
    *out = bt;
    return 0;
}
struct QuadIn { const double *Ts; double R; const double *x0, *xF, *ob, *xWS, *timeWS; int dual_ws, dist; };
struct QuadOut { double *xp, *up, *ts; int *exitflag; double *lp, *slp, *info; };
static int quad_upload_range(obca_quad_batch *bt, const QuadIn &in, int lo, int n) {
    if (n < 1 || n > bt->cap) { bt->err = "obca_quad_batch_upload: more instances than the batch was created for"; return -1; }
    bt->B = n; bt->solved = 0; bt->adv_n = 0;      // (an upload empties the log of obca_advance.h)
    const int N1 = bt->N + 1; const QDevBufs &d = bt->d;
    if (bt->h_prob.reserve(bt->err, (size_t)bt->cap * d.s_prob)) return -2;
    for (int i = 0; i < n; i++) {
        const size_t g = (size_t)lo + i;
        double *p = bt->h_prob + (size_t)i * d.s_prob;
        memset(p, 0, sizeof(double) * QPH_SIZE);
        p[QPH_TS] = in.Ts[g]; p[QPH_R] = in.R; p[QPH_TWS] = in.timeWS[g]; p[QPH_DWS] = in.dual_ws ? 1.0 : 0.0; p[QPH_DIST] = in.dist ? 1.0 : 0.0;
        memcpy(p + QPH_X0, in.x0 + QX * g, sizeof(double) * QX); memcpy(p + QPH_XF, in.xF + QX * g, sizeof(double) * QX);
        memcpy(p + QPH_OB, in.ob + (size_t)QOB * QL * g, sizeof(double) * QOB * QL);
        memcpy(p + QPH_SIZE, in.xWS + (size_t)QX * N1 * g, sizeof(double) * QX * N1);
    }
    use_device(bt->device);
    HIPCHK(bt, hipMemcpyAsync(d.prob, bt->h_prob, (size_t)n * d.s_prob * sizeof(double), hipMemcpyHostToDevice, bt->stream));
    bt->uploaded = 1;
    return 0;
}
static int quad_solve(obca_quad_batch *bt, const obca_opts *opts);
static int quad_download_range(obca_quad_batch *bt, const QuadOut &o, int lo) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    use_device(bt->device);
    const size_t W = (size_t)l.so;                          // outputs are a prefix of the iterate: x, u, t, lam, s
    if (bt->h_z.reserve(bt->err, (size_t)bt->cap * W) || bt->h_info.reserve(bt->err, (size_t)bt->cap * 8)) return -2;
    hipLaunchKernelGGL(obca_gather_rows_kernel, dim3(B, (unsigned)((W + 1023) / 1024)), dim3(256), 0, bt->stream, bt->stage, W, (const double *)d.z, d.s_z);
    HIPCHK(bt, hipGetLastError());
    HIPCHK(bt, hipMemcpyAsync(bt->h_z, bt->stage, (size_t)B * W * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
    HIPCHK(bt, hipMemcpyAsync(bt->h_info, d.info, (size_t)B * 8 * sizeof(double), hipMemcpyDeviceToHost, bt->stream));
    HIPCHK(bt, hipStreamSynchronize(bt->stream));
    for (int i = 0; i < B; i++) {
        const size_t g = (size_t)lo + i;
        const double *z = bt->h_z + (size_t)i * W;
        if (o.xp) memcpy(o.xp + g * QX * N1, z + l.x, sizeof(double) * QX * N1);
        if (o.up) memcpy(o.up + g * QU * N, z + l.u, sizeof(double) * QU * N);
        if (o.ts) for (int k = 0; k < N1; k++) o.ts[g * N1 + k] = z[l.t];                                 /* QuadcopterSignedDist.jl:293 */
        if (o.lp) memcpy(o.lp + g * QL * QOB * N1, z + l.lam, sizeof(double) * QL * QOB * N1);            /* [l1;..;l5] stacked, :295 */
        if (o.slp) memcpy(o.slp + g * QOB * N1, z + l.s, sizeof(double) * QOB * N1);
        if (o.exitflag) o.exitflag[g] = (int)bt->h_info[(size_t)i * 8 + 7];
        if (o.info) memcpy(o.info + g * 8, bt->h_info + (size_t)i * 8, sizeof(double) * 8);
    }
    return 0;
}

extern "C" {

int obca_quadcopter_default_opts(obca_opts *o) {
    if (obca_default_opts(o)) return -1;
    o->max_iter = 3000; o->dw_min = 1e-10;            /* QuadcopterSignedDist.jl:28-31: no max_iter (IPOPT default), min_hessian_perturbation 1e-10 */
    return 0;
}
int obca_quadcopter_reference_opts(obca_opts *o) {
    if (obca_quadcopter_default_opts(o)) return -1;
    o->max_soc = 4;                                    /* IPOPT default max_soc; recalc_y stays 0: QuadcopterSignedDist.jl:29 sets recalc_y = "no" */
    o->lsq_init = 1;                                   /* IPOPT default: least-squares initial multipliers, constr_mult_init_max = 1e3 */
    o->obj_scaling = 1;                                /* IPOPT default: gradient-based scaling; on this NLP it is the objective factor 100 / 2 100 */
    return 0;
}
int obca_quad_batch_create(obca_ctx *ctx, int B, int N, obca_quad_batch **out) {
    if (!ctx || !out) return -1;
    return batch_create_on(ctx, ctx->device, ctx->stream, B, N, out, ctx->err);
}
int obca_quad_batch_destroy(obca_quad_batch *bt) {
    if (!bt) return -1;
    use_device(bt->device);
    free_dev(bt); core_release(bt); bt->h_z.release(); bt->sd.release(); bt->gp.release(); bt->gp_paths.release();
    delete bt; return 0;
}
#ifdef OBCA_PROFILE
int obca_quad_batch_debug_phase_cycles(obca_quad_batch *bt, double *out) { return bt ? core_phase_cycles(bt, bt->d.prof, out, "obca_quad_batch_debug_phase_cycles: copy failed") : -1; }
#endif
int obca_quad_batch_scratch_bytes(const obca_quad_batch *bt, long long *bytes) { return core_scratch_bytes(bt, bytes); }
int obca_quad_batch_upload(obca_quad_batch *bt, const double *Ts, double R, const double *x0, const double *xF, const double *ob,
                           const double *xWS, const double *timeWS, int dual_ws, int dist) {
    if (!bt) return -1;
    if (!Ts || !x0 || !xF || !ob || !xWS || !timeWS) { bt->ctx->err = "obca_quad_batch_upload: NULL argument"; return -1; }
    QuadIn in = {Ts, R, x0, xF, ob, xWS, timeWS, dual_ws, dist};
    int rc = quad_upload_range(bt, in, 0, bt->cap);
    if (!rc && hipStreamSynchronize(bt->stream) != hipSuccess) { bt->err = "obca_quad_batch_upload: stream sync failed"; rc = -2; }
    return fin(bt, rc);
}
}  // extern "C"
static int quad_solve(obca_quad_batch *bt, const obca_opts *opts) {
    if (!bt->uploaded) { bt->err = "obca_quad_batch_solve: nothing uploaded"; return -1; }
    obca_opts o; if (opts) o = *opts; else obca_quadcopter_default_opts(&o);
    if (o.max_soc < 0 || o.max_soc > 16) { bt->err = "opts.max_soc must be in 0 .. 16"; return -1; }
    if (o.restoration < 0 || o.restoration > 2) { bt->err = "opts.restoration must be 0, 1 or 2"; return -1; }
    if (o.recalc_y != 0) { bt->err = "quadcopter solve: recalc_y is a switch of the parking kernels only (the reference's quadcopter call sets recalc_y = \"no\", QuadcopterSignedDist.jl:29); the quadcopter kernel would ignore it -- refusing instead"; return -1; }
    Opts ko; memcpy(&ko, &o, sizeof ko);
    use_device(bt->device);
    HIPCHK(bt, hipEventRecord(bt->e0, bt->stream));
    hipLaunchKernelGGL(obca_quad_ipm_kernel, dim3(bt->B), dim3(QNT), (size_t)(bt->N + 2) * (QS + QU) * sizeof(double), bt->stream, bt->B, bt->N, bt->d, ko, o.max_soc, o.lsq_init != 0, o.obj_scaling != 0);
    HIPCHK(bt, hipGetLastError());
    HIPCHK(bt, hipEventRecord(bt->e1, bt->stream));
    bt->solved = 1;
    return 0;
}
// the quadcopter check of the batch's instances: resident (x == nullptr: the last solution in d.z) or a caller's trajectory (host arrays of the whole call, instance lo + i),
// which travels up densely packed as [ x | u | timeScale (N + 1) | lambda ] per instance.  Only QV_OUT doubles per instance come back.
static int quad_validate_range(obca_quad_batch *bt, const double *x, const double *u, const double *ts, const double *lam, double tol, int lo, int *ok, double *viol) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    const bool host = x != nullptr;
    const size_t nx = (size_t)QX * N1, nu = (size_t)QU * N, nl = (size_t)QL * QOB * N1, W = nx + nu + N1 + nl;
    quad::QLay l; quad::q_make_layout(N, l);
    return run_validate(bt, bt->val, host ? W : 0, host, QV_OUT, [&](int i, double *a) {
        const size_t g = (size_t)lo + i;
        memcpy(a, x + g * nx, sizeof(double) * nx); memcpy(a + nx, u + g * nu, sizeof(double) * nu);
        memcpy(a + nx + nu, ts + g * N1, sizeof(double) * N1); memcpy(a + nx + nu + N1, lam + g * nl, sizeof(double) * nl);
    }, [&] {
        if (host) hipLaunchKernelGGL(obca_validate_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)bt->val.d_in, W, 0, (int)nx, (int)(nx + nu), 1, (int)(nx + nu + N1), tol, bt->val.d_out);
        else hipLaunchKernelGGL(obca_validate_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.z, d.s_z, l.x, l.u, l.t, 0, l.lam, tol, bt->val.d_out);
    }, [&](int i, const double *o) {
        const size_t g = (size_t)lo + i;
        if (viol) memcpy(viol + g * QV_NCLS, o, sizeof(double) * QV_NCLS);
        if (ok) ok[g] = o[QV_NCLS] != 0.0;
    });
}
// the clearance of the batch's quadcopter instances between their nodes (obca_clearance.h): resident (ts == nullptr: the last solution in d.z, its one t) or a caller's trajectory
// that quad_upload_range has just put behind the problem header (the slot of the warm start), with ts: (N + 1) per instance of the call
static int quad_clearance_range(obca_quad_batch *bt, const double *ts, int S, double need, int lo, double *out) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    return run_validate(bt, bt->clr, ts ? (size_t)N1 : 0, ts != nullptr, CL_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        if (ts) hipLaunchKernelGGL(obca_clearance_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.prob + QPH_SIZE, d.s_prob, (const double *)bt->clr.d_in, (size_t)N1, 1, S, need, bt->clr.d_out);
        else hipLaunchKernelGGL(obca_clearance_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.z + l.x, d.s_z, (const double *)d.z + l.t, d.s_z, 0, S, need, bt->clr.d_out);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * CL_OUT, o, sizeof(double) * CL_OUT); });
}
// the prediction for the batch's quadcopter instances (obca_predict.h): quad_clearance_range with the rates (PR_QIN x 5 per instance of the call), whether a profile is kept
// and the caller's profile array; the rates and a host-pointer call's timeScale travel up as [ rates | timeScale (N + 1) ] per instance
static int quad_predict_range(obca_quad_batch *bt, const double *ts, const double *rates, int S, double need, bool keep, int lo, double *out, double *profile) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    if (int rc = predict_reserve(bt, S, keep)) return rc;
    const size_t s_rt = (size_t)PR_QIN * QOB, s_in = s_rt + (ts ? (size_t)N1 : 0), s_prof = (size_t)N * S + 1;
    const int rc = run_validate(bt, bt->prd, s_in, true, PR_OUT, [&](int i, double *a) {
        memcpy(a, rates + ((size_t)lo + i) * s_rt, sizeof(double) * s_rt);
        if (ts) memcpy(a + s_rt, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        const double *in = (const double *)bt->prd.d_in; double *prof = keep ? (double *)bt->prd_w : nullptr;
        if (ts) hipLaunchKernelGGL(obca_predict_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.prob + QPH_SIZE, d.s_prob, in + s_rt, s_in, 1,
                                   in, s_in, S, need, (double *)bt->prd.d_out, prof, s_prof);
        else hipLaunchKernelGGL(obca_predict_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.z + l.x, d.s_z, (const double *)d.z + l.t, d.s_z, 0,
                                in, s_in, S, need, (double *)bt->prd.d_out, prof, s_prof);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * PR_OUT, o, sizeof(double) * PR_OUT); });
    return predict_finish(bt, rc, S, keep, lo, profile);
}
// the rollout of the batch's quadcopter instances (obca_rollout.h): resident (ts == nullptr: the last solution in d.z, its one t) or a caller's trajectory -- x as
// quad_upload_range has put it behind the problem header, timeScale and u of the call travelling up as [ timeScale (N + 1) | u 4 x N ] per instance
static int quad_rollout_range(obca_quad_batch *bt, const double *u, const double *ts, int S, int restart, double need, int lo, double *out, double *X) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    if (int rc = rollout_reserve(bt, QX, S)) return rc;
    const size_t W = (size_t)N1 + (size_t)QU * N, sp = roll::rollout_pose_len(N, S), sx = roll::rollout_state_len(N, QX);
    const int rc = run_validate(bt, bt->rol, ts ? W : 0, ts != nullptr, RO_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1); memcpy(a + N1, u + ((size_t)lo + i) * QU * N, sizeof(double) * QU * N);
    }, [&] {
        const double *in = bt->rol.d_in;
        if (ts) hipLaunchKernelGGL(obca_rollout_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.prob + QPH_SIZE, d.s_prob, in + N1, W, in, W, 1,
                                   S, restart, need, (double *)bt->rol_w, sp, rollout_states_at(bt, S), sx, (double *)bt->rol.d_out);
        else hipLaunchKernelGGL(obca_rollout_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.z + l.x, d.s_z, (const double *)d.z + l.u, d.s_z,
                                (const double *)d.z + l.t, d.s_z, 0, S, restart, need, (double *)bt->rol_w, sp, rollout_states_at(bt, S), sx, (double *)bt->rol.d_out);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * RO_OUT, o, sizeof(double) * RO_OUT); });
    return rollout_finish(bt, rc, QX, S, lo, X);
}
// the closed-loop rollout of the batch's quadcopter instances (obca_track.h): quad_rollout_range with the modes, the weights and dx0; per instance
// [ dx0 12 | timeScale (N + 1) | u 4 x N (the last two: host-pointer calls) ] travels up
static int quad_track_range(obca_quad_batch *bt, const double *u, const double *ts, int S, int feedback, int clamp, const trk::Weights &w, const double *dx0, double need, int lo, double *out, double *X, double *K) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &qd = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    const TrackDims d = track_dims(bt, QX, QU, S);
    if (int rc = track_reserve(bt, d)) return rc;
    const size_t W = (size_t)QX + (ts ? (size_t)N1 + (size_t)QU * N : 0);
    const int rc = run_validate(bt, bt->trk, W, true, TK_OUT, [&](int i, double *a) {
        if (dx0) memcpy(a, dx0 + ((size_t)lo + i) * QX, sizeof(double) * QX); else memset(a, 0, sizeof(double) * QX);
        if (ts) { memcpy(a + QX, ts + ((size_t)lo + i) * N1, sizeof(double) * N1); memcpy(a + QX + N1, u + ((size_t)lo + i) * QU * N, sizeof(double) * QU * N); }
    }, [&] {
        const double *in = bt->trk.d_in;
        if (ts) hipLaunchKernelGGL(obca_track_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)qd.prob, qd.s_prob, (const double *)qd.prob + QPH_SIZE, qd.s_prob, in + QX + N1, W, in + QX, W, 1,
                                   in, W, dx0 ? 1 : 0, S, feedback, clamp, w, need, (double *)bt->trk_w, d.ab, track_poses_at(bt, d), d.pose, track_states_at(bt, d), d.st, (double *)bt->trk_K, d.gain, (double *)bt->trk.d_out);
        else hipLaunchKernelGGL(obca_track_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)qd.prob, qd.s_prob, (const double *)qd.z + l.x, qd.s_z, (const double *)qd.z + l.u, qd.s_z,
                                (const double *)qd.z + l.t, qd.s_z, 0, in, W, dx0 ? 1 : 0, S, feedback, clamp, w, need, (double *)bt->trk_w, d.ab, track_poses_at(bt, d), d.pose, track_states_at(bt, d), d.st,
                                (double *)bt->trk_K, d.gain, (double *)bt->trk.d_out);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * TK_OUT, o, sizeof(double) * TK_OUT); });
    return track_finish(bt, rc, d, S, lo, X, K);
}
// the ensemble about the batch's quadcopter instances (obca_ensemble.h): quad_track_range with the members, dx0 and dub; per instance
// [ dx0 12 M | dub 4 M | timeScale (N + 1) | u 4 x N (the last two: host-pointer calls) ] travels up
static int quad_ensemble_range(obca_quad_batch *bt, const double *u, const double *ts, int S, int M, int feedback, int clamp, const trk::Weights &w, const double *dx0, const double *dub, double need,
                               int lo, double *out, double *mem, double *fin) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &qd = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    const EnsDims d = ensemble_dims(bt, QX, QU, M);
    if (int rc = ensemble_reserve(bt, d)) return rc;
    const size_t W0 = (size_t)(QX + QU) * M, W = W0 + (ts ? (size_t)N1 + (size_t)QU * N : 0);
    const int rc = run_validate(bt, bt->ens, W, true, EN_OUT, [&](int i, double *a) {
        ensemble_pack(d, dx0, dub, (size_t)lo + i, a);
        if (ts) { memcpy(a + W0, ts + ((size_t)lo + i) * N1, sizeof(double) * N1); memcpy(a + W0 + N1, u + ((size_t)lo + i) * QU * N, sizeof(double) * QU * N); }
    }, [&] {
        const double *in = bt->ens.d_in;
        if (ts) hipLaunchKernelGGL(obca_ensemble_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)qd.prob, qd.s_prob, (const double *)qd.prob + QPH_SIZE, qd.s_prob, in + W0 + N1, W, in + W0, W, 1,
                                   in, W, S, M, feedback, clamp, w, need, (double *)bt->ens_w, d.ab, (double *)bt->ens_K, d.gain, (double *)bt->ens_mem, (double *)bt->ens_fin, (double *)bt->ens.d_out);
        else hipLaunchKernelGGL(obca_ensemble_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, (const double *)qd.prob, qd.s_prob, (const double *)qd.z + l.x, qd.s_z, (const double *)qd.z + l.u, qd.s_z,
                                (const double *)qd.z + l.t, qd.s_z, 0, in, W, S, M, feedback, clamp, w, need, (double *)bt->ens_w, d.ab, (double *)bt->ens_K, d.gain, (double *)bt->ens_mem, (double *)bt->ens_fin,
                                (double *)bt->ens.d_out);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * EN_OUT, o, sizeof(double) * EN_OUT); });
    return ensemble_finish(bt, rc, d, lo, mem, fin);
}
// the certificate of the batch's quadcopter instances (obca_certify.h): quad_clearance_range with need, slack and max_steps, then the caller's iv
// one step of the batch's quadcopter instances (obca_advance.h): per instance [ kick 12 | xF_new 12 ] travels up where either is given
static int quad_advance_run(obca_quad_batch *bt, int shift, int S, const double *kick, const double *xF_new, double need, double *out) {
    const int B = bt->B, N = bt->N;
    if (int rc = advance_reserve(bt, QX, shift, S)) return rc;
    const size_t sp = adv::advance_pose_len(shift, S), sx = adv::advance_state_len(shift, QX);
    const int rc = run_validate(bt, bt->adv, 2 * QX, kick || xF_new, AV_OUT, [&](int i, double *a) {
        if (kick) memcpy(a, kick + (size_t)i * QX, sizeof(double) * QX); else memset(a, 0, sizeof(double) * QX);
        if (xF_new) memcpy(a + QX, xF_new + (size_t)i * QX, sizeof(double) * QX); else memset(a + QX, 0, sizeof(double) * QX);
    }, [&] {
        hipLaunchKernelGGL(obca_advance_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, N, shift, bt->d, S, (const double *)bt->adv.d_in, kick ? 1 : 0, xF_new ? 1 : 0, need, (double *)bt->adv_w, sp,
                           bt->adv_w + (size_t)B * sp, sx, (double *)bt->adv_st, bt->adv_cap ? (double *)bt->adv_log : nullptr, (size_t)bt->adv_cap * QX, (size_t)bt->adv_n * QX,
                           bt->adv_cap ? (double)(bt->adv_n + shift) : -1.0, (double *)bt->adv.d_out);
    }, [&](int i, const double *o) { memcpy(out + (size_t)i * AV_OUT, o, sizeof(double) * AV_OUT); });
    return advance_finish(bt, rc, shift);
}
static int quad_certify_range(obca_quad_batch *bt, const double *ts, double need, double slack, int max_steps, int lo, double *out, double *iv) {
    const int B = bt->B, N = bt->N, N1 = N + 1; const QDevBufs &d = bt->d;
    quad::QLay l; quad::q_make_layout(N, l);
    if (int rc = certify_reserve(bt)) return rc;
    const size_t lds = cert::certify_work_len(N, QOB) * sizeof(double);
    const int rc = run_validate(bt, bt->cer, ts ? (size_t)N1 : 0, ts != nullptr, CT_OUT, [&](int i, double *a) {
        memcpy(a, ts + ((size_t)lo + i) * N1, sizeof(double) * N1);
    }, [&] {
        if (ts) hipLaunchKernelGGL(obca_certify_quad_kernel, dim3(B), dim3(QNT), lds, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.prob + QPH_SIZE, d.s_prob, (const double *)bt->cer.d_in, (size_t)N1, 1,
                                   need, slack, max_steps, (double *)bt->cer_iv, (double *)bt->cer.d_out);
        else hipLaunchKernelGGL(obca_certify_quad_kernel, dim3(B), dim3(QNT), lds, bt->stream, B, N, (const double *)d.prob, d.s_prob, (const double *)d.z + l.x, d.s_z, (const double *)d.z + l.t, d.s_z, 0,
                                need, slack, max_steps, (double *)bt->cer_iv, (double *)bt->cer.d_out);
    }, [&](int i, const double *o) { memcpy(out + ((size_t)lo + i) * CT_OUT, o, sizeof(double) * CT_OUT); });
    return certify_finish(bt, rc, lo, iv);
}
// instances (one wavefront each) resident per CU, as OBCA_RESIDENT_PER_CU for the parking kernel: what pick_chunk sizes a quadcopter chunk by
static const int QUAD_RESIDENT_PER_CU = (QNT == 64 ? 4 : 2) * OBCA_QUAD_WAVES_PER_EU;
// parking_chunks for the quadcopter; the slot's cached batch only has to hold the chunk at hand
template <typename Op>
static int quad_chunks(obca_ctx *ctx, int B, int N, const QuadIn &in, Op &&op /* int(obca_quad_batch *, int lo) */) {
    const int chunk = pick_chunk(ctx, B, QUAD_RESIDENT_PER_CU);
    return run_chunks(ctx, B, chunk, [&](Slot &s, int lo, int n, std::string &err) -> int {
        int rc = slot_batch(ctx, s, s.qb, obca_quad_batch_destroy, n, std::min(chunk, B), N, err);
        if (rc) return rc;
        obca_quad_batch *bt = s.qb;
        rc = quad_upload_range(bt, in, lo, n);
        if (!rc) rc = op(bt, lo);
        if (rc) err = bt->err;
        return rc;
    });
}
static int quadcopter_call(obca_ctx *ctx, int B, int N, const QuadIn &in, const obca_opts *opts, const QuadOut &out) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!in.Ts || !in.x0 || !in.xF || !in.ob || !in.xWS || !in.timeWS) { ctx->err = "NULL argument"; return -1; }
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) -> int {
        const int rc = quad_solve(bt, opts);
        return rc ? rc : quad_download_range(bt, out, lo);
    });
}
extern "C" {
int obca_quad_batch_solve(obca_quad_batch *bt, const obca_opts *opts) { if (!bt) return -1; return fin(bt, quad_solve(bt, opts)); }
int obca_quad_batch_shift_warm_start(obca_quad_batch *bt, int shift, const double *x0_new, const double *xF_new) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    if (!bt->uploaded) { ctx->err = "obca_quad_batch_shift_warm_start: nothing uploaded"; return -1; }
    if (shift < 0 || shift > bt->N) { ctx->err = "obca_quad_batch_shift_warm_start: shift out of range 0..N"; return -1; }
    if (!bt->solved) { ctx->err = "obca_quad_batch_shift_warm_start: nothing has been solved since the last upload or shift"; return -1; }
    const size_t n = (size_t)bt->B * QX;
    for (const double *a : {x0_new, xF_new})
        for (size_t i = 0; a && i < n; i++)
            if (!(a[i] - a[i] == 0.0)) { ctx->err = std::string("obca_quad_batch_shift_warm_start: non-finite entry in ") + (a == x0_new ? "x0_new" : "xF_new"); return -1; }
    use_device(bt->device);
    const double *dx0 = nullptr, *dxF = nullptr;
    if (x0_new || xF_new) {   // staged through the pinned problem buffer and the (idle) device staging buffer of the batch: [ x0_new | xF_new ], nothing to free on the error paths
        if (bt->h_prob.reserve(bt->err, 2 * n)) return fin(bt, -2);
        if (x0_new) { memcpy(bt->h_prob, x0_new, n * sizeof(double)); dx0 = bt->stage; }
        if (xF_new) { memcpy(bt->h_prob + n, xF_new, n * sizeof(double)); dxF = bt->stage + n; }
        const size_t lo = x0_new ? 0 : n, hi = xF_new ? 2 * n : n;      // only the halves that were filled travel
        if (hipMemcpyAsync(bt->stage + lo, bt->h_prob + lo, (hi - lo) * sizeof(double), hipMemcpyHostToDevice, bt->stream) != hipSuccess) { ctx->err = "obca_quad_batch_shift_warm_start: H2D failed"; return -2; }
    }
    hipLaunchKernelGGL(obca_quad_shift_kernel, dim3(bt->B), dim3(QNT), 0, bt->stream, bt->B, bt->N, shift, bt->d, dx0, dxF);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bt->stream) != hipSuccess) { ctx->err = "obca_quad_batch_shift_warm_start: kernel failed"; return -2; }
    bt->solved = 0;                                     // d.z still holds the previous solution, but the problem (x0, xF, warm start) has moved on
    return 0;
}
int obca_quad_batch_sync(obca_quad_batch *bt) { return core_sync(bt, "obca_quad_batch_sync: hipStreamSynchronize failed"); }
int obca_quad_batch_kernel_ms(obca_quad_batch *bt, float *ipm_ms) {
    if (!bt || !ipm_ms) return -1;
    if (hipEventElapsedTime(ipm_ms, bt->e0, bt->e1) != hipSuccess) { bt->ctx->err = "obca_quad_batch_kernel_ms: events not ready"; return -2; }
    return 0;
}
int obca_quad_batch_validate(obca_quad_batch *bt, double tol, int *ok, double *viol) {
    if (!bt) return -1;
    if (!ok) { bt->ctx->err = "obca_quad_batch_validate: NULL argument"; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_validate: nothing has been solved since the last upload"; return -1; }
    return fin(bt, quad_validate_range(bt, nullptr, nullptr, nullptr, nullptr, tol > 0 ? tol : 1e-3, 0, ok, viol));
}
int obca_quad_batch_validate_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->val.ev, ms, "obca_quad_batch_validate_ms: no validate call has run on this batch") : -1; }
int obca_quadcopter_constr_satisfaction_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *x0, const double *xF, const double *ob,
                                              const double *x, const double *u, const double *timeScale, const double *lambda, double tol, int *ok, double *viol) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_constr_satisfaction_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !x0 || !xF || !ob || !x || !u || !timeScale || !lambda || !ok) { ctx->err = "obca_quadcopter_constr_satisfaction_batch: NULL argument"; return -1; }
    const std::vector<double> one((size_t)B, 1.0);                 // timeWS of a solve: no check reads it
    const QuadIn in = {Ts, R, x0, xF, ob, x, one.data(), 0, 0};
    const double tl = tol > 0 ? tol : 1e-3;
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_validate_range(bt, x, u, timeScale, lambda, tl, lo, ok, viol); });
}
int obca_quad_batch_clearance(obca_quad_batch *bt, int substeps, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_quad_batch_clearance: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { bt->ctx->err = std::string("obca_quad_batch_clearance: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_clearance: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_clearance_range(bt, nullptr, substeps, need, 0, out));
}
int obca_quad_batch_clearance_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->clr.ev, ms, "obca_quad_batch_clearance_ms: no clearance call has run on this batch") : -1; }
int obca_quadcopter_clearance_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *timeScale, int substeps, double need, double *out) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_clearance_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !timeScale || !out) { ctx->err = "obca_quadcopter_clearance_batch: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { ctx->err = std::string("obca_quadcopter_clearance_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the check reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_clearance_range(bt, timeScale, substeps, need, lo, out); });
}
int obca_quad_batch_predict_clearance(obca_quad_batch *bt, const double *rates, int substeps, double need, int keep_profile, double *out) {
    if (!bt) return -1;
    if (!out || !rates) { bt->ctx->err = "obca_quad_batch_predict_clearance: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { bt->ctx->err = std::string("obca_quad_batch_predict_clearance: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_predict_clearance: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_predict_range(bt, nullptr, rates, substeps, need, keep_profile != 0, 0, out, nullptr));
}
int obca_quad_batch_predict_clearance_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->prd.ev, ms, "obca_quad_batch_predict_clearance_ms: no predict call has run on this batch") : -1; }
int obca_quad_batch_predict_profile(obca_quad_batch *bt, double *out, int capacity) { return bt ? predict_fetch(bt, out, capacity, "obca_quad_batch_predict_profile") : -1; }
int obca_quadcopter_predict_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *timeScale, int substeps, double need, double *out,
                                  const double *rates, double *profile) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_predict_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !timeScale || !out || !rates) { ctx->err = "obca_quadcopter_predict_batch: NULL argument"; return -1; }
    if (const char *bad = clr::clearance_check_args(substeps, need)) { ctx->err = std::string("obca_quadcopter_predict_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the call reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_predict_range(bt, timeScale, rates, substeps, need, profile != nullptr, lo, out, profile); });
}
int obca_quad_batch_rollout(obca_quad_batch *bt, int substeps, int restart, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_quad_batch_rollout: NULL argument"; return -1; }
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { bt->ctx->err = std::string("obca_quad_batch_rollout: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_rollout: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_rollout_range(bt, nullptr, nullptr, substeps, restart, need, 0, out, nullptr));
}
int obca_quad_batch_rollout_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->rol.ev, ms, "obca_quad_batch_rollout_ms: no rollout has run on this batch") : -1; }
int obca_quad_batch_rollout_states(obca_quad_batch *bt, double *X) { return bt ? rollout_states(bt, QX, X, "obca_quad_batch_rollout_states") : -1; }
int obca_quadcopter_rollout_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *u, const double *timeScale,
                                  int substeps, int restart, double need, double *out, double *X) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_rollout_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !u || !timeScale || !out) { ctx->err = "obca_quadcopter_rollout_batch: NULL argument"; return -1; }
    if (const char *bad = roll::rollout_check_args(substeps, restart, need)) { ctx->err = std::string("obca_quadcopter_rollout_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the call reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_rollout_range(bt, u, timeScale, substeps, restart, need, lo, out, X); });
}
int obca_quad_batch_track(obca_quad_batch *bt, int substeps, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_quad_batch_track: NULL argument"; return -1; }
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, QX, QU, need)) { bt->ctx->err = std::string("obca_quad_batch_track: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_track: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_track_range(bt, nullptr, nullptr, substeps, feedback, clamp, trk::make_weights(q, r, qf, QX, QU), dx0, need, 0, out, nullptr, nullptr));
}
int obca_quad_batch_track_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->trk.ev, ms, "obca_quad_batch_track_ms: no track call has run on this batch") : -1; }
int obca_quad_batch_track_states(obca_quad_batch *bt, double *X) { return bt ? track_fetch(bt, QX, QU, false, X, "obca_quad_batch_track_states") : -1; }
int obca_quad_batch_track_gains(obca_quad_batch *bt, double *K) { return bt ? track_fetch(bt, QX, QU, true, K, "obca_quad_batch_track_gains") : -1; }
int obca_quadcopter_track_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *u, const double *timeScale,
                                int substeps, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, double need, double *out, double *X, double *K) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_track_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !u || !timeScale || !out) { ctx->err = "obca_quadcopter_track_batch: NULL argument"; return -1; }
    if (const char *bad = trk::track_check_args(substeps, feedback, clamp, q, r, qf, QX, QU, need)) { ctx->err = std::string("obca_quadcopter_track_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the call reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    const trk::Weights w = trk::make_weights(q, r, qf, QX, QU);
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_track_range(bt, u, timeScale, substeps, feedback, clamp, w, dx0, need, lo, out, X, K); });
}
int obca_quad_batch_ensemble(obca_quad_batch *bt, int substeps, int members, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, const double *dub,
                             double need, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_quad_batch_ensemble: NULL argument"; return -1; }
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, QX, QU, need)) { bt->ctx->err = std::string("obca_quad_batch_ensemble: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_ensemble: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_ensemble_range(bt, nullptr, nullptr, substeps, members, feedback, clamp, trk::make_weights(q, r, qf, QX, QU), dx0, dub, need, 0, out, nullptr, nullptr));
}
int obca_quad_batch_ensemble_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->ens.ev, ms, "obca_quad_batch_ensemble_ms: no ensemble call has run on this batch") : -1; }
int obca_quad_batch_ensemble_members(obca_quad_batch *bt, double *mem) { return bt ? ensemble_fetch(bt, QX, false, mem, "obca_quad_batch_ensemble_members") : -1; }
int obca_quad_batch_ensemble_final(obca_quad_batch *bt, double *fin) { return bt ? ensemble_fetch(bt, QX, true, fin, "obca_quad_batch_ensemble_final") : -1; }
int obca_quadcopter_ensemble_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *u, const double *timeScale,
                                   int substeps, int members, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, const double *dub, double need,
                                   double *out, double *mem, double *fin) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_ensemble_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !u || !timeScale || !out) { ctx->err = "obca_quadcopter_ensemble_batch: NULL argument"; return -1; }
    if (const char *bad = ens::ensemble_check_args(substeps, members, feedback, clamp, q, r, qf, QX, QU, need)) { ctx->err = std::string("obca_quadcopter_ensemble_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the call reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    const trk::Weights w = trk::make_weights(q, r, qf, QX, QU);
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_ensemble_range(bt, u, timeScale, substeps, members, feedback, clamp, w, dx0, dub, need, lo, out, mem, fin); });
}
int obca_quad_batch_advance(obca_quad_batch *bt, int shift, int substeps, const double *kick, const double *xF_new, double need, double *out) {
    if (!bt) return -1;
    if (int rc = advance_refuse(bt, "obca_quad_batch_advance", shift, substeps, need, out)) return rc;
    for (size_t i = 0; xF_new && i < (size_t)bt->B * QX; i++)
        if (!(xF_new[i] - xF_new[i] == 0.0)) { bt->ctx->err = "obca_quad_batch_advance: non-finite entry in xF_new"; return -1; }
    return fin(bt, quad_advance_run(bt, shift, substeps, kick, xF_new, need, out));
}
int obca_quad_batch_advance_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->adv.ev, ms, "obca_quad_batch_advance_ms: no advance has run on this batch") : -1; }
int obca_quad_batch_advance_state(obca_quad_batch *bt, double *X) { return bt ? advance_state(bt, QX, X, "obca_quad_batch_advance_state") : -1; }
int obca_quad_batch_advance_log(obca_quad_batch *bt, int capacity_nodes) { return bt ? advance_log(bt, QX, capacity_nodes, "obca_quad_batch_advance_log") : -1; }
int obca_quad_batch_advance_log_states(obca_quad_batch *bt, double *X, int *nodes) { return bt ? advance_log_states(bt, QX, X, nodes, "obca_quad_batch_advance_log_states") : -1; }

// obca_scene_edit.h for the quadcopter: SE_QIN doubles per box go up, the kernel edits the QPH_OB words of d.prob in place
int obca_quad_batch_move_obstacles(obca_quad_batch *bt, const double *motion, const double *inflate, int *status) {
    if (!bt) return -1;
    if (!status) { bt->ctx->err = "obca_quad_batch_move_obstacles: NULL argument"; return -1; }
    if (!bt->uploaded) { bt->ctx->err = "obca_quad_batch_move_obstacles: nothing uploaded"; return -1; }
    const int B = bt->B;
    return fin(bt, run_validate(bt, bt->mov, (size_t)QOB * SE_QIN, true, 1, [&](int i, double *a) {
        for (int j = 0; j < QOB; j++) {
            const size_t g = (size_t)i * QOB + j;
            for (int q = 0; q < 3; q++) a[SE_QIN * j + q] = motion ? motion[3 * g + q] : 0.0;
            a[SE_QIN * j + 3] = inflate ? inflate[g] : 0.0;
        }
    }, [&] {
        hipLaunchKernelGGL(obca_move_quad_kernel, dim3(B), dim3(QNT), 0, bt->stream, B, bt->d.prob, bt->d.s_prob, (const double *)bt->mov.d_in, (double *)bt->mov.d_out);
    }, [&](int i, const double *o) { status[i] = o[0] != 0.0; }));
}
int obca_quad_batch_move_obstacles_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->mov.ev, ms, "obca_quad_batch_move_obstacles_ms: no move call has run on this batch") : -1; }
int obca_quad_batch_obstacles_download(obca_quad_batch *bt, double *ob) {
    if (!bt) return -1;
    if (!ob) { bt->ctx->err = "obca_quad_batch_obstacles_download: NULL argument"; return -1; }
    if (!bt->uploaded) { bt->ctx->err = "obca_quad_batch_obstacles_download: nothing uploaded"; return -1; }
    use_device(bt->device);
    if (hipStreamSynchronize(bt->stream) != hipSuccess ||
        hipMemcpy2D(ob, sizeof(double) * QOB * QL, bt->d.prob + QPH_OB, bt->d.s_prob * sizeof(double), sizeof(double) * QOB * QL, (size_t)bt->B, hipMemcpyDeviceToHost) != hipSuccess) {
        bt->ctx->err = "obca_quad_batch_obstacles_download: copy failed"; return -2;
    }
    return 0;
}

int obca_quad_batch_certify(obca_quad_batch *bt, double need, double slack, int max_steps, double *out) {
    if (!bt) return -1;
    if (!out) { bt->ctx->err = "obca_quad_batch_certify: NULL argument"; return -1; }
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { bt->ctx->err = std::string("obca_quad_batch_certify: ") + bad; return -1; }
    if (!bt->uploaded || !bt->solved) { bt->ctx->err = "obca_quad_batch_certify: nothing has been solved since the last upload or shift"; return -1; }
    return fin(bt, quad_certify_range(bt, nullptr, need, slack, max_steps, 0, out, nullptr));
}
int obca_quad_batch_certify_ms(obca_quad_batch *bt, float *ms) { return bt && ms ? core_elapsed_ms(bt->ctx, bt->cer.ev, ms, "obca_quad_batch_certify_ms: no certify call has run on this batch") : -1; }
int obca_quad_batch_certify_intervals(obca_quad_batch *bt, double *iv) { return bt ? certify_fetch(bt, iv, "obca_quad_batch_certify_intervals") : -1; }
int obca_quadcopter_certify_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob, const double *x, const double *timeScale, double need, double slack, int max_steps,
                                  double *out, double *iv) {
    if (!ctx) return -1;
    if (B < 1 || N < 2 || N > OBCA_QUAD_NMAX) { ctx->err = "obca_quadcopter_certify_batch: need B>=1, 2<=N<=OBCA_QUAD_NMAX"; return -1; }
    if (!Ts || !ob || !x || !timeScale || !out) { ctx->err = "obca_quadcopter_certify_batch: NULL argument"; return -1; }
    if (const char *bad = cert::certify_check_args(need, slack, max_steps)) { ctx->err = std::string("obca_quadcopter_certify_batch: ") + bad; return -1; }
    const std::vector<double> zero((size_t)B * QX, 0.0), one((size_t)B, 1.0);      // start, goal and timeWS of a solve: the call reads none of them
    const QuadIn in = {Ts, R, zero.data(), zero.data(), ob, x, one.data(), 0, 0};
    return quad_chunks(ctx, B, N, in, [&](obca_quad_batch *bt, int lo) { return quad_certify_range(bt, timeScale, need, slack, max_steps, lo, out, iv); });
}
int obca_quad_batch_download(obca_quad_batch *bt, double *xp, double *up, double *ts, int *exitflag, double *lp, double *slp, double *info) {
    if (!bt) return -1;
    QuadOut o = {xp, up, ts, exitflag, lp, slp, info};
    return fin(bt, quad_download_range(bt, o, 0));
}
int obca_quadcopter_signed_dist_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *x0, const double *xF,
                                      const double *ob, const double *xWS, const double *uWS, const double *timeWS, int dual_ws,
                                      const obca_opts *opts, double *xp, double *up, double *timeScale, int *exitflag, double *lp,
                                      double *slp, double *info) {
    (void)uWS;                                         /* the reference ignores it too: inputs start at the hover speed, :202 */
    QuadIn in = {Ts, R, x0, xF, ob, xWS, timeWS, dual_ws, 0};
    QuadOut o = {xp, up, timeScale, exitflag, lp, slp, info};
    return quadcopter_call(ctx, B, N, in, opts, o);
}
int obca_quadcopter_dist_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *x0, const double *xF,
                               const double *ob, const double *xWS, const double *uWS, const double *timeWS, int dual_ws,
                               const obca_opts *opts, double *xp, double *up, double *timeScale, int *exitflag, double *lp, double *info) {
    (void)uWS;                                         /* QuadcopterDist.jl:196 */
    QuadIn in = {Ts, R, x0, xF, ob, xWS, timeWS, dual_ws, 1};
    QuadOut o = {xp, up, timeScale, exitflag, lp, nullptr, info};
    return quadcopter_call(ctx, B, N, in, opts, o);
}

/* ---- solved quadcopter batches on a finer horizon (obca_quad_subdivide.h, include/obca_quad_subdivide.h) */
int obca_quad_batch_subdivide_into(obca_quad_batch *dst, obca_quad_batch *src, int factor, double margin, const int *sel, int n, int *status) {
    if (!dst || !src) return -1;
    return into_call("obca_quad_batch_subdivide_into", dst, src, dst->sd, factor, "nothing has been solved on the source since its last upload or shift",
                     qsd::subdivide_check_args(n, src->N, factor, margin), sel, n, status, [&] { dst->B = n; dst->solved = 0; return 0; },
                     [&](const int *dsel, int *dstatus) {
        hipLaunchKernelGGL(obca_quad_subdivide_batch_kernel, dim3(n), dim3(QNT), 0, dst->stream, n, src->N, factor, margin, dsel, src->d, dst->d, dstatus);
    });
}

int obca_quad_batch_subdivide_ms(obca_quad_batch *dst, float *ms) {
    return dst && ms ? core_elapsed_ms(dst->ctx, dst->sd.ev, ms, "obca_quad_batch_subdivide_ms: no subdivide call has written into this batch") : -1;
}

int obca_quadcopter_subdivide_batch(obca_ctx *ctx, int B, int N, int factor, const double *Ts, const double *x, const double *timeScale, double *Ts_f, double *x_f) {
    if (!ctx) return -1;
    const char *bad = qsd::subdivide_check_args(B, N, factor, 0.0);
    if (!bad && !(Ts && x && Ts_f && x_f)) bad = "NULL argument";
    if (bad) { ctx->err = std::string("obca_quadcopter_subdivide_batch: ") + bad; return -1; }
    use_device(ctx->device);
    KernelStage &w = ctx->qsd;
    if (int rc = w.ev.ensure(ctx->err)) return rc;
    const size_t Nf = (size_t)N * factor, nx = (size_t)B * QX * (N + 1), nt = timeScale ? (size_t)B * (N + 1) : 0, nin = B + nx + nt, nxf = (size_t)B * QX * (Nf + 1);
    if (w.dev.reserve(nin + B + nxf, ctx->stream) != hipSuccess) { ctx->err = "obca_quadcopter_subdivide_batch: hipMalloc failed"; return -2; }
    if (w.host.reserve(ctx->err, nin)) return -2;
    double *h = w.host, *d = w.dev;      // one contiguous transfer up: [ Ts B | x | timeScale ]
    memcpy(h, Ts, sizeof(double) * B); memcpy(h + B, x, sizeof(double) * nx);
    if (nt) memcpy(h + B + nx, timeScale, sizeof(double) * nt);
    double *dTsf = d + nin, *dxf = dTsf + B;
    const bool up = hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    return launch_timed(ctx->err, "obca_quadcopter_subdivide_batch", ctx->stream, w.ev, up, [&] {
        hipLaunchKernelGGL(obca_quad_subdivide_host_kernel, dim3(B), dim3(QNT), 0, ctx->stream, B, N, factor, (const double *)d, (const double *)(d + B), (const double *)(nt ? d + B + nx : nullptr), dTsf, dxf);
    }, {{Ts_f, dTsf, (size_t)B * sizeof(double)}, {x_f, dxf, nxf * sizeof(double)}});
}

}  // extern "C"

/* ---------------------------------------------------------------- the parking planner on the device.  LAST in this file: obca_hybrid.h switches fp contraction off from its
   include to the end of the translation unit, and no other kernel may be compiled under that. */
#include "obca_hybrid.h"
#include "../../include/obca_plan_device.h"
// the resident route's packing (its kernel is defined in the header): behind the planner's text, whose names it uses and under whose contraction rule it is compiled
#include "obca_plan_resident.h"
#include "../../include/obca_plan_resident.h"
#include "../../include/obca_plan_resident_check.h"
// the quadcopter's resident route (its kernel is defined in the header, over obca_plan3d.h): here because obca_plan3d.h switches contraction off at file scope too
#include "obca_quad_plan_resident.h"
#include "../../include/obca_quad_plan_resident.h"

// the parking planner (obca_hybrid.h): `slots` persistent workgroups, workgroup s runs the searches s, s + slots, ... in its slot of the planner's memory.  LDS: the
// holonomic map (nmap floats, padded to an even count), then the bucket heads and control words.
// SCENES false: one field F for the batch, its blocked cells from the host (obca_hybrid_astar_batch).  SCENES true: search i runs in the field of instance i, put together
// from the instance's record in S, and finds the blocked cells itself (obca_scene_astar_batch); F and blocked are not read.
template <bool SCENES>
__global__ __launch_bounds__(HY_NT) void obca_hybrid_kernel(int B, int slots, const hy::Params *__restrict__ Pp, hy::Field F, hy::Fields S, const unsigned char *__restrict__ blocked,
                                                            const double *__restrict__ inst, char *slotmem, size_t slot_bytes, double *paths, int *dirs, int *counts, int *nexp, int *rounds) {
    extern __shared__ float hy_lds[];
    const hy::Params &P = *Pp;
    if ((int)blockIdx.x >= slots) return;
    const hy::SlotMem M = hy::carve(slotmem + (size_t)blockIdx.x * slot_bytes, P.ncell, P.maxnodes, P.maxchunks);
    int *li = (int *)(hy_lds + ((P.nmap + 1) & ~1));
    if (!SCENES) __builtin_assume(blocked != nullptr);      // (the host never launches this instantiation without the map: the search's own blocked test is not compiled into it)
    for (int i = blockIdx.x; i < B; i += slots)
        hy::search(P, SCENES ? hy::field_of(S, i) : F, SCENES ? nullptr : blocked, inst + (size_t)i * 10, M, hy_lds, li, paths + (size_t)i * P.cap * 3, dirs + (size_t)i * P.cap,
                   counts + i, nexp + i, rounds + i);
}

// ---- the parking planner on the device (obca_hybrid.h, include/obca_plan_device.h) and the same planner with every search in the obstacle field of its own instance
// (include/obca_plan_scenes.h).  The two entry points share the slots and the staging block; each has its own events and its own instantiation of the kernel.
#define OBCA_HYBRID_BUDGET ((size_t)16 << 30)      // bytes the slots take by default
static inline size_t up8(size_t n) { return (n + 7) / 8 * 8; }
// The device side of a call of B searches with the parameter block P, shared by the host-pointer entry points (hybrid_call) and the resident route
// (obca_batch_plan_warm_start): the slots, the staging block [ n_in bytes of input: Params | inst B x 10 | field data | paths | dirs | counts expansions rounds ] and the LDS
// attribute of `kernel` (`own`: its index).  The context's device is selected.  hybrid_launch then launches the kernel over that block.
struct HybridRun {
    int B, cap, slots, lds; size_t sb, o_inst, o_paths, o_dirs, o_cnt; char *d;
    int *counts() const { return (int *)(d + o_cnt); }
};
static int hybrid_reserve(obca_ctx *ctx, const char *entry, int own, decltype(&obca_hybrid_kernel<false>) kernel, int B, int cap, const hy::Params &P, int mn, int mc, size_t n_in, HybridRun &r) {
    HybridBufs &h = ctx->hyb;
    auto fail = [&](const char *what) { ctx->err = std::string(entry) + ": " + what; h.release(); return -2; };
    // the slots: as many as configured, else what the budget holds, never more than searches
    const size_t sb = hy::slot_bytes(P.ncell, mn, mc);
    int slots = h.slots ? h.slots : (int)std::min<size_t>(OBCA_HYBRID_MAXSLOTS, std::max<size_t>(1, OBCA_HYBRID_BUDGET / sb));
    slots = std::min(slots, B);
    if (!h.slotmem || h.nslots < slots || h.ncell != P.ncell || h.nodes != mn || h.chunks != mc) {
        if (h.slotmem) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(h.slotmem); h.slotmem = nullptr; h.nslots = 0; }
        if (hipMalloc((void **)&h.slotmem, sb * slots) != hipSuccess) { h.slotmem = nullptr; ctx->err = std::string(entry) + ": hipMalloc of the slots failed (fewer slots or nodes: obca_hybrid_configure)"; return -2; }
        h.slot_bytes = sb; h.nslots = slots; h.ncell = P.ncell; h.nodes = mn; h.chunks = mc; h.slot_allocs++;
        bool ok = true;      // claim words and cell table: all ones; a search leaves them so
        for (int s = 0; s < slots && ok; s++) ok = hipMemsetAsync(h.slotmem + (size_t)s * sb, 0xFF, hy::slot_init_bytes(P.ncell), ctx->stream) == hipSuccess;
        if (!ok) return fail("hipMemsetAsync failed");
    }
    r.B = B; r.cap = cap; r.slots = slots; r.sb = sb;
    r.o_inst = up8(sizeof(hy::Params));
    r.o_paths = n_in; r.o_dirs = r.o_paths + (size_t)B * cap * 24; r.o_cnt = r.o_dirs + up8((size_t)B * cap * 4);
    const size_t n_all = r.o_cnt + up8((size_t)3 * B * 4);
    h.serial++;      // whatever an earlier call left in the block is gone from here on
    if (h.io_bytes < n_all) {
        if (h.io) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(h.io); h.io = nullptr; h.io_bytes = 0; }
        if (hipMalloc((void **)&h.io, n_all) != hipSuccess) { h.io = nullptr; return fail("hipMalloc failed"); }
        h.io_bytes = n_all; h.io_allocs++;
    }
    r.d = h.io;
    r.lds = (((P.nmap + 1) & ~1) + HY_LDS_INTS) * (int)sizeof(float);
    if (r.lds > h.lds_set[own]) {
        if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, r.lds) != hipSuccess) return fail("hipFuncSetAttribute failed");
        h.lds_set[own] = r.lds;
    }
    return 0;
}
static void hybrid_launch(obca_ctx *ctx, decltype(&obca_hybrid_kernel<false>) kernel, const HybridRun &r, const hy::Field &F, const hy::Fields &S, const unsigned char *blocked) {
    int *dcnt = r.counts();
    hipLaunchKernelGGL(kernel, dim3(r.slots), dim3(HY_NT), r.lds, ctx->stream, r.B, r.slots, (const hy::Params *)r.d, F, S, blocked, (const double *)(r.d + r.o_inst),
                       ctx->hyb.slotmem, r.sb, (double *)(r.d + r.o_paths), (int *)(r.d + r.o_dirs), dcnt, dcnt + r.B, dcnt + 2 * r.B);
}
static inline void hybrid_sizes(const obca_ctx *ctx, int &mn, int &mc) {
    mn = ctx->hyb.max_nodes ? ctx->hyb.max_nodes : OBCA_HYBRID_MAXNODES; mc = ctx->hyb.max_chunks ? ctx->hyb.max_chunks : hy::default_chunks(mn);
}

// What both entry points do around their own validation and packing.  One block travels up: [ Params | inst B x 10 | the entry's field data ].  make(mn, mc, P, inst, up, o_fld)
// checks the arguments (a text refuses the call), fills P and inst and sizes `up` to hold its field data from byte o_fld on; bind(d, F, S) then builds the device-side Field
// (shared field; it returns the blocked map) or Fields (per-instance fields) over that data at `d` on the device.  One block comes down: [ paths | dirs | counts | expansions | rounds ].
// `kernel` is the entry's instantiation of obca_hybrid_kernel, `own` its index (0: shared field, 1: per-instance fields) to the events and the LDS attribute of its own.
// A failed device call behind the slots' allocation releases the planner's memory: the slots may hold a half-finished search, the next call starts from fresh ones.
template <typename Make, typename Bind>
static int hybrid_call(obca_ctx *ctx, const char *entry, int own, decltype(&obca_hybrid_kernel<false>) kernel, int B, double *paths, int *dirs, int cap, int *counts, int *expansions, int *rounds, Make &&make, Bind &&bind) {
    if (!ctx) return -1;
    HybridBufs &h = ctx->hyb; EventPair &ev = h.ev[own];
    int mn, mc; hybrid_sizes(ctx, mn, mc);
    hy::Params P; std::vector<double> inst; std::vector<char> up;
    const size_t o_inst = up8(sizeof(hy::Params)), o_fld = o_inst + (size_t)std::max(B, 0) * 10 * 8;
    const std::string bad = (paths && dirs && counts) ? make(mn, mc, P, inst, up, o_fld) : std::string("NULL output array");
    if (!bad.empty()) { ctx->err = std::string(entry) + ": " + bad; return -1; }
    use_device(ctx->device);
    if (int rc = ev.ensure(ctx->err)) return rc;
    ev.timed = 0;
    const size_t n_in = up.size();
    HybridRun r;
    if (int rc = hybrid_reserve(ctx, entry, own, kernel, B, cap, P, mn, mc, n_in, r)) return rc;
    memcpy(up.data(), &P, sizeof P); memcpy(up.data() + o_inst, inst.data(), inst.size() * 8);
    char *d = r.d;
    hy::Field F = hy::Field(); hy::Fields S = hy::Fields();
    const unsigned char *blocked = bind(d + o_fld, F, S);
    int *tail = (int *)up.data();      // once `up` has travelled, its head (Params and inst: more than 3 B ints) takes the three count arrays on the way back
    const bool sent = hipMemcpyAsync(d, up.data(), n_in, hipMemcpyHostToDevice, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;      // (`up` is pageable)
    const int rc = launch_timed(ctx->err, entry, ctx->stream, ev, sent, [&] { hybrid_launch(ctx, kernel, r, F, S, blocked); },
                                {{paths, d + r.o_paths, (size_t)B * cap * 24}, {dirs, d + r.o_dirs, (size_t)B * cap * 4}, {tail, r.counts(), (size_t)3 * B * 4}});
    if (rc) { h.release(); return rc; }
    for (int i = 0; i < B; i++) { counts[i] = tail[i]; if (expansions) expansions[i] = tail[B + i]; if (rounds) rounds[i] = tail[2 * B + i]; }
    return 0;
}

extern "C" {

int obca_hybrid_configure(obca_ctx *ctx, int slots, int max_nodes, int max_chunks) {
    if (!ctx) return -1;
    if (slots < 0 || slots > OBCA_HYBRID_MAXSLOTS || max_nodes < 0 || max_nodes > OBCA_HYBRID_MAXNODES || max_chunks < 0 || max_chunks > (1 << 24)) {
        ctx->err = "obca_hybrid_configure: need 0 <= slots <= OBCA_HYBRID_MAXSLOTS, 0 <= max_nodes <= OBCA_HYBRID_MAXNODES, 0 <= max_chunks <= 2^24"; return -1;
    }
    ctx->hyb.slots = slots; ctx->hyb.max_nodes = max_nodes; ctx->hyb.max_chunks = max_chunks;
    return 0;
}

// one field for the batch; its blocked cells come from the host.  Field data: [ A | b | rn | vert | v off voff (ints) | blocked (bytes) ]
int obca_hybrid_astar_batch(obca_ctx *ctx, int B, const double *starts, const double *goals, int nOb, const int *vOb, const double *A, const double *b,
                            const double ego[4], double L, const double XYbounds[4], const double *opts, int nopts, double bucket_width,
                            double *paths, int *dirs, int cap, int *counts, int *expansions, int *rounds) {
    hy::HostField W; std::vector<unsigned char> blocked;
    size_t M_ = 0, o_int = 0, o_blk = 0;
    return hybrid_call(ctx, "obca_hybrid_astar_batch", 0, obca_hybrid_kernel<false>, B, paths, dirs, cap, counts, expansions, rounds,
                              [&](int mn, int mc, hy::Params &P, std::vector<double> &inst, std::vector<char> &up, size_t o_fld) -> std::string {
        if (const char *bad = hy::make_params(B, starts, goals, nOb, vOb, A, b, ego, L, XYbounds, opts, nopts, bucket_width, cap, mn, mc, P, W, blocked, inst)) return bad;
        M_ = W.b.size();
        const size_t nv = W.vert.size();
        o_int = (4 * M_ + nv) * 8; o_blk = o_int + up8((size_t)(3 * nOb + 2) * 4);
        up.assign(o_fld + up8(o_blk + blocked.size()), 0);
        char *u = up.data() + o_fld;
        if (M_) { memcpy(u, W.A.data(), 2 * M_ * 8); memcpy(u + 2 * M_ * 8, W.b.data(), M_ * 8); memcpy(u + 3 * M_ * 8, W.rn.data(), M_ * 8); }
        if (nv) memcpy(u + 4 * M_ * 8, W.vert.data(), nv * 8);
        int *ip = (int *)(u + o_int);
        for (int j = 0; j < nOb; j++) ip[j] = W.v[j];
        for (int j = 0; j <= nOb; j++) { ip[nOb + j] = W.off[j]; ip[2 * nOb + 1 + j] = W.voff[j]; }
        memcpy(u + o_blk, blocked.data(), blocked.size());
        return std::string();
    }, [&](const char *d, hy::Field &F, hy::Fields &) {
        F.nOb = nOb; F.v = (const int *)(d + o_int); F.off = F.v + nOb; F.voff = F.off + nOb + 1;
        F.A = (const double *)d; F.b = F.A + 2 * M_; F.rn = F.b + M_; F.vert = F.rn + M_;
        return (const unsigned char *)(d + o_blk);
    });
}

int obca_hybrid_ms(obca_ctx *ctx, float *ms) {
    return ctx && ms ? core_elapsed_ms(ctx, ctx->hyb.ev[0], ms, "obca_hybrid_ms: no search has run on this context") : -1;
}

// every search in the field of its own instance, put together on the device from the instance's record; the search finds the blocked cells itself.
// Field data: [ A | b | rn | nrm | vert | rec (B x 4) v off voff (ints) ]
int obca_scene_astar_batch(obca_ctx *ctx, int B, const double *starts, const double *goals, const int *nOb, const int *vOb, const double *A, const double *b,
                           const double ego[4], double L, const double XYbounds[4], const double *opts, int nopts, double bucket_width,
                           double *paths, int *dirs, int cap, int *counts, int *expansions, int *rounds) {
    hy::HostFields W;
    size_t M_ = 0, o_rec = 0;
    return hybrid_call(ctx, "obca_scene_astar_batch", 1, obca_hybrid_kernel<true>, B, paths, dirs, cap, counts, expansions, rounds,
                             [&](int mn, int mc, hy::Params &P, std::vector<double> &inst, std::vector<char> &up, size_t o_fld) -> std::string {
        const std::string bad = hy::make_scenes(B, starts, goals, nOb, vOb, A, b, ego, L, XYbounds, opts, nopts, bucket_width, cap, mn, mc, P, W, inst);
        if (!bad.empty()) return bad;
        M_ = W.b.size();
        const size_t nv = W.vert.size(), nob = W.v.size(), noff = W.off.size();      // (noff = nob + B)
        o_rec = (5 * M_ + nv) * 8;
        up.assign(o_fld + up8(o_rec + ((size_t)4 * B + nob + 2 * noff) * 4), 0);
        char *u = up.data() + o_fld;
        if (M_) {
            memcpy(u, W.A.data(), 2 * M_ * 8); memcpy(u + 2 * M_ * 8, W.b.data(), M_ * 8); memcpy(u + 3 * M_ * 8, W.rn.data(), M_ * 8);
            memcpy(u + 4 * M_ * 8, W.nrm.data(), M_ * 8);
        }
        if (nv) memcpy(u + 5 * M_ * 8, W.vert.data(), nv * 8);
        int *ip = (int *)(u + o_rec);
        memcpy(ip, W.rec.data(), (size_t)4 * B * 4);
        if (nob) memcpy(ip + 4 * B, W.v.data(), nob * 4);
        memcpy(ip + 4 * B + nob, W.off.data(), noff * 4); memcpy(ip + 4 * B + nob + noff, W.voff.data(), noff * 4);
        return bad;
    }, [&](const char *d, hy::Field &, hy::Fields &S) {
        S.rec = (const int *)(d + o_rec); S.v = S.rec + 4 * B; S.off = S.v + W.v.size(); S.voff = S.off + W.off.size();
        S.A = (const double *)d; S.b = S.A + 2 * M_; S.rn = S.b + M_; S.nrm = S.rn + M_; S.vert = S.nrm + M_;
        return (const unsigned char *)nullptr;
    });
}

int obca_scene_astar_ms(obca_ctx *ctx, float *ms) {
    return ctx && ms ? core_elapsed_ms(ctx, ctx->hyb.ev[1], ms, "obca_scene_astar_ms: no per-instance search has run on this context") : -1;
}

// ---- the resident route (obca_plan_resident.h, include/obca_plan_resident.h): packing -> the per-instance search -> the warm start, all three reading and writing device
// memory, on the batch's stream (the context's: the batch is one of the primary device).  The staging block's input part holds [ Params | inst | the packed fields
// (plr::Layout) | status B ]: only Params travels up, only counts, expansions, rounds and status come down.
int obca_batch_plan_warm_start(obca_batch *bt, const double *opts, int nopts, double bucket_width, int cap, int use_xF, double v_nom, double a_max,
                               int *counts, int *status, int *expansions, int *rounds) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    const char *entry = "obca_batch_plan_warm_start";
    auto refuse = [&](const std::string &what) { ctx->err = std::string(entry) + ": " + what; return -1; };
    if (!counts || !status) return refuse("NULL counts or status");
    if (cap < 2 || cap > OBCA_PATH_WS_MAXNODES) return refuse("need 2 <= cap <= OBCA_PATH_WS_MAXNODES");
    if (!bt->uploaded || !bt->have_geo) return refuse("nothing uploaded by obca_batch_upload (a batch that obca_batch_refine_into filled starts from a solution)");
    if (bt->device != ctx->device || bt->stream != ctx->stream) return refuse("the batch is not one of its context's primary device");
    if (const char *bad = pw::path_ws_check_args(bt->B, bt->N, cap, v_nom, 1.0, a_max, true)) return refuse(bad);
    const int B = bt->B;
    if ((double)B * bt->nObMax * PLR_NV > 2e9 || (double)B * bt->MMax > 2e9) return refuse("the batch is too large for the planner's 32-bit offsets");
    // the parameter block: make_params with no field and no poses of the caller's (one pose at the origin: P depends on neither), as make_scenes calls it
    int mn, mc; hybrid_sizes(ctx, mn, mc);
    hy::Params P; hy::HostField none; std::vector<unsigned char> free_map; std::vector<double> pose;
    const double origin[3] = {0.0, 0.0, 0.0};
    if (const char *bad = hy::make_params(1, origin, origin, 0, nullptr, nullptr, nullptr, bt->ego, bt->L, bt->XYb, opts, nopts, bucket_width, cap, mn, mc, P, none, free_map, pose)) return refuse(bad);
    use_device(bt->device);
    PlanRun &pr = bt->plan;
    for (EventPair &e : pr.ev) { if (int rc = e.ensure(ctx->err)) return rc; e.timed = 0; }
    pr.serial = 0;
    const plr::Layout lay = plr::layout(B, bt->nObMax, bt->MMax);
    const size_t o_st = up8(sizeof(hy::Params)) + lay.bytes;
    HybridRun r;
    if (int rc = hybrid_reserve(ctx, entry, 1, obca_hybrid_kernel<true>, B, cap, P, mn, mc, o_st + up8((size_t)B * 4), r)) return rc;
    const plr::Block blk = plr::block_at(r.d + r.o_inst, lay);      // (inst first: where hybrid_launch points the search's instance records)
    int *dst = (int *)(r.d + o_st);
    const double far_ = hy::host_far(bt->XYb);
    // from here on the record and the start iterate may be rewritten, whatever becomes of the call (obca_batch_set_path_warm_start)
    bt->solved = 0; bt->have_duals = 0;
    static_assert(sizeof P == 1288, "tools/plan_resident_rate.py records this size as what the call sends up");
    const bool sent = hipMemcpyAsync(r.d, &P, sizeof P, hipMemcpyHostToDevice, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;      // (P is pageable)
    std::vector<int> down((size_t)4 * B);
    int rc = launch_timed(ctx->err, entry, ctx->stream, pr.ev[0], sent, [&] {
        hipLaunchKernelGGL(plr::obca_plan_pack_kernel, dim3(B), dim3(PLR_NT), 0, ctx->stream, B, bt->nObMax, bt->MMax, far_, (const double *)bt->d.prob, bt->d.s_prob, blk);
    }, {});
    if (!rc) rc = launch_timed(ctx->err, entry, ctx->stream, pr.ev[1], true, [&] { hybrid_launch(ctx, obca_hybrid_kernel<true>, r, hy::Field(), plr::fields_of(blk), nullptr); }, {});
    if (!rc) rc = launch_timed(ctx->err, entry, ctx->stream, pr.ev[2], true, [&] {
        hipLaunchKernelGGL(obca_path_ws_batch_kernel, dim3(B), dim3(OB_NT), 0, ctx->stream, B, bt->N, (const double *)(r.d + r.o_paths), (const int *)(r.d + r.o_dirs), (const int *)r.counts(),
                           cap, cap, use_xF ? 1 : 0, v_nom, a_max, bt->d, dst);
    }, {{down.data(), r.counts(), (size_t)3 * B * sizeof(int)}, {down.data() + (size_t)3 * B, dst, (size_t)B * sizeof(int)}});
    if (rc) { ctx->hyb.release(); return rc; }
    for (int i = 0; i < B; i++) { counts[i] = down[i]; if (expansions) expansions[i] = down[B + i]; if (rounds) rounds[i] = down[2 * B + i]; status[i] = down[(size_t)3 * B + i]; }
    pr.serial = ctx->hyb.serial; pr.cap = cap; pr.B = B; pr.nObMax = bt->nObMax; pr.MMax = bt->MMax; pr.o_inst = r.o_inst; pr.o_paths = r.o_paths; pr.o_dirs = r.o_dirs;
    return 0;
}

int obca_batch_plan_ms(obca_batch *bt, float *pack_ms, float *search_ms, float *ws_ms) {
    if (!bt || !pack_ms || !search_ms || !ws_ms) return -1;
    float *out[3] = {pack_ms, search_ms, ws_ms};
    for (int k = 0; k < 3; k++) if (int rc = core_elapsed_ms(bt->ctx, bt->plan.ev[k], out[k], "obca_batch_plan_ms: no plan call has run on this batch")) return rc;
    return 0;
}

int obca_batch_plan_download(obca_batch *bt, double *paths, int *dirs, int cap, double *inst) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx; const PlanRun &pr = bt->plan; const HybridBufs &h = ctx->hyb;
    if (!pr.serial || pr.serial != h.serial || !h.io) { ctx->err = "obca_batch_plan_download: no plan of this batch is in the planner's staging block (none has run, or a later planner call of the context took it)"; return -1; }
    if (!paths && !dirs && !inst) return pr.cap;      // the query: how many rows the arrays of a download need
    if (cap != pr.cap) { ctx->err = "obca_batch_plan_download: cap is not the last call's"; return -1; }
    use_device(bt->device);
    const size_t B = pr.B;
    bool ok = true;
    if (paths) ok = ok && hipMemcpyAsync(paths, h.io + pr.o_paths, B * cap * 24, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    if (dirs) ok = ok && hipMemcpyAsync(dirs, h.io + pr.o_dirs, B * cap * 4, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    if (inst) ok = ok && hipMemcpyAsync(inst, h.io + pr.o_inst, B * 80, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || !ok) { ctx->err = "obca_batch_plan_download: copy failed"; return -2; }
    return 0;
}

// the diagnostic of include/obca_plan_resident_check.h: the block the packing kernel of the last obca_batch_plan_warm_start wrote, as it lies on the device
int obca_batch_packed_block(obca_batch *bt, double *block, int ndoubles, int *dims) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx; const PlanRun &pr = bt->plan; const HybridBufs &h = ctx->hyb;
    if (!dims) { ctx->err = "obca_batch_packed_block: NULL dims"; return -1; }
    if (!pr.serial || pr.serial != h.serial || !h.io) { ctx->err = "obca_batch_packed_block: no plan of this batch is in the planner's staging block (none has run, or a later planner call of the context took it)"; return -1; }
    const size_t need = plr::layout(pr.B, pr.nObMax, pr.MMax).bytes / 8;
    if (need > 2000000000u) { ctx->err = "obca_batch_packed_block: the block is too large for this call"; return -1; }
    dims[0] = pr.B; dims[1] = pr.nObMax; dims[2] = pr.MMax; dims[3] = (int)need; dims[4] = h.slot_allocs; dims[5] = h.io_allocs;
    if (!block) return 0;
    if ((size_t)std::max(ndoubles, 0) < need) { ctx->err = "obca_batch_packed_block: the array is shorter than dims[3] doubles"; return -1; }
    use_device(bt->device);
    if (hipMemcpyAsync(block, h.io + pr.o_inst, need * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "obca_batch_packed_block: copy failed"; return -2; }
    return 0;
}

// ---- the quadcopter's resident route (obca_quad_plan_resident.h, include/obca_quad_plan_resident.h): the grid search from the records of an uploaded batch, on the batch's
// stream.  The stage holds ints [ sel n | counts B | sweeps B ]: the selection, -4 in every count and 0 in every sweep go up in one copy, the kernel overwrites the words of
// the instances it plans, counts and sweeps come down.
int obca_quad_batch_grid_plan_warm_start(obca_quad_batch *bt, double clear, const double room[3], double res, int cap, const int *sel, int n, const double *timeWS, int *counts, int *sweeps) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    const char *entry = "obca_quad_batch_grid_plan_warm_start";
    auto refuse = [&](const std::string &what) { ctx->err = std::string(entry) + ": " + what; return -1; };
    const int B = bt->B;
    int dims[3];
    if (const char *bad = qpr::check_args(B, bt->N, clear, room, res, cap, sel, n, timeWS, counts, dims)) return refuse(bad);
    if (!bt->uploaded) return refuse("nothing uploaded");
    if (bt->device != ctx->device || bt->stream != ctx->stream) return refuse("the batch is not one of its context's primary device");
    if (!sel) n = B;
    use_device(bt->device);
    KernelStage &w = bt->gp;
    if (int rc = w.ev.ensure(bt->err)) return fin(bt, rc);
    const size_t nints = (size_t)n + 2 * (size_t)B, npath = (size_t)B * cap * 3;
    if (w.dev.reserve((nints + 1) / 2, bt->stream) != hipSuccess || bt->gp_paths.reserve(npath, bt->stream) != hipSuccess) { ctx->err = std::string(entry) + ": hipMalloc failed"; return -2; }
    if (w.host.reserve(bt->err, (nints + 1) / 2)) return fin(bt, -2);
    const int ncell = dims[0] * dims[1] * dims[2], lds = (ncell + 4) * (int)sizeof(float);
    if (lds > ctx->gp_lds) {
        if (hipFuncSetAttribute((const void *)qpr::obca_quad_plan_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) { ctx->err = std::string(entry) + ": hipFuncSetAttribute failed"; return -2; }
        ctx->gp_lds = lds;
    }
    int *hs = (int *)w.host.p, *dsel = (int *)w.dev.p, *dcnt = dsel + n, *dsw = dcnt + B;
    for (int j = 0; j < n; j++) hs[j] = sel ? sel[j] : j;
    for (int i = 0; i < B; i++) { hs[n + i] = OBCA_QUAD_PLAN_SKIPPED; hs[n + B + i] = 0; }
    // from here on the records may be rewritten, whatever becomes of the call: the batch counts as unsolved, as after an upload
    bt->solved = 0; bt->gp_cap = 0;
    const bool up = hipMemcpyAsync(dsel, hs, nints * sizeof(int), hipMemcpyHostToDevice, bt->stream) == hipSuccess &&
                    hipMemsetAsync(bt->gp_paths.p, 0, npath * sizeof(double), bt->stream) == hipSuccess;      // (the rows of a skipped instance read as zeros)
    const QDevBufs &d = bt->d;
    const int rc = launch_timed(ctx->err, entry, bt->stream, w.ev, up, [&] {
        hipLaunchKernelGGL(qpr::obca_quad_plan_resident_kernel, dim3(n), dim3(PL3_NT), lds, bt->stream, (const int *)dsel, n, B, bt->N, d.prob, d.s_prob, clear, room[0], room[1], room[2], res,
                           dims[0], dims[1], dims[2], bt->gp_paths.p, cap, dcnt, dsw, timeWS ? 1 : 0, timeWS ? *timeWS : 0.0);
    }, {{hs + n, dcnt, (size_t)2 * B * sizeof(int)}});
    if (rc) return rc;
    memcpy(counts, hs + n, (size_t)B * sizeof(int));
    if (sweeps) memcpy(sweeps, hs + n + B, (size_t)B * sizeof(int));
    bt->gp_cap = cap;
    return 0;
}

int obca_quad_batch_grid_plan_ms(obca_quad_batch *bt, float *ms) {
    return bt && ms ? core_elapsed_ms(bt->ctx, bt->gp.ev, ms, "obca_quad_batch_grid_plan_ms: no plan call has run on this batch") : -1;
}

int obca_quad_batch_grid_plan_download(obca_quad_batch *bt, double *paths, int cap) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    if (bt->gp_cap < 2) { ctx->err = "obca_quad_batch_grid_plan_download: no plan call has run on this batch"; return -1; }
    if (!paths) return bt->gp_cap;      // the query: how many rows per instance the array of a download needs
    if (cap != bt->gp_cap) { ctx->err = "obca_quad_batch_grid_plan_download: cap is not the last call's"; return -1; }
    use_device(bt->device);
    if (hipMemcpyAsync(paths, bt->gp_paths.p, (size_t)bt->B * cap * 3 * sizeof(double), hipMemcpyDeviceToHost, bt->stream) != hipSuccess || hipStreamSynchronize(bt->stream) != hipSuccess) {
        ctx->err = "obca_quad_batch_grid_plan_download: copy failed"; return -2;
    }
    return 0;
}

int obca_quad_batch_start_download(obca_quad_batch *bt, double *xWS, double *timeWS) {
    if (!bt) return -1;
    obca_ctx *ctx = bt->ctx;
    if (!xWS && !timeWS) { ctx->err = "obca_quad_batch_start_download: NULL arguments"; return -1; }
    if (!bt->uploaded) { ctx->err = "obca_quad_batch_start_download: nothing uploaded"; return -1; }
    const QDevBufs &d = bt->d; const size_t B = bt->B, nws = (size_t)QX * (bt->N + 1);
    use_device(bt->device);
    // through the pinned problem staging of the batch (an upload refills it, the shift uses it as scratch the same way): the records as they lie
    if (bt->h_prob.reserve(bt->err, (size_t)bt->cap * d.s_prob)) return fin(bt, -2);
    if (hipMemcpyAsync(bt->h_prob, d.prob, B * d.s_prob * sizeof(double), hipMemcpyDeviceToHost, bt->stream) != hipSuccess || hipStreamSynchronize(bt->stream) != hipSuccess) {
        ctx->err = "obca_quad_batch_start_download: copy failed"; return -2;
    }
    for (size_t i = 0; i < B; i++) {
        const double *p = bt->h_prob + i * d.s_prob;
        if (xWS) memcpy(xWS + i * nws, p + QPH_SIZE, nws * sizeof(double));
        if (timeWS) timeWS[i] = p[QPH_TWS];
    }
    return 0;
}

}  // extern "C"
