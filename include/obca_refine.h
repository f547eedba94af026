/*
 * obca_refine.h -- C ABI of the refinement of solved parking batches onto a finer horizon on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_refine.h).
 *
 * Both NLPs hold the obstacle separation at the N + 1 nodes only; obca_batch_clearance (include/obca_clearance.h) finds the solutions that lose it between the nodes.  The
 * remedy for a constraint held at the nodes is a finer grid: these calls turn instance i of a solved batch with horizon N into an instance of the SAME NLP with horizon
 * N' = factor N (r = factor, 1 .. OBCA_REFINE_MAXFACTOR, r N <= OBCA_NMAX), started from the solution.  Write q = k r + s with 0 <= s < r; q = r N is the last node.
 *   problem   : every word of the record as uploaded (x0, xF, bounds, L, the obstacles' unit rows, fixTime, formulation) except Ts' = Ts / r
 *   reference : rx, ry, ryaw: ref'[q] = ref[k] + (s / r)(ref[k+1] - ref[k]), ref[k] itself at s = 0
 *   x         : x'[q] = node k of the solution at s = 0 (and x'[r N] = x_N), bit for bit; else the bicycle step of ParkingSignedDist.jl:147-150 from node k with u_k over
 *               (s / r) t Ts (t: the solution's timeScale, 1 with fixTime) -- the pose obca_batch_clearance samples as (k, s) at substeps = r: the refined NLP constrains the
 *               very poses that call looked at
 *   u, t      : u'[q] = u_k (zero-order hold), t' = 1
 *   lam, mu   : duals = 0: none, the destination's next solve runs DualMultWS (the contract of obca_batch_set_path_warm_start); duals = 1: stage q takes the
 *               multipliers of stage q / r as stored, and the destination counts as having a dual warm start
 * status[j] -- 0: refined from the solution; 1: the source's last solve ended with exit flag 0 or its iterate (x, u, t; with duals also lam, mu) is not finite: refined the
 * same way from the source's start iterate (with duals: the uploaded multipliers, or zeros); -1: that is not finite either: x' = u' = 0, t' = 1, zero multipliers.
 * One wavefront per destination instance, one launch per call, nothing but `status` crosses the bus in the resident call.
 * Return values: 0; -1 bad arguments (see each call); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_REFINE_H
#define OBCA_REFINE_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_REFINE_MAXFACTOR 32     /* largest factor */

/* Instance sel[j] of `src` becomes instance j of `dst` (duplicates allowed); sel: n indices or NULL = 0 .. n-1; status: n.  -1: a NULL batch or status, dst == src or
 * batches of different contexts, `src` not solved since its last upload, shift or path warm start, dst's horizon != factor * src's, factor outside
 * 1 .. OBCA_REFINE_MAXFACTOR, n < 1 or above dst's capacity, an index outside 0 .. B_src - 1, duals not 0 or 1.  Afterwards `dst` holds n instances, uploaded and not solved:
 * obca_batch_solve runs them, obca_batch_download returns lambda in the caller's row scaling and the packed outputs in the order of the selection.  Both batches use their
 * context's stream: the call is ordered behind src's solve. */
int obca_batch_refine_into(obca_batch *dst, obca_batch *src, int factor, int duals, const int *sel /* n, or NULL = 0 .. n-1 */, int n, int *status /* n */);
/* duration of the last refine kernel into this batch [ms], measured with HIP events on its stream */
int obca_batch_refine_ms(obca_batch *dst, float *ms);
/* the primal part for any trajectories, host arrays in and out, one launch: x 4 x (N + 1), u 2 x N per instance, timeScale (N + 1) x B or NULL (= 1), used per stage as in
 * obca_parking_clearance_batch; Ts_f: B (= Ts / factor), x_f: 4 x (factor N + 1) x B, u_f: 2 x factor N x B.  An instance with a non-finite number among its Ts, x, u,
 * timeScale gets NaN in all three outputs.  1 <= N, factor N <= OBCA_NMAX. */
int obca_parking_refine_batch(obca_ctx *ctx, int B, int N, int factor, const double *Ts, double L, const double *x, const double *u,
                              const double *timeScale /* (N + 1) x B or NULL = 1 */, double *Ts_f, double *x_f, double *u_f);

#ifdef __cplusplus
}
#endif
#endif
