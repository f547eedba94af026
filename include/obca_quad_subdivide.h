/*
 * obca_quad_subdivide.h -- C ABI of the refinement of solved quadcopter batches onto a finer horizon on the GPU (exported by libobca_hip.so; kernel text:
 * obca_amd/csrc/obca_quad_subdivide.h).  The parking counterpart is include/obca_refine.h.
 *
 * The quadcopter NLP holds the obstacle separation at the N + 1 nodes only; obca_quad_batch_clearance (include/obca_clearance.h) finds the solutions that lose it between the
 * nodes.  These calls turn instance i of a solved batch with horizon N into an instance of the SAME NLP with horizon N' = factor N (r = factor,
 * 1 .. OBCA_QUAD_SUBDIVIDE_MAXFACTOR, r N <= OBCA_QUAD_NMAX), started from the solution.  Write q = k r + s with 0 <= s < r; q = r N is the last node.
 *   problem   : every word of the record as uploaded or shifted (x0, xF, the boxes, the formulation) except Ts' = Ts / r and R' = R + margin (margin >= 0; a finer grid shrinks
 *               the cut between the nodes but the chord across a box's rounded corner always sags inside: a small margin closes it)
 *   warm start: all 12 states.  x'[q] = node k of the solution at s = 0 (and x'[r N] = x_N), bit for bit; positions at s > 0: p_k + (s / r) t Ts v_k, the forward-Euler partial
 *               step (QuadcopterSignedDist.jl:138-140) and the point obca_quad_batch_clearance samples as (k, s) at substeps = r -- the refined NLP constrains the very points
 *               that call looked at; the other nine states at s > 0: x_k + (s / r)(x_{k+1} - x_k)
 *   timeWS, dual_ws: the solution's t, 1 (closed-form duals of the new positions) -- as obca_quad_batch_shift_warm_start leaves them.  Inputs restart at hover and slacks at 1 as
 *               every quadcopter solve does: there is no `duals` option
 * status[j] -- 0: refined from the solution; 1: the source's last solve ended with exit flag 0 (nothing is then read from its iterate) or x / t of its iterate are not finite:
 * all 12 states interpolated linearly from the source's own uploaded warm start, timeWS and dual_ws as uploaded; -1: that warm start is not finite either: zeros, timeWS = 1,
 * dual_ws = 1.
 * One wavefront per destination instance, one launch per call, nothing but the selection and `status` crosses the bus in the resident call.
 * Return values: 0; -1 bad arguments (see each call); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_QUAD_SUBDIVIDE_H
#define OBCA_QUAD_SUBDIVIDE_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_QUAD_SUBDIVIDE_MAXFACTOR 32     /* largest factor */

/* Instance sel[j] of `src` becomes instance j of `dst` (duplicates allowed); sel: n indices or NULL = 0 .. n-1; status: n.  -1: a NULL batch or status, dst == src or
 * batches of different contexts or streams, `src` not solved since its last upload or shift, dst's horizon != factor * src's, factor outside
 * 1 .. OBCA_QUAD_SUBDIVIDE_MAXFACTOR, factor * N > OBCA_QUAD_NMAX, n < 1 or above dst's capacity, an index outside 0 .. B_src - 1, a negative or non-finite margin; both
 * batches stay as they were.  Afterwards `dst` holds n instances, uploaded and not solved: obca_quad_batch_solve runs them, obca_quad_batch_download returns them in the order
 * of the selection, obca_quad_batch_validate and obca_quad_batch_clearance use R + margin (clearance against the true radius: need = -margin).  Both batches use their
 * context's stream: the call is ordered behind src's solve. */
int obca_quad_batch_subdivide_into(obca_quad_batch *dst, obca_quad_batch *src, int factor, double margin, const int *sel /* n, or NULL = 0 .. n-1 */, int n, int *status /* n */);
/* duration of the last subdivide kernel into this batch [ms], measured with HIP events on its stream */
int obca_quad_batch_subdivide_ms(obca_quad_batch *dst, float *ms);
/* the trajectory part for any trajectories, host arrays in and out, one launch: x 12 x (N + 1) per instance, stage-contiguous, and timeScale (N + 1) x B as
 * obca_quadcopter_clearance_batch takes them, timeScale used per stage, NULL = 1; Ts_f: B (= Ts / factor), x_f: 12 x (factor N + 1) x B.  An instance with a non-finite number
 * among its Ts, x, timeScale gets NaN in both outputs, no other instance is touched.  1 <= N, factor N <= OBCA_QUAD_NMAX. */
int obca_quadcopter_subdivide_batch(obca_ctx *ctx, int B, int N, int factor, const double *Ts, const double *x, const double *timeScale /* (N + 1) x B or NULL = 1 */,
                                    double *Ts_f, double *x_f);

#ifdef __cplusplus
}
#endif
#endif
