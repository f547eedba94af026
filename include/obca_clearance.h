/*
 * obca_clearance.h -- C ABI of the clearance check BETWEEN the nodes of a trajectory on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_clearance.h).
 *
 * Both NLPs hold the obstacle separation at the N + 1 nodes only, and the validate calls of include/obca_hip.h look at the same rows at the same nodes.  These calls sample
 * every interval `substeps` (S, 1 .. OBCA_CLR_MAXSUB) times with the discretisation's own partial step and compute the distance of every sample to every obstacle anew:
 * samples q = k S + s (k = 0 .. N-1, s = 0 .. S-1) and q = N S (node N), N S + 1 per instance; the node samples are those with s = 0 and the last one.
 *   parking   : the pose of (k, s) is the bicycle step of ParkingSignedDist.jl:147-150 from node k with u_k over (s / S) timeScale[k] Ts; its clearance to obstacle j is the
 *               DualMultWS distance of that pose (the car's rectangle against the polygon), 0 below OBCA_CLR_TOUCH: 0 means "touches or overlaps", no penetration depth.
 *   quadcopter: the point p_k + (s / S) timeScale[k] Ts v_k (QuadcopterSignedDist.jl:138-140); clearance = its Euclidean distance to box j (0 inside) - R, so >= -R.
 * One wavefront per instance, one launch per call; OBCA_CLR_OUT doubles per instance come back:
 *   [0] min        the smallest clearance over all samples and obstacles        [1] min_nodes  the same over the node samples only
 *   [2] sample     q of the minimum (ties: the smallest q, then the smallest j) [3] obstacle   j of the minimum
 *   [4] below      number of samples whose smallest clearance is < need         [5] samples    N S + 1
 *   [6] bad        1: a non-finite number in the trajectory (Ts, x, u, timeScale) or among the clearances; then [0], [1], [8..] are NaN, [2] = [3] = -1, [4] = [5]
 *   [7] 0          [8 .. 23] the smallest clearance per obstacle, +inf behind the instance's obstacles (the quadcopter uses 5)
 * Array layouts and obstacle conventions are those of obca_parking_constraints_batch and obca_quadcopter_constr_satisfaction_batch; the trajectory is packed by the upload
 * code of the solves (rows normalised the same way), so a host-pointer call on a downloaded solution sees the numbers the resident call sees.
 * Return values: 0; -1 bad arguments (substeps outside 1 .. OBCA_CLR_MAXSUB, a non-finite need, a NULL array, a horizon out of range, a resident batch on which nothing
 * has been solved since the last upload, shift or path warm start); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_CLEARANCE_H
#define OBCA_CLEARANCE_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_CLR_OUT 24        /* doubles per instance */
#define OBCA_CLR_MAXSUB 32     /* most sub-steps per interval */
#define OBCA_CLR_TOUCH 1e-7    /* a parking distance below this is reported as 0 */

/* the last solution of a resident batch (the iterate is read, nothing is written to the batch); out: OBCA_CLR_OUT x B */
int obca_batch_clearance(obca_batch *bt, int substeps, double need, double *out);
/* duration of the last obca_batch_clearance kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_clearance_ms(obca_batch *bt, float *ms);
/* any trajectories: x 4 x (N + 1), u 2 x N per instance, timeScale (N + 1) x B or NULL (= 1); 1 <= N <= OBCA_NMAX; chunked over the slots and devices of the context */
int obca_parking_clearance_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                                 const int *nOb, const int *vOb, const double *A, const double *b,
                                 const double *x, const double *u, const double *timeScale, int substeps, double need, double *out);

int obca_quad_batch_clearance(obca_quad_batch *bt, int substeps, double need, double *out);
int obca_quad_batch_clearance_ms(obca_quad_batch *bt, float *ms);
/* x 12 x (N + 1) per instance, timeScale (N + 1) x B, ob 5 x 6 per instance as [hi; -lo]; 2 <= N <= OBCA_QUAD_NMAX */
int obca_quadcopter_clearance_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                    const double *x, const double *timeScale, int substeps, double need, double *out);

#ifdef __cplusplus
}
#endif
#endif
