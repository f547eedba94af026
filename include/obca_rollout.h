/*
 * obca_rollout.h -- C ABI of the rollout of trajectories on the CONTINUOUS vehicle models on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_rollout.h).
 *
 * The validate and clearance calls measure a solution against the NLP's own discretisation.  These calls apply the inputs to the model the discretisation stands for:
 * u_k is held over interval k of length timeScale[k] Ts and the model is integrated with classical RK4, `substeps` (S, 1 .. OBCA_ROLL_MAXSUB) equal steps per interval.
 *   parking   : x' = v cos psi, y' = v sin psi, psi' = v tan(delta) / L, v' = a    (ParkingSignedDist.jl:147-150 steps this bicycle with the midpoint rule)
 *   quadcopter: the rigid body that QuadcopterSignedDist.jl:138-155 steps with forward Euler, the gyroscopic products at the current rates
 *   restart 0 : chain -- the open loop from x[:, 0]: X_0 = x[:, 0], X_{k+1} = the state S steps after X_k
 *   restart 1 : every interval starts at the trajectory's own node: X_{k+1} = the state S steps after x[:, k] -- the defect of one interval, nothing compounds
 * Samples are those of include/obca_clearance.h, q = k S + s and q = N S: sample (k, s >= 1) is the state after s steps of interval k, sample (k, 0) is X_k (chain) or the
 * node x[:, k] (restart), the last sample likewise.  Their clearance is computed as the clearance calls compute it.
 * One wavefront per instance, one launch per call; OBCA_ROLL_OUT doubles per instance come back:
 *   [0] bad       1: a non-finite number in the trajectory (Ts, x, u, timeScale), or a rolled state that is not finite or steps across cos x[3] = 0 (the quadcopter's
 *                 pitch through pi/2: the continuous state diverges there); then [1], [3..9], [16], [17], [24..] are NaN, [2] = [18] = [19] = -1, [20] = [21]
 *   [1] dev_pos   the largest |P(X_k) - P(x_k)|_2 over the nodes k = 1 .. N       [2] dev_node  its node (ties: the smallest)
 *   [3] dev_att   parking |psi|, quadcopter max-abs over states 4-6               [4] dev_vel   parking |v|, quadcopter Euclidean over states 7-9
 *   [5] dev_rate  quadcopter max-abs over states 10-12, parking 0                 [6 .. 9] the same four at node N
 *   [10] restart  [11] S  [12 .. 15] 0
 *   [16 .. 39]    the OBCA_CLR_OUT doubles of include/obca_clearance.h for the samples, field for field
 * The rolled node states X stay on the device until the *_states call fetches them, (N + 1) x nx per instance (nx = 4 / 12), stage after stage; NaN where bad.
 * Array layouts and obstacle conventions are those of the clearance calls.  The resident calls read the last solution and write nothing into the batch.
 * Return values: 0; -1 bad arguments (restart outside 0 / 1, substeps outside 1 .. OBCA_ROLL_MAXSUB, a non-finite need, a NULL array, a horizon out of range, a resident
 * batch on which nothing has been solved since the last upload, shift or path warm start, *_states before a rollout of the batch); -2 device error.  The message is
 * obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_ROLLOUT_H
#define OBCA_ROLLOUT_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_ROLL_OUT 40        /* doubles per instance */
#define OBCA_ROLL_CLR 16        /* where the clearance record starts */
#define OBCA_ROLL_MAXSUB 32     /* most RK4 steps per interval */

/* the last solution of a resident batch on the bicycle; out: OBCA_ROLL_OUT x B */
int obca_batch_rollout(obca_batch *bt, int substeps, int restart, double need, double *out);
/* duration of the last obca_batch_rollout kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_rollout_ms(obca_batch *bt, float *ms);
/* the node states of the last obca_batch_rollout on this batch; X: (N + 1) x 4 per instance */
int obca_batch_rollout_states(obca_batch *bt, double *X);
/* any trajectories: x 4 x (N + 1), u 2 x N per instance, timeScale (N + 1) x B or NULL (= 1); 1 <= N <= OBCA_NMAX; X: (N + 1) x 4 x B or NULL; chunked over the slots */
int obca_parking_rollout_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                               const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, int substeps, int restart, double need, double *out, double *X);

int obca_quad_batch_rollout(obca_quad_batch *bt, int substeps, int restart, double need, double *out);
int obca_quad_batch_rollout_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_rollout_states(obca_quad_batch *bt, double *X);
/* x 12 x (N + 1), u 4 x N per instance, timeScale (N + 1) x B, ob 5 x 6 per instance as [hi; -lo]; 2 <= N <= OBCA_QUAD_NMAX; X: (N + 1) x 12 x B or NULL */
int obca_quadcopter_rollout_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                  const double *x, const double *u, const double *timeScale, int substeps, int restart, double need, double *out, double *X);

#ifdef __cplusplus
}
#endif
#endif
