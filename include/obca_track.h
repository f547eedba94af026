/*
 * obca_track.h -- C ABI of the closed-loop rollout: time-varying LQR gains about a trajectory and the tracked trajectory on the CONTINUOUS vehicle models, on the GPU
 * (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_track.h).
 *
 * The rollout calls (obca_rollout.h) apply the solved inputs open loop.  These calls execute a trajectory the standard way: a finite-horizon LQR about it.
 *   interval map: Phi_k(X, U) = the state after `substeps` (S, 1 .. OBCA_ROLL_MAXSUB) classical RK4 steps of timeScale[k] Ts / S from X with U held -- what the rollout
 *                 applies; A_k = dPhi_k/dX, B_k = dPhi_k/dU at (x_k, u_k), by forward-mode tangents through the same steps (no finite differences)
 *   gains       : P_N = diag(qf); k = N-1 .. 0: G = diag(r) + B'PB, K_k = -G^-1 B'PA (unpivoted Cholesky), P <- diag(q) + A'PA + (B'PA)' K_k, P <- (P + P')/2
 *   closed loop : X_0 = x[:, 0] + dx0; U_k = u_k + K_k (X_k - x_k) if `feedback`, else u_k; if `clamp`, clipped to the NLP's own input bounds (parking |delta| <= 0.6,
 *                 |a| <= 0.4; quadcopter 1.2 <= u <= 7.8); X_{k+1} = Phi_k(X_k, U_k)
 * The feedback is evaluated at the nodes and HELD over the interval; state differences are taken raw, no angle is wrapped.
 * One wavefront per instance, one launch per call; OBCA_TRK_OUT doubles per instance come back:
 *   [0 .. 39]  the record of include/obca_rollout.h for the chain, field for field: deviations of X_k from x_k over k = 1 .. N, the clearance record of the N S + 1
 *              samples with `need`; [10] = 0, [11] = S
 *   [40] feedback   [41] clamp   [42] saturated: the number of intervals in which an input was clipped
 *   [43] du_max     the largest |U_k - u_k| over all inputs and intervals   [44] du_node  its interval (ties: the smallest)
 *   [45] dx0_pos    |dx0| of the position part (0 without dx0)              [46], [47] 0
 * [0] bad = 1: what the rollout calls bad (a non-finite number in the trajectory or among the rolled states, a quadcopter step across cos x[3] = 0), a dx0 that is not
 * finite, or a pivot of a G that is not finite and positive.  Then [0 .. 39] are the rollout's bad record, [42] = [44] = -1, [43] = [45] = NaN, and the gains and node
 * states of the instance are NaN.  An instance is marked alone.
 * The gains K (N x nu x nx per instance, stage after stage, K_k row-major: u = u_k + K_k (X_k - x_k)) and the node states X ((N + 1) x nx per instance) stay on the device
 * until the *_gains / *_states calls fetch them.  The resident calls read the last solution and write nothing into the batch; the node states of an earlier rollout
 * (obca_batch_rollout_states) stay valid.
 * Array layouts, obstacle conventions and chunking are those of the rollout calls.  Return values: 0; -1 bad arguments (those of the rollout calls; feedback or clamp
 * outside 0 / 1; a NULL weight array; a q or qf entry that is negative or not finite; an r entry that is not positive or not finite; *_states / *_gains before a track
 * call on the batch); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_TRACK_H
#define OBCA_TRACK_H
#include "obca_rollout.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_TRK_OUT 48         /* doubles per instance */

/* the last solution of a resident batch tracked on the bicycle; dx0: 4 x B or NULL; out: OBCA_TRK_OUT x B */
int obca_batch_track(obca_batch *bt, int substeps, int feedback, int clamp, const double q[4], const double r[2], const double qf[4], const double *dx0, double need, double *out);
/* duration of the last obca_batch_track kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_track_ms(obca_batch *bt, float *ms);
/* the node states of the last obca_batch_track on this batch; X: (N + 1) x 4 per instance */
int obca_batch_track_states(obca_batch *bt, double *X);
/* its gains; K: N x 2 x 4 per instance */
int obca_batch_track_gains(obca_batch *bt, double *K);
/* any trajectories: the arguments of obca_parking_rollout_batch up to timeScale; X: (N + 1) x 4 x B or NULL; K: N x 2 x 4 x B or NULL; chunked over the slots */
int obca_parking_track_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                             const int *nOb, const int *vOb, const double *A, const double *b,
                             const double *x, const double *u, const double *timeScale, int substeps, int feedback, int clamp,
                             const double q[4], const double r[2], const double qf[4], const double *dx0, double need, double *out, double *X, double *K);

/* the quadcopter: dx0 12 x B or NULL */
int obca_quad_batch_track(obca_quad_batch *bt, int substeps, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, double need, double *out);
int obca_quad_batch_track_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_track_states(obca_quad_batch *bt, double *X);
/* K: N x 4 x 12 per instance */
int obca_quad_batch_track_gains(obca_quad_batch *bt, double *K);
/* the arguments of obca_quadcopter_rollout_batch up to timeScale; X: (N + 1) x 12 x B or NULL; K: N x 4 x 12 x B or NULL */
int obca_quadcopter_track_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                const double *x, const double *u, const double *timeScale, int substeps, int feedback, int clamp,
                                const double q[12], const double r[4], const double qf[12], const double *dx0, double need, double *out, double *X, double *K);

#ifdef __cplusplus
}
#endif
#endif
