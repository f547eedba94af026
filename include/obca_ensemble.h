/*
 * obca_ensemble.h -- C ABI of the closed-loop ensemble: up to 64 disturbed closed-loop rollouts about every trajectory of a batch, on the CONTINUOUS vehicle models, on the GPU
 * (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_ensemble.h).
 *
 * The closed-loop call (obca_track.h) rolls the loop from ONE start offset.  These calls answer how far the vehicle strays, and how close it comes to the obstacles, over a
 * spread of start offsets and actuator biases.  Models, interval map, RK4, `substeps` (S) and the zero-order hold are those of obca_track.h.
 *   gains       : K_k of obca_track.h for the weights q, r, qf; computed once per instance and shared by all members
 *   member m    : m = 0 .. members - 1, 1 <= members (M) <= OBCA_ENS_MMAX.  X_0 = x[:, 0] + dx0[m]; commanded input u_k + K_k (X_k - x_k) if `feedback`, else u_k;
 *                 applied input U_k = commanded + dub[m], clipped to the NLP's own input bounds if `clamp`; X_{k+1} = Phi_k(X_k, U_k).  dub is a constant input bias per
 *                 member (an actuator offset).
 *   clearance   : every sample a member passes (q = k S + s, and q = N S) is measured as the rollout calls measure it; the member keeps its smallest clearance (ties: the
 *                 smallest sample, then the smallest obstacle) and the number of samples under `need`
 * One wavefront per instance, one member per lane, one launch per call.
 * Per member OBCA_ENS_MEM doubles, which stay on the device until the *_members calls fetch them:
 *   [0] bad   [1] dev_pos: the largest position deviation of X_k from x_k over k = 1 .. N   [2] its node   [3] end_pos: the same at node N
 *   [4] dev_att   [5] dev_vel   [6] dev_rate: attitude, velocity and body-rate deviations over k = 1 .. N, as obca_rollout.h takes them
 *   [7] min: the smallest clearance   [8] its sample   [9] its obstacle   [10] below: samples under `need`
 *   [11] saturated: intervals in which an input was clipped   [12] du_max: the largest |U_k - u_k|   [13] its interval   [14] |dx0[m]| of the position part   [15] 0
 * [0] bad = 1: a dx0[m] or dub[m] that is not finite, a rolled state or a clearance that is not finite, a quadcopter step across cos x[3] = 0.  That member alone is
 * marked: its real fields are NaN, its index and count fields -1, its final state NaN.
 * Per instance OBCA_ENS_OUT doubles come back:
 *   [0] bad   [1] M   [2] S   [3] feedback   [4] clamp   [5] members_bad   [6] members_hit: good members with a sample under `need`
 *   [7] members_sat: good members with a clipped interval   [8] min over the good members   [9] its member   [10] its sample   [11] its obstacle
 *   [12] dev_pos, the largest   [13] its member   [14] its node   [15] end_pos, the largest   [16] its member   [17] dev_att   [18] dev_vel   [19] dev_rate
 *   [20] du_max   [21] its member   [22] its interval   [23] mean of end_pos   [24] mean of min   [25] below, summed   [26 .. 31] 0
 * Ties go to the smaller member; means are taken over the good members, added in ascending member order.
 * [0] bad = 1: what obca_track.h marks for the whole instance (a non-finite number in the trajectory, Ts or the time scale; a pivot of a G that is not finite and
 * positive).  Then every member is bad, the real fields of the instance record are NaN, its indices and counts -1.  Every member bad but the instance not: [5] = M, the
 * other counts 0, real fields NaN, indices -1.
 * The final states X_N of the members (M x nx per instance) also stay on the device until the *_final calls fetch them.  The resident calls read the last solution and
 * write nothing into the batch; the states of an earlier rollout or closed-loop call stay valid.
 * Array layouts: dx0 is nx x M x B (each member's nx contiguous, members of an instance together) or NULL (all zeros); dub is nu x M x B or NULL (all zeros).  Obstacle
 * conventions and chunking are those of the rollout calls.  Return values: 0; -1 bad arguments (those of obca_track.h; members outside 1 .. OBCA_ENS_MMAX; *_members /
 * *_final before an ensemble call on the batch); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_ENSEMBLE_H
#define OBCA_ENSEMBLE_H
#include "obca_track.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_ENS_MEM 16         /* doubles per member */
#define OBCA_ENS_OUT 32         /* doubles per instance */
#define OBCA_ENS_MMAX 64        /* most members per instance */

/* the ensemble about the last solution of a resident batch, on the bicycle; dx0: 4 x members x B or NULL; dub: 2 x members x B or NULL; out: OBCA_ENS_OUT x B */
int obca_batch_ensemble(obca_batch *bt, int substeps, int members, int feedback, int clamp, const double q[4], const double r[2], const double qf[4], const double *dx0, const double *dub, double need, double *out);
/* duration of the last obca_batch_ensemble kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_ensemble_ms(obca_batch *bt, float *ms);
/* the member records of the last obca_batch_ensemble on this batch; mem: members x OBCA_ENS_MEM per instance */
int obca_batch_ensemble_members(obca_batch *bt, double *mem);
/* their final states; fin: members x 4 per instance */
int obca_batch_ensemble_final(obca_batch *bt, double *fin);
/* any trajectories: the arguments of obca_parking_track_batch up to timeScale; mem: members x OBCA_ENS_MEM x B or NULL; fin: members x 4 x B or NULL; chunked over the slots */
int obca_parking_ensemble_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                                const int *nOb, const int *vOb, const double *A, const double *b,
                                const double *x, const double *u, const double *timeScale, int substeps, int members, int feedback, int clamp,
                                const double q[4], const double r[2], const double qf[4], const double *dx0, const double *dub, double need, double *out, double *mem, double *fin);

/* the quadcopter: dx0 12 x members x B or NULL; dub 4 x members x B or NULL */
int obca_quad_batch_ensemble(obca_quad_batch *bt, int substeps, int members, int feedback, int clamp, const double q[12], const double r[4], const double qf[12], const double *dx0, const double *dub, double need, double *out);
int obca_quad_batch_ensemble_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_ensemble_members(obca_quad_batch *bt, double *mem);
/* fin: members x 12 per instance */
int obca_quad_batch_ensemble_final(obca_quad_batch *bt, double *fin);
/* the arguments of obca_quadcopter_track_batch up to timeScale; mem: members x OBCA_ENS_MEM x B or NULL; fin: members x 12 x B or NULL */
int obca_quadcopter_ensemble_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                   const double *x, const double *u, const double *timeScale, int substeps, int members, int feedback, int clamp,
                                   const double q[12], const double r[4], const double qf[12], const double *dx0, const double *dub, double need, double *out, double *mem, double *fin);

#ifdef __cplusplus
}
#endif
#endif
