/*
 * obca_advance.h -- C ABI of one step of the closed receding-horizon loop on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_advance.h).
 *
 * obca_batch_solve solves, obca_batch_rollout applies a solution to the continuous vehicle model, obca_batch_shift_warm_start restarts from the last solution advanced
 * by `shift` stages.  An advance call does the last two together for a solved resident batch, in one launch, one wavefront per instance:
 *   plant   : the continuous model of include/obca_rollout.h is integrated from X0 of the instance's problem record (the plant's state: what the upload or the last
 *             advance left there) over the intervals 0 .. shift-1 of the last solution, u_k held over t_k Ts, `substeps` (1 .. OBCA_ROLL_MAXSUB) classical RK4 steps
 *             per interval -- the chain of obca_batch_rollout(restart 0) with a horizon of `shift` instead of N
 *   kick    : nx doubles per instance (nx = 4 / 12) or NULL, added to the state after the last step: the process disturbance.  The result is the plant state; it
 *             stays on the device (obca_batch_advance_state fetches it) and is the measurement of the restart
 *   measure : the shift * substeps + 1 driven samples (before the kick) against the obstacles, as the rollout calls measure theirs
 *   restart : what obca_batch_shift_warm_start(shift, x0_new = the plant state) / obca_quad_batch_shift_warm_start(shift, x0_new = the plant state, xF_new) does, by the
 *             same device function, the state read from device memory.  Every rule of include/obca_hip.h for those calls holds
 *   log     : obca_batch_advance_log(bt, capacity_nodes) allocates B x capacity x nx doubles on the device (0 frees it); every advance then appends the `shift` node
 *             states it drove through, the last one after the kick; obca_batch_advance_log_states downloads them, `nodes` x nx per instance.  An upload empties the log
 * OBCA_ADV_OUT doubles per instance come back, the head and clearance layout of include/obca_rollout.h:
 *   [0] bad       1 marks this instance ALONE: a non-finite number among Ts, the time scale, X0, the solution's nodes 0 .. shift and inputs 0 .. shift-1 or the kick, a rolled
 *                 state that is not finite or steps across cos x[3] = 0, a kicked state that is not finite.  Then the fields are those of a bad rollout record ([13], [14]
 *                 NaN), the plant state is NaN, and the instance's problem record, start iterate and log rows keep every bit: it was not advanced and not restarted
 *   [1 .. 5]      the largest deviations of the plant (before the kick) from the solution's own nodes k = 1 .. shift -- the model mismatch the next solve absorbs --, [2] the
 *                 node; [6 .. 9] the same four at node `shift`.  shift 0: [1], [3 .. 5] are 0, [2] is -1, [6 .. 9] compare X0 with the solution's node 0
 *   [10] 0   [11] substeps   [12] shift   [13] the driven time sum t_k Ts   [14] the position distance of the plant state to the goal of the next solve (xF, or xF_new)
 *   [15] the nodes in the log after this call, -1 without a log
 *   [16 .. 39]    the OBCA_CLR_OUT doubles of include/obca_clearance.h for the driven samples, field for field
 * After the call the batch counts as unsolved, exactly as after a shift call (a bad instance solves again from the start it had).  shift 0 is legal: the plant stands,
 * the plant state is X0 + kick.  There is no host-pointer variant -- a closed loop needs a resident batch -- and no feedback inside the step: here the re-solve is the
 * feedback, include/obca_track.h is the tool between two re-solves.
 * Return values: 0; -1 refused before anything is launched or written (nothing solved since the last upload, shift or advance; shift outside 0 .. N; substeps outside
 * 1 .. OBCA_ROLL_MAXSUB; a non-finite need; a non-finite entry of xF_new; the log would overflow; a NULL `out`; *_state before an advance, *_log_states without a log);
 * -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_ADVANCE_H
#define OBCA_ADVANCE_H
#include "obca_rollout.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_ADV_OUT 40         /* doubles per instance */

/* one closed-loop step of a solved resident batch; kick: 4 x B or NULL; out: OBCA_ADV_OUT x B */
int obca_batch_advance(obca_batch *bt, int shift, int substeps, const double *kick, double need, double *out);
/* duration of the last obca_batch_advance kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_advance_ms(obca_batch *bt, float *ms);
/* the plant state the last obca_batch_advance left on the device; X: 4 x B (NaN where bad) */
int obca_batch_advance_state(obca_batch *bt, double *X);
/* allocate (capacity_nodes > 0) or free (0) the log of driven node states; it starts empty */
int obca_batch_advance_log(obca_batch *bt, int capacity_nodes);
/* the log: *nodes logged so far, X: nodes x 4 per instance (X may be NULL: only the count) */
int obca_batch_advance_log_states(obca_batch *bt, double *X, int *nodes);

/* the same for the quadcopter; kick, xF_new: 12 x B or NULL */
int obca_quad_batch_advance(obca_quad_batch *bt, int shift, int substeps, const double *kick, const double *xF_new, double need, double *out);
int obca_quad_batch_advance_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_advance_state(obca_quad_batch *bt, double *X);
int obca_quad_batch_advance_log(obca_quad_batch *bt, int capacity_nodes);
int obca_quad_batch_advance_log_states(obca_quad_batch *bt, double *X, int *nodes);

#ifdef __cplusplus
}
#endif
#endif
