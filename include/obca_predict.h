/*
 * obca_predict.h -- C ABI of the clearance of a HELD trajectory against obstacles that MOVE while it is executed, on the GPU (exported by libobca_hip.so; kernel text:
 * obca_amd/csrc/obca_predict.h).
 *
 * The clearance calls of include/obca_clearance.h read the obstacles as they stand at the instant of the call and hold them for the whole horizon.  These calls measure
 * every sample against the obstacles where they will be when the vehicle gets there, given a constant rate per obstacle.  The samples are exactly those of the clearance
 * calls (q = k S + s and q = N S, the same poses); new is the time a sample is reached: cum[0] = 0, cum[k+1] = cum[k] + timeScale[k] summed in stage order,
 * tau_q = (cum[k] + (s / S) timeScale[k]) Ts.  A resident batch has its one t (1 with fixTime) for every stage.
 *   parking   : OBCA_PRD_PIN doubles per obstacle, [vx, vy, w, cx, cy, g]: the motion, pivot and inflation of obca_batch_move_obstacles (include/obca_scene_edit.h) read as
 *               rates.  At sample q obstacle j is the image that call would make of it with motion (vx, vy, w) tau_q about the pivot (cx, cy), grown by g tau_q (g: a growth
 *               rate of the margin, prediction uncertainty that widens with time; g < 0 shrinks).  The clearance of the pose to the moved rows is the DualMultWS distance with
 *               the OBCA_CLR_TOUCH rule.
 *   quadcopter: OBCA_PRD_QIN doubles per box, [vx, vy, vz, g]: the box moved by v tau_q and grown by g tau_q on all six sides; clearance = distance of the point - R.
 * The records of the batch are never written: the rows are moved in registers.  One wavefront per instance, one launch per call; OBCA_PRD_OUT doubles per instance:
 *   [0 .. 23]  the record of include/obca_clearance.h, same layout and meaning (min, min_nodes, sample, obstacle, below, samples, bad, 0, 16 per-obstacle minima)
 *   [24] first           q of the first sample whose smallest clearance is < need (-1: none)
 *   [25] t_first         its tau in seconds (+inf: none) -- an instance with a finite t_first is one to re-solve now
 *   [26] first_obstacle  the smallest j under need at that sample (-1: none)
 *   [27] t_min           tau of sample [2]
 *   [28] horizon         tau of the last sample
 *   [29] moving          obstacles of the instance whose vx, vy(, vz), w or g is not 0 (a pivot alone moves nothing)
 *   [30], [31] 0
 * bad ([6] = 1): a non-finite number in the trajectory, a non-finite rate, or a moved row that is not finite marks its instance alone; then [0 .. 23] are the bad record of
 * the clearance calls, [24] = [26] = -1, [25] = [27] = [28] = NaN, [29] = 0.
 * Profile.  With keep_profile != 0 the smallest clearance of every sample over the obstacles stays on the device, N S + 1 doubles per instance (NaN for a bad instance):
 * 8 B (N S + 1) bytes, at most 8 B (OBCA_NMAX x 32 + 1) = 32 776 B bytes -- 537 MB at B = 16 384, N = 128, S = 32; 84 MB at N = 80, S = 8.  The buffer is allocated by the
 * first call that asks, sized for that call, grown when a later call needs more, and freed with the batch.  obca_*_predict_profile downloads it.
 * Return values: 0; -1 bad arguments (substeps outside 1 .. OBCA_CLR_MAXSUB, a non-finite need, a NULL array, a horizon out of range, a resident batch on which nothing
 * has been solved since the last upload or shift, a profile download before any call that kept one, a capacity below B (N S + 1)); -2 device error.  The message is
 * obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_PREDICT_H
#define OBCA_PREDICT_H
#include "obca_clearance.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_PRD_OUT 32        /* doubles per instance */
#define OBCA_PRD_PIN 6         /* doubles per parking obstacle: vx, vy, w, cx, cy, g */
#define OBCA_PRD_QIN 4         /* doubles per box: vx, vy, vz, g */

/* the last solution of a resident batch (the iterate and the records are read, nothing is written to the batch); rates: OBCA_PRD_PIN per obstacle, packed over the
   obstacles of all instances in upload order; out: OBCA_PRD_OUT x B */
int obca_batch_predict_clearance(obca_batch *bt, const double *rates, int substeps, double need, int keep_profile, double *out);
/* duration of the last obca_batch_predict_clearance kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_predict_clearance_ms(obca_batch *bt, float *ms);
/* the profile the last call with keep_profile != 0 left on the device: (N S + 1) x B doubles into out; capacity: the doubles out has room for */
int obca_batch_predict_profile(obca_batch *bt, double *out, int capacity);
/* any trajectories: the arguments of obca_parking_clearance_batch, then rates (packed like A's obstacles) and profile ((N S + 1) x B, or NULL) */
int obca_parking_predict_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                               const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, int substeps, double need, double *out,
                               const double *rates, double *profile);

/* rates: OBCA_PRD_QIN x 5 per instance */
int obca_quad_batch_predict_clearance(obca_quad_batch *bt, const double *rates, int substeps, double need, int keep_profile, double *out);
int obca_quad_batch_predict_clearance_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_predict_profile(obca_quad_batch *bt, double *out, int capacity);
/* the arguments of obca_quadcopter_clearance_batch, then rates and profile ((N S + 1) x B, or NULL) */
int obca_quadcopter_predict_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                  const double *x, const double *timeScale, int substeps, double need, double *out,
                                  const double *rates, double *profile);

#ifdef __cplusplus
}
#endif
#endif
