/*
 * obca_path_ws.h -- C ABI of the parking warm start from planner paths on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_path_ws.h).
 *
 * Stands between obca_plan_hybrid_astar_batch2 (include/obca_plan.h) and the parking solve: the dense arrays that call writes -- paths B x cap x 3 (x, y, yaw per node),
 * dirs B x cap (+1 / -1 per node), counts B -- go in, the warm start of planner.path_to_warm_start comes out: the path resampled at N + 1 uniform arc lengths, speed
 * +-v_nom (0 at both ends and where the direction changes), Ts = length / (N v_nom), acceleration and steering from the differences.  a_max > 0 sends the speed profile
 * through the velocity smoother of the reference's pipeline (main.jl:222-231, veloSmooth.jl) with that acceleration; 0 leaves it as it is.
 * One wavefront per instance, one launch per call.  There is no CPU fallback.  The Hybrid A* search itself stays on the host.
 * Arrays are caller-allocated host memory, instance-major: xF B x 4 ("4 x B" read as Julia reads it), xWS B x (N+1) x 4, uWS B x N x 2 (steering, acceleration), Ts B --
 * the orientation obca_parking_signed_dist_batch and obca_batch_upload take, with rx, ry, ryaw = rows 0-2 of xWS.
 *
 * status[i]: 0 written; -1 counts[i] < 2 (no path); -2 counts[i] > cap or > OBCA_PATH_WS_MAXNODES; -3 a non-finite pose among the rows in use (or in the goal);
 * -4 the path length is not positive.  Only rows below counts[i] are ever read, and none of an instance whose status is -1 or -2.
 * Return values: 0; -1 bad arguments (B < 1, N outside 1 .. OBCA_NMAX, cap < 2, v_nom or L not positive and finite, a_max negative or not finite, a NULL array, a batch
 * that was never uploaded); -2 device error.  The message is obca_last_error's.
 */
#ifndef OBCA_PATH_WS_H
#define OBCA_PATH_WS_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_PATH_WS_MAXNODES 1024   /* nodes of the longest path */

/* Host arrays in, host arrays out.  xF (may be NULL): the goal replaces the last pose of every path, so that the warm start ends on the terminal state of the NLP.
 * The outputs of an instance whose status is negative are zeros.  Only the path rows below max(counts) travel to the device. */
int obca_parking_path_warm_start_batch(obca_ctx *ctx, int B, int N, const double *paths, const int *dirs, const int *counts, int cap, const double *xF,
                                       double v_nom, double L, double a_max, double *Ts, double *xWS, double *uWS, int *status);

/* The same into a resident batch that obca_batch_upload has filled (its xWS / uWS may have been NULL): on the device Ts, the tracking reference rx, ry, ryaw and the
 * x, u part of the start iterate are rewritten, t = 1, the multipliers cleared (the next solve runs DualMultWS); L is the uploaded one, and with use_xF the uploaded
 * goal replaces the last pose.  An instance whose status is negative keeps what was uploaded.  obca_batch_validate refuses until the next solve. */
int obca_batch_set_path_warm_start(obca_batch *bt, const double *paths, const int *dirs, const int *counts, int cap, int use_xF, double v_nom, double a_max, int *status);

/* duration of the last obca_batch_set_path_warm_start kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_path_ws_ms(obca_batch *bt, float *ms);

#ifdef __cplusplus
}
#endif
#endif
