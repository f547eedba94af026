/*
 * obca_plan_resident.h -- C ABI of the RESIDENT route of the parking planner: the warm starts of an uploaded batch, planned on the GPU from what the batch holds
 * (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_plan_resident.h; the host-pointer calls it stands beside: include/obca_plan_scenes.h, include/obca_path_ws.h).
 *
 * obca_batch_upload leaves per instance a problem record on the device: x0, xF, the obstacle counts and the half-space rows as UNIT rows.  A packing kernel puts the
 * search's obstacle field and poses together from that record (one wavefront per instance), obca_scene_astar_batch's search runs in it -- the same kernel, the same option
 * array, slots (obca_hybrid_configure) and counts codes -- and obca_batch_set_path_warm_start's kernel reads the search's paths where they lie and writes Ts, the tracking
 * reference and the x / u start of every instance that has a path.  ego, L and XYbounds are the uploaded ones.  Only the per-instance ints come back.
 *
 * Return values of the calls: 0; -1 bad arguments; -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 * counts[i]: as obca_scene_astar_batch -- nodes of the path (>= 2); 0 no path; -1 more than `cap` nodes; -2 the start or goal pose collides with the instance's own field;
 * -3 a sizing limit of the slot was hit.  status[i]: as obca_batch_set_path_warm_start -- 0 written; -1 no path (every count below 2); -3 a non-finite pose; -4 the path
 * length is not positive.  An instance with a negative status keeps its uploaded start, to the last bit.
 */
#ifndef OBCA_PLAN_RESIDENT_H
#define OBCA_PLAN_RESIDENT_H
#include "obca_plan_scenes.h"
#include "obca_path_ws.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Plans every instance of an uploaded batch in its own obstacle field and writes the warm start into the batch.  Nothing but the per-instance ints crosses the bus.
 * opts, nopts, bucket_width: obca_scene_astar_batch's; cap: rows of a path, 2 .. OBCA_PATH_WS_MAXNODES; use_xF, v_nom, a_max: obca_batch_set_path_warm_start's.
 * -1, decided on the host before anything is launched: a NULL counts or status, a cap outside its range, what obca_scene_astar_batch refuses of the options, a batch
 * with nothing uploaded by obca_batch_upload (the destination of obca_batch_refine_into is one: it starts from a solution), a batch that is not one of its context's
 * primary device.  The batch counts as unsolved afterwards and its next solve runs DualMultWS. */
int obca_batch_plan_warm_start(obca_batch *bt, const double *opts, int nopts, double bucket_width, int cap,
                               int use_xF, double v_nom, double a_max,
                               int *counts /* B */, int *status /* B */, int *expansions /* B or NULL */, int *rounds /* B or NULL */);
/* HIP-event durations of the three kernels of the last call on this batch: packing, search, warm start */
int obca_batch_plan_ms(obca_batch *bt, float *pack_ms, float *search_ms, float *ws_ms);
/* What the last call planned, for plots and tests: paths B x cap x 3, dirs B x cap (either may be NULL), and, if inst != NULL, the B x 10 instance records the packing
 * kernel wrote (start x, y, yaw, sin, cos; goal x, y, yaw, sin, cos).  cap: the last call's -- with all three arrays NULL nothing is copied, `cap` is not read and the
 * return value IS the last call's cap (>= 2), for a caller that has to size its arrays.  The paths lie in the planner's staging block of the context: -1 once another
 * planner call of the context has used it. */
int obca_batch_plan_download(obca_batch *bt, double *paths, int *dirs, int cap, double *inst);

#ifdef __cplusplus
}
#endif
#endif
