/*
 * obca_quad_plan_resident.h -- C ABI of the RESIDENT route of the quadcopter's grid planner: the warm starts of an uploaded quadcopter batch, planned on the GPU from what
 * the batch holds (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_quad_plan_resident.h over obca_amd/csrc/obca_plan3d.h; the host-pointer calls it stands
 * beside: include/obca_plan3d.h, a library and context of their own).
 *
 * obca_quad_batch_upload leaves per instance a problem record on the device: x0, xF, the five boxes, the warm start.  One workgroup per selected instance runs the search
 * of obca_plan3d_paths_batch from those numbers -- the same grid, `blocked` test, relaxation and descent, the same kernel text -- and writes what
 * obca_plan3d_warm_start_batch would return as xWS (rows 0-2 the path resampled at N + 1 uniform arc lengths, rows 3-11 zero) into the record of every instance that has a
 * path.  An instance without one keeps its record to the last bit.  Only the selection goes up and two ints per instance come down.
 *
 * The names carry `grid_plan`: the parking route's three entry points (include/obca_plan_resident.h) are `obca_batch_plan_*`, and a name of this header never contains one
 * of those.
 *
 * Return values of the calls: 0; -1 bad arguments; -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 * counts[i]: as obca_plan3d_paths_batch -- way-points of the path (>= 2); 0 no path; -1 more than `cap` way-points; -2 the start or goal point is blocked, or a start,
 * goal or box coordinate of the record is not finite; -3 the relaxation hit its sweep bound (cannot happen) -- or OBCA_QUAD_PLAN_SKIPPED for an instance outside the selection.
 */
#ifndef OBCA_QUAD_PLAN_RESIDENT_H
#define OBCA_QUAD_PLAN_RESIDENT_H
#include "obca_hip.h"
#include "obca_plan3d.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_QUAD_PLAN_SKIPPED (-4)   /* counts[i] of an instance that was not selected */

/* Plans the selected instances of an uploaded batch and writes their warm starts into it.  clear, room, res: obca_plan3d_paths_batch's; cap: rows of a path in the batch's
 * path buffer, 2 .. OBCA_PLAN3D_WS_CAP; sel: n distinct indices in 0 .. B - 1, or NULL = all B instances (n is not read then); timeWS: NULL = every instance keeps its
 * time scale, else ONE finite value > 0 that the planned instances (count >= 2) get; sweeps (B, may be NULL): relaxation sweeps, 0 for a skipped instance.
 * -1, decided on the host before anything is allocated, launched or written: what obca_plan3d_paths_batch refuses of clear, room, res, cap and the grid size; a cap above
 * OBCA_PLAN3D_WS_CAP; a NULL counts; an index of sel outside 0 .. B - 1 or twice in it; n outside 1 .. B with sel; a timeWS that is not finite and positive; a batch with
 * nothing uploaded; a batch that is not one of its context's primary device.  The kernel runs on the batch's stream and the call returns when it has finished.  Afterwards
 * the batch counts as unsolved, as after obca_quad_batch_upload. */
int obca_quad_batch_grid_plan_warm_start(obca_quad_batch *bt, double clear, const double room[3], double res, int cap,
                                         const int *sel, int n, const double *timeWS, int *counts /* B */, int *sweeps /* B or NULL */);
/* HIP-event duration of the last call's kernel on this batch [ms] */
int obca_quad_batch_grid_plan_ms(obca_quad_batch *bt, float *ms);
/* The way-points of the last call, for plots and tests: paths B x cap x 3 (start point, chain of grid nodes, goal point; the rows behind the count, and every row of an
 * instance the last call skipped, are zero).  cap: the last call's -- with paths NULL nothing is copied, `cap` is not read and the return value IS the last call's cap
 * (>= 2), for a caller that has to size its array.  -1 before the first call on this batch. */
int obca_quad_batch_grid_plan_download(obca_quad_batch *bt, double *paths, int cap);
/* The start the next solve of the batch begins from, read from the problem records as they lie on the device: xWS 12 x (N+1) x B (the layout obca_quad_batch_upload
 * takes), timeWS B; either may be NULL.  Works on every uploaded batch -- after an upload, a plan, obca_quad_batch_shift_warm_start, on the destination of
 * obca_quad_batch_subdivide_into -- and changes nothing. */
int obca_quad_batch_start_download(obca_quad_batch *bt, double *xWS, double *timeWS);

#ifdef __cplusplus
}
#endif
#endif
