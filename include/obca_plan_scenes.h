/*
 * obca_plan_scenes.h -- C ABI of the parking planner on the GPU with PER-INSTANCE obstacle fields: B searches per call, every search in the field of its own instance
 * (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_hybrid.h; the shared-field call it stands beside: include/obca_plan_device.h).
 *
 * The search is obca_hybrid_astar_batch's, word for word: the same option array, grid (one per call: ego, L, XYbounds and the options are shared by the batch), cell key,
 * motion primitives, cost terms, collision predicate, heuristic, rounds, return values, counts codes and dense output.  What differs is where the obstacle field comes
 * from: nOb[i] obstacles per instance, their row counts, rows and right-hand sides packed instance after instance as obca_parking_signed_dist_batch takes them.  The cells
 * of the holonomic map that a disc of the car's half width cannot stand on are found by the search itself, at its start, from the rows of its own field (the shared-field
 * call gets them from the host), so nothing of one instance's field is seen by another.  The slots and pools are obca_hybrid_configure's.
 *
 * Return values of the calls: 0; -1 bad arguments; -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 * counts[i]: as in obca_plan_device.h -- nodes of the path (>= 2); 0 no path; -1 more than `cap` nodes; -2 the start or goal pose collides with the instance's OWN field
 * (that instance alone); -3 a sizing limit of the slot was hit (that search alone).
 */
#ifndef OBCA_PLAN_SCENES_H
#define OBCA_PLAN_SCENES_H
#include "obca_plan_device.h"
#ifdef __cplusplus
extern "C" {
#endif

/* B searches, each in its own obstacle field: starts, goals B x 3; nOb: B obstacle counts (0 is legal: a free field inside XYbounds); vOb: sum(nOb) row counts; A:
 * (rows of all instances) x 2, b: rows of all instances -- packed as in obca_parking_signed_dist_batch; paths B x cap x 3, dirs B x cap (rows beyond the count are zero),
 * counts, expansions, rounds: B (expansions, rounds may be NULL).  -1, decided on the host before anything is launched, allocated or written: what obca_hybrid_astar_batch
 * refuses, a NULL nOb (or vOb, A, b with an obstacle in the batch), and per instance a negative or more than OBCA_HYBRID_MAXOB obstacles, a row count outside
 * 1 .. OBCA_HYBRID_MAXROWS, a row that is not finite: the message names the first such instance. */
int obca_scene_astar_batch(obca_ctx *ctx, int B, const double *starts, const double *goals, const int *nOb, const int *vOb, const double *A, const double *b,
                           const double ego[4], double L, const double XYbounds[4], const double *opts, int nopts, double bucket_width,
                           double *paths, int *dirs, int cap, int *counts, int *expansions, int *rounds);
/* duration of the last per-instance search kernel of the context [ms], measured with HIP events of its own on the context's stream (obca_hybrid_ms keeps reporting the
 * last shared-field search) */
int obca_scene_astar_ms(obca_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
