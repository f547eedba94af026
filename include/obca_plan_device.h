/*
 * obca_plan_device.h -- C ABI of the parking planner on the GPU: a round-synchronous Hybrid A*, B searches per call, one workgroup per search
 * (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_hybrid.h; the host planner it stands beside: include/obca_plan.h).
 *
 * The problem is obca_plan_hybrid_astar_batch2's: the same obstacles (convex H-representations), ego, L, XYbounds, the same option array (OBCA_PLAN_NOPTS doubles, the same
 * meaning and defaults), cell key, motion primitives, cost terms, collision predicate, heuristic, return codes and dense output.  What differs is the ORDER of expansion: the
 * open set is kept in buckets of width `bucket_width` in f = g + h, and a ROUND expands every entry of the lowest non-empty bucket at once.  Every decision of a round is a
 * minimum over a set that is fixed when the round starts (per cell: the cheapest candidate, ties to the lowest (parent cell, primitive); per round: the cheapest finish, ties
 * to the lowest cell), so the result does not depend on the order in which lanes, waves or bucket entries run.  The search part calls no libm; only
 * the Reeds-Shepp curves do (analytic expansion, option 15), which is where a device result may differ from a host build of the same text.
 * g is kept in fp32 (the claim word orders candidates by its bits).  The analytic expansion is tried on every popped node within 6 Rmin of the goal and on those whose
 * cell index is a multiple of 16 (the host's `every 16th expansion` depends on the pop order).  The lattice heuristic (options 16, 17) is refused.
 *
 * Return values of the calls: 0; -1 bad arguments; -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 * counts[i]: nodes of the path (>= 2); 0 no path (open set empty; the live entries of the next round would pass max expansions -- expansions <= max expansions always --; the round bound reached); -1 more than `cap` nodes; -2 the start or goal pose
 * collides; -3 a sizing limit of the slot was hit (node pool, chunk pool) -- that search alone ends, its neighbours are unaffected.
 */
#ifndef OBCA_PLAN_DEVICE_H
#define OBCA_PLAN_DEVICE_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_HYBRID_MAXMAP 35000          /* cells of the holonomic map (nx * ny): one fp32 word per cell in the workgroup's LDS beside the bucket heads */
#define OBCA_HYBRID_MAXCELLS 6000000      /* (nx + 1) * (ny + 1) * nyaw cells of the search */
#define OBCA_HYBRID_MAXSLOTS 256          /* searches in flight = persistent workgroups */
#define OBCA_HYBRID_MAXNODES (1 << 20)    /* default and largest node pool of a slot (nodes of one search) */
#define OBCA_HYBRID_CHUNK 16              /* ints of a bucket chunk: the link and 15 entries */
#define OBCA_HYBRID_WINDOW 1024           /* bucket heads in LDS; entries beyond the window wait in the far list */
#define OBCA_HYBRID_MAXOB 16              /* obstacles */
#define OBCA_HYBRID_MAXROWS 12            /* rows of one obstacle */
#define OBCA_HYBRID_MAXSTEER 15           /* steering samples per side (option 4) */
#define OBCA_HYBRID_DEFAULT_WIDTH 0.2     /* bucket width used for bucket_width <= 0 */

/* Slots of the context's planner: `slots` searches in flight (0 = by memory budget, at most OBCA_HYBRID_MAXSLOTS), each with a pool of `max_nodes` nodes
 * (0 = OBCA_HYBRID_MAXNODES) and `max_chunks` bucket chunks (0 = max_nodes / 4 + 4 OBCA_HYBRID_WINDOW).  Takes effect at the next search; -1: a value out of range. */
int obca_hybrid_configure(obca_ctx *ctx, int slots, int max_nodes, int max_chunks);
/* B searches in one obstacle field (shared by the batch, as obca_plan_hybrid_astar_batch2): starts, goals B x 3; paths B x cap x 3, dirs B x cap (rows beyond the count
 * are zero), counts, expansions, rounds: B (expansions, rounds may be NULL).  -1: a NULL array, B < 1, cap < 2, nopts outside 0 .. OBCA_PLAN_NOPTS, a non-finite number
 * in the input, an option out of range, a negative cost option, the lattice heuristic, a grid beyond OBCA_HYBRID_MAXMAP / OBCA_HYBRID_MAXCELLS, an obstacle field beyond the limits above. */
int obca_hybrid_astar_batch(obca_ctx *ctx, int B, const double *starts, const double *goals, int nOb, const int *vOb, const double *A, const double *b,
                            const double ego[4], double L, const double XYbounds[4], const double *opts, int nopts, double bucket_width,
                            double *paths, int *dirs, int cap, int *counts, int *expansions, int *rounds);
/* duration of the last search kernel of the context [ms], measured with HIP events on its stream */
int obca_hybrid_ms(obca_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
