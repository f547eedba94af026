/*
 * obca_plan3d.h -- C ABI of libobca_plan3d.so: the quadcopter's 3-D grid planner on the GPU, B searches per call, one workgroup per search.
 *
 * Stands where mainQuadcopter.jl:124-128 calls a_star_3D.jl, like obca_plan_astar3d of include/obca_plan.h (the host search, one instance per call), and answers
 * what that call answers: the same grid (n = floor(room / res) + 1 nodes per axis), the same `blocked` test of a node (fp64, inclusive comparisons, boxes inflated
 * by `clear`), 26 neighbours with edge weight (float)(res sqrt(dx^2 + dy^2 + dz^2)), only the neighbour node tested.  It is NOT that A*: the cost-to-go of every
 * node is relaxed in the workgroup's LDS until nothing changes, then the path descends from the start (obca_amd/csrc/obca_plan3d.h).  The path has the optimal cost;
 * among paths of equal cost it may be another one than the host search picks.
 * A library of its own: libobca_hip.so and libobca_plan.so neither contain nor need it.  There is no CPU fallback: without a device obca_plan3d_create fails.
 * Arrays are caller-allocated host memory, fp64, instance-major: starts / goals B x 3, x0 / xF B x 12 (rows 0-2 the position), boxes B x nBox x 6
 * ("6 x nBox x B" read as Julia reads it), each box [xmax,ymax,zmax,-xmin,-ymin,-zmin] as in include/obca_hip.h.
 */
#ifndef OBCA_PLAN3D_H
#define OBCA_PLAN3D_H
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_PLAN3D_MAXCELLS 40000   /* grid nodes: one fp32 word each in the 160 KiB of LDS a workgroup may use on gfx950 (the shipped room at res 0.25: 41 x 41 x 21 = 35 301) */
#define OBCA_PLAN3D_MAXBOX 8         /* boxes per instance */
#define OBCA_PLAN3D_NMAX 128         /* longest horizon of the warm start (= OBCA_QUAD_NMAX of include/obca_hip.h) */
#define OBCA_PLAN3D_WS_CAP 1024      /* way-points of the longest path obca_plan3d_warm_start_batch resamples */

/* A planner on `device`.  Returns 0; -1 bad arguments; -2 no such device / device error (obca_plan3d_last_error(NULL) says which). */
int obca_plan3d_create(int device, void **ctx);
int obca_plan3d_destroy(void *ctx);
/* the message of the last failed call on ctx (NULL: of the last failed obca_plan3d_create of this thread) */
const char *obca_plan3d_last_error(void *ctx);

/* B searches.  paths: B x cap x 3, way-points of instance i from paths[3 cap i]: the start point, the chain of grid nodes, the goal point;
 * the rows behind them are written as zeros.
 * counts[i]: what obca_plan_astar3d returns for instance i -- the number of way-points (>= 2), 0 = no path, -2 = start or goal point blocked -- or -1 = the path has more
 * than cap way-points, -3 = the relaxation did not settle within its bound of one sweep per grid node (cannot happen; the loop is bounded all the same).
 * sweeps (B, may be NULL): relaxation sweeps of instance i.
 * Returns 0; -1 bad arguments (B < 1, cap < 2, nBox outside 0 .. OBCA_PLAN3D_MAXBOX, res or room not positive, more than OBCA_PLAN3D_MAXCELLS nodes, a start / goal /
 * box / clear that is not finite); -2 device error. */
int obca_plan3d_paths_batch(void *ctx, int B, const double *starts, const double *goals, int nBox, const double *boxes, double clear, const double room[3],
                            double res, double *paths, int cap, int *counts, int *sweeps);

/* The same searches, each path resampled at N + 1 uniform arc lengths as scenarios.quad_warm_start(x0, xF, N, via = chain) does it, written as the warm start of the
 * quadcopter solve: xWS B x (N+1) x 12 ("12 x (N+1) x B" of include/obca_hip.h), rows 0-2 the positions, rows 3-11 zero; obca_quadcopter_signed_dist_batch and
 * obca_quad_batch_upload take it as it is.  counts as above (-1: more than OBCA_PLAN3D_WS_CAP way-points); the warm start of an instance whose count is < 2 is all zero.
 * Returns 0; -1 bad arguments (as above, or N outside 1 .. OBCA_PLAN3D_NMAX); -2 device error. */
int obca_plan3d_warm_start_batch(void *ctx, int B, int N, const double *x0, const double *xF, int nBox, const double *boxes, double clear, const double room[3],
                                 double res, double *xWS, int *counts);

/* duration of the last call's kernel on the device [ms], measured with HIP events on its stream */
int obca_plan3d_kernel_ms(void *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
