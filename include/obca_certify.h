/*
 * obca_certify.h -- C ABI of the clearance CERTIFICATE along the whole path of a trajectory on the GPU (exported by libobca_hip.so; kernel text: obca_amd/csrc/obca_certify.h).
 *
 * The clearance calls (obca_clearance.h) look at `substeps` poses per interval and say nothing about what lies between them.  These calls walk every (interval, obstacle)
 * pair by conservative advancement: the distance between convex bodies is 1-Lipschitz in the largest displacement of the moving body's points, so a pose with clearance c
 * clears the stretch of path on which no point of the vehicle moves farther than c, and the next sample is taken at the end of that stretch.
 *   path       : the one the clearance calls sample.  Interval k = 0 .. N-1 is tau in [0, h_k], h_k = timeScale[k] Ts (a resident batch: the solution's single t, 1 with
 *                fixTime), counted in ticks m = 0 .. OBCA_CERT_TICKS (G): tau = h_k m / G.  parking: the bicycle step of ParkingSignedDist.jl:147-150 from node k with u_k
 *                over tau; quadcopter: p_k + tau v_k.  At m = 0 the pose is the node itself.  Node N is one further sample per obstacle.  The certificate is about THIS
 *                piecewise path: the end of interval k and node k + 1 differ by the dynamics residual of the solve; node k + 1 is checked as the first sample of interval k + 1.
 *   clearance  : of a pose, as in obca_clearance.h (parking: the DualMultWS distance, 0 below OBCA_CLR_TOUCH; quadcopter: distance of the point to the box - R)
 *   speed bound: Lambda_k, constant over the interval.  parking, v = x_k[3], a = u_k[1], tn = |tan u_k[0]|, |h| = |h_k|: V = max(|v|, |v + h a|), Sm = max(|v|, |v + h a / 2|),
 *                rho the car point farthest from the reference point; Lambda_k = V + |h| Sm |v| tn / (2 L) + rho V tn / L.  quadcopter: Lambda_k = |v_k|.
 *   advancement: per (k, j) from m = 0: c = clearance at tick m (c < need: VIOLATED); e = c >= need ? c - need + slack : slack; the sample covers
 *                dm = G - m ticks if Lambda_k |h| == 0 or e >= Lambda_k |h| (G - m) / G, else dm = clamp(floor(G e / (Lambda_k |h|)), 1, G - m); proven on that stretch:
 *                clearance >= c - Lambda_k |h| dm / G.  lb = the smallest such bound, seen = the smallest c.  An item still running after max_steps samples is UNDECIDED
 *                (lb = -inf).
 *   guarantees : min(need, seen) - slack <= lb <= the true minimum over the path <= seen for every decided item; a decided instance with no violation has clearance
 *                >= need - slack on the whole path.  With `need` above every clearance the call is uniform sampling at spacing slack / Lambda.
 * One wavefront per instance, one launch per call, no atomics; OBCA_CERT_OUT doubles per instance come back:
 *   [0] lb            [1] seen          [2] interval, [3] tick, [4] obstacle of seen (ties: the smallest interval, then tick, then obstacle)
 *   [5] violated      number of intervals (node N counts as one) with a sample under need
 *   [6] interval, [7] tick, [8] obstacle of the first violation in that order; -1 if none
 *   [9] undecided     items            [10] samples taken in total             [11] most samples in one item        [12] the largest Lambda_k
 *   [13] certified    1 iff not bad, violated == 0 and undecided == 0           [14] bad                             [15] 0
 * bad = 1: a non-finite number in the trajectory (Ts, x, u, timeScale), among the clearances or in a Lambda_k |h|; that instance alone is marked: [0], [1], [12] NaN,
 * [2..4], [6..8] -1, [5] = N + 1, [9] = the items, [10] = [11] = [13] = 0.
 * Per interval 2 doubles [lb_k, seen_k] (the smallest over the obstacles; k = 0 .. N, N is node N; NaN for a bad instance) stay on the device until the *_intervals calls
 * fetch them.  The resident calls read the last solution and write nothing into the batch; validate's and clearance's state stay as they were.
 * Array layouts, obstacle conventions and chunking are those of obca_clearance.h.  Return values: 0; -1 bad arguments (a non-finite need; slack not finite or not > 0;
 * max_steps outside 1 .. OBCA_CERT_TICKS; a NULL array; a horizon out of range; a resident batch on which nothing has been solved; *_intervals before a certify call on
 * the batch); -2 device error.  The message is obca_last_error's.  There is no CPU fallback.
 */
#ifndef OBCA_CERTIFY_H
#define OBCA_CERTIFY_H
#include "obca_clearance.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBCA_CERT_OUT 16         /* doubles per instance */
#define OBCA_CERT_TICKS 4096     /* ticks per interval; most samples of one item */

/* the last solution of a resident batch; out: OBCA_CERT_OUT x B */
int obca_batch_certify(obca_batch *bt, double need, double slack, int max_steps, double *out);
/* duration of the last obca_batch_certify kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_certify_ms(obca_batch *bt, float *ms);
/* [lb_k, seen_k] of the last obca_batch_certify on this batch; iv: 2 x (N + 1) per instance */
int obca_batch_certify_intervals(obca_batch *bt, double *iv);
/* any trajectories: the arguments of obca_parking_clearance_batch up to timeScale; iv: 2 x (N + 1) x B or NULL; chunked over the slots and devices of the context */
int obca_parking_certify_batch(obca_ctx *ctx, int B, int N, const double *Ts, double L, const double ego[4],
                               const int *nOb, const int *vOb, const double *A, const double *b,
                               const double *x, const double *u, const double *timeScale, double need, double slack, int max_steps, double *out, double *iv);

int obca_quad_batch_certify(obca_quad_batch *bt, double need, double slack, int max_steps, double *out);
int obca_quad_batch_certify_ms(obca_quad_batch *bt, float *ms);
int obca_quad_batch_certify_intervals(obca_quad_batch *bt, double *iv);
/* the arguments of obca_quadcopter_clearance_batch up to timeScale; iv: 2 x (N + 1) x B or NULL */
int obca_quadcopter_certify_batch(obca_ctx *ctx, int B, int N, const double *Ts, double R, const double *ob,
                                  const double *x, const double *timeScale, double need, double slack, int max_steps, double *out, double *iv);

#ifdef __cplusplus
}
#endif
#endif
