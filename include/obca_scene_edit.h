/*
 * obca_scene_edit.h -- C ABI of a changing scene on the GPU: the obstacles of a resident batch moved and inflated in place (exported by libobca_hip.so; kernel text:
 * obca_amd/csrc/obca_scene_edit.h).
 *
 * obca_batch_upload writes the obstacles of a batch once, and an upload forgets the last solution, its multipliers, the plant state and the advance log.  A move call edits
 * the obstacle words of the problem records where they lie, one wavefront per instance, one launch.  Every other call of the library reads the obstacles from those records,
 * so after a move obca_batch_solve, _validate, _clearance, _certify, _rollout, _track, _ensemble, _advance, _refine_into and _plan_warm_start see the scene as it is now, and
 * obca_batch_shift_warm_start / obca_batch_advance restart in it.  The call works on an UPLOADED batch, solved or not, and changes neither the solved state nor the start
 * iterate, the solution, the log or any word of a record other than the obstacle words.  What an earlier call computed and kept (certify intervals, rollout states, ...)
 * describes the scene it was computed in.
 * Parking (obca_batch_move_obstacles): the arrays are packed per obstacle in upload order, nOb_total rows.
 *   motion  : (dx, dy, dtheta) per obstacle, or NULL (zeros)
 *   pivot   : (cx, cy) per obstacle, the centre of the rotation, or NULL (the world origin)
 *   inflate : m per obstacle [m], may be negative, or NULL (zeros)
 *   The obstacle {p : A p <= b} becomes its image under p' = R(dtheta)(p - c) + c + d and then grows by m: a' = R(dtheta) a, b' = b + a'.(c + d) - a.c + m on the
 *   unit-length rows the record holds (the row lengths obca_batch_upload divided out stay what they were; a download scales lambda by them as before).  dtheta == 0: the
 *   words of A keep their bits; an obstacle with all six numbers zero keeps every bit.  Row counts, offsets and the formulation flag are never written.
 * Quadcopter (obca_quad_batch_move_obstacles): the boxes are axis-aligned, 5 per instance; motion: (dx, dy, dz) per box, inflate: m per box; a box [ub(3), -lb(3)] becomes
 *   [ub + d + m, -(lb + d) + m].  R is not touched.
 * status (B ints): 0 moved; 1 marks this instance ALONE -- a non-finite motion, pivot, inflation or result -- and its record keeps every bit: all or nothing per instance.
 * obca_batch_obstacles_download returns the rows as the device holds them: A (2 x M_total) and b (M_total) packed as obca_batch_upload takes them, UNIT LENGTH -- they
 * are not scaled back by the row lengths of the upload; obca_quad_batch_obstacles_download the 6 x 5 x B box words.
 * Return values: 0; -1 refused before anything is launched or written (nothing uploaded, a NULL status / output); -2 device error.  The message is obca_last_error's.
 * There is no CPU fallback.
 */
#ifndef OBCA_SCENE_EDIT_H
#define OBCA_SCENE_EDIT_H
#include "obca_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* motion: 3 x nOb_total or NULL; pivot: 2 x nOb_total or NULL; inflate: nOb_total or NULL; status: B */
int obca_batch_move_obstacles(obca_batch *bt, const double *motion, const double *pivot, const double *inflate, int *status);
/* duration of the last obca_batch_move_obstacles kernel on this batch [ms], measured with HIP events on its stream */
int obca_batch_move_obstacles_ms(obca_batch *bt, float *ms);
/* the unit-length rows of the records: A 2 x M_total, b M_total (either may be NULL) */
int obca_batch_obstacles_download(obca_batch *bt, double *A, double *b);

/* motion: 3 x 5 x B or NULL; inflate: 5 x B or NULL; status: B */
int obca_quad_batch_move_obstacles(obca_quad_batch *bt, const double *motion, const double *inflate, int *status);
int obca_quad_batch_move_obstacles_ms(obca_quad_batch *bt, float *ms);
/* ob: 6 x 5 x B */
int obca_quad_batch_obstacles_download(obca_quad_batch *bt, double *ob);

#ifdef __cplusplus
}
#endif
#endif
