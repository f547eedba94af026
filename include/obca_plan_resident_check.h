/*
 * obca_plan_resident_check.h -- a DIAGNOSTIC of the resident route of the parking planner (include/obca_plan_resident.h), exported by libobca_hip.so for tests and for
 * looking at a plan that went wrong: what the packing kernel wrote on the device, which no product call hands out.
 */
#ifndef OBCA_PLAN_RESIDENT_CHECK_H
#define OBCA_PLAN_RESIDENT_CHECK_H
#include "obca_plan_resident.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The block the packing kernel of the batch's last obca_batch_plan_warm_start wrote, byte for byte as the search read it: the instance records and the obstacle fields of
 * all instances at fixed strides (the layout of obca_amd/csrc/obca_plan_resident.h; words no instance uses are whatever the memory held).  dims (6 ints, always written):
 * instances, the block's obstacles and rows per instance, its length in doubles, and how often the context's planner has allocated its slots and its staging block so far.
 * block: NULL (dims only), or an array of ndoubles >= dims[3] doubles.  0; -1: NULL bt or dims, an array that is too short, no plan of this batch in the staging block (none
 * has run, or another planner call of the context has used it since); -2: device error. */
int obca_batch_packed_block(obca_batch *bt, double *block, int ndoubles, int *dims /* 6 */);

#ifdef __cplusplus
}
#endif
#endif
