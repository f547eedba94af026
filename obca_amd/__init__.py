"""obca_amd -- MI355X-native batched OBCA (optimization-based collision avoidance) parking NLP solver.

Host-side mirror of the reference's Julia entry points over the C ABI of libobca_hip.so (include/obca_hip.h).
The HIP library is the only compute path: importing works anywhere, but every solve raises if the library or a gfx950
device is missing -- there is no CPU fallback.
"""
from .api import (ObcaError, Context, Batch, ParkingSignedDist, ParkingDist, DualMultWS, parking_signed_dist_batch, dualmult_ws_batch,
                  default_opts, ipopt_opts, warm_restart_opts, selftest, library_path, build_library, QuadBatch, QuadcopterSignedDist, QuadcopterDist,
                  quadcopter_signed_dist_batch, quadcopter_default_opts, quadcopter_ipopt_opts, quad_warm_restart_opts,
                  parking_constraints_batch, ParkingConstraints, quadcopter_constr_satisfaction_batch, constrSatisfaction, VIOL_NAMES, QUAD_VIOL_NAMES,
                  parking_clearance_batch, quadcopter_clearance_batch, parking_rollout_batch, quadcopter_rollout_batch, parking_track_batch, quadcopter_track_batch,
                  parking_ensemble_batch, quadcopter_ensemble_batch, ensemble_offsets, parking_certify_batch, quadcopter_certify_batch, parking_predict_batch, quadcopter_predict_batch, TRACK_Q_PARKING, TRACK_R_PARKING, TRACK_QF_PARKING, TRACK_Q_QUAD, TRACK_R_QUAD, TRACK_QF_QUAD, parking_refine_batch, REFINE_STATUS, quadcopter_refine_batch, QUAD_REFINE_STATUS,
                  hybrid_astar_batch, hybrid_configure, hybrid_ms, HYBRID_STATUS, scene_astar_batch, scene_ms, QUAD_PLAN_STATUS)

__all__ = ["ObcaError", "Context", "Batch", "ParkingSignedDist", "ParkingDist", "DualMultWS", "parking_signed_dist_batch",
           "dualmult_ws_batch", "default_opts", "ipopt_opts", "warm_restart_opts", "selftest", "library_path", "build_library", "QuadBatch", "QuadcopterSignedDist", "QuadcopterDist",
           "quadcopter_signed_dist_batch", "quadcopter_default_opts", "quadcopter_ipopt_opts", "quad_warm_restart_opts",
           "parking_constraints_batch", "ParkingConstraints", "quadcopter_constr_satisfaction_batch", "constrSatisfaction", "VIOL_NAMES", "QUAD_VIOL_NAMES",
           "parking_clearance_batch", "quadcopter_clearance_batch", "parking_rollout_batch", "quadcopter_rollout_batch", "parking_track_batch", "quadcopter_track_batch",
           "parking_ensemble_batch", "quadcopter_ensemble_batch", "ensemble_offsets", "parking_certify_batch", "quadcopter_certify_batch", "parking_predict_batch", "quadcopter_predict_batch", "TRACK_Q_PARKING", "TRACK_R_PARKING", "TRACK_QF_PARKING", "TRACK_Q_QUAD", "TRACK_R_QUAD", "TRACK_QF_QUAD", "parking_refine_batch", "REFINE_STATUS", "quadcopter_refine_batch", "QUAD_REFINE_STATUS",
           "hybrid_astar_batch", "hybrid_configure", "hybrid_ms", "HYBRID_STATUS", "scene_astar_batch", "scene_ms", "QUAD_PLAN_STATUS"]
