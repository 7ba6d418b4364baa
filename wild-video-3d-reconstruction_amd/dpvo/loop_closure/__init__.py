"""Loop-closure back end: keypoint triangulation, point-cloud alignment and
Sim(3) pose-graph optimisation (reference dpvo/loop_closure/).  Retrieval,
detection and matching (NetVLAD, DISK + LightGlue) are not part of this
package: a caller brings keypoint tracks and matches
(``DPVO.close_loop_from_tracks``), matched 3-D points
(``DPVO.close_loop_from_points``) or the relative Sim3 between two keyframes
(``DPVO.close_loop``)."""
from .long_term import triangulate_keypoints
from .optim_utils import (SE3_to_Sim3, draw_samples, make_Sim3, perform_updates, ransac_umeyama, ransac_umeyama_gpu,
                          residual, run_DPVO_PGO_sychronize, umeyama_alignment)

__all__ = ["SE3_to_Sim3", "draw_samples", "make_Sim3", "perform_updates", "ransac_umeyama", "ransac_umeyama_gpu",
           "residual", "run_DPVO_PGO_sychronize", "triangulate_keypoints", "umeyama_alignment"]
