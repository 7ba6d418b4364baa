"""Loop closure (reference dpvo/loop_closure/): descriptor retrieval and loop
detection (``Retrieval``, csrc/retrieval.hip), the keyframe image cache
(``ImageCache``), keypoint triangulation, point-cloud alignment and Sim(3)
pose-graph optimisation, driven by ``LongTermLoopClosure`` behind
``cfg.loop_enabled``.  Keypoint detection and matching (DISK + LightGlue in
the reference) are not part of this package: they arrive as one object,
``DPVO(..., loop_frontend=)``.  A caller with its own detection logic can still
bring keypoint tracks and matches (``DPVO.close_loop_from_tracks``), matched
3-D points (``DPVO.close_loop_from_points``) or the relative Sim3 between two
keyframes (``DPVO.close_loop``)."""
from .long_term import LongTermLoopClosure, triangulate_keypoints
from .optim_utils import (SE3_to_Sim3, draw_samples, make_Sim3, perform_updates, ransac_umeyama, ransac_umeyama_gpu,
                          residual, run_DPVO_PGO_sychronize, umeyama_alignment)
from .retrieval import ImageCache, Retrieval

__all__ = ["ImageCache", "LongTermLoopClosure", "Retrieval", "SE3_to_Sim3", "draw_samples", "make_Sim3",
           "perform_updates", "ransac_umeyama", "ransac_umeyama_gpu", "residual", "run_DPVO_PGO_sychronize",
           "triangulate_keypoints", "umeyama_alignment"]
