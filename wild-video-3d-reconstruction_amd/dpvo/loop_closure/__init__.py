"""Loop-closure back end: Sim(3) pose-graph optimisation and point-cloud
alignment (reference dpvo/loop_closure/).  Retrieval and matching (NetVLAD,
DISK + LightGlue) are not part of this package: a caller brings the relative
Sim3 between two keyframes and hands it to ``DPVO.close_loop``."""
from .optim_utils import (SE3_to_Sim3, make_Sim3, perform_updates, ransac_umeyama, residual,
                          run_DPVO_PGO_sychronize, umeyama_alignment)

__all__ = ["SE3_to_Sim3", "make_Sim3", "perform_updates", "ransac_umeyama", "residual",
           "run_DPVO_PGO_sychronize", "umeyama_alignment"]
