"""Patch-graph state container (reference dpvo/patchgraph.py:13-140).

Layout in HBM (all on the tracker's GPU):
  poses_      [N, 7]  fp32  world->camera [t, q]
  patches_    [N, M, 3, P, P] fp32  (x, y, inverse depth) at 1/RES resolution
  intrinsics_ [N, 4]  fp32  (fx, fy, cx, cy) / RES
  points_     [N*M, 3] fp32, colors_ [N, M, 3] u8, index_ [N, M] i64
  edges ii/jj/kk [E] i64, hidden state net [1, E, DIM] fp16
"""
import numpy as np
import torch

from . import projective_ops as pops
from .lietorch import SE3
from .utils import matrix_to_quaternion


class PatchGraph:
    def __init__(self, cfg, P, DIM, pmem, M, ht_resized, wd_resized, RES, device="cuda", **kwargs):
        self.cfg, self.P, self.pmem, self.DIM = cfg, P, pmem, DIM
        self.n = 0  # frames
        self.m = 0  # patches
        self.M = M
        self.N = cfg.BUFFER_SIZE
        dev = torch.device(device)
        f32 = dict(dtype=torch.float, device=dev)
        self.tstamps_ = np.zeros(self.N, dtype=np.int64)
        self.poses_ = torch.zeros(self.N, 7, **f32)
        self.poses_[:, 6] = 1.0
        self.patches_ = torch.zeros(self.N, M, 3, P, P, **f32)
        self.patches_est_ = torch.zeros(self.N, M, 3, P, P, **f32)
        self.intrinsics_ = torch.zeros(self.N, 4, **f32)
        self.points_ = torch.zeros(self.N * M, 3, **f32)
        self.colors_ = torch.zeros(self.N, M, 3, dtype=torch.uint8, device=dev)
        self.index_ = torch.zeros(self.N, M, dtype=torch.long, device=dev)
        self.index_map_ = torch.zeros(self.N, dtype=torch.long, device=dev)
        self.delta = {}  # relative poses of removed keyframes
        self.loop_ii = torch.zeros(0, dtype=torch.long, device=dev)  # loops closed so far (close_loop)
        self.loop_jj = torch.zeros(0, dtype=torch.long, device=dev)

        net_kw = {k: v for k, v in kwargs.items() if k in ("dtype",)}
        self.net = torch.zeros(1, 0, DIM, device=dev, **net_kw)
        empty = lambda: torch.zeros(0, dtype=torch.long, device=dev)
        self.ii, self.jj, self.kk = empty(), empty(), empty()
        self.ii_inac, self.jj_inac, self.kk_inac = empty(), empty(), empty()
        self.weight = torch.zeros(1, 0, 2, **f32)
        self.target = torch.zeros(1, 0, 2, **f32)
        self.weight_inac = torch.zeros(1, 0, 2, **f32)
        self.target_inac = torch.zeros(1, 0, 2, **f32)
        self.ht_resized, self.wd_resized, self.RES = ht_resized, wd_resized, RES

    @property
    def poses(self):
        return self.poses_.view(1, self.N, 7)

    @property
    def patches(self):
        return self.patches_.view(1, self.N * self.M, 3, self.P, self.P)

    @property
    def intrinsics(self):
        return self.intrinsics_.view(1, self.N, 4)

    @property
    def ix(self):
        return self.index_.view(-1)

    def edges_loop(self):
        return

    def normalize(self):
        """rescale depths to unit mean and re-anchor poses on frame 0 (patchgraph.py:68-79)."""
        s = self.patches_[:self.n, :, 2].mean()
        self.patches_[:self.n, :, 2] /= s
        self.poses_[:self.n, :3] *= s
        for t, (t0, dP) in self.delta.items():
            self.delta[t] = (t0, dP.scale(s))
        self.poses_[:self.n] = (SE3(self.poses_[:self.n]) * SE3(self.poses_[[0]]).inv()).data
        pops.point_cloud_centre(SE3(self.poses), self.patches[:, :self.m], self.intrinsics, self.ix[:self.m],
                                out=self.points_[:self.m])

    def close_loop(self, i, j, far_rel_pose, iters=30):
        """the tail of the reference's loop closer (loop_closure/long_term.py:253-287)
        for a caller who brings the matcher: far_rel_pose, Sim3 data [t, q, s],
        is the measured T_j T_i^-1 between the world-to-camera frames i and j
        (what ransac_umeyama gives for frame i's points matched to frame j's).
        The earlier loops' constraints are rebuilt from the current poses with
        scale 1, the Sim(3) pose graph over poses_[:n] is optimised on the GPU
        (cuda_ba.pgo) and poses, inverse depths and the removed frames' deltas
        below safe_i = max(loop_ii) + 1 are corrected.  Returns safe_i."""
        from .loop_closure.optim_utils import SE3_to_Sim3, run_DPVO_PGO_sychronize
        n, dev = self.n, self.poses_.device
        far = far_rel_pose.data if hasattr(far_rel_pose, "group_id") else torch.as_tensor(far_rel_pose)
        far = far.to(device=dev, dtype=torch.float64).reshape(1, 8)
        loop_poses = far
        if self.loop_ii.numel():
            Gi, Gj = SE3(self.poses_[self.loop_ii]), SE3(self.poses_[self.loop_jj])
            loop_poses = torch.cat((SE3_to_Sim3((Gj * Gi.inv()).data).to(torch.float64), far))
        loop_ii = torch.cat((self.loop_ii, torch.tensor([int(i)], device=dev)))
        loop_jj = torch.cat((self.loop_jj, torch.tensor([int(j)], device=dev)))
        pred_poses = SE3(self.poses_[:n]).inv().data
        out = run_DPVO_PGO_sychronize(pred_poses, loop_poses, loop_ii, loop_jj, iters=iters)
        self.loop_ii, self.loop_jj = loop_ii, loop_jj
        safe_i = out.shape[0]
        res, s = out.float().split([7, 1], dim=1)
        s1 = torch.ones(n, device=dev)
        s1[:safe_i] = s.squeeze(1)
        self.poses_[:safe_i] = SE3(res).inv().data
        self.patches_[:safe_i, :, 2] /= s.view(safe_i, 1, 1, 1)
        self._rescale_deltas(s1)
        # the cached point cloud follows the poses and depths
        pops.point_cloud_centre(SE3(self.poses), self.patches[:, :self.m], self.intrinsics, self.ix[:self.m],
                                out=self.points_[:self.m])
        return safe_i

    def close_loop_from_points(self, i, j, i_pts, j_pts, iterations=400, threshold=0.5, min_inliers=30,
                               max_depth=20.0, rng=None):
        """the reference's close_loop from its depth gate on
        (loop_closure/long_term.py:218-287) for a caller who brings matched
        3-D points: i_pts [N, 3] in camera i's frame and j_pts [N, 3], the
        same points in camera j's frame (GPU tensors, row k matched to row k).
        Pairs where either point lies at z >= max_depth are dropped; the
        Sim(3) between the clouds comes from RANSAC + Umeyama on the device
        (ransac_umeyama_gpu, `iterations` samples from the numpy Generator or
        seed rng); with at least min_inliers pairs and inliers the loop is
        closed: returns close_loop(i, j, far_rel_pose), the index safe_i.
        Otherwise returns False and leaves the patch graph untouched."""
        from .loop_closure.optim_utils import ransac_umeyama_gpu
        i_pts, j_pts = torch.as_tensor(i_pts), torch.as_tensor(j_pts)
        if i_pts.dim() != 2 or i_pts.shape[1] != 3 or j_pts.shape != i_pts.shape:
            raise RuntimeError("close_loop_from_points: i_pts and j_pts must both be [N, 3]")
        near = (i_pts[:, 2] < max_depth) & (j_pts[:, 2] < max_depth)
        i_pts, j_pts = i_pts[near], j_pts[near]
        if i_pts.shape[0] < min_inliers:
            return False
        far_rel_pose, inliers = ransac_umeyama_gpu(i_pts, j_pts, iterations=iterations, threshold=threshold, rng=rng)
        if far_rel_pose is None or inliers < min_inliers:
            return False
        return self.close_loop(i, j, far_rel_pose)

    def close_loop_from_tracks(self, i, j, tracks_i, tracks_j, match_i, match_j, ba_iterations=6, max_residual=2.0,
                               **kwargs):
        """close_loop for a caller who brings a detector and a matcher and
        nothing else (loop_closure/long_term.py:210-287).  tracks_i: (kps_prev,
        kps, kps_next), each [n_i, 2], the full-resolution pixel positions of
        frame i's keypoints in the keyframes i - 1, i, i + 1; tracks_j the same
        for frame j; match_i, match_j [K]: the matcher's index pairs (keypoint
        match_i[k] of frame i is keypoint match_j[k] of frame j).  Both frames
        are triangulated (loop_closure.triangulate_keypoints), a match survives
        when both of its keypoints were kept, and the matched points go to
        close_loop_from_points (whose keywords pass through)."""
        from .loop_closure.long_term import triangulate_keypoints
        dev = self.poses_.device
        pts_i, keep_i = triangulate_keypoints(self, i, *tracks_i, iterations=ba_iterations, max_residual=max_residual)
        pts_j, keep_j = triangulate_keypoints(self, j, *tracks_j, iterations=ba_iterations, max_residual=max_residual)
        match_i = torch.as_tensor(match_i, device=dev).long().view(-1)
        match_j = torch.as_tensor(match_j, device=dev).long().view(-1)
        if match_i.numel() != match_j.numel():
            raise RuntimeError("close_loop_from_tracks: match_i and match_j must have one length")
        # the reference compacts both clouds by their keep masks and the matcher then indexes the
        # compacted clouds; with matches over the original keypoints that is: position of the
        # keypoint among the kept ones = cumsum(keep) - 1
        both = keep_i[match_i] & keep_j[match_j]
        slot_i, slot_j = keep_i.cumsum(0) - 1, keep_j.cumsum(0) - 1
        i_pts = pts_i[keep_i][slot_i[match_i[both]]]
        j_pts = pts_j[keep_j][slot_j[match_j[both]]]
        return self.close_loop_from_points(i, j, i_pts, j_pts, **kwargs)

    def _rescale_deltas(self, s):
        """scale the relative poses of removed frames by the scale of the
        surviving frame their chain of deltas ends on (long_term.py:180-192)"""
        scale_of = {int(self.tstamps_[k]): s[k] for k in range(self.n)}
        for t, (t0, dP) in self.delta.items():
            src = t
            while src in self.delta:
                src = self.delta[src][0]
            self.delta[t] = (t0, dP.scale(scale_of[src]))

    def _prior_patch(self, idx, depth):
        """frame idx's patches with the inverse of the median metric depth
        under each patch's 3x3 (full-resolution) sample points."""
        patch = self.patches_[idx]
        xs = torch.clamp(patch[:, 0].long() * self.RES, 0, depth.shape[1] - 1)
        ys = torch.clamp(patch[:, 1].long() * self.RES, 0, depth.shape[0] - 1)
        med = torch.median(depth[ys, xs].view(patch.shape[0], -1), dim=1).values
        patch[:, 2] = 1 / med.view(-1, 1, 1)
        return patch

    def set_prior_depth(self, idx, depth):
        """initialise frame idx's patch depth from a metric depth map (patchgraph.py:97-110)."""
        if depth is None:
            return
        patch = self._prior_patch(idx, depth)
        self.patches_est_[idx] = patch
        self.patches_[idx] = patch

    def init_from_prior(self, depths, poses, indices, images=None):
        """known depths and camera poses for the frames in `indices`
        (patchgraph.py:112-140): depths, a list of full-resolution metric
        depth maps [H, W]; poses [N, 4, 4] camera->world matrices, stored
        inverted (world->camera) as [t, qx, qy, qz, qw].  As in the reference
        the depth is written through the patches_[idx] view (so patches_ and
        patches_est_ both get it)."""
        depths = torch.stack(list(depths), dim=0)
        dpvo_poses = create_se3_from_mat(torch.as_tensor(poses, device=depths.device, dtype=torch.float)).inv()
        for idx in indices:
            self.patches_est_[idx] = self._prior_patch(idx, depths[idx])
            self.poses_[idx] = dpvo_poses[idx].data


def create_se3_from_mat(mats):
    """[N, 4, 4] -> SE3 with data [t, qx, qy, qz, qw] (patchgraph.py:142-148)."""
    q = matrix_to_quaternion(mats[:, :3, :3])[:, [1, 2, 3, 0]]
    return SE3(torch.cat([mats[:, :3, 3], q], dim=1))
