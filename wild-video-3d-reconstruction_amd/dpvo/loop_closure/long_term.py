"""Keypoint triangulation for loop closure (reference
dpvo/loop_closure/long_term.py:104-140), composed from this package's kernels:
the fused reprojection (projective_ops.transform), the structure-only bundle
adjustment (fastba.BA with an empty pose window) and iproj.  Detection and
matching are the caller's: the keypoints arrive as tracks over three frames.
"""
import torch

from .. import fastba
from .. import projective_ops as pops
from ..lietorch import SE3


def triangulate_keypoints(pg, i, kps_prev, kps, kps_next, iterations=6, max_residual=2.0):
    """3-D points of n keypoints of keyframe i from their tracks into the
    keyframes i - 1 and i + 1.  kps_prev, kps, kps_next [n, 2]: the
    full-resolution pixel positions of the same keypoints in frames i - 1, i
    and i + 1 (GPU tensors).

    The reference's mini patch graph: one patch per keypoint at kps with the
    median inverse depth of frame i's patches, the edges (1 -> 0) and (1 -> 2)
    of every patch with the other two positions as targets and unit weights,
    the three poses, the intrinsics at full resolution (x RES).  A
    structure-only BA (t0 = t1 = 3) refines the inverse depths; a keypoint is
    kept when the larger of its two reprojection residuals is below
    max_residual pixels.

    -> (points [n, 3] fp32 in camera i's frame, keep [n] bool), on the device."""
    i, n_frames = int(i), int(pg.n)
    if i < 1 or i + 1 >= n_frames:
        raise RuntimeError(f"triangulate_keypoints: frame {i} needs both neighbours inside [0, {n_frames})")
    dev = pg.poses_.device
    kps_prev, kps, kps_next = (torch.as_tensor(k).to(device=dev, dtype=torch.float32) for k in (kps_prev, kps, kps_next))
    n = kps.shape[0]
    if kps.dim() != 2 or kps.shape[1] != 2 or kps_prev.shape != kps.shape or kps_next.shape != kps.shape or n < 1:
        raise RuntimeError("triangulate_keypoints: kps_prev, kps, kps_next must be [n, 2] with n >= 1")
    c = pg.P // 2
    kk = torch.arange(n, device=dev).repeat(2)
    ii = torch.ones(2 * n, device=dev, dtype=torch.long)
    jj = torch.zeros(2 * n, device=dev, dtype=torch.long)
    jj[n:] = 2

    disp = pg.patches_[i, :, 2, c, c].median()
    patches = torch.cat((kps, torch.ones(n, 1, device=dev) * disp), dim=-1)
    patches = patches[None, :, :, None, None].repeat(1, 1, 1, pg.P, pg.P).contiguous()
    target = torch.cat((kps_prev, kps_next))[None].contiguous()
    weight = torch.ones_like(target)
    poses = pg.poses[:, i - 1:i + 2].clone()
    intrinsics = pg.intrinsics[:, i - 1:i + 2].clone() * pg.RES

    lmbda = torch.as_tensor([1e-3], device=dev)
    fastba.BA(SE3(poses), patches, intrinsics, target, weight, lmbda, ii, jj, kk, 3, 3, iterations=iterations)

    coords = pops.transform(SE3(poses), patches, intrinsics, ii, jj, kk)[:, :, c, c]
    residual = (coords - target).norm(dim=-1).view(2, n)     # the edges of keypoint k are rows k and n + k
    keep = residual.max(dim=0).values < max_residual

    points = pops.iproj(patches, intrinsics[:, torch.ones(n, device=dev, dtype=torch.long)])
    points = points[0, :, c, c, :3] / points[0, :, c, c, 3:]
    return points, keep
