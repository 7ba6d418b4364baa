"""The long-term loop closer (reference dpvo/loop_closure/long_term.py).

triangulate_keypoints (:104-140) is composed from this package's kernels: the
fused reprojection (projective_ops.transform), the structure-only bundle
adjustment (fastba.BA with an empty pose window) and iproj.

LongTermLoopClosure (:20-287) drives retrieval, loop detection, the image
cache and the Sim(3) back end natively.  Keypoint detection and matching
(DISK + LightGlue in the reference) need weights this package does not ship:
they arrive as one `frontend` object.
"""
import torch

from .. import fastba
from .. import projective_ops as pops
from ..lietorch import SE3
from .retrieval import NMS, SKIP_WINDOW, ImageCache, Retrieval


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


class LongTermLoopClosure:
    """retrieval -> detection -> close_loop, with the reference's methods.

    frontend: any object with
      tracks(images, frames) -> (kps_prev, kps, kps_next, feats): images
        [3, 3, ht, wd] uint8 on the device, the cached frames (f - 1, f, f + 1)
        = frames; the keypoints [n_f, 2] are the full-resolution pixel
        positions of frame f's keypoints in the three frames, feats whatever
        match() wants;
      match(feats_i, feats_j) -> (match_i, match_j): index pairs over the
        keypoints tracks() returned.
    rng: the RANSAC sample source handed to close_loop_from_tracks (a numpy
    Generator or a seed; None: its default)."""

    def __init__(self, cfg, pg, nvlad_db, frontend, ht, wd, skip_window=SKIP_WINDOW, nms=NMS, capacity=None,
                 rng=None):
        for name in ("tracks", "match"):
            if not callable(getattr(frontend, name, None)):
                raise TypeError(f"LongTermLoopClosure: frontend needs a {name}() method")
        self.cfg, self.pg, self.frontend, self.rng = cfg, pg, frontend, rng
        dev = pg.poses_.device
        capacity = int(capacity if capacity is not None else pg.N)
        self.retrieval = Retrieval(nvlad_db, capacity, dev, skip_window=skip_window, nms=nms)
        self.imcache = ImageCache(capacity, ht, wd, dev)
        self.lc_count = 0

    def __call__(self, image, n, tstamp):
        self.retrieval(image, n, tstamp)
        self.imcache(image, n)

    def keyframe(self, k):
        self.retrieval.keyframe(k)
        self.imcache.keyframe(k)

    def attempt_loop_closure(self, n):
        cands = self.retrieval.detect_loop(thresh=self.cfg.LOOP_RETR_THRESH,
                                           num_repeat=self.cfg.LOOP_CLOSE_WINDOW_SIZE)
        lc_result = False
        if cands is not None:
            i, j = cands
            lc_result = self.close_loop(i, j, n)
            self.lc_count += int(bool(lc_result))
            if lc_result:
                self.retrieval.confirm_loop(i, j)
            self.retrieval.found.clear()
        # the frames that left the removal window can no longer be dropped: final
        self.retrieval.save_up_to(n - self.cfg.REMOVAL_WINDOW - 2)
        self.imcache.save_up_to(n - self.cfg.REMOVAL_WINDOW - 1)
        return lc_result

    def terminate(self, n):
        self.retrieval.save_up_to(n - 1)
        self.imcache.save_up_to(n - 1)
        self.attempt_loop_closure(n)
        self.imcache.close()
        self.retrieval.close()

    def lc_callback(self):
        """nothing to collect: the pose-graph optimisation ran inside close_loop"""

    def close_loop(self, i, j, n):
        tracks, feats = [], []
        for f in (i, j):
            frames = (f - 1, f, f + 1)
            kps_prev, kps, kps_next, ft = self.frontend.tracks(self.imcache.load_frames(frames), frames)
            tracks.append((kps_prev, kps, kps_next))
            feats.append(ft)
        match_i, match_j = self.frontend.match(feats[0], feats[1])
        kwargs = {} if self.rng is None else {"rng": self.rng}
        return self.pg.close_loop_from_tracks(i, j, tracks[0], tracks[1], match_i, match_j, **kwargs)
