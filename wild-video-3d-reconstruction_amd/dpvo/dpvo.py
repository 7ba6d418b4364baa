"""DPVO tracker (reference dpvo/dpvo.py:22-875), hot path on MI355X.

Public API kept: DPVO(cfg, network, ht, wd, ...), __call__(tstamp, image,
depth, mask, intrinsics), update(), keyframe(), terminate(),
terminate_keyframe(), get_pts_clr_intri(), global_bundle_adjustment().
Visualisation (rerun/viewer), inlier-ratio records and SuperPoint are out of
scope.  Loop closure (cfg.loop_enabled) runs natively from
retrieval to the pose graph; its keypoint detector and matcher are the
caller's (loop_frontend=).

MI355X-specific choices (all behind the same API):
  * the fmap rings are stored channel-last ([pmem, H, W, C], exposed through
    the reference's [1, pmem, C, H, W] shape) so altcorr streams 256-byte
    pixel rows; both pyramid levels run in one fused launch;
  * reproject / point cloud are single fused launches;
  * fastba.neighbors and BA stay on the device (no host round trip).
"""
import torch
import torch.nn.functional as F

import _dpvo_hot as H
import cuda_corr
import cuda_ba
import update_ops

from . import altcorr, fastba
from . import projective_ops as pops
from .lietorch import SE3, stack
from .net import VONet
from .patchgraph import PatchGraph
from .utils import Timer, flatmeshgrid


CORR_DIM, CORR_ROW = 882, 896  # 2 levels x 7 x 7 x 3 x 3 features; padded row
_NO_MASK = float(2 ** 31 - 1)  # the valid-cell word while no masked frame has been seen


def _ring(pmem, C, h, w, channel_last, **kw):
    if channel_last:
        return torch.zeros(1, pmem, h, w, C, **kw).permute(0, 1, 4, 2, 3)
    return torch.zeros(1, pmem, C, h, w, **kw)


class DPVO:
    def __init__(self, cfg, network, ht=480, wd=640, viz=False, path="", nvlad_db=None, rerun=False,
                 device="cuda", loop_frontend=None):
        """cfg.loop_enabled builds the long-term loop closer (dpvo.py:101-102):
        retrieval over nvlad_db, loop detection, the image cache and the
        Sim(3) back end are native; keypoint detection and matching come from
        loop_frontend (loop_closure.LongTermLoopClosure).  With loop closure on,
        cfg.DEFER_KEYFRAME loses its overlap: every __call__ applies the
        keyframe decision at its end, before the loop closer compares
        keyframe indices."""
        if viz or rerun:
            raise NotImplementedError("visualisation is out of scope for the MI355X hot-path build")
        self.long_term_lc = None
        if getattr(cfg, "loop_enabled", False) and (nvlad_db is None or loop_frontend is None):
            # the reference builds DISK + LightGlue here from remote weights; this
            # build takes them from the caller
            raise NotImplementedError("cfg.loop_enabled: loop closure needs both nvlad_db= (the precomputed "
                                      "descriptors) and loop_frontend= (keypoint tracks and matches)")
        self.cfg = cfg
        self.device = torch.device(device)
        self.load_weights(network)
        self.is_initialized = False
        self.enable_timing = False
        self.M = cfg.PATCHES_PER_FRAME
        self.N = cfg.BUFFER_SIZE
        self.enable_global_ba = cfg.ENABLE_GLOBAL_BA
        self.distance_thresh = cfg.DISTANCE_THRESH
        self.use_distance_edges = cfg.USE_DISTANCE_EDGES
        self.ht, self.wd = ht, wd
        self.tlist = []
        self.counter = 0
        self.viewer = None
        self.path = path

        self.pmem = self.mem = 36
        if self.enable_global_ba:
            self.pmem = self.N  # every frame's features kept for the global pass
        dt = torch.half if cfg.MIXED_PRECISION else torch.float
        self.kwargs = kw = {"device": self.device, "dtype": dt}
        DIM, P, RES = self.DIM, self.P, self.RES
        self.imap_ = torch.zeros(self.pmem, self.M, DIM, **kw)
        self.gmap_ = torch.zeros(self.pmem, self.M, 128, P, P, **kw)
        self.image_buffer_ = torch.zeros(self.mem, 3, ht, wd, dtype=torch.uint8, device=self.device)
        h, w = ht // RES, wd // RES
        cl = getattr(cfg, "CHANNEL_LAST_FMAPS", True)
        self.fmap1_ = _ring(self.pmem, 128, h, w, cl, **kw)
        self.fmap2_ = _ring(self.pmem, 128, h // 4, w // 4, cl, **kw)
        self.pyramid = (self.fmap1_, self.fmap2_)
        self.pg = PatchGraph(cfg, P, DIM, self.pmem, self.M, h, w, RES, device=self.device, dtype=dt)
        self.warm_up = 10
        self._lmbda = torch.as_tensor([1e-4], device=self.device)
        # BA status words (cuda_ba.forward(status=)): the last call's, and the
        # first failure since the last host check -- update() never syncs
        self._ba_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ba_fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        # the fewest valid mask cells of a natively masked frame since the last
        # host check (Patchifier.last_mask_cells); None until a mask is seen
        self._mask_cells = None
        self._ugraph = None
        self._identity = SE3.Identity(1, device=self.device)
        if getattr(cfg, "loop_enabled", False):
            from .loop_closure import LongTermLoopClosure
            self.long_term_lc = LongTermLoopClosure(cfg, self.pg, nvlad_db, loop_frontend, ht, wd)

    # ------------------------------------------------------------------ state views
    @property
    def poses(self):
        return self.pg.poses_.view(1, self.N, 7)

    @property
    def patches(self):
        return self.pg.patches_.view(1, self.N * self.M, 3, 3, 3)

    @property
    def patches_est(self):
        return self.pg.patches_est_.view(1, self.N * self.M, 3, 3, 3)

    @property
    def intrinsics(self):
        return self.pg.intrinsics_.view(1, self.N, 4)

    @property
    def ix(self):
        return self.pg.index_.view(-1)

    @property
    def imap(self):
        return self.imap_.view(1, self.pmem * self.M, self.DIM)

    @property
    def gmap(self):
        return self.gmap_.view(1, self.pmem * self.M, 128, 3, 3)

    @property
    def n(self):
        return self.pg.n

    @n.setter
    def n(self, v):
        self.pg.n = v

    @property
    def m(self):
        return self.pg.m

    @m.setter
    def m(self, v):
        self.pg.m = v

    # ------------------------------------------------------------------ weights
    def load_weights(self, network):
        if isinstance(network, str):
            from collections import OrderedDict
            state = torch.load(network, map_location="cpu", weights_only=True)
            clean = OrderedDict((k.replace("module.", ""), v) for k, v in state.items() if "update.lmbda" not in k)
            self.network = VONet()
            self.network.load_state_dict(clean)
        else:
            self.network = network
        self.DIM, self.RES, self.P = self.network.DIM, self.network.RES, self.network.P
        self.network.to(self.device).eval()

    # ------------------------------------------------------------------ outputs
    def get_pts_clr_intri(self, inlier=False):
        self.flush_keyframe()
        m = self.pg.m
        pts = pops.point_cloud_centre(SE3(self.poses), self.patches[:, :m], self.intrinsics, self.ix[:m])
        points = pts.cpu().numpy()
        colors = self.pg.colors_.view(-1, 3)[:m].cpu().numpy() * 255.0
        d = self.pg.patches_[:self.n][..., self.P // 2, self.P // 2]
        med = d[:, :, 2].median(dim=1).values
        mask = ((d[:, :, -1] > med[:, None]) & (d[:, :, -1] < 4.0 * med[:, None])).view(-1).cpu().numpy()
        intrinsic = self.pg.intrinsics_[0].cpu().numpy() * self.RES
        return points[mask], colors[mask], (intrinsic, self.ht, self.wd)

    def get_pose(self, t):
        self.flush_keyframe()
        if t in self.traj:
            return SE3(self.traj[t])
        t0, dP = self.pg.delta[t]
        return dP * self.get_pose(t0)

    def terminate(self):
        self.flush_keyframe()
        self.check_ba()
        if self.long_term_lc is not None:
            self.long_term_lc.terminate(self.n)
        if self.enable_global_ba:
            self.global_bundle_adjustment()
        self.traj = {self.pg.tstamps_[i].item(): self.pg.poses_[i] for i in range(self.n)}
        poses = stack([self.get_pose(t) for t in range(self.counter)], dim=0)
        poses = poses.inv().data.cpu().numpy()
        return poses, torch.as_tensor(self.tlist, dtype=torch.float64).numpy()

    def terminate_keyframe(self):
        self.flush_keyframe()
        if self.long_term_lc is not None:
            self.long_term_lc.terminate(self.n)
        self.traj = {self.pg.tstamps_[i].item(): self.pg.poses_[i] for i in range(self.n)}
        poses = stack([SE3(self.pg.poses_[i]) for i in range(self.n)], dim=0).inv().data.cpu().numpy()
        return poses, torch.as_tensor([self.pg.tstamps_[i] for i in range(self.n)], dtype=torch.float64).numpy()

    # ------------------------------------------------------------------ loop closure (PGO back end)
    @property
    def loop_ii(self):
        return self.pg.loop_ii

    @property
    def loop_jj(self):
        return self.pg.loop_jj

    def close_loop(self, i, j, far_rel_pose):
        """close the loop between keyframes i and j given their measured
        relative Sim3 far_rel_pose = [t, q, s] (T_j T_i^-1, world-to-camera
        frames) -- the reference's close_loop after its matcher
        (loop_closure/long_term.py:253-287): Sim(3) pose-graph optimisation on
        the GPU, then poses, depths, removed-frame deltas and the point cloud
        below max(loop_ii) + 1 are corrected in place (PatchGraph.close_loop).
        update() reads poses_ / patches_ afresh on every call (also when
        graph-captured: the buffers are written in place), so nothing else is
        cached.  This entry is for a caller with its own retrieval and
        matching; cfg.loop_enabled drives the same back end from the native
        retrieval."""
        self.flush_keyframe()
        self.check_ba()
        return self.pg.close_loop(i, j, far_rel_pose)

    def close_loop_from_points(self, i, j, i_pts, j_pts, **kwargs):
        """close_loop for matched 3-D points of the keyframes i and j (each in
        its own camera frame): the depth gate, RANSAC + Umeyama on the GPU and
        the inlier gates of long_term.py:218-251, then close_loop.  False (and
        an untouched patch graph) when a gate fails, else safe_i
        (PatchGraph.close_loop_from_points)."""
        self.flush_keyframe()
        self.check_ba()
        return self.pg.close_loop_from_points(i, j, i_pts, j_pts, **kwargs)

    def close_loop_from_tracks(self, i, j, tracks_i, tracks_j, match_i, match_j, **kwargs):
        """close_loop for a caller who brings a detector and a matcher: the
        three-frame keypoint tracks of both keyframes and the matcher's index
        pairs; triangulation, alignment and the pose-graph optimisation run
        here (PatchGraph.close_loop_from_tracks)."""
        self.flush_keyframe()
        self.check_ba()
        return self.pg.close_loop_from_tracks(i, j, tracks_i, tracks_j, match_i, match_j, **kwargs)

    # ------------------------------------------------------------------ hot path
    def corr(self, coords, indicies=None, slots=None, order=None):
        """2-level local correlation -> [1, E, 882] (dpvo.py:326-333), one fused launch.
        slots: the ring slots (kk mod M pmem, jj mod pmem) when the caller has them;
        order: the edges grouped by target frame (the matrix-core kernel's
        visiting order) when the caller has it."""
        if slots is not None:
            ii1, jj1 = slots
        else:
            ii, jj = indicies if indicies is not None else (self.pg.kk, self.pg.jj)
            ii1 = ii % (self.M * self.pmem)
            jj1 = jj % self.pmem
        E = len(ii1)
        out = table = None
        if self.gmap_.dtype == torch.float16:
            # rows padded to 896 (zeros past 882): the update operator's first
            # Linear reads them as 16-byte aligned GEMM rows without a copy
            buf = self._corr_rows(E)
            out = buf[:E, :CORR_DIM].unsqueeze(0)
            if not getattr(self.cfg, "EXACT_CORR", False) and getattr(self.cfg, "CHANNEL_LAST_FMAPS", True):
                # matrix cores, fp32 accumulation (csrc/corrmfma.hip)
                # edges grouped by target frame: one frame's map per XCD L2 at a time
                if order is None:
                    order = cuda_corr.edge_order(jj1, self.pmem)
                return altcorr.corr_pyramid_mfma(self._gmap_table(mfma=True), self.gmap.shape[1], self.pyramid,
                                                 coords, ii1, jj1, out=out, order=order).view(1, E, -1)
            table = self._gmap_table()
        return altcorr.corr_pyramid(self.gmap, self.pyramid, coords, ii1, jj1, 3, (1, 4), out=out,
                                    table=table).view(1, E, -1)

    def _gmap_table(self, mfma=False):
        """The gmap ring packed for altcorr (the exact kernel's scalar-operand
        table, or the matrix-core kernel's [patch][pixel][channel] transpose),
        re-packed only when the ring changed (torch's in-place version counter:
        new keyframes)."""
        key = (self.gmap_.data_ptr(), self.gmap_._version, mfma)
        if getattr(self, "_gtab_key", None) != key:
            pack = cuda_corr.pack_mfma if mfma else cuda_corr.pack
            old = getattr(self, "_gtab", None)
            self._gtab = pack(self.gmap, out=old if getattr(self, "_gtab_mfma", None) == mfma else None)
            self._gtab_key, self._gtab_mfma = key, mfma
        return self._gtab

    def _corr_rows(self, E):
        buf = getattr(self, "_corr_buf", None)
        if buf is None or buf.shape[0] < E:
            buf = torch.zeros(max(E, 1024) * 5 // 4, CORR_ROW, dtype=torch.float16, device=self.device)
            self._corr_buf = buf
        return buf

    def reproject(self, indicies=None):
        """patch kk from frame ii into frame jj -> [1, E, 2, P, P] (dpvo.py:335-339)."""
        ii, jj, kk = indicies if indicies is not None else (self.pg.ii, self.pg.jj, self.pg.kk)
        return pops.transform_fused(SE3(self.poses), self.patches, self.intrinsics, ii, jj, kk, chw=True)

    def append_factors(self, kk, jj):
        self.pg.jj = torch.cat([self.pg.jj, jj])
        self.pg.kk = torch.cat([self.pg.kk, kk])
        self.pg.ii = torch.cat([self.pg.ii, self.ix[kk]])
        self.pg.net = torch.cat([self.pg.net, torch.zeros(1, len(kk), self.DIM, **self.kwargs)], dim=1)

    def remove_factors(self, m, store, counts=None):
        """Boolean-mask compaction of the edge state (dpvo.py:349-364).  Each
        ``x[mask]`` is a host synchronisation (the output size); here the mask
        becomes an index once per side and every tensor is gathered with it.
        store: True (keep the removed edges as inactive factors), False, or a
        mask inside m: only those are kept.  counts: (edges kept, edges
        stored) when the caller already read them (keyframe() does, in its one
        host read): the indices then come from nonzero_static, with no
        synchronisation at all."""
        assert self.pg.ii.numel() == self.pg.weight.shape[1]
        if counts is not None and self.NATIVE_COMPACTION and self._compact_native(m, store, *counts):
            return
        if counts is None:
            index = lambda mask, _: torch.nonzero(mask).squeeze(1)
            counts = (None, None)
        else:
            index = lambda mask, size: torch.nonzero_static(mask, size=size).squeeze(1)
        if store is not False:
            rem = index(m if store is True else store, counts[1])
            for name, src, dim in (("ii_inac", self.pg.ii, 0), ("jj_inac", self.pg.jj, 0), ("kk_inac", self.pg.kk, 0),
                                   ("weight_inac", self.pg.weight, 1), ("target_inac", self.pg.target, 1)):
                self._append_inactive(name, src, rem, dim)
        keep = index(~m, counts[0])
        self.pg.weight = self.pg.weight[:, keep]
        self.pg.target = self.pg.target[:, keep]
        self.pg.ii, self.pg.jj, self.pg.kk = self.pg.ii[keep], self.pg.jj[keep], self.pg.kk[keep]
        # the kept rows of the edge state go to the front of a buffer with room
        # for the next frame's edges: its append then zeroes the new rows in
        # place instead of concatenating the whole state (146 MB at C3)
        net = self.pg.net
        n_keep = keep.numel()
        cap = H.new_empty(net, 1, n_keep + self._edge_slack(), net.shape[2])
        torch.index_select(net, 1, keep, out=cap[:, :n_keep])
        self._net_cap = cap
        self.pg.net = cap[:, :n_keep]

    def _inactive_reserve(self, name, src, add, dim):
        """room for `add` more rows of src's kind at the end of pg.<name>, in a
        buffer that doubles when full: the inactive lists grow every frame,
        and re-concatenating them would copy all of them each time.  Returns
        (the tail to write, the grown list)."""
        cur = getattr(self.pg, name)
        n0 = cur.shape[dim]
        caps = self.__dict__.setdefault("_inac_caps", {})
        cap = caps.get(name)
        if cap is None or cur.data_ptr() != cap.data_ptr() or cap.shape[dim] < n0 + add or not cur.is_contiguous():
            size = list(src.shape)
            size[dim] = max(2 * (n0 + add), 4096)
            cap = H.new_empty(src, size)
            cap.narrow(dim, 0, n0).copy_(cur)
            caps[name] = cap
        return cap.narrow(dim, n0, add), cap.narrow(dim, 0, n0 + add)

    def _append_inactive(self, name, src, rem, dim):
        """pg.<name> = cat(pg.<name>, src[rem]) along dim (dpvo.py:353-357),
        the rows gathered straight into the list's spare room"""
        cur = getattr(self.pg, name)
        if cur.dtype != src.dtype:   # torch.cat's type promotion
            setattr(self.pg, name, torch.cat((cur, src.index_select(dim, rem)), dim=dim))
            return
        tail, grown = self._inactive_reserve(name, src, rem.numel(), dim)
        torch.index_select(src, dim, rem, out=tail)
        setattr(self.pg, name, grown)

    # remove_factors through dpvo_compact_edges when the sizes are known.  Off:
    # its row move measured slower than torch's gather (102-146 vs ~45 us for
    # the 146 MB edge state at C3; profiles/r3/NOTES.md), so the two paths end
    # level; kept for the equality test and further work
    NATIVE_COMPACTION = False

    _INACTIVE = (("ii_inac", "ii", 0), ("jj_inac", "jj", 0), ("kk_inac", "kk", 0), ("weight_inac", "weight", 1),
                 ("target_inac", "target", 1))

    def _compact_native(self, m, store, n_keep, n_store):
        """remove_factors with known sizes as one native compaction
        (dpvo_compact_edges: two launches for the index fields, weights,
        targets, the edge state and the inactive-list appends).  False when
        the edge state's layout does not allow it (the caller then uses the
        torch path)."""
        pg = self.pg
        E = pg.ii.numel()
        w, t, net = pg.weight, pg.target, pg.net
        if not (w.dim() == 3 and w.shape[:2] == (1, E) and t.shape == w.shape and t.dtype == w.dtype and
                w.is_contiguous() and t.is_contiguous() and net.dim() == 3 and net.shape[:2] == (1, E) and
                net.is_contiguous() and (net.shape[2] * net.element_size()) % 16 == 0 and net.data_ptr() % 16 == 0
                and all(x.dtype == torch.int64 and x.is_contiguous() for x in (pg.ii, pg.jj, pg.kk))
                and all(getattr(pg, a).dtype == getattr(pg, b).dtype for a, b, _ in self._INACTIVE)):
            return False
        if n_keep == 0 or E == 0:
            return False
        mode = 1 if store is True else 0 if store is False else 2
        if n_store == 0:   # nothing to append (and empty tails have no address)
            mode = 0
        rm = m.contiguous().view(torch.uint8)
        sm = store.contiguous().view(torch.uint8) if mode == 2 else None
        ii_k, jj_k, kk_k = (H.empty(n_keep, dtype=torch.int64, device=self.device) for _ in range(3))
        w_k, t_k = H.new_empty(w, 1, n_keep, w.shape[2]), H.new_empty(t, 1, n_keep, t.shape[2])
        cap = H.new_empty(net, 1, n_keep + self._edge_slack(), net.shape[2])
        tails, grown = {}, {}
        if mode:
            for name, src, dim in self._INACTIVE:
                tails[name], grown[name] = self._inactive_reserve(name, getattr(pg, src), n_store, dim)
        tp = lambda name: tails[name].data_ptr() if mode else None
        nb = H.lib().dpvo_compact_edges_workspace_bytes(E)
        ws = H.empty(nb, dtype=torch.uint8, device=self.device)
        H.check(H.lib().dpvo_compact_edges(
            E, rm.data_ptr(), sm.data_ptr() if sm is not None else None, mode, pg.ii.data_ptr(), pg.jj.data_ptr(),
            pg.kk.data_ptr(), w.data_ptr(), t.data_ptr(), w.shape[2] * w.element_size(), net.data_ptr(),
            net.shape[2] * net.element_size(), ii_k.data_ptr(), jj_k.data_ptr(), kk_k.data_ptr(), w_k.data_ptr(),
            t_k.data_ptr(), cap.data_ptr(), tp("ii_inac"), tp("jj_inac"), tp("kk_inac"), tp("weight_inac"),
            tp("target_inac"), ws.data_ptr(), nb, H.stream_of(net)))
        for name, g in grown.items():
            setattr(pg, name, g)
        pg.ii, pg.jj, pg.kk, pg.weight, pg.target = ii_k, jj_k, kk_k, w_k, t_k
        self._net_cap = cap
        pg.net = cap[:, :n_keep]
        return True

    def _edge_slack(self):
        """rows one frame's append adds at most: forward and backward edges
        of PATCH_LIFETIME frames (dpvo.py:756-769)"""
        return 2 * self.M * (self.cfg.PATCH_LIFETIME + 1)

    def _append_net_rows(self, E0, E1):
        """pg.net grown from E0 to E1 rows of zeros (dpvo.py:341-347): in place
        when the compaction left room behind it, else one concatenation"""
        cap = getattr(self, "_net_cap", None)
        net = self.pg.net
        if (cap is not None and net.data_ptr() == cap.data_ptr() and net.shape[1] == E0 and E1 <= cap.shape[1]
                and net.dim() == 3 and net.is_contiguous()):
            self.pg.net = cap[:, :E1]
            self.pg.net[:, E0:].zero_()
        else:
            self.pg.net = torch.cat([net, net.new_zeros(1, E1 - E0, self.DIM)], dim=1)

    def motion_probe(self):
        """median flow of a trial update on the newest frame (dpvo.py:366-381)."""
        kk = torch.arange(self.pg.m - self.M, self.pg.m, device=self.device)
        jj = self.n * torch.ones_like(kk)
        ii = self.ix[kk]
        net = torch.zeros(1, len(ii), self.DIM, **self.kwargs)
        coords = self.reproject(indicies=(ii, jj, kk))
        with torch.autocast("cuda", enabled=self.cfg.MIXED_PRECISION):
            corr = self.corr(coords, indicies=(kk, jj))
            ctx = self.imap[:, kk % (self.M * self.pmem)]
            net, (delta, weight, _) = self.network.update(net, ctx, corr, None, ii, jj, kk)
        return torch.quantile(delta.norm(dim=-1).float(), 0.5)

    def motionmag(self, i, j):
        return self._motionmag_dev(i, j)[0].item()

    def _motionmag_dev(self, i, j):
        """[mean flow of the (i -> j) edges, of the (j -> i) edges]
        (dpvo.py:507-514), one native launch, left on the device."""
        return pops.motion_mag_pair(SE3(self.poses), self.patches, self.intrinsics, self.pg.ii, self.pg.jj,
                                    self.pg.kk, i, j, beta=0.5)

    def update(self, t0=None):
        """One keyframe of the hot loop (dpvo.py:711-749).  t0: optional lower
        bound of the optimised pose window (the reference's max(t0_, t0 or 1),
        :730-731).

        With cfg.DEFER_BA_CHECK (the default) nothing here reads the device:
        a BA Cholesky failure (the reference raises inside update(),
        ba_cuda.cu:521) lands in a device status word and is raised by the
        next host read -- keyframe()'s, check_ba(), terminate(), or the end of
        the initialisation updates in __call__ -- so it surfaces up to one
        frame later than in the reference.  The same word first receives the
        window-key check (an edge outside the 64-frame key window); BA then
        skips the step instead of updating depths from merged groups.
        DEFER_BA_CHECK = False restores the immediate raise."""
        self.flush_keyframe()
        defer = getattr(self.cfg, "DEFER_BA_CHECK", True)
        if defer:
            self._ba_status.zero_()
        with Timer("other", enabled=self.enable_timing):
            coords = self.reproject()
            # the edges grouped by patch once, on the device: the update
            # operator's SoftAgg over kk and temporal neighbours, and BA's
            # per-patch reduction all read this CSR
            if self._window_keys():
                # the ring slots (context rows, corr) and both group-bys over the
                # window keys in four launches (an edge outside the window sets
                # the deferred failure word: the next keyframe() / check_ba() raises)
                # (+ the edges grouped by target frame: altcorr's visiting order)
                ctx_idx, jslot, kk_groups, ij_groups, order = update_ops.window_group_by(
                    self.pg.ii, self.pg.jj, self.pg.kk, self.M, self.n - 64, self.M * self.pmem, self.pmem,
                    flag=self._ba_status if defer else self._ba_fail, jj_order=True)
                slots = (ctx_idx, jslot)
            else:
                kk_groups, ij_groups = self._kk_groups(), self._ij_groups()
                ctx_idx = self.pg.kk % (self.M * self.pmem)
                slots = order = None
            with torch.autocast("cuda", enabled=True):
                corr = self.corr(coords, slots=slots, order=order)
                # ctx = imap[:, kk % (M pmem)] (dpvo.py:718), gathered by the consumer
                self.pg.net, (delta, weight, _) = self.network.update(self.pg.net, self.imap, corr, None, self.pg.ii,
                                                                      self.pg.jj, self.pg.kk, inp_idx=ctx_idx,
                                                                      index_bounds=(self.N * self.M, self.N),
                                                                      kk_groups=kk_groups, ij_groups=ij_groups)
            centre = coords[..., self.P // 2, self.P // 2]
            if delta.dtype == torch.float16 and weight.dtype == torch.float16 and delta.stride(2) == 1:
                target, weight = update_ops.edge_targets(centre, delta, weight)   # one launch
            else:
                weight = weight.float()
                target = centre + delta.float()
        self.pg.target = target
        self.pg.weight = weight
        with Timer("BA", enabled=self.enable_timing):
            t0_ = self.n - self.cfg.OPTIMIZATION_WINDOW if self.is_initialized else 1
            t0 = max(t0_, t0 or 1)
            fastba.BA(self.poses, self.patches, self.intrinsics, target, weight, self._lmbda, self.pg.ii, self.pg.jj,
                      self.pg.kk, t0, self.n, getattr(self.cfg, "BA_ITERATIONS", 2), csr=kk_groups[1:],
                      status=self._ba_status if defer else None, keep_status=defer, **self._depth_prior())
            if defer:   # keep the first failure until a host read looks at it
                torch.where(self._ba_fail == 0, self._ba_status, self._ba_fail, out=self._ba_fail)
            m = self.pg.m
            pops.point_cloud_centre(SE3(self.poses), self.patches[:, :m], self.intrinsics, self.ix[:m],
                                    out=self.pg.points_[:m])

    def update_get_corr(self):
        """dpvo.py:660-687: update() whose BA failure is caught and reported as
        a warning (the reference's bare ``except``), returning (points of all
        m stored patches [m, 3], target [1, E, 2]).  The reference stores the
        points into ``self.points_``, which DPVO does not have (its
        AttributeError at :686 makes the method unusable there); they go to
        ``pg.points_`` here, where update() writes them.  Like the reference it
        leaves pg.target / pg.weight as they were.  Only a Cholesky failure of
        THIS call becomes the warning: failures pending from earlier update()s
        and the window-key flag (-2) raise, as their next host read would."""
        defer = getattr(self.cfg, "DEFER_BA_CHECK", True)
        if defer:
            self.check_ba()   # earlier updates' status: raised, never swallowed here
        saved = (self.pg.target, self.pg.weight)
        try:
            self.update()
            status = int(self._ba_fail.item()) if defer else 0
        except RuntimeError as e:
            if "cholesky" not in str(e):
                raise
            status = 1
            # the immediate raise left update() before its point refresh; the
            # reference catches around BA only and still recomputes the points
            m = self.pg.m
            pops.point_cloud_centre(SE3(self.poses), self.patches[:, :m], self.intrinsics, self.ix[:m],
                                    out=self.pg.points_[:m])
        finally:
            target = self.pg.target
            self.pg.target, self.pg.weight = saved
        if status > 0:
            self._ba_fail.zero_()
            print("Warning BA failed...")
        elif status:
            self._ba_fail.zero_()
            cuda_ba.raise_for_status(status)
        # a fresh tensor, as the reference returns (pg.points_ is rewritten by
        # the next update())
        return self.pg.points_[:self.pg.m].clone(), target

    def _depth_prior(self):
        """BA's depth-prior arguments (cfg.DEPTH_PRIOR_BA: the call the reference
        holds commented out, dpvo.py:736-745): the persistent patches_est_
        buffer and a host constant, so nothing new is read inside update()."""
        if not getattr(self.cfg, "DEPTH_PRIOR_BA", False):
            return {}
        return dict(patches_est=self.patches_est, prior_mu=float(getattr(self.cfg, "DEPTH_PRIOR_MU", 2.0)))

    def _window_keys(self):
        """True when every edge of the sliding window has n - 64 <= ii, jj < n
        (see _ij_groups) for this config."""
        return (self.cfg.REMOVAL_WINDOW + self.cfg.PATCH_LIFETIME + 2 <= 64 and
                getattr(self.cfg, "WINDOW_IJ_KEY", True))

    def _kk_groups(self):
        """The edges grouped by patch (the update operator's SoftAgg over kk,
        its temporal neighbours and BA's per-patch reduction all read this
        CSR).  Patch kk lives in frame kk // M = ii >= n - 64 (see _ij_groups),
        so kk - M (n - 64) is a key below 64 M in the same order: the same
        groups from a counting sort over 64 M bins instead of N M."""
        if not self._window_keys():
            return update_ops.group_by(self.pg.kk, key_bits=update_ops.key_bits_for(self.N * self.M))
        return update_ops.group_by(self.pg.kk - self.M * (self.n - 64), key_bits=update_ops.key_bits_for(64 * self.M))

    def _ij_groups(self):
        """The update operator's SoftAgg over frame pairs groups the edges by
        ii * 12345 + jj (net.py:88), a key the device group-by must radix-sort
        (~80 us at C3).  Inside the sliding window every edge has
        n - 64 <= jj, ii < n: the patch frame ii >= n - REMOVAL_WINDOW - 1
        (keyframe() retires older ones, dpvo.py:654-658) and the target
        jj >= ii - PATCH_LIFETIME (dpvo.py:756-769).  So (ii - b) * 64 + (jj - b),
        b = n - 64, is a 12-bit key in the same lexicographic order: the same
        groups in the same order (bit-identical results) by a counting sort.
        None (the operator's own key) when the config's windows could exceed it."""
        if not self._window_keys():
            return None
        b = self.n - 64
        key = (self.pg.ii - b) * 64 + (self.pg.jj - b)
        return update_ops.group_by(key, key_bits=12)

    def check_ba(self, status=None):
        """raise the reference's BA error (ba_cuda.cu:521) if an update() since
        the last check failed; status: that word already read by the caller."""
        if status is None:
            status = int(self._ba_fail.item())
            if self._mask_cells is not None:
                cells = int(self._mask_cells.item())
                self._mask_cells.fill_(_NO_MASK)
                self.check_mask_cells(cells)
        if status:
            self._ba_fail.zero_()
            cuda_ba.raise_for_status(status)

    def check_mask_cells(self, cells):
        """a masked frame needs PATCHES_PER_FRAME valid cells (the reference
        fails at its view(n, patches_per_image), net.py:144-145); cells: the
        fewest of the frames since the last check, as read by the caller."""
        if cells < self.M:
            raise RuntimeError(f"the mask left {int(cells)} valid cells on a frame, fewer than "
                               f"PATCHES_PER_FRAME = {self.M}")

    def update_graphed(self, t0=None):
        """update(), replayed from a HIP graph while the patch graph is
        unchanged.  The first call for a given edge set runs update() eagerly
        and captures it (no host synchronisation happens inside update());
        later calls replay it: one launch instead of ~60 from Python.  The
        capture is keyed on everything its kernels' arguments depend on (edge
        tensors, n, t0, the gmap ring's version); keyframe() / new frames
        change the key and the next call captures again."""
        if not getattr(self.cfg, "DEFER_BA_CHECK", True):
            raise RuntimeError("update_graphed needs cfg.DEFER_BA_CHECK (no host read inside update())")
        # a deferred keyframe() decision changes the edges: apply it before the
        # replay key is formed (the reference's order is keyframe, then update)
        self.flush_keyframe()
        key = (self.pg.ii.data_ptr(), self.pg.jj.data_ptr(), self.pg.kk.data_ptr(), self.pg.ii.numel(), self.n,
               t0, self.gmap_._version, self.pg.net.data_ptr(), self.pg.net.shape)
        if self._ugraph is not None and self._ugraph[0] == key:
            self._ugraph[1].replay()
            self.pg.target, self.pg.weight = self._ugraph[2]
            return
        self._ugraph = None
        self.update(t0)                    # this call's update, eagerly (also warms every cache)
        net_in = self.pg.net               # the state the graph reads and (copied back) writes
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.update(t0)
            net_in.copy_(self.pg.net)
        outs = (self.pg.target, self.pg.weight)
        self.pg.net = net_in
        self._ugraph = ((self.pg.ii.data_ptr(), self.pg.jj.data_ptr(), self.pg.kk.data_ptr(), self.pg.ii.numel(),
                         self.n, t0, self.gmap_._version, net_in.data_ptr(), net_in.shape), g, outs)

    def keyframe(self):
        """drop a redundant keyframe, retire old edges (dpvo.py:605-658).

        With cfg.DEFER_KEYFRAME the decision's one host read is deferred: this
        call only enqueues the device work (both outcomes' edge masks, the
        motion magnitudes, the BA status, the NaN check) and an asynchronous
        copy of its values, and the next __call__ applies the decision after
        enqueueing its frame's encoders -- the GPU runs them while the host
        waits for the copy and launches the bookkeeping, instead of idling.
        The state is the reference's once the decision is applied: by the next
        __call__, update(), update_graphed(), terminate(), terminate_keyframe(),
        global_bundle_adjustment(), get_pts_clr_intri(), get_pose() or
        flush_keyframe().  The plain state views (n, m, poses, patches, pg.*)
        do NOT apply it: call flush_keyframe() before reading them.  With
        cfg.loop_enabled the same __call__ applies it at its end (the loop
        closer compares keyframe indices), so nothing is overlapped."""
        self.flush_keyframe()
        pend = self._keyframe_begin()
        if getattr(self.cfg, "DEFER_KEYFRAME", False):
            self._kf_pending = pend
        else:
            self._keyframe_finish(pend)

    def flush_keyframe(self):
        """apply a deferred keyframe() decision (cfg.DEFER_KEYFRAME), if any."""
        pend = getattr(self, "_kf_pending", None)
        if pend is not None:
            self._kf_pending = None
            self._keyframe_finish(pend)

    def _keyframe_begin(self):
        k = self.n - self.cfg.KEYFRAME_INDEX
        i, j = k - 1, k + 1
        RW = self.cfg.REMOVAL_WINDOW
        # the edge state of both outcomes, formed before the decision: keep
        # (edges whose patch left the removal window, :654-658) and drop (the
        # edges of frame k go, :616-617, the frames above k move down by one,
        # then the retirement); with one host read for both motion directions
        # (the reference reads each, :609), the deferred BA status of the
        # update()s since the last one, the pose-NaN check of the keep path
        # (:647, its own read there) and the compaction sizes -- so the
        # compaction needs no synchronisation of its own.  Four launches.
        mm = self._motionmag_dev(i, j)
        masks, idx_d, vals = pops.keyframe_masks(self.pg.ii, self.pg.jj, self.pg.kk, self.ix, k, self.M, self.n, RW,
                                                 mm, self._ba_fail, self.pg.poses_[k])
        host = getattr(self, "_kf_host", None)
        if host is None:
            host = self._kf_host = torch.empty(8, dtype=torch.float64, pin_memory=True)
        host[:7].copy_(vals, non_blocking=True)
        # the masked frames' fewest valid cells ride on the same read
        host[7] = _NO_MASK
        if self._mask_cells is not None:
            host[7:].copy_(self._mask_cells, non_blocking=True)
            self._mask_cells.fill_(_NO_MASK)
        ev = torch.cuda.Event()
        ev.record()
        return dict(k=k, E=self.pg.kk.numel(), old_keep=masks[0], old_d=masks[1], rm_d=masks[2], idx_d=idx_d,
                    thresh=self.cfg.KEYFRAME_THRESH, event=ev)

    def _keyframe_finish(self, pd):
        pd["event"].synchronize()
        vals = self._kf_host.tolist()
        k, E = pd["k"], pd["E"]
        self.check_mask_cells(vals[7])
        self.check_ba(int(vals[2]))
        n_old_keep, n_old_d, n_rm_d = (int(v) for v in vals[4:7])
        m = vals[0] + vals[1]
        if m / 2 < pd["thresh"]:
            t0, t1 = self.pg.tstamps_[k - 1:k + 1].tolist()
            self.pg.delta[t1] = (t0, pops.pose_relative(self.pg.poses_[k], self.pg.poses_[k - 1]))
            # x[x > k] -= 1, formed by keyframe_masks: no mask-size synchronisation
            self.pg.ii, self.pg.jj, self.pg.kk = pd["idx_d"].unbind(0)
            # frames k+1 .. n-1 move down by one in every per-frame buffer, one
            # launch (the reference's per-frame loop, :626-639, reads each
            # source before overwriting it, as the kernel's ascending walk does)
            n = self.n
            if n - 1 > k:
                self.pg.tstamps_[k:n - 1] = self.pg.tstamps_[k + 1:n].copy()
                bufs = [(b, 0, 0) for b in (self.pg.colors_, self.pg.poses_, self.pg.patches_, self.pg.patches_est_,
                                            self.pg.intrinsics_)]
                bufs += [(self.imap_, 0, self.pmem), (self.gmap_, 0, self.pmem), (self.fmap1_, 1, self.pmem),
                         (self.fmap2_, 1, self.pmem), (self.image_buffer_, 0, self.mem)]
                pops.frame_shift(bufs, k, n)
            self.n -= 1
            self.pg.m -= self.M
            self.keyframes_dropped = getattr(self, "keyframes_dropped", 0) + 1
            if self.long_term_lc is not None:
                self.long_term_lc.keyframe(k)
            # frame k's edges and the retired ones in one compaction (stable,
            # so the same order as the reference's two)
            self.remove_factors(pd["rm_d"], store=pd["old_d"], counts=(E - n_rm_d, n_old_d))
        elif vals[3]:
            raise Exception("Error: the estimated pose is nan!")
        else:
            self.remove_factors(pd["old_keep"], store=True, counts=(E - n_old_keep, n_old_keep))

    # ------------------------------------------------------------------ global BA (C4)
    def compute_keyframe_distance(self, i, j, beta=0.5):
        if i >= self.n or j >= self.n:
            return float("inf")
        M, d = self.M, self.device
        fi = lambda a, b: pops.flow_mag(SE3(self.poses), self.patches, self.intrinsics,
                                        torch.full((M,), a, device=d, dtype=torch.long),
                                        torch.full((M,), b, device=d, dtype=torch.long),
                                        torch.arange(M * a, M * (a + 1), device=d), beta=beta)
        return (0.5 * (fi(i, j).mean() + fi(j, i).mean())).item()

    def get_distance_based_edges(self):
        """(ii, jj) device tensors: the sequential edges, then every (i, j),
        j >= i + 2, whose keyframe distance is below DISTANCE_THRESH, in the
        reference's row-major order (dpvo.py:409-429).  All pair distances come
        from one keyframe_flow launch and one compaction -- the reference's
        loop makes two flow_mag calls and a host read per pair."""
        d = self.device
        if not self.use_distance_edges or self.n < 2:
            e = torch.zeros(0, dtype=torch.long, device=d)
            return e, e
        n = self.n
        D = pops.keyframe_flow(SE3(self.poses), self.patches, self.intrinsics, n, self.M, beta=0.5)
        dist = 0.5 * (D + D.t())
        near = torch.triu(dist < self.distance_thresh, diagonal=2).nonzero()
        seq = torch.arange(n - 1, device=d)
        return torch.cat([seq, near[:, 0]]), torch.cat([seq + 1, near[:, 1]])

    def _distance_edges_loop(self):
        """the reference's pair loop (dpvo.py:409-429), for tests"""
        if not self.use_distance_edges or self.n < 2:
            return [], []
        ii = list(range(self.n - 1))
        jj = list(range(1, self.n))
        for i in range(self.n):
            for j in range(i + 2, self.n):
                if self.compute_keyframe_distance(i, j) < self.distance_thresh:
                    ii.append(i)
                    jj.append(j)
        return ii, jj

    def global_corr(self, coords, ii, jj, kk):
        return self.corr(coords, (kk, jj))

    def global_bundle_adjustment(self):
        """one fastba pass over every keyframe (dpvo.py:436-505)."""
        self.flush_keyframe()
        if not self.enable_global_ba or self.n < 2:
            return
        if self.use_distance_edges:
            ii_e, jj_e = self.get_distance_based_edges()
        else:
            ii_e, jj_e = list(range(self.n - 1)), list(range(1, self.n))
            for i in range(0, self.n, 5):
                for j in range(i + 10, min(i + 20, self.n)):
                    ii_e.append(i)
                    jj_e.append(j)
        if len(ii_e) == 0:
            return
        d, M = self.device, self.M
        ie = torch.as_tensor(ii_e, device=d)
        je = torch.as_tensor(jj_e, device=d)
        ii = ie.repeat_interleave(M)
        jj = je.repeat_interleave(M)
        kk = (ie[:, None] * M + torch.arange(M, device=d)[None]).reshape(-1)
        coords = self.reproject((ii, jj, kk))
        with torch.autocast("cuda", enabled=True):
            corr = self.global_corr(coords, ii, jj, kk)
            ctx = self.imap[:, kk]
            net = torch.zeros(1, len(ii), self.DIM, **self.kwargs)
            net, (delta, weight, _) = self.network.update(net, ctx, corr, None, ii, jj, kk)
        target = coords[..., self.P // 2, self.P // 2] + delta.float()
        try:
            fastba.BA(self.poses, self.patches, self.intrinsics, target, weight.float(), self._lmbda, ii, jj, kk, 1,
                      self.n, 2, **self._depth_prior())
        except Exception as e:  # the reference logs and carries on (dpvo.py:499-501)
            print(f"Global BA failed: {e}")

    # ------------------------------------------------------------------ ingest
    def _edges_forw(self):
        r = self.cfg.PATCH_LIFETIME
        t0, t1 = self.M * max(self.n - r, 0), self.M * max(self.n - 1, 0)
        return flatmeshgrid(torch.arange(t0, t1, device=self.device),
                            torch.arange(self.n - 1, self.n, device=self.device), indexing="ij")

    def _edges_back(self):
        r = self.cfg.PATCH_LIFETIME
        t0, t1 = self.M * max(self.n - 1, 0), self.M * max(self.n, 0)
        return flatmeshgrid(torch.arange(t0, t1, device=self.device),
                            torch.arange(max(self.n - r, 0), self.n, device=self.device), indexing="ij")

    def __call__(self, tstamp, image, depth, mask, intrinsics):
        """track one frame (dpvo.py:771-875)."""
        if self.pg.n + 1 >= self.pg.N and getattr(self, "_kf_pending", None) is None:
            raise Exception(f'The buffer size is too small. You can increase it using "--buffer {self.N * 2}"')
        with torch.autocast("cuda", enabled=self.cfg.MIXED_PRECISION):
            fmap, gmap, imap, patches, _, clr = self.network.patchify(
                image, patches_per_image=self.cfg.PATCHES_PER_FRAME, gradient_bias=self.cfg.GRADIENT_BIAS,
                return_color=True, mask=mask)
        cells = self.network.patchify.last_mask_cells
        if cells is not None:   # a natively masked frame: too few cells raise at the next host check
            if self._mask_cells is None:
                self._mask_cells = torch.full((1,), _NO_MASK, dtype=torch.float64, device=self.device)
            torch.minimum(self._mask_cells, cells, out=self._mask_cells)
        # the previous frame's deferred keyframe decision (cfg.DEFER_KEYFRAME),
        # its host read overlapping this frame's encoders
        self.flush_keyframe()
        if self.pg.n + 1 >= self.pg.N:
            raise Exception(f'The buffer size is too small. You can increase it using "--buffer {self.N * 2}"')
        n = self.n
        self.tlist.append(tstamp)
        self.pg.tstamps_[n] = self.counter
        self.pg.intrinsics_[n] = intrinsics / self.RES
        self.pg.colors_[n] = ((clr[0, :, [2, 1, 0]] + 0.5) * (255.0 / 2)).to(torch.uint8)
        self.pg.index_[n + 1] = n + 1
        self.pg.index_map_[n + 1] = self.pg.m + self.pg.M
        if n > 1:
            if self.cfg.MOTION_MODEL == "DAMPED_LINEAR":
                # Exp(s Log(P1 P2^-1)) P1 in one launch (five lietorch calls in the reference)
                *_, a, b, c = [1] * 3 + self.tlist
                pops.pose_extrapolate(self.pg.poses_, n, self.cfg.MOTION_DAMPING * ((c - b) / (b - a)))
            else:
                self.pg.poses_[n] = self.pg.poses_[n - 1]
        patches[:, :, 2] = torch.rand_like(patches[:, :, 2, 0, 0, None, None])
        ref_depth = None
        if self.is_initialized:
            if depth is not None and mask is not None:
                s = torch.median(self.pg.patches_[n - 3:n, :, 2])
                ref_depth = (1 / s) / torch.median(depth[mask]) * depth
                patches[:, :, 2] = ref_depth[mask].median()
            elif depth is not None:
                ref_depth = depth
        elif depth is not None:
            ref_depth = depth
        self.pg.patches_[n] = patches
        if ref_depth is not None:
            self.pg.set_prior_depth(n, ref_depth)

        slot = n % self.pmem
        self.imap_[slot] = imap.squeeze()
        self.gmap_[slot] = gmap.squeeze()
        self.fmap1_[:, slot] = fmap[0]   # avg_pool2d(fmap[0], 1, 1) (dpvo.py:840) is the identity
        self.fmap2_[:, slot] = F.avg_pool2d(fmap[0], 4, 4)
        self.image_buffer_[n % self.mem] = image
        if self.long_term_lc is not None:
            self.long_term_lc(image, n, self.counter)
        self.counter += 1
        if n > 0 and not self.is_initialized:
            if self.motion_probe() < 2.0:
                self.pg.delta[self.counter - 1] = (self.counter - 2, self._identity[0])
                return
        self.pg.n += 1
        self.pg.m += self.M
        # forward then backward edges (dpvo.py:799-800) in one append: the
        # index lists in one launch (update_ops.append_edges = _edges_forw,
        # _edges_back and append_factors' concatenations), the edge state
        # (net: E x 384 fp32) reallocated once per frame, not twice
        E0 = self.pg.ii.numel()
        self.pg.ii, self.pg.jj, self.pg.kk = update_ops.append_edges(self.pg.ii, self.pg.jj, self.pg.kk, self.ix,
                                                                     self.n, self.M, self.cfg.PATCH_LIFETIME)
        self._append_net_rows(E0, self.pg.ii.numel())
        if self.n == self.warm_up and not self.is_initialized:
            self.is_initialized = True
            for _ in range(12):
                self.update()
            self.check_ba()   # the initialisation's deferred BA status (one host read, once)
        elif self.is_initialized:
            self.update()
            self.keyframe()
        if self.long_term_lc is not None:
            # the (deferred) keyframe decision first: the loop closer compares keyframe indices
            self.flush_keyframe()
            self.long_term_lc.attempt_loop_closure(self.n)
            self.long_term_lc.lc_callback()
