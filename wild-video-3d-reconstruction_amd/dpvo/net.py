"""Patchifier and learned update operator (reference dpvo/net.py:28-176).

These are the hot path's callers and stay PyTorch (hipBLASLt GEMMs); their
native pieces -- altcorr.patchify and fastba.neighbors -- run on the HIP
library.  Parameter names follow the reference so dpvo.pth loads unchanged.
Training (VONet.forward, net.py:355-440) is out of scope for this build.
"""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import update_ops

from . import altcorr, fastba
from .blocks import GatedResidual, GradientClip, SoftAgg
from .extractor import BasicEncoder4
from .utils import coords_grid_with_index

DIM = 384


class Update(nn.Module):
    def __init__(self, p):
        super().__init__()
        mlp = lambda: nn.Sequential(nn.Linear(DIM, DIM), nn.ReLU(inplace=True), nn.Linear(DIM, DIM))
        self.c1, self.c2 = mlp(), mlp()
        self.norm = nn.LayerNorm(DIM, eps=1e-3)
        self.agg_kk = SoftAgg(DIM)
        self.agg_ij = SoftAgg(DIM)
        self.gru = nn.Sequential(nn.LayerNorm(DIM, eps=1e-3), GatedResidual(DIM),
                                 nn.LayerNorm(DIM, eps=1e-3), GatedResidual(DIM))
        self.corr = nn.Sequential(nn.Linear(2 * 49 * p * p, DIM), nn.ReLU(inplace=True), nn.Linear(DIM, DIM),
                                  nn.LayerNorm(DIM, eps=1e-3), nn.ReLU(inplace=True), nn.Linear(DIM, DIM))
        self.d = nn.Sequential(nn.ReLU(inplace=False), nn.Linear(DIM, 2), GradientClip())
        self.w = nn.Sequential(nn.ReLU(inplace=False), nn.Linear(DIM, 2), GradientClip(), nn.Sigmoid())
        self._pk = None

    FUSED = True  # inference under fp16 autocast runs the fused HIP path (class-level switch for A/B tests)
    CORR_CHAIN3 = True  # the corr MLP + first LayerNorm as one three-GEMM launch (False: two launches)
    FUSE_AGG_ADD = True  # the agg_kk row add inside agg_ij's f / g launch (False: a rowadd_ln pass; same bits)
    # the first GRU chain forms its residual norm(net + agg_kk + agg_ij) in its
    # epilogue (rowadd_ln writes only the fp16 rows; False: the fp32 rows too; same bits)
    FUSE_GRU_RES = True

    # ------------------------------------------------------------ fused path
    def _packed(self):
        """fp16 GEMM operands (what autocast casts the parameters to), rebuilt when any parameter changes."""
        key = tuple((q.data_ptr(), q._version) for q in self.parameters())
        if self._pk is not None and self._pk[0] == key:
            return self._pk[1]
        P = update_ops.pack_linear
        ln = lambda m: (m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous(), m.eps)
        # chain operands and the plain GEMMs read their W k-blocked (update_ops.kblock)
        KB = lambda wb: (update_ops.kblock(wb[0]), wb[1])
        agg = lambda a: (KB(P(a.f.weight, a.f.bias)), KB(P(a.g.weight, a.g.bias)), KB(P(a.h.weight, a.h.bias)))
        gr = lambda g: (KB(P(g.gate[0].weight, g.gate[0].bias)), KB(P(g.res[0].weight, g.res[0].bias)),
                        KB(P(g.res[2].weight, g.res[2].bias)))
        pk = {
            "corr": (KB(P(self.corr[0].weight, self.corr[0].bias)), KB(P(self.corr[2].weight, self.corr[2].bias)),
                     ln(self.corr[3]), KB(P(self.corr[5].weight, self.corr[5].bias))),
            "corr5": P(self.corr[5].weight, self.corr[5].bias),   # (the two-launch variant's rowgemm)
            "norm": ln(self.norm),
            "c1": (KB(P(self.c1[0].weight, self.c1[0].bias)), KB(P(self.c1[2].weight, self.c1[2].bias))),
            "c2": (KB(P(self.c2[0].weight, self.c2[0].bias)), KB(P(self.c2[2].weight, self.c2[2].bias))),
            "agg_kk": agg(self.agg_kk), "agg_ij": agg(self.agg_ij),
            "gru": (ln(self.gru[0]), gr(self.gru[1]), ln(self.gru[2]), gr(self.gru[3])),
            "heads": (torch.cat([self.d[1].weight, self.w[1].weight]).detach().half().contiguous(),
                      torch.cat([self.d[1].bias, self.w[1].bias]).detach().half().contiguous()),
        }
        self._pk = (key, pk)
        return pk

    def _fusable(self, net, inp, corr):
        return (not torch.is_grad_enabled() and net.is_cuda and net.dtype == torch.float32 and
                inp.dtype == torch.float16 and corr.dtype == torch.float16 and net.shape[0] == 1 and
                torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16 and
                self.FUSED)

    def _forward_fused(self, net, inp, corr, ii, jj, kk, inp_idx=None, index_bounds=None, kk_groups=None,
                       ij_groups=None):
        """The same dataflow as the reference under autocast, in 19 full-row
        fused GEMMs (csrc/rowgemm.hip; the corr MLP + LayerNorm as one
        three-GEMM chain, 4 more Linear->ReLU->Linear pairs chained; 11
        launches) + 2 SoftAggs: every Linear is an fp16
        GEMM with fp32 accumulate; residual adds, LayerNorms, gating and the
        d/w heads run in fp32 in the GEMM epilogues."""
        U = update_ops
        pk = self._packed()
        E = net.shape[1]
        c = corr[0]
        if c.stride(0) < 896 or c.data_ptr() % 16:
            padded = torch.zeros(E, 896, dtype=torch.float16, device=c.device)
            padded[:, :c.shape[1]] = c
            c = padded
        c0, c1, cln, c2 = pk["corr"]
        # inp rows gathered inside the epilogue when the caller passes the index
        # (DPVO.update: imap[:, kk % (M pmem)], dpvo.py:718) -- no E x 384 copy
        res16, res16_idx = (inp[0], inp_idx) if inp_idx is not None else (inp[0].contiguous(), None)
        if self.CORR_CHAIN3:
            # the corr MLP (Linear -> ReLU -> Linear -> LN -> ReLU -> Linear) and
            # norm(net + inp + .) in one launch, both intermediates on chip
            n32, n16, _ = U.rowchain(c, *c0, *c2, flags1=U.RELU, mid=(*c1, cln), flags=U.RES | U.LN, res32=net[0],
                                     res16=res16, res16_idx=res16_idx, ln=pk["norm"], want32=True)
        else:   # two launches, the LN'd intermediate through HBM (bit-identical)
            _, h, _ = U.rowchain(c, *c0, *c1, flags1=U.RELU, flags=U.LN | U.LN_RELU, ln=cln)
            n32, n16, _ = U.rowgemm(h, *pk["corr5"], flags=U.RES | U.LN, res32=net[0], res16=res16,
                                    res16_idx=res16_idx, ln=pk["norm"], want32=True)
        # the kk group-by (SoftAgg below) also yields the temporal neighbours:
        # fastba.neighbors(kk, jj) without a second sort
        # radix-sort key widths: from the caller's index bounds (the tracker
        # knows its buffer: kk < N M, ii, jj < N), else full 64-bit keys
        kk_bits, ij_bits = 64, 64
        if index_bounds is not None:
            kk_bits = U.key_bits_for(index_bounds[0])
            # (ii, jj) keys stay on the radix path: ~500 distinct pairs spread
            # over N^2 counting bins cost more to scan (40 us at N = 2048) and
            # to count (same-bin atomics) than the radix sort does
            ij_bits = U.key_bits_for(index_bounds[1] * 12345 + 12345)
        if kk_groups is None:
            kk_groups = U.group_by(kk, key_bits=kk_bits)
        ix, jx = U.neighbors_csr(jj, kk_groups[1], kk_groups[2], kk_groups[3], E)
        for (la, lb), nb in ((pk["c1"], ix), (pk["c2"], jx)):
            n32, n16, _ = U.rowchain(n16, *la, *lb, flags1=U.RELU, a_idx=nb, flags=U.RES, res32=n32, want32=True)
        ln0, gr1, ln1, gr2 = pk["gru"]
        kk_add = None
        for (pf, pg_, ph), ij, ln in ((pk["agg_kk"], False, None), (pk["agg_ij"], True, ln0)):
            # unique(key) + CSR on the device (no host sync); G stays on the device
            if not ij:
                gid, offs, perm, G = kk_groups
            elif ij_groups is not None:   # (the caller's window key: ii * 12345 + jj is not formed)
                gid, offs, perm, G = ij_groups
            else:
                gid, offs, perm, G = U.group_by(ii * 12345 + jj, key_bits=ij_bits)
            if kk_add is not None and self.FUSE_AGG_ADD:
                # the agg_kk row add formed as the f / g GEMMs stage their A rows
                # (the fp16 rows of net + agg_kk(net) never reach HBM)
                f16, g16 = U.rowgemm_pair_pre(n32, *kk_add, *pf, *pg_)
            else:
                f16, g16 = U.rowgemm_pair(n16, *pf, *pg_)
            # frame-pair groups are few and long (~190 edges at C3): split over waves
            y = U.softagg_csr(f16, g16, offs, perm, G, E, long_groups=ij)
            _, hy, _ = U.rowgemm(y, *ph, M_dev=G)
            if kk_add is None:
                # net + agg_kk(net): only its fp16 rows (agg_ij's GEMM operand) are
                # stored -- or none (FUSE_AGG_ADD); the fp32 sum is recomputed by
                # the next add, in order
                if not self.FUSE_AGG_ADD:
                    _, n16 = U.rowadd_ln(n32, hy, gid, want32=False)
                kk_add = (hy, gid)
            elif self.FUSE_GRU_RES:
                _, n16 = U.rowadd_ln(n32, *kk_add, c16=hy, c_idx=gid, ln=ln, want32=False)
                gru_pre = (n32, kk_add[0], kk_add[1], hy, gid, ln)
            else:
                n32, n16 = U.rowadd_ln(n32, *kk_add, c16=hy, c_idx=gid, ln=ln)
        # gru = LN0 (fused above), GatedResidual, LN1, GatedResidual; then the d / w heads
        for gr, last in ((gr1, False), (gr2, True)):
            pgate, pr1, pr2 = gr
            # the gate Linear + sigmoid runs in the same launch (gate kept on chip)
            if last:
                n32, _, heads = U.rowchain(n16, *pr1, *pr2, flags1=U.RELU, flags=U.GATE | U.HEADS, res32=n32,
                                           gate=pgate, heads=pk["heads"], want32=True, want16=False)
            elif self.FUSE_GRU_RES:
                n32, n16, _ = U.rowchain(n16, *pr1, *pr2, flags1=U.RELU, flags=U.GATE | U.LN, gate=pgate, ln=ln1,
                                         want32=True, pre=gru_pre)
            else:
                n32, n16, _ = U.rowchain(n16, *pr1, *pr2, flags1=U.RELU, flags=U.GATE | U.LN, res32=n32,
                                         gate=pgate, ln=ln1, want32=True)
        return n32[None], (heads[None, :, :2], heads[None, :, 2:], None)

    def forward(self, net, inp, corr, flow, ii, jj, kk, inp_idx=None, index_bounds=None, kk_groups=None,
                ij_groups=None):
        """edge hidden state -> (new state, (delta, weight, None)) (net.py:75-93).

        Optional, not in the reference: inp_idx -- inp is then the un-gathered
        context ring and the rows are inp[:, inp_idx]; index_bounds =
        (num_patches, num_frames) -- kk < num_patches and ii, jj < num_frames,
        which narrows the fused path's radix sorts; kk_groups / ij_groups =
        update_ops.group_by(kk) / group_by(ii * 12345 + jj), when the caller
        already has them."""
        if self._fusable(net, inp, corr) and (inp_idx is None or inp.is_contiguous()):
            return self._forward_fused(net, inp, corr, ii, jj, kk, inp_idx, index_bounds, kk_groups, ij_groups)
        if inp_idx is not None:
            inp = inp[:, inp_idx]
        net = self.norm(net + inp + self.corr(corr))
        ix, jx = fastba.neighbors(kk, jj)  # temporal neighbours of the same patch, on the device
        net = net + self.c1(self._neighbour(net, ix))
        net = net + self.c2(self._neighbour(net, jx))
        net = net + self.agg_kk(net, kk)
        net = net + self.agg_ij(net, ii * 12345 + jj)
        net = self.gru(net)
        return net, (self.d(net), self.w(net), None)


    @staticmethod
    def _neighbour(net, ix):
        """mask_ix * net[:, ix] (net.py:82-85).  Inference: one native gather
        that writes zeros for ix < 0 and casts straight to the autocast dtype
        the following Linear would cast to anyway."""
        if torch.is_grad_enabled() and net.requires_grad:
            return (ix >= 0).to(net.dtype).view(1, -1, 1) * net[:, ix]
        dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else net.dtype
        return update_ops.gather_rows(net[0], ix, dtype=dt)[None]


class Patchifier(nn.Module):
    def __init__(self, patch_size=3):
        super().__init__()
        self.patch_size = patch_size
        self.fnet = BasicEncoder4(output_dim=128, norm_fn="instance")
        self.inet = BasicEncoder4(output_dim=DIM, norm_fn="none")
        # inference ingest from one captured HIP graph (see _forward_graphed);
        # False = the eager launches
        self.graphed = True
        self._graph = self._graph_key = None
        self._native = None
        # after a natively masked forward(): the number of valid mask cells, int32 [1] on the device
        self.last_mask_cells = None

    # fp16-autocast inference runs both encoders on the HIP library
    # (encoder_ops / csrc/encoder.hip); False = the modules' torch forward
    NATIVE_ENCODERS = True
    # beside them, gradient_bias and mask= choose their centres on the device
    # (csrc/select.hip) and take the native / graphed ingest; False = the torch
    # branches of forward()
    NATIVE_SELECT = True

    def _native_encoders(self):
        if self._native is None:
            import encoder_ops
            self._native = encoder_ops.NativeEncoders(self.fnet, self.inet)
        return self._native

    def _use_native(self, amp_dtype, image):
        """the native encoders take uint8 frames (the reference accepts any
        dtype: other frames run the torch encoders)"""
        return (self.NATIVE_ENCODERS and amp_dtype == torch.float16 and not torch.is_grad_enabled() and
                image.dtype == torch.uint8 and self.fnet.norm_fn == "instance" and self.inet.norm_fn == "none")

    def _image_gradient(self, images):
        gray = ((images + 0.5) * (255.0 / 2)).sum(dim=2)
        dx = gray[..., :-1, 1:] - gray[..., :-1, :-1]
        dy = gray[..., 1:, :-1] - gray[..., :-1, :-1]
        return F.avg_pool2d(torch.sqrt(dx ** 2 + dy ** 2), 4, 4)

    def forward(self, images, patches_per_image=80, disps=None, gradient_bias=False, return_color=False, mask=None,
                sp_extractor=None):
        """image [3,H,W] uint8 -> fmap, gmap, imap, patches, index[, colours] (net.py:260-325)."""
        if sp_extractor is not None:
            raise NotImplementedError("SuperPoint keypoints are out of scope")
        self.last_mask_cells = None
        amp = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None
        # gradient_bias wins over the mask, as in the branches below
        mode = "gradient" if gradient_bias else "mask" if mask is not None else "uniform"
        frame_ok = disps is None and images.is_cuda and images.dim() == 3
        # the two selections are native only beside the native encoders; every
        # other input keeps the torch branch below
        mode_ok = mode == "uniform" or (
            self.NATIVE_SELECT and frame_ok and self._use_native(amp, images) and images.shape[0] == 3 and
            (mode == "gradient" or (mask.is_cuda and tuple(mask.shape) == tuple(images.shape[-2:]))))
        if self.graphed and mode_ok and frame_ok and not torch.is_grad_enabled():
            return self._forward_graphed(images, patches_per_image, return_color, mode, mask)
        if self._use_native(amp, images) and mode_ok and frame_ok:
            rnd = self._draw(images, patches_per_image, mode, mask)
            x, y = self._centres(images, patches_per_image, mode, rnd)
            fmap, gmap, imap, patches, clr = self._ingest(images, x, y, return_color, "native")
            index = torch.zeros(patches_per_image, dtype=torch.long, device=images.device)
            return (fmap, gmap, imap, patches, index) + ((clr,) if return_color else ())
        images = 2 * (images[None, None] / 255.0) - 0.5
        fmap = self.fnet(images) / 4.0
        imap = self.inet(images) / 4.0
        b, n, c, h, w = fmap.shape
        dev = images.device

        if gradient_bias:
            g = self._image_gradient(images)
            x = torch.randint(1, w - 1, size=[n, 3 * patches_per_image], device=dev)
            y = torch.randint(1, h - 1, size=[n, 3 * patches_per_image], device=dev)
            score = altcorr.patchify(g[0, :, None], torch.stack([x, y], -1).float(), 0).view(n, -1)
            top = torch.argsort(score, dim=1)[:, -patches_per_image:]
            x, y = torch.gather(x, 1, top), torch.gather(y, 1, top)
        elif mask is not None:
            valid = (torch.nonzero(mask, as_tuple=False) / 4).floor()
            valid = valid[(valid[:, 1] < w - 1) & (valid[:, 0] < h - 1)]
            valid = torch.unique(valid, dim=0)
            pick = valid[torch.randperm(valid.shape[0], device=valid.device)[:n * patches_per_image]]
            x, y = pick[:, 1].view(n, -1), pick[:, 0].view(n, -1)
        else:
            x = torch.randint(1, w - 1, size=[n, patches_per_image], device=dev)
            y = torch.randint(1, h - 1, size=[n, patches_per_image], device=dev)
        gmap, imap, patches, clr = self._gather(images, fmap, imap, x, y, disps, return_color)
        index = torch.arange(n, device=dev).view(n, 1).repeat(1, patches_per_image).reshape(-1)
        if return_color:
            return fmap, gmap, imap, patches, index, clr
        return fmap, gmap, imap, patches, index

    def _gather(self, images, fmap, imap, x, y, disps, return_color, imap_at=None):
        """the four altcorr.patchify gathers at the chosen centres (net.py:301-315).
        imap_at: inet's output already evaluated at the centres (native encoders):
        patchify(imap, coords, 0) at integer centres is that row exactly."""
        b, n, c, h, w = fmap.shape
        P = self.patch_size
        coords = torch.stack([x, y], dim=-1).float()
        if imap_at is not None:
            imap = imap_at.float().view(b, -1, DIM, 1, 1)
        else:
            imap = altcorr.patchify(imap[0], coords, 0).view(b, -1, DIM, 1, 1)
        gmap = altcorr.patchify(fmap[0], coords, P // 2).view(b, -1, 128, P, P)
        clr = altcorr.patchify(images[0], 4 * (coords + 0.5), 0).view(b, -1, 3) if return_color else None
        if disps is None:
            disps = torch.ones(b, n, h, w, device=fmap.device)
        grid, _ = coords_grid_with_index(disps, device=fmap.device)
        patches = altcorr.patchify(grid[0], coords, P // 2).view(b, -1, 3, P, P)
        return gmap, imap, patches, clr

    def _ingest(self, image, x, y, return_color, encoders=None):
        """forward() after the centre draw: fixed shapes, no host syncs -- the
        body of the captured graph.  encoders: (fnet, inet) to run instead of
        the modules' own (the graph's fp16 copies), or "native": both networks
        on the HIP library (encoder_ops, 11 launches), inet only at the centres."""
        if encoders == "native":
            nat = self._native_encoders()
            fmap, imap_at = nat.run(image, x, y)
            if self.patch_size == 3:   # the four gathers in one launch (bit-identical to _gather)
                gm, im, patches, clr = nat.gather(image, fmap, imap_at, x, y, return_color)
            else:
                images = 2 * (image[None, None] / 255.0) - 0.5 if return_color else None
                gm, im, patches, clr = self._gather(images, fmap, None, x, y, None, return_color, imap_at=imap_at)
            return fmap, gm, im, patches, clr
        fnet, inet = encoders or (self.fnet, self.inet)
        images = 2 * (image[None, None] / 255.0) - 0.5
        fmap = fnet(images) / 4.0
        imap = inet(images) / 4.0
        return (fmap,) + self._gather(images, fmap, imap, x, y, None, return_color)

    def _forward_graphed(self, image, M, return_color, mode="uniform", mask=None):
        """forward() with the ~300 encoder / patchify launches replayed from
        one HIP graph.  The random inputs of the centre choice (_draw) are
        drawn eagerly with the same calls, in the same order, as the eager path
        (the encoders draw no random numbers), so the results are identical to
        forward()'s; the graph reads them from static buffers and, in the
        gradient and mask modes, makes the choice itself (_centres).  Outputs
        are returned as clones: the next replay overwrites the graph's own.
        One graph is kept and the mode is part of its key: a stream that
        alternates modes (masked and unmasked frames, say) pays two warm-up
        ingests and a capture at every switch -- a known cost; a graph per
        mode would remove it."""
        dev = image.device
        rnd = self._draw(image, M, mode, mask)
        amp = torch.is_autocast_enabled("cuda")
        # the captured kernels hold raw parameter / buffer addresses and the
        # autocast dtype: any re-placement (.to(), .half(), load_state_dict
        # with assign=True), in-place update or a different autocast dtype re-captures
        tensors = (tuple((t.data_ptr(), t._version) for t in self.parameters()) +
                   tuple(t.data_ptr() for t in self.buffers()))
        # (a change of mode captures again: one graph is kept)
        key = (tuple(image.shape), image.dtype, M, bool(return_color), amp,
               torch.get_autocast_dtype("cuda") if amp else None, dev, tensors, mode)
        if self._graph_key != key:
            self._capture(image, rnd, return_color, amp, key)
        self._g_in[0].copy_(image)
        for buf, r in zip(self._g_in[1], rnd):
            buf.copy_(r)
        self._graph.replay()
        fmap, gmap, imap, patches, clr = (t.clone() if t is not None else None for t in self._g_out)
        if mode == "mask":
            self.last_mask_cells = self._g_cells.clone()
        index = torch.zeros(M, dtype=torch.long, device=dev)
        if return_color:
            return fmap, gmap, imap, patches, index, clr
        return fmap, gmap, imap, patches, index

    @staticmethod
    def _map_size(image):
        H, W = image.shape[-2:]
        return ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2  # conv1 (s2) then layer2 (s2)

    @classmethod
    def _draw_centres(cls, image, M):
        """the default centre draw of forward() (net.py:292-294), on the stride-4 map"""
        h, w = cls._map_size(image)
        x = torch.randint(1, w - 1, size=[1, M], device=image.device)
        y = torch.randint(1, h - 1, size=[1, M], device=image.device)
        return x, y

    def _draw(self, image, M, mode, mask):
        """the random inputs of one frame's centre choice -- everything that
        differs from frame to frame besides the frame; fixed shapes.  uniform:
        the centres themselves; gradient: the 3 M candidates, the same two
        randint calls as the torch branch (net.py:127-128); mask: the mask as
        bytes (nonzero = set, any dtype) and one random key per cell."""
        if mode == "uniform":
            return self._draw_centres(image, M)
        if mode == "gradient":
            return self._draw_centres(image, 3 * M)
        h, w = self._map_size(image)
        keys = torch.randint(0, 2 ** 31 - 1, (h * w,), dtype=torch.int32, device=image.device)
        return mask.ne(0).to(torch.uint8), keys

    def _centres(self, image, M, mode, rnd):
        """the M patch centres from _draw's inputs: launches of fixed shape and
        no host read (csrc/select.hip), so part of the captured graph.  The
        mask mode leaves the number of valid cells, a device word, in
        last_mask_cells: fewer than M means repeated centres, for the caller
        to refuse (DPVO does, where the reference fails at its view())."""
        if mode == "uniform":
            return rnd
        import encoder_ops
        if mode == "gradient":
            x, y = encoder_ops.select_gradient(image, rnd[0], rnd[1], M)
        else:
            x, y, self.last_mask_cells = encoder_ops.select_mask(rnd[0], rnd[1], M, *self._map_size(image))
        return x.view(1, M), y.view(1, M)

    def _capture(self, image, rnd, return_color, amp, key):
        self._graph = self._graph_key = None
        mode, M = key[-1], key[2]
        static = (image.clone(), tuple(r.clone() for r in rnd))

        def body(enc):
            x, y = self._centres(static[0], M, mode, static[1])
            return self._ingest(static[0], x, y, return_color, enc)
        side = torch.cuda.Stream(device=image.device)
        side.wait_stream(torch.cuda.current_stream(image.device))
        dt = key[5] or torch.float16
        # under autocast every convolution casts its fp32 weight and bias to the
        # autocast dtype on each call (the cast cache is off inside a graph):
        # ~50 cast kernels per frame.  The graph runs copies of the encoders
        # already in that dtype -- the same values the casts produce, so the
        # same convolutions (bit-identical to the eager path, test_gpu_tracker)
        enc = None
        if amp and self._use_native(dt, image):
            enc = "native"
        elif amp:
            enc = tuple(copy.deepcopy(m).to(dt) for m in (self.fnet, self.inet))
        with torch.cuda.stream(side), torch.autocast("cuda", dtype=dt, enabled=amp, cache_enabled=False):
            for _ in range(2):  # warm-up: MIOpen solver selection, allocator pools
                body(enc)
        torch.cuda.current_stream(image.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.autocast("cuda", dtype=dt, enabled=amp, cache_enabled=False):
            out = body(enc)
        self._graph, self._graph_key, self._g_in, self._g_out = graph, key, static, out
        self._g_cells = self.last_mask_cells   # (mask mode: the graph's own count word)
        self._g_enc = enc   # the graph holds their parameters' addresses


class VONet(nn.Module):
    def __init__(self, use_viewer=False):
        super().__init__()
        self.P = 3
        self.patchify = Patchifier(self.P)
        self.update = Update(self.P)
        self.DIM = DIM
        self.RES = 4

    def forward(self, *args, **kwargs):
        raise NotImplementedError("VONet training (net.py:355-440) is out of scope for the MI355X hot-path build")
