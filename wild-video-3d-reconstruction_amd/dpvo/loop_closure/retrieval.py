"""Loop-closure retrieval and the keyframe image cache (reference
dpvo/loop_closure/retrieval/), device-resident.

Retrieval keeps the keyframes' global descriptors in one [capacity, D] device
buffer indexed by the current keyframe index and searches it with
cuda_ba.retrieval_query (csrc/retrieval.hip): no subprocess, no queues between
processes, one kernel call and one device->host copy per save_up_to().  The
loop-detection rules (score threshold, NMS against confirmed loops, num_repeat
consecutive retrievals) are the reference's, on the host.

ImageCache keeps the keyframes' images in one [capacity, 3, ht, wd] uint8
device buffer: no JPEG, no disk.
"""
from collections import deque

import numpy as np
import torch

import cuda_ba

from .. import projective_ops as pops

NMS = 50           # keyframe distance below which a retrieved pair repeats a confirmed loop
SKIP_WINDOW = 50   # the newest keyframes a query does not search


class Retrieval:
    """RetrievalNetVLAD without the subprocess.

    nvlad_db: the precomputed descriptors by frame counter -- an object with
    .nvlad_db (a [T, D] tensor or anything indexable by the counter), or the
    [T, D] tensor itself, on either device.

    Rows below `stored` are final (searchable); the rows stored .. count - 1
    are pending: a dropped keyframe renumbers them (keyframe(k))."""

    def __init__(self, nvlad_db, capacity, device, skip_window=SKIP_WINDOW, nms=NMS):
        self.device = torch.device(device)
        self.capacity, self.skip_window, self.nms = int(capacity), int(skip_window), int(nms)
        src = getattr(nvlad_db, "nvlad_db", nvlad_db)
        if torch.is_tensor(src):
            if src.dim() != 2:
                raise RuntimeError("Retrieval: the descriptor table must be [T, D]")
            src = src.to(device=self.device, dtype=torch.float32)
        self.source = src
        self.db = None        # [capacity, D] fp32, allocated with the first descriptor
        self.stored = 0
        self.count = 0
        self.prev_loop_closes = []
        self.found = []
        self.results = deque()   # (n, score, j) in ascending n, j None without candidates

    def __call__(self, image, n, tstamp):
        """descriptor of frame counter tstamp -> row n (image: unused, the reference's signature)"""
        n = int(n)
        desc = torch.as_tensor(self.source[tstamp]).to(device=self.device, dtype=torch.float32).reshape(-1)
        if self.db is None:
            if desc.numel() % 4:
                raise RuntimeError(f"Retrieval: the descriptor length {desc.numel()} must be a multiple of 4")
            self.db = torch.zeros(self.capacity, desc.numel(), dtype=torch.float32, device=self.device)
        if not self.stored <= n <= self.count or n >= self.capacity:
            raise RuntimeError(f"Retrieval: row {n} is not pending (final below {self.stored}, {self.count} written, "
                               f"capacity {self.capacity})")
        self.db[n] = desc
        self.count = max(self.count, n + 1)

    def keyframe(self, k):
        """keyframe k was dropped: the pending rows above it move down by one"""
        k = int(k)
        if k >= self.count:
            return
        if k < self.stored:
            raise RuntimeError(f"Retrieval: keyframe {k} is final already (rows below {self.stored} are)")
        if k + 1 < self.count:
            self.db[k:self.count - 1] = self.db[k + 1:self.count].clone()
        self.count -= 1

    def save_up_to(self, c):
        """rows stored .. c become final; all of them are queried in one call"""
        hi = min(int(c), self.count - 1)
        if hi < self.stored:
            return
        rows = list(range(self.stored, hi + 1))
        val, idx = cuda_ba.retrieval_query(self.db[:hi + 1], rows, self.skip_window, top_k=1)
        pairs = torch.cat((val.double(), idx.double()), dim=1).cpu().tolist()   # fp32 and row indices: exact in fp64
        for n, (score, j) in zip(rows, pairs):
            j = int(j)
            self.results.append((n, float(score), j) if j >= 0 else (n, 0.0, None))
        self.stored = hi + 1

    @property
    def being_processed(self):
        return len(self.results)

    def confirm_loop(self, i, j):
        """record the closed loop, so that later retrievals near it are dropped"""
        assert i > j
        self.prev_loop_closes.append((i, j))

    def _repetition_check(self, idx, num_repeat):
        """(i, j) of the middle of the last num_repeat retrievals when they are consecutive frames"""
        if len(self.found) < num_repeat:
            return None
        latest = self.found[-num_repeat:]
        b = latest[0][0]
        i, j = latest[num_repeat // 2]
        if (1 + idx - b) == num_repeat:
            return (i, max(j, 1))   # max(j, 1): the triplet is centred on j
        return None

    def detect_loop(self, thresh, num_repeat=1):
        """consume queued retrievals until one completes a detection"""
        while self.results:
            x = self._detect_loop(thresh, num_repeat)
            if x is not None:
                return x
        return None

    def _detect_loop(self, thresh, num_repeat=1):
        i, score, j = self.results.popleft()
        if score < thresh:
            return None
        assert i > j
        dists_sq = [(np.square(i - a) + np.square(j - b)) for a, b in self.prev_loop_closes]
        if min(dists_sq, default=np.inf) < np.square(self.nms):
            return None
        self.found.append((i, j))
        return self._repetition_check(i, num_repeat)

    def close(self):
        self.results.clear()


class ImageCache:
    """the keyframes' images on the device: capacity x 3 x ht x wd bytes"""

    def __init__(self, capacity, ht, wd, device):
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.buffer = torch.zeros(self.capacity, 3, int(ht), int(wd), dtype=torch.uint8, device=self.device)
        self.stored = 0
        self.count = 0

    def __call__(self, image, n):
        n = int(n)
        image = torch.as_tensor(image)
        if image.dtype != torch.uint8 or image.shape != self.buffer.shape[1:]:
            raise RuntimeError(f"ImageCache: need a uint8 image {tuple(self.buffer.shape[1:])}, got {image.dtype} "
                               f"{tuple(image.shape)}")
        if not self.stored <= n <= self.count or n >= self.capacity:
            raise RuntimeError(f"ImageCache: slot {n} is not pending (final below {self.stored}, {self.count} "
                               f"written, capacity {self.capacity})")
        self.buffer[n] = image.to(self.device)
        self.count = max(self.count, n + 1)

    def keyframe(self, k):
        """keyframe k was dropped: the pending slots above it move down by one"""
        k = int(k)
        if k >= self.count:
            return
        if k < self.stored:
            raise RuntimeError(f"ImageCache: keyframe {k} is final already (slots below {self.stored} are)")
        pops.frame_shift([(self.buffer, 0, 0)], k, self.count)
        self.count -= 1

    def save_up_to(self, c):
        self.stored = max(self.stored, min(int(c) + 1, self.count))

    def load_frames(self, idxs, device=None):
        idxs = [int(i) for i in idxs]
        if any(i < 0 or i >= self.stored for i in idxs):
            raise RuntimeError(f"ImageCache: frames {idxs} are not all final (slots below {self.stored} are)")
        out = self.buffer[torch.tensor(idxs, dtype=torch.long).to(self.device)]
        return out if device is None else out.to(device)

    def close(self):
        pass
