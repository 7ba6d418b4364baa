"""Generate tests/golden/retrieval_ref.npz: the loop-detection state machine
pinned to the reference's own code.

Runs ONLY in the build container, on the CPU, where the read-only reference
checkout is mounted at /root/reference.  The reference's RetrievalNetVLAD
(dpvo/loop_closure/retrieval/retrieval_netvlad.py, loaded by file path: it
imports torch, numpy and einops only) is driven with a stub database whose
query_online restates dpvo/netvlad_retrieval.py:89-104 (hloc, which that
module imports, is absent).  The fixture is data: the descriptors, the event
script and what the reference returned and held after every detect_loop.

Script: 150 frames, D = 64, unit rows; frames t >= 100 are noisy copies of
t - 95 (a revisit); a few keyframe(k) drops among the pending frames; every
frame save_up_to(n - 24) and detect_loop(0.5, 3), confirm_loop + found.clear()
on a detection; a final flush.

Usage:  python tests/golden/make_golden_retrieval.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/dpvo/loop_closure/retrieval/retrieval_netvlad.py"

T, D, REVISIT, LAG = 150, 64, 100, 95
PENDING, THRESH, REPEAT = 24, 0.5, 3
# frame -> the keyframe dropped after it was added, counted back from the newest (all pending)
DROPS = {12: 3, 40: 4, 41: 4, 77: 2, 109: 3, 131: 5}
OP_CALL, OP_KEYFRAME, OP_SAVE, OP_DETECT, OP_CONFIRM = range(5)


class StubDB:
    """nvlad_db[tstamp] and the online table of RetrievalNetVLADOffline"""

    def __init__(self, desc):
        self.nvlad_db = desc
        self.netvlad_db_online = torch.zeros_like(desc)

    def insert_desc(self, idx, desc):
        self.netvlad_db_online[idx] = desc

    def query_online(self, idx, skip_window=-1, top_k=10):   # netvlad_retrieval.py:89-104
        query_desc = self.netvlad_db_online[idx].detach().clone()
        if idx <= skip_window:
            return None, None
        if skip_window < 0:
            skip_window = idx
        db_descs = self.netvlad_db_online[0:idx - skip_window].detach().clone()
        sim = torch.matmul(db_descs, query_desc.unsqueeze(0).T)
        return torch.topk(sim, min(len(sim), top_k), dim=0)


def descriptors():
    rng = np.random.default_rng(20240)
    x = rng.normal(size=(T, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    for t in range(REVISIT, T):
        x[t] = x[t - LAG] + 0.04 * rng.normal(size=D)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def ragged(lists):
    flat = np.array([p for l in lists for p in l], np.int64).reshape(-1, 2)
    return flat, np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)


def main():
    spec = importlib.util.spec_from_file_location("ref_retrieval_netvlad", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    desc = descriptors()
    r = ref.RetrievalNetVLAD(StubDB(torch.from_numpy(desc)))
    image = np.zeros((2, 2, 3), np.uint8)
    events, returns, found, prev = [], [], [], []

    def detect():
        x = r.detect_loop(THRESH, REPEAT)
        events.append((OP_DETECT, 0, 0))
        returns.append(x if x is not None else (-1, -1))
        if x is not None:
            r.confirm_loop(*x)
            r.found.clear()
            events.append((OP_CONFIRM, x[0], x[1]))
        found.append([(int(a), int(b)) for a, b in r.found])
        prev.append([(int(a), int(b)) for a, b in r.prev_loop_closes])
        return x

    n = 0
    try:
        for t in range(T):
            r(image, n, t)
            events.append((OP_CALL, n, t))
            n += 1
            if t in DROPS:
                k = n - DROPS[t]
                r.keyframe(k)
                events.append((OP_KEYFRAME, k, 0))
                n -= 1
            r.save_up_to(n - PENDING)
            events.append((OP_SAVE, n - PENDING, 0))
            detect()
        r.save_up_to(n - 1)
        events.append((OP_SAVE, n - 1, 0))
        while detect() is not None:
            pass
    finally:
        r.close()
    returns = np.array(returns, np.int64)
    assert (returns[:, 0] >= 0).sum() >= 2, "the script must detect the revisit more than once"
    found_flat, found_off = ragged(found)
    prev_flat, prev_off = ragged(prev)
    np.savez_compressed(os.path.join(HERE, "retrieval_ref.npz"), desc=desc, events=np.array(events, np.int64),
                        returns=returns, found=found_flat, found_off=found_off, prev=prev_flat, prev_off=prev_off,
                        skip_window=np.int64(ref.SKIP_WINDOW), nms=np.int64(ref.NMS), thresh=np.float64(THRESH),
                        repeat=np.int64(REPEAT))
    print(f"{len(events)} events, detections: {returns[returns[:, 0] >= 0].tolist()}, final n = {n}")


if __name__ == "__main__":
    main()
