"""The loop closer's front half on the device: Retrieval against the recorded
run of the reference's RetrievalNetVLAD, ImageCache against a list model,
LongTermLoopClosure on the triangulation scene of loop_align_ref, and the
hooks in DPVO."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loop_align_ref as L
import retrieval_ref as R

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("source", ["device tensor", "host tensor", "object"])
def test_retrieval_replays_the_reference_recording(source, poisoned):
    """the same detect_loop returns and found / prev_loop_closes lists as the
    reference recorded, through keyframe drops, on fp32 device scores"""
    from dpvo.loop_closure import Retrieval
    fx = R.load_fixture()
    # no decision of the script is within rounding of the threshold (fp64 scores, the fp32 bound)
    assert R.top1_margin(fx) > 0.05
    desc = torch.from_numpy(fx["desc"])
    db = {"device tensor": desc.cuda(), "host tensor": desc, "object": SimpleNamespace(nvlad_db=list(desc))}[source]
    r = Retrieval(db, 160, "cuda", skip_window=int(fx["skip_window"]), nms=int(fx["nms"]))
    assert R.replay(fx, r, lambda n, t: r(None, n, t)) == 2
    assert r.being_processed == 0 and r.stored == r.count == 144
    # the rows hold the surviving frames' descriptors, in order
    kept = list(range(150))
    for op, a, b in fx["events"].tolist():
        if op == R.OP_KEYFRAME:
            del kept[a]
    assert torch.equal(r.db[:r.count].cpu(), desc[kept])
    r.close()


def test_retrieval_queues_zero_without_candidates_and_refuses_final_rows(poisoned):
    from dpvo.loop_closure import Retrieval
    desc = T(R.unit_rows(12, 8, seed=1))
    r = Retrieval(desc, 12, "cuda", skip_window=3, nms=2)
    for n in range(6):
        r(None, n, n)
    r.save_up_to(4)
    assert [x[0] for x in r.results] == [0, 1, 2, 3, 4]
    assert [x[1:] for x in list(r.results)[:4]] == [(0.0, None)] * 4 and r.results[4][2] == 0
    with pytest.raises(RuntimeError, match="final"):
        r.keyframe(2)
    with pytest.raises(RuntimeError, match="pending"):
        r(None, 3, 3)
    with pytest.raises(RuntimeError, match="pending"):
        r(None, 7, 7)
    assert r.detect_loop(2.0, 3) is None and r.being_processed == 0


def test_image_cache_equals_a_list_model(poisoned):
    from dpvo.loop_closure import ImageCache
    ht, wd = 6, 10
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (3, ht, wd), generator=g, dtype=torch.uint8) for _ in range(12)]
    cache, model = ImageCache(10, ht, wd, "cuda"), []
    for t in range(7):
        cache(images[t].cuda(), len(model))
        model.append(images[t])
    cache.keyframe(3)
    del model[3]
    cache.save_up_to(2)
    cache.keyframe(5)       # the newest
    del model[5]
    cache(images[7], len(model))          # a host image
    model.append(images[7])
    cache(images[8].cuda(), len(model) - 1)   # a frame that was not kept is overwritten
    model[-1] = images[8]
    cache.keyframe(3)
    del model[3]
    with pytest.raises(RuntimeError, match="final"):
        cache.keyframe(1)
    with pytest.raises(RuntimeError, match="not all final"):
        cache.load_frames([2, 3])
    cache.save_up_to(100)
    assert cache.stored == cache.count == len(model) == 5
    got = cache.load_frames([4, 0, 3, 3])
    assert got.shape == (4, 3, ht, wd) and got.dtype == torch.uint8 and got.is_cuda
    assert torch.equal(got.cpu(), torch.stack([model[i] for i in (4, 0, 3, 3)]))
    assert torch.equal(cache.buffer[:5].cpu(), torch.stack(model))
    with pytest.raises(RuntimeError, match="uint8"):
        cache(images[9].float(), 5)


class SceneFrontend:
    """the scene's tracks by frame, every keypoint matched to itself; checks what it is handed"""

    def __init__(self, n, ht, wd):
        self.sc, self.n, self.shape, self.calls = L.scene(n), n, (3, 3, ht, wd), []

    def tracks(self, images, frames):
        assert images.shape == self.shape and images.dtype == torch.uint8 and images.is_cuda
        assert [int(v) for v in images[:, 0, 0, 0].tolist()] == [10 + f for f in frames]
        f = frames[1]
        assert frames == (f - 1, f, f + 1)
        self.calls.append(("tracks", f))
        prev, kps, nxt = (T(k) for k in self.sc["tracks"][f])
        return prev, kps, nxt, f

    def match(self, feats_i, feats_j):
        self.calls.append(("match", feats_i, feats_j))
        m = torch.arange(self.n, device="cuda")
        return m, m


def scene_descriptors():
    """8 unit rows: frames 4, 5, 6 are near copies of 0, 1, 2; 3 and 7 on their own"""
    d = R.unit_rows(8, 64, seed=2).astype(np.float64)
    noise = R.unit_rows(8, 64, seed=3)
    for f in (4, 5, 6):
        d[f] = d[f - 4] + 0.1 * noise[f]
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("per_frame", [False, True])
def test_long_term_loop_closure_closes_the_scene_loop(per_frame, poisoned):
    """frames 4, 5, 6 retrieve 0, 1, 2: close_loop(5, 1) exactly once, and the
    patch graph is bit-identical to close_loop_from_tracks(5, 1, ...) by hand"""
    from dpvo.loop_closure import LongTermLoopClosure
    n, ht, wd = 300, 8, 12
    desc = scene_descriptors()
    ref, bound = R.scores(desc, [4, 5, 6, 7], 2)
    assert np.argmax(ref[:3], axis=1).tolist() == [0, 1, 2]
    assert (ref[:3].max(axis=1) - bound.max() > 0.5).all() and ref[3].max() + bound.max() < 0.5
    cfg = SimpleNamespace(REMOVAL_WINDOW=0, LOOP_RETR_THRESH=0.5, LOOP_CLOSE_WINDOW_SIZE=3)
    pg, by_hand = L.make_patch_graph(n), L.make_patch_graph(n)
    fe = SceneFrontend(n, ht, wd)
    lc = LongTermLoopClosure(cfg, pg, T(desc), fe, ht, wd, skip_window=2, nms=2, rng=5)
    closed = []
    orig = lc.close_loop
    lc.close_loop = lambda i, j, m: closed.append((i, j, m)) or orig(i, j, m)
    image = lambda f: torch.full((3, ht, wd), 10 + f, dtype=torch.uint8, device="cuda")
    results = []
    for f in range(L.SCENE_FRAMES):
        lc(image(f), f, f)
        if per_frame:
            results.append(lc.attempt_loop_closure(f + 1))
            lc.lc_callback()
    assert not any(results) and not closed      # frame 6 is final only at the end (REMOVAL_WINDOW + 2 behind)
    lc.terminate(L.SCENE_FRAMES)
    assert closed == [(L.SCENE_I, L.SCENE_J, L.SCENE_FRAMES)] and lc.lc_count == 1
    assert fe.calls == [("tracks", 5), ("tracks", 1), ("match", 5, 1)]
    assert lc.retrieval.prev_loop_closes == [(5, 1)] and lc.retrieval.found == []

    sc = L.scene(n)
    tracks = {f: tuple(T(k) for k in sc["tracks"][f]) for f in (L.SCENE_I, L.SCENE_J)}
    m = torch.arange(n, device="cuda")
    safe = by_hand.close_loop_from_tracks(L.SCENE_I, L.SCENE_J, tracks[L.SCENE_I], tracks[L.SCENE_J], m, m, rng=5)
    assert safe == L.SCENE_I + 1
    for name in ("poses_", "patches_", "points_", "loop_ii", "loop_jj"):
        a, b = getattr(pg, name), getattr(by_hand, name)
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name

    # a second attempt: nothing is queued, and the pair would fall to the NMS anyway
    before = pg.poses_.clone()
    assert lc.attempt_loop_closure(L.SCENE_FRAMES) is False and len(closed) == 1
    lc.retrieval.results.extend([(4, 0.9, 0), (5, 0.9, 1), (6, 0.9, 2)])
    assert lc.attempt_loop_closure(L.SCENE_FRAMES) is False and len(closed) == 1 and lc.lc_count == 1
    assert lc.retrieval.found == [] and torch.equal(before, pg.poses_)


def test_failed_closure_is_not_confirmed(poisoned):
    from dpvo.loop_closure import LongTermLoopClosure
    cfg = SimpleNamespace(REMOVAL_WINDOW=0, LOOP_RETR_THRESH=0.5, LOOP_CLOSE_WINDOW_SIZE=3)
    pg = L.make_patch_graph(300)
    fe = SimpleNamespace(tracks=None, match=None)
    with pytest.raises(TypeError, match="tracks"):
        LongTermLoopClosure(cfg, pg, T(scene_descriptors()), fe, 8, 12)
    fe = SimpleNamespace(tracks=lambda images, frames: (None, None, None, None), match=lambda a, b: (None, None))
    lc = LongTermLoopClosure(cfg, pg, T(scene_descriptors()), fe, 8, 12, skip_window=2, nms=2)
    lc.close_loop = lambda i, j, m: False
    lc.retrieval.results.extend([(4, 0.9, 0), (5, 0.9, 1), (6, 0.9, 2)])
    assert lc.attempt_loop_closure(8) is False
    assert lc.lc_count == 0 and lc.retrieval.prev_loop_closes == [] and lc.retrieval.found == []


class Recorder:
    """LongTermLoopClosure's calls in order, passed on to the real object"""

    def __init__(self, inner, slam, log):
        self.inner, self.slam, self.log = inner, slam, log
        self.retrieval, self.imcache = inner.retrieval, inner.imcache

    def __call__(self, image, n, tstamp):
        self.log.append(("frame", n, tstamp))
        self.inner(image, n, tstamp)

    def keyframe(self, k):
        self.log.append(("keyframe", k))
        self.inner.keyframe(k)

    def attempt_loop_closure(self, n):
        self.log.append(("attempt", n, getattr(self.slam, "_kf_pending", None) is None, self.slam.n))
        return self.inner.attempt_loop_closure(n)

    def lc_callback(self):
        self.log.append(("callback",))

    def terminate(self, n):
        self.log.append(("terminate", n))
        self.inner.terminate(n)


def test_dpvo_drives_the_loop_closer():
    """cfg.loop_enabled with DEFER_KEYFRAME on a stream that keeps and drops
    keyframes: per frame (frame, [keyframe,] attempt, callback) with the
    keyframe decision applied before the attempt; after terminate() the
    descriptor rows and the cached images are those of the surviving keyframes"""
    from dpvo.config import make_cfg
    from dpvo.dpvo import DPVO
    from dpvo.net import VONet
    from dpvo.synthetic import image_stream
    intr = torch.tensor([320.0, 320.0, 320.0, 240.0], device="cuda")
    frames = list(image_stream(24))
    desc = torch.from_numpy(R.unit_rows(24, 64, seed=4))
    torch.manual_seed(0)
    net = VONet()
    with torch.no_grad():
        net.update.d[1].weight.mul_(40.0)  # random weights: make the motion probe pass
    cfg = make_cfg("fast", BUFFER_SIZE=64, DEFER_KEYFRAME=True, loop_enabled=True)
    fe = SimpleNamespace(tracks=lambda images, frames: None, match=lambda a, b: None)
    log, calls = [], [0]
    with torch.no_grad():
        slam = DPVO(cfg, net, ht=384, wd=512, nvlad_db=desc, loop_frontend=fe)
        assert slam.long_term_lc.retrieval.capacity == slam.pg.N
        slam.long_term_lc = Recorder(slam.long_term_lc, slam, log)
        orig_kf = slam.keyframe

        def keyframe():
            slam.cfg.KEYFRAME_THRESH = float("inf") if calls[0] % 3 == 0 else -1.0
            calls[0] += 1
            orig_kf()
        slam.keyframe = keyframe
        torch.manual_seed(1)
        for t, img in frames:
            mark = len(log)
            slam(t, img, None, None, intr)
            kinds = [e[0] for e in log[mark:]]
            assert kinds[0] == "frame" and log[mark][2] == t
            assert kinds[1:] in ([], ["attempt", "callback"], ["keyframe", "attempt", "callback"]), kinds
            if len(kinds) > 1:
                assert log[-2] == ("attempt", slam.n, True, slam.n)   # the decision is applied, n is current
        n = slam.n
        slam.terminate()
    drops = [e for e in log if e[0] == "keyframe"]
    assert len(drops) == slam.keyframes_dropped > 0 and calls[0] > len(drops)
    assert log[-1] == ("terminate", n)
    r, c = slam.long_term_lc.retrieval, slam.long_term_lc.imcache
    assert r.stored == r.count == c.stored == c.count == n
    stamps = [int(v) for v in slam.pg.tstamps_[:n]]
    assert torch.equal(r.db[:n].cpu(), desc[stamps])
    assert torch.equal(c.buffer[:n], torch.stack([frames[t][1] for t in stamps]))
