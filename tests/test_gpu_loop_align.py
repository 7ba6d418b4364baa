"""Loop-closure alignment and triangulation on the GPU (csrc/align.hip through
cuda_ba.ransac_sim3 / umeyama, dpvo.loop_closure.ransac_umeyama_gpu /
triangulate_keypoints, PatchGraph.close_loop_from_points / _from_tracks)
against the fp64 numpy restatement of tests/loop_align_ref.py.  The fixtures'
conditions (no residual within 1e-9 of the threshold, well-conditioned
inliers, an unambiguous residual gate) are checked in test_loop_align_host.py;
they are what lets the counts, winners and masks be compared exactly."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loop_align_ref as L

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the fixtures are read-only


def _bits(outs):
    return [o.contiguous().view(torch.uint8).cpu() for o in outs]


def _run(c, early_exit=L.EARLY_EXIT, samples=None):
    import cuda_ba
    samples = c["samples"] if samples is None else samples
    return cuda_ba.ransac_sim3(T(c["src"]), T(c["dst"]), T(samples), c["threshold"], early_exit=early_exit)


# ---------------------------------------------------------------------------
# alignment against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("early_exit", [L.EARLY_EXIT, -1])
@pytest.mark.parametrize("name", sorted(L.CASES))
def test_ransac_matches_the_restatement(name, early_exit, poisoned):
    """counts of every hypothesis, the winner and the mask equal the
    restatement's exactly; the refit is within 1e-9 of numpy's umeyama_alignment
    on the same mask (rotation matrices, t relative to max(1, |t|), s relative
    to s) -- the bar test_pgo_host.py holds that numpy function to.  Measured:
    profiles/loop_align/NOTES.md."""
    c, r = L.case(name), L.restated(name, early_exit)
    sim3, counts, mask, info = _run(c, early_exit)
    assert sim3.dtype == torch.float64 and counts.dtype == torch.int32 and mask.dtype == torch.bool
    assert sim3.is_cuda and counts.is_cuda and mask.is_cuda and info.is_cuda
    assert np.array_equal(counts.cpu().numpy(), r["counts"])
    assert info.tolist() == r["info"]
    assert np.array_equal(mask.cpu().numpy(), r["mask"])
    errs = L.refit_errors(sim3.cpu().numpy(), r["refit"])
    print(name, early_exit, "winner", r["winner"], "count", r["info"][2], "refit errors (R, t, s)", errs)
    assert max(errs) <= 1e-9


def test_fp32_and_int64_inputs_are_converted(poisoned):
    import cuda_ba
    c = L.case("n65")
    src, dst = c["src"].astype(np.float32), c["dst"].astype(np.float32)
    r = L.restate(src.astype(np.float64), dst.astype(np.float64), c["samples"], c["threshold"])
    assert r["undecided"].sum() == 0
    sim3, counts, mask, info = cuda_ba.ransac_sim3(T(src), T(dst), T(c["samples"].astype(np.int64)), c["threshold"])
    assert np.array_equal(counts.cpu().numpy(), r["counts"]) and info.tolist() == r["info"]
    assert max(L.refit_errors(sim3.cpu().numpy(), r["refit"])) <= 1e-9


def test_crafted_samples(poisoned):
    """-1 exactly for the collinear triple (its covariance has rank 1
    exactly), a repeated index, an index equal to N and a negative one; code
    1 when no sample is valid"""
    c = L.crafted()
    r = L.restate(c["src"], c["dst"], c["samples"], c["threshold"])
    sim3, counts, mask, info = _run(c)
    assert np.array_equal(counts.cpu().numpy(), r["counts"])
    assert [h for h, k in enumerate(counts.tolist()) if k == -1] == c["bad"]
    assert info.tolist() == r["info"] and np.array_equal(mask.cpu().numpy(), r["mask"])
    assert max(L.refit_errors(sim3.cpu().numpy(), r["refit"])) <= 1e-9
    sim3, counts, mask, info = _run(c, samples=c["samples"][c["bad"]])
    assert counts.tolist() == [-1] * len(c["bad"])
    assert info.tolist() == [1, -1, 0, 0]
    assert torch.isnan(sim3).all() and not mask.any()


def test_ransac_umeyama_gpu_is_the_numpy_function(poisoned):
    """the same Generator: the same inlier count and transformation as the numpy ransac_umeyama"""
    from dpvo.loop_closure import ransac_umeyama, ransac_umeyama_gpu
    for name in ("n64", "exit"):
        c = L.case(name)
        H = len(c["samples"])
        R, t, s, inliers = ransac_umeyama(c["src"], c["dst"], iterations=H, threshold=c["threshold"], rng=c["seed"])
        sim3, got = ransac_umeyama_gpu(T(c["src"]), T(c["dst"]), iterations=H, threshold=c["threshold"], rng=c["seed"])
        assert got == inliers and sim3.shape == (1, 8) and sim3.dtype == torch.float64 and sim3.is_cuda
        assert max(L.refit_errors(sim3.cpu().numpy(), (R, t, s))) <= 1e-9
    c = L.crafted()
    assert ransac_umeyama_gpu(T(c["src"][:10]), T(c["dst"][:10]), iterations=5, threshold=0.1, rng=0) == (None, 0)


# ---------------------------------------------------------------------------
# the refit on its own
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n3", "n65", "big"])
def test_umeyama_with_and_without_a_mask(name, poisoned):
    import cuda_ba
    from dpvo.loop_closure import umeyama_alignment
    c = L.case(name)
    src, dst = c["src"], c["dst"]
    sim3, info = cuda_ba.umeyama(T(src), T(dst))
    errs = L.refit_errors(sim3.cpu().numpy(), umeyama_alignment(src.T, dst.T))
    print(name, "all points: errors", errs)
    assert info.tolist() == [0, -1, 0, len(src)] and max(errs) <= 1e-9
    if len(src) > 3:
        keep = np.ones(len(src), bool)
        keep[c["bad"]] = False
        keep[::7] = False
        for m in (T(keep), T(keep.astype(np.uint8))):
            sim3, info = cuda_ba.umeyama(T(src), T(dst), m)
            errs = L.refit_errors(sim3.cpu().numpy(), umeyama_alignment(src[keep].T, dst[keep].T))
            assert info.tolist() == [0, -1, 0, int(keep.sum())] and max(errs) <= 1e-9
        print(name, "masked: errors", errs)


def test_rank_deficient_cloud_is_code_2(poisoned):
    import cuda_ba
    c = L.crafted()
    sim3, info = cuda_ba.umeyama(T(c["src"][:10]), T(c["dst"][:10]))
    assert info.tolist() == [2, -1, 0, 10] and torch.isnan(sim3).all()
    line = np.zeros(len(c["src"]), bool)
    line[:10] = True
    sim3, info = cuda_ba.umeyama(T(c["src"]), T(c["dst"]), T(line))
    assert info.tolist() == [2, -1, 0, 10] and torch.isnan(sim3).all()
    sim3, info = cuda_ba.umeyama(T(c["src"]), T(c["dst"]), T(np.zeros(len(c["src"]), bool)))
    assert info.tolist() == [2, -1, 0, 0] and torch.isnan(sim3).all()


# ---------------------------------------------------------------------------
# repeatability and refusals
# ---------------------------------------------------------------------------
def test_bitwise_repeatable_under_two_poison_bytes(poisoned):
    import _dpvo_hot as H
    import cuda_ba
    for c in (L.case("big"), L.crafted()):
        a = _bits(_run(c))
        b = _bits(_run(c))
        ua = _bits(cuda_ba.umeyama(T(c["src"]), T(c["dst"])))
        H.set_poison(0x00)
        z = _bits(_run(c))
        uz = _bits(cuda_ba.umeyama(T(c["src"]), T(c["dst"])))
        H.set_poison(0xFF)
        for x, y in zip(a + a + ua, b + z + uz):
            assert torch.equal(x, y)


def test_refusals(poisoned):
    import _dpvo_hot as H
    import cuda_ba
    c = L.case("n4")
    src, dst, smp = T(c["src"]), T(c["dst"]), T(c["samples"])
    with pytest.raises(RuntimeError, match="3 <= N"):
        cuda_ba.ransac_sim3(src[:2], dst[:2], smp, 0.5)
    with pytest.raises(RuntimeError, match="3 <= N"):
        cuda_ba.umeyama(src[:2], dst[:2])
    with pytest.raises(RuntimeError, match="1 <= H"):
        cuda_ba.ransac_sim3(src, dst, smp[:0], 0.5)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="threshold must be finite and > 0"):
            cuda_ba.ransac_sim3(src, dst, smp, bad)
    with pytest.raises(RuntimeError, match=r"\[N, 3\]"):
        cuda_ba.ransac_sim3(src, dst[:3], smp, 0.5)
    with pytest.raises(RuntimeError, match="integer tensor"):
        cuda_ba.ransac_sim3(src, dst, smp.double(), 0.5)
    with pytest.raises(RuntimeError, match="mask must be"):
        cuda_ba.umeyama(src, dst, torch.ones(3, dtype=torch.bool, device="cuda"))
    # null pointers and a short workspace, at the C ABI
    lib = H.lib()
    N, nh = 4, 4
    s32 = smp.int()
    sim3 = torch.zeros(8, dtype=torch.float64, device="cuda")
    counts = torch.zeros(nh, dtype=torch.int32, device="cuda")
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    nbytes = lib.dpvo_sim3_workspace_bytes(N, nh)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    good = [H.ptr(src), H.ptr(dst), N, H.ptr(s32), nh, 0.5, 100, H.ptr(sim3), H.ptr(counts), H.ptr(mask), H.ptr(info),
            H.ptr(ws), nbytes, H.stream_of(src)]
    null = ctypes.c_void_p(0)
    for slot, msg in ((0, "src / dst / samples missing"), (3, "src / dst / samples missing"), (7, "outputs missing"),
                      (9, "outputs missing"), (11, "workspace too small"), (12, "workspace too small")):
        args = list(good)
        args[slot] = nbytes - 1 if slot == 12 else null
        assert lib.dpvo_sim3_ransac(*args) != 0
        assert msg in lib.dpvo_hot_last_error().decode()
    ugood = [H.ptr(src), H.ptr(dst), N, null, H.ptr(sim3), H.ptr(info), H.ptr(ws), nbytes, H.stream_of(src)]
    for slot, msg in ((1, "src / dst missing"), (5, "outputs missing"), (6, "workspace too small"),
                      (7, "workspace too small")):
        args = list(ugood)
        args[slot] = 0 if slot == 7 else null
        assert lib.dpvo_sim3_umeyama(*args) != 0
        assert msg in lib.dpvo_hot_last_error().decode()
    assert lib.dpvo_sim3_ransac(*good) == 0 and lib.dpvo_sim3_umeyama(*ugood) == 0   # the unmodified calls pass
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# triangulation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 300])
def test_triangulation_matches_the_oracle(n, poisoned):
    """keep equal to the restatement's; inverse depths and points of the kept
    keypoints within 1e-3 relative of the oracle's structure-only run (the
    bar DESIGN section 4 gives fastba against ba.py)"""
    from dpvo.loop_closure import triangulate_keypoints
    pg, sc = L.make_patch_graph(n), L.scene(n)
    before = (pg.poses_.clone(), pg.patches_.clone())
    for frame in (L.SCENE_I, L.SCENE_J):
        ref = L.triangulate_ref(n, frame)
        points, keep = triangulate_keypoints(pg, frame, *(T(k) for k in sc["tracks"][frame]))
        assert points.shape == (n, 3) and keep.shape == (n,) and keep.dtype == torch.bool and points.is_cuda
        keep, points = keep.cpu().numpy(), points.double().cpu().numpy()
        assert np.array_equal(keep, ref["keep"])
        disp = 1.0 / points[:, 2]
        print(n, frame, "kept", int(keep.sum()), "inverse depth rel err", np.abs(disp / ref["disp"] - 1)[keep].max(),
              "points rel err", (np.abs(points - ref["points"]) / np.abs(ref["points"]).max(1, keepdims=True))[keep].max())
        np.testing.assert_allclose(disp[keep], ref["disp"][keep], rtol=1e-3, atol=0)
        scale = np.linalg.norm(ref["points"][keep], axis=1, keepdims=True)
        assert (np.abs(points[keep] - ref["points"][keep]) <= 1e-3 * scale).all()
    assert torch.equal(pg.poses_, before[0]) and torch.equal(pg.patches_, before[1])   # the patch graph is only read


def test_triangulation_refuses_frames_without_neighbours(poisoned):
    from dpvo.loop_closure import triangulate_keypoints
    pg, sc = L.make_patch_graph(1), L.scene(1)
    tracks = [T(k) for k in sc["tracks"][L.SCENE_I]]
    for frame in (0, -1, L.SCENE_FRAMES - 1, L.SCENE_FRAMES):
        with pytest.raises(RuntimeError, match="needs both neighbours"):
            triangulate_keypoints(pg, frame, *tracks)
    with pytest.raises(RuntimeError, match=r"\[n, 2\]"):
        triangulate_keypoints(pg, 2, tracks[0], tracks[1][:0], tracks[2])


# ---------------------------------------------------------------------------
# public calls
# ---------------------------------------------------------------------------
def _state(pg):
    return dict(poses=pg.poses_.clone(), patches=pg.patches_.clone(), points=pg.points_.clone(),
                delta={t: (t0, dP.data.clone()) for t, (t0, dP) in pg.delta.items()},
                loops=(pg.loop_ii.clone(), pg.loop_jj.clone()))


def _same_state(a, b):
    assert torch.equal(a["poses"], b["poses"]) and torch.equal(a["patches"], b["patches"])
    assert torch.equal(a["points"], b["points"])
    assert a["delta"].keys() == b["delta"].keys()
    for t in a["delta"]:
        assert a["delta"][t][0] == b["delta"][t][0] and torch.equal(a["delta"][t][1], b["delta"][t][1])
    assert torch.equal(a["loops"][0], b["loops"][0]) and torch.equal(a["loops"][1], b["loops"][1])


def _loop_points(gt, i, j, N, rng, zmax=15.0, share=0.2):
    """N points in camera i's frame (z in [2, zmax)) and the same points in
    camera j's, from the ground-truth trajectory, with 0.01 of noise and the
    given share of the pairs grossly wrong"""
    import pgo_helpers as P
    Tg = P.sim3_inv(P.se3_to_sim3(gt))
    far = P.sim3_mul(Tg[[j]], P.sim3_inv(Tg[[i]]))[0]           # T_j T_i^-1, scale 1
    z = rng.uniform(2.0, zmax, N)
    x = np.stack([rng.uniform(-0.5, 0.5, N) * z, rng.uniform(-0.5, 0.5, N) * z, z], 1)
    y = far[7] * x @ L.quat_to_matrix(far[3:7]).T + far[:3] + 0.01 * rng.normal(size=(N, 3))
    bad = rng.choice(N, int(share * N), replace=False)
    y[bad, :2] += rng.choice([-1.0, 1.0], (len(bad), 2)) * rng.uniform(5, 10, (len(bad), 2))
    return x, y


def test_close_loop_from_points_is_the_hand_call(poisoned):
    """on the drifted circle of test_gpu_pgo.py: the same safe_i and bit-identical
    poses, patches, deltas and points as close_loop(i, j, far) called by hand
    with ransac_umeyama_gpu's result on the pairs nearer than max_depth"""
    from dpvo.loop_closure import ransac_umeyama_gpu
    from test_gpu_pgo import _patch_graph
    pg, gt, _ = _patch_graph()
    hand, _, _ = _patch_graph()
    i, j = 40, 2
    rng = np.random.default_rng(11)
    x, y = _loop_points(gt, i, j, 240, rng, zmax=24.0)     # about a fifth of the pairs beyond max_depth = 20
    near = (x[:, 2] < 20.0) & (y[:, 2] < 20.0)
    assert 30 < near.sum() < len(x)
    far, inliers = ransac_umeyama_gpu(T(x[near]), T(y[near]), iterations=400, threshold=0.5, rng=3)
    assert inliers >= 30
    want = hand.close_loop(i, j, far)
    before = _state(pg)
    got = pg.close_loop_from_points(i, j, T(x), T(y), rng=3)
    assert got == want == i + 1 and got is not False
    _same_state(_state(pg), _state(hand))
    assert not torch.equal(before["poses"], pg.poses_)
    # fp32 points are accepted as well
    pg32, _, _ = _patch_graph()
    assert pg32.close_loop_from_points(i, j, T(x).float(), T(y).float(), rng=3) == i + 1


def test_close_loop_from_points_gates(poisoned):
    """False, and nothing changed bitwise: 29 surviving pairs; every point
    beyond max_depth; fewer than min_inliers inliers"""
    from test_gpu_pgo import _patch_graph
    pg, gt, _ = _patch_graph()
    i, j = 40, 2
    rng = np.random.default_rng(12)
    x, y = _loop_points(gt, i, j, 60, rng, share=0.0)
    before = _state(pg)
    x29, y29 = x.copy(), y.copy()
    x29[29:45, 2] += 30.0                                   # 16 pairs too deep in frame i,
    y29[45:, 2] += 30.0                                     # 15 in frame j: 29 survive
    assert int(((x29[:, 2] < 20) & (y29[:, 2] < 20)).sum()) == 29
    assert pg.close_loop_from_points(i, j, T(x29), T(y29), rng=0) is False
    _same_state(_state(pg), before)
    x30 = x29.copy()
    x30[29, 2] = x[29, 2]                                   # 30 survive: the gate is at min_inliers
    assert pg.close_loop_from_points(i, j, T(x30), T(y29), rng=0, min_inliers=30) is not False
    pg, gt, _ = _patch_graph()
    before = _state(pg)
    deep = x.copy()
    deep[:, 2] += 20.0
    assert pg.close_loop_from_points(i, j, T(deep), T(y), rng=0) is False
    _same_state(_state(pg), before)
    noise = np.random.default_rng(13).uniform(1.0, 15.0, (60, 3))
    assert pg.close_loop_from_points(i, j, T(x), T(noise), rng=0, threshold=0.05) is False   # inliers < 30
    _same_state(_state(pg), before)


def test_dpvo_methods_flush_and_check_first(poisoned):
    from dpvo.dpvo import DPVO
    calls = []
    pg = SimpleNamespace(close_loop_from_points=lambda *a, **k: calls.append(("points", a, k)) or 7,
                         close_loop_from_tracks=lambda *a, **k: calls.append(("tracks", a, k)) or 8)
    stub = SimpleNamespace(pg=pg, flush_keyframe=lambda: calls.append("flush"), check_ba=lambda: calls.append("check"))
    assert DPVO.close_loop_from_points(stub, 5, 1, "a", "b", rng=2) == 7
    assert calls == ["flush", "check", ("points", (5, 1, "a", "b"), dict(rng=2))]
    del calls[:]
    assert DPVO.close_loop_from_tracks(stub, 5, 1, "ti", "tj", "mi", "mj", threshold=0.3) == 8
    assert calls == ["flush", "check", ("tracks", (5, 1, "ti", "tj", "mi", "mj"), dict(threshold=0.3))]


def test_close_loop_from_tracks_recovers_the_scene_sim3(poisoned):
    """the triangulation scene seen from two frame triplets, every keypoint
    matched to itself: the far_rel_pose handed to close_loop against the
    scene's true Sim3, within 10x the fp64 restatement's own error on the
    scene (the fp32 BA depths sit under it).  Measured:
    profiles/loop_align/NOTES.md."""
    n = 300
    pg, sc = L.make_patch_graph(n), L.scene(n)
    R, t, s, _ = L.tracks_far_ref(n)
    ref_err = L.far_error((R, t, s), sc["far"])
    seen = []
    closer = pg.close_loop
    pg.close_loop = lambda i, j, far: seen.append(far.clone()) or closer(i, j, far)
    match = torch.arange(n, device="cuda")
    tracks = {f: tuple(T(k) for k in sc["tracks"][f]) for f in (L.SCENE_I, L.SCENE_J)}
    got = pg.close_loop_from_tracks(L.SCENE_I, L.SCENE_J, tracks[L.SCENE_I], tracks[L.SCENE_J], match, match, rng=5)
    assert got == L.SCENE_I + 1 and len(seen) == 1
    far = seen[0].cpu().numpy().reshape(8)
    err = L.far_error((L.quat_to_matrix(far[3:7]), far[:3], far[7]), sc["far"])
    print("far_rel_pose error: device", err, "restatement", ref_err)
    assert err <= 10 * ref_err
    assert torch.isfinite(pg.poses_).all() and torch.isfinite(pg.patches_).all()
    assert pg.loop_ii.tolist() == [L.SCENE_I] and pg.loop_jj.tolist() == [L.SCENE_J]
    # matches of rejected keypoints are dropped, the rest mapped onto the compacted clouds:
    # the reversed match list gives the same pairs in the reverse order
    pg2 = L.make_patch_graph(n)
    pts = []
    pg2.close_loop_from_points = lambda i, j, a, b, **k: pts.append((a, b)) or False
    pg2.close_loop_from_tracks(L.SCENE_I, L.SCENE_J, tracks[L.SCENE_I], tracks[L.SCENE_J], match, match)
    pg2.close_loop_from_tracks(L.SCENE_I, L.SCENE_J, tracks[L.SCENE_I], tracks[L.SCENE_J], match.flip(0), match.flip(0))
    both = L.triangulate_ref(n, L.SCENE_I)["keep"] & L.triangulate_ref(n, L.SCENE_J)["keep"]
    assert pts[0][0].shape == (int(both.sum()), 3)
    assert torch.equal(pts[0][0], pts[1][0].flip(0)) and torch.equal(pts[0][1], pts[1][1].flip(0))
