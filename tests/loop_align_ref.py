"""fp64 numpy restatement of the loop-closure alignment (csrc/align.hip:
RANSAC over 3-point Umeyama models on the caller's samples, the winner rule,
the inlier mask, the refit) and of the keypoint triangulation
(dpvo.loop_closure.triangulate_keypoints), with the fixtures of
test_loop_align_host.py / test_gpu_loop_align.py.

The per-hypothesis model and the refit are the package's numpy
``umeyama_alignment`` (LAPACK SVD); the triangulation is ``oracle.ba_forward``
(structure only) plus ``oracle.transform``.  Test infrastructure only.
"""
import functools

import numpy as np

EARLY_EXIT = 100


# ---------------------------------------------------------------------------
# alignment
# ---------------------------------------------------------------------------
def hypothesis(src, dst, idx):
    """(R, t, s) of one 3-point sample, or None: an index outside [0, N), a
    repeated index, or a degenerate covariance (umeyama_alignment's rule)"""
    from dpvo.loop_closure import umeyama_alignment
    N = len(src)
    idx = [int(v) for v in idx]
    if min(idx) < 0 or max(idx) >= N or len(set(idx)) < 3:
        return None
    R, t, s = umeyama_alignment(src[idx].T, dst[idx].T)
    return None if t is None else (R, t, s)


def residuals(src, dst, model):
    """the reference's expression: |(x @ (s R)^T + t) - y|, sqrt of the sum of squares"""
    R, t, s = model
    moved = src @ (R * s).T + t
    return np.sum((moved - dst) ** 2, axis=1) ** 0.5


def pick_winner(counts, early_exit):
    """the first hypothesis with count > early_exit (early_exit < 0: never),
    else the first with the largest count; -1 when no hypothesis has an inlier"""
    counts = np.asarray(counts)
    if early_exit >= 0:
        above = np.nonzero(counts > early_exit)[0]
        if len(above):
            return int(above[0])
    if len(counts) == 0 or counts.max() < 1:
        return -1
    return int(np.argmax(counts))      # the first maximum


def restate(src, dst, samples, threshold, early_exit=EARLY_EXIT):
    """-> dict(counts [H] (-1: invalid or degenerate), undecided [H] (points
    whose residual is within 1e-9 max(1, threshold) of the threshold), winner,
    mask [N], refit = (R, t, s) or None, info = [code, winner, count, points])"""
    from dpvo.loop_closure import umeyama_alignment
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    H = len(samples)
    counts = np.full(H, -1, np.int64)
    undecided = np.zeros(H, np.int64)
    models = [None] * H
    for h in range(H):
        models[h] = hypothesis(src, dst, samples[h])
        if models[h] is None:
            continue
        r = residuals(src, dst, models[h])
        counts[h] = int((r < threshold).sum())
        undecided[h] = int((np.abs(r - threshold) < 1e-9 * max(1.0, threshold)).sum())
    winner = pick_winner(counts, early_exit)
    out = dict(counts=counts, undecided=undecided, winner=winner, models=models)
    if winner < 0:
        out.update(mask=np.zeros(len(src), bool), refit=None, info=[1, -1, 0, 0])
        return out
    mask = residuals(src, dst, models[winner]) < threshold
    R, t, s = umeyama_alignment(src[mask].T, dst[mask].T)
    refit = None if t is None else (R, t, s)
    out.update(mask=mask, refit=refit, info=[0 if refit else 2, winner, int(counts[winner]), int(mask.sum())])
    return out


def quat_to_matrix(q):
    """[x y z w] -> rotation matrix"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def refit_errors(sim3, refit):
    """(rotation, translation, scale) errors of a device sim3 [t, q, s] against
    (R, t, s): max |R - R'|, |t - t'| / max(1, |t|), |s - s'| / s"""
    R, t, s = refit
    sim3 = np.asarray(sim3, np.float64).reshape(8)
    return (float(np.abs(quat_to_matrix(sim3[3:7]) - R).max()),
            float(np.abs(sim3[:3] - t).max() / max(1.0, np.linalg.norm(t))),
            float(abs(sim3[7] - s) / s))


def random_similarity(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.uniform(-3, 3, 3), float(rng.uniform(0.5, 2.0))


# name -> (N, H, outlier share, noise, threshold): N around the wave (63, 64,
# 65) and below it (3, 4), more than one workgroup of hypotheses (H = 64, 400),
# H = 1; "exit" has several hypotheses above EARLY_EXIT with different counts,
# the cases up to N = 65 have none
CASES = {
    "n3": (3, 1, 0.0, 0.01, 0.5),
    "n4": (4, 4, 0.0, 0.01, 0.5),
    "n63": (63, 4, 0.3, 0.01, 0.1),
    "n64": (64, 64, 0.3, 0.01, 0.1),
    "n65": (65, 64, 0.3, 0.01, 0.1),
    "exit": (200, 64, 0.4, 0.02, 0.06),
    "big": (6000, 400, 0.5, 0.02, 0.5),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(src, dst [N, 3], samples [H, 3] (the sequence numpy's
    ransac_umeyama draws from default_rng(seed + 1)), threshold, truth, bad)"""
    from dpvo.loop_closure import draw_samples
    N, H, share, noise, threshold = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(seed)
    R, t, s = random_similarity(rng)
    src = rng.normal(size=(N, 3)) * 2
    dst = s * src @ R.T + t + noise * rng.normal(size=(N, 3))
    nbad = int(round(share * N))
    bad = rng.choice(N, nbad, replace=False)
    dst[bad] += rng.choice([-1.0, 1.0], (nbad, 3)) * rng.uniform(5, 10, (nbad, 3))   # gross: 5-10 units per axis
    samples = draw_samples(N, H, seed + 1)
    for a in (src, dst, samples):
        a.setflags(write=False)
    return dict(src=src, dst=dst, samples=samples, threshold=threshold, truth=(R, t, s), bad=bad, seed=seed + 1)


@functools.lru_cache(maxsize=None)
def restated(name, early_exit=EARLY_EXIT):
    c = case(name)
    return restate(c["src"], c["dst"], c["samples"], c["threshold"], early_exit)


@functools.lru_cache(maxsize=None)
def crafted():
    """N = 40 points under y = 2 x + 1; the first 10 are the integers k on the
    x axis (their covariance has rank 1 exactly: one non-zero entry), the rest
    a noisy cloud.  Samples: collinear, a repeated index, an index equal to N,
    a negative index, and two valid ones."""
    rng = np.random.default_rng(40)
    N = 40
    src = rng.normal(size=(N, 3)) * 2
    src[:10] = np.outer(np.arange(10.0), [1.0, 0.0, 0.0])
    dst = 2.0 * src + 1.0
    dst[10:] += 0.01 * rng.normal(size=(N - 10, 3))
    samples = np.array([[0, 1, 2], [12, 12, 15], [11, 20, N], [-1, 3, 14], [10, 21, 33], [3, 7, 9], [15, 16, 30]])
    bad = [0, 1, 2, 3, 5]
    for a in (src, dst, samples):
        a.setflags(write=False)
    return dict(src=src, dst=dst, samples=samples, threshold=0.1, bad=bad)


# ---------------------------------------------------------------------------
# triangulation scene
# ---------------------------------------------------------------------------
RES = 4
SCENE_FRAMES = 8      # frames 0-2: the triplet of j = 1; frames 4-6: the triplet of i = 5
SCENE_I, SCENE_J = 5, 1
SCENE_SCALE = 1.2     # the j triplet's baselines (so its triangulated points) are this much too long
DISP0 = 0.2           # inverse depth of the frames' own patches (the triangulation's starting value)


def _quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def _act(pose, X):
    """world-to-camera pose [t, q] on points [n, 3]"""
    return X @ quat_to_matrix(pose[3:]).T + pose[:3]


def _project(pose, intr, X):
    Xc = _act(pose, X)
    return np.stack([intr[0] * Xc[:, 0] / Xc[:, 2] + intr[2], intr[1] * Xc[:, 1] / Xc[:, 2] + intr[3]], 1)


@functools.lru_cache(maxsize=None)
def scene(n):
    """n world points at depth 2-10 in front of two triplets of cameras with a
    0.5 baseline along x (so the epipolar lines are close to horizontal).
    Tracks: exact projections + 0.2 px noise; a tenth of the tracks is shifted
    by 8-12 px in y (across the epipolar line: the depth cannot absorb it) in
    the previous or the next frame.  The poses of the j triplet the patch graph
    holds have their baselines stretched by SCENE_SCALE.

    -> dict(poses [8, 7] fp32 world-to-camera (the patch graph's), intrinsics
    [4] at 1/RES, tracks {frame: (prev, kps, next) [n, 2] fp32}, shifted
    {frame: bool [n]}, depth {frame: true z in camera frame}, far = the true
    Sim3 [t, q, s] from camera i's points to the j triplet's)"""
    rng = np.random.default_rng(1000 + n)
    intr = np.array([80.0, 80.0, 80.0, 60.0])                 # at 1/RES: a 640 x 480 image
    full = intr * RES
    # world points in front of camera SCENE_I (identity)
    z = rng.uniform(2.0, 10.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    true = np.zeros((SCENE_FRAMES, 7))
    true[:, 6] = 1.0
    qj = _quat([0.1, 1.0, 0.05], 0.12)                         # camera j: turned and moved a little
    tj = np.array([0.25, -0.1, 0.3])
    for f in range(SCENE_FRAMES):
        if f <= 3:      # the j side: x_c = R_j (x_w) + t_j - baseline
            true[f, 3:] = qj
            true[f, :3] = tj - np.array([0.5 * (f - SCENE_J), 0.02 * (f - SCENE_J), 0.0])
        else:
            true[f, :3] = -np.array([0.5 * (f - SCENE_I), -0.02 * (f - SCENE_I), 0.0])
    held = true.copy()
    for f in range(0, 4):   # stretch the j side's baselines about frame j
        held[f, :3] = true[SCENE_J, :3] + SCENE_SCALE * (true[f, :3] - true[SCENE_J, :3])
    tracks, shifted, depth = {}, {}, {}
    for f in (SCENE_I, SCENE_J):
        uv = [_project(true[g], full, X) + 0.2 * rng.normal(size=(n, 2)) for g in (f - 1, f, f + 1)]
        sh = np.zeros(n, bool)
        sh[rng.choice(n, n // 10, replace=False)] = True
        which = rng.integers(0, 2, n) * 2                       # frame 0 or 2 of the triplet
        for k in np.nonzero(sh)[0]:
            uv[which[k]][k, 1] += rng.choice([-1.0, 1.0]) * rng.uniform(8.0, 12.0)
        tracks[f] = tuple(u.astype(np.float32) for u in uv)
        shifted[f] = sh
        depth[f] = _act(true[f], X)[:, 2]
    far = np.concatenate([SCENE_SCALE * tj, qj, [SCENE_SCALE]])
    return dict(poses=held.astype(np.float32), intrinsics=intr.astype(np.float32), tracks=tracks, shifted=shifted,
                depth=depth, far=far, n=n)


@functools.lru_cache(maxsize=None)
def triangulate_ref(n, frame, iterations=6, max_residual=2.0):
    """the restatement of triangulate_keypoints on scene(n): oracle.ba_forward
    structure only, oracle.transform, the residual gate, iproj in fp64 ->
    dict(points [n, 3], keep [n], disp [n], worst [n] = the larger residual)"""
    from oracle import oracle
    sc = scene(n)
    prev, kps, nxt = sc["tracks"][frame]
    poses = sc["poses"][frame - 1:frame + 2]
    intr = np.tile(sc["intrinsics"] * RES, (3, 1)).astype(np.float32)
    patches = np.concatenate([kps, np.full((n, 1), DISP0, np.float32)], 1)[:, :, None, None].repeat(3, 2).repeat(3, 3)
    target = np.concatenate([prev, nxt])
    weight = np.ones_like(target)
    kk = np.tile(np.arange(n), 2)
    ii = np.ones(2 * n, np.int64)
    jj = np.concatenate([np.zeros(n, np.int64), np.full(n, 2, np.int64)])
    _, pat, st = oracle.ba_forward(poses, patches, intr, target, weight, 1e-3, ii, jj, kk, 3, 3, iterations)
    assert st == 0
    coords = oracle.transform(poses, pat, intr, ii, jj, kk)[0, :, 1, 1]
    worst = np.linalg.norm(coords - target, axis=-1).reshape(2, n).max(0)
    disp = pat[:, 2, 1, 1].astype(np.float64)
    f = intr[1].astype(np.float64)
    pts = np.stack([(kps[:, 0] - f[2]) / f[0], (kps[:, 1] - f[3]) / f[1], np.ones(n)], 1) / disp[:, None]
    return dict(points=pts, keep=worst < max_residual, disp=disp, worst=worst)


def tracks_far_ref(n, iterations=400, threshold=0.5, seed=5):
    """the restatement of close_loop_from_tracks' far_rel_pose on scene(n),
    every keypoint of frame i matched to the same keypoint of frame j ->
    (R, t, s, inliers)"""
    from dpvo.loop_closure import ransac_umeyama
    a, b = triangulate_ref(n, SCENE_I), triangulate_ref(n, SCENE_J)
    both = a["keep"] & b["keep"]
    return ransac_umeyama(a["points"][both], b["points"][both], iterations=iterations, threshold=threshold, rng=seed)


def far_error(model, far):
    """max over |R - R'|, |t - t'|, |s - s'| of (R, t, s) against Sim3 data [t, q, s]"""
    R, t, s = model
    far = np.asarray(far, np.float64)
    return float(max(np.abs(R - quat_to_matrix(far[3:7])).max(), np.abs(t - far[:3]).max(), abs(s - far[7])))


def make_patch_graph(n, M=4):
    """a PatchGraph on the GPU holding scene(n): 8 frames, every patch at inverse depth DISP0"""
    from types import SimpleNamespace

    import torch
    from dpvo.patchgraph import PatchGraph
    sc = scene(n)
    pg = PatchGraph(SimpleNamespace(BUFFER_SIZE=16), 3, 384, 36, M, 120, 160, RES, device="cuda")
    nf = SCENE_FRAMES
    g = torch.Generator().manual_seed(0)
    pg.n, pg.m = nf, nf * M
    pg.poses_[:nf] = torch.from_numpy(sc["poses"]).cuda()
    pg.patches_[:nf, :, :2] = (torch.rand(nf, M, 2, 3, 3, generator=g) * 100).cuda()
    pg.patches_[:nf, :, 2] = DISP0
    pg.intrinsics_[:nf] = torch.from_numpy(sc["intrinsics"]).cuda()
    pg.index_[:nf] = torch.arange(nf, device="cuda")[:, None]
    pg.tstamps_[:nf] = np.arange(nf)
    return pg
