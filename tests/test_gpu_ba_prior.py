"""The depth-prior term of the native bundle adjustment (dpvo_ba_forward_prior,
cuda_ba.forward(patches_est=, prior_mu=)) on the GPU.

Parity is against the reference's own Python BA (dpvo/ba.py:151-159, run as
imported code into tests/golden/ba_prior_ref.npz) with the project's bar for
GPU fastba against ba.py: assert_close_rel at rtol 2e-3.  The closed form
(all weights zero: C = mu L, u = -mu L (d - est), so one iteration moves a
patch with a prior to d + mu / (mu + lmbda) (est - d)) is held to 1e-5
relative: a handful of fp32 roundings (6e-8 each) on values of the depth's
magnitude.  Everything else here is bit identity.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from tests_helpers import same

pytestmark = pytest.mark.gpu
LMBDA = 1e-4
PATHS = ["deterministic", "atomic", "sparse"]


def T(a, d="cuda:0"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def assert_close_rel(got, ref, rtol, floor=1e-5):
    """test_gpu_fastba.assert_close_rel: norm-wise per tensor, and per element where |ref| > 1e-3."""
    assert np.linalg.norm(got - ref) <= rtol * max(np.linalg.norm(ref), floor)
    big = np.abs(ref) > 1e-3
    assert np.all(np.abs(got[big] - ref[big]) <= rtol * np.abs(ref[big]) + floor)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "ba_prior_ref.npz")))


def case_of(gold, case):
    return {k[len(case) + 1:]: v for k, v in gold.items() if k.startswith(case + "_")}


def run(c, path="deterministic", est="fixture", mu=2.0, iters=None, csr=False, weight=None, patches=None, edges=None):
    """one cuda_ba.forward on case c -> (poses, patches) as numpy; est: "fixture", None or an array"""
    import cuda_ba
    import update_ops
    p = T(c["poses"])
    q = T(c["patches"] if patches is None else patches)[None]
    ii, jj, kk = (T(x) for x in (edges if edges is not None else (c["ii"], c["jj"], c["kk"])))
    e = c["patches_est"] if isinstance(est, str) else est
    kw = {} if e is None else dict(patches_est=T(e)[None], prior_mu=mu)
    if csr:
        kw["csr"] = update_ops.group_by(kk)[1:]
    old = cuda_ba.DETERMINISTIC, cuda_ba.SPARSE
    cuda_ba.DETERMINISTIC, cuda_ba.SPARSE = path != "atomic", path == "sparse"
    try:
        cuda_ba.forward(p, q, T(c["intrinsics"]), T(c["target"]), T(c["weight"] if weight is None else weight),
                        torch.tensor([LMBDA], device="cuda:0"), ii, jj, kk, int(c["t0"]), int(c["t1"]),
                        int(c["iters"]) if iters is None else iters, **kw)
    finally:
        cuda_ba.DETERMINISTIC, cuda_ba.SPARSE = old
    torch.cuda.synchronize()
    return p.cpu().numpy(), q[0].cpu().numpy()


def bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", ["window", "full", "structure"])
def test_parity_with_the_reference_python_ba(gold, case, path):
    """(the structure-only case has no pose window, so SPARSE = True leaves it
    on the deterministic path, as for the plain call)"""
    c = case_of(gold, case)
    gp, gq = run(c, path)
    print(f"{case}/{path}: poses off by {np.abs(gp - c['poses_out']).max():.3g}, depths by "
          f"{np.abs(gq[:, 2, 1, 1] / c['patches_out'][:, 2, 1, 1] - 1).max():.3g} relative")
    assert_close_rel(gp, c["poses_out"], rtol=2e-3)
    assert_close_rel(gq[:, 2, 1, 1], c["patches_out"][:, 2, 1, 1], rtol=2e-3)
    assert np.array_equal(gq[:, :2], c["patches"][:, :2])          # x, y untouched
    assert np.array_equal(gq[:, 2], np.broadcast_to(gq[:, 2, 1:2, 1:2], gq[:, 2].shape))   # depth written to the 3x3


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", ["window", "full", "structure"])
def test_plain_call_still_matches_the_prior_less_reference(gold, case, path):
    c = case_of(gold, case)
    gp, gq = run(c, path, est=None)
    assert_close_rel(gp, c["poses_out0"], rtol=2e-3)
    assert_close_rel(gq[:, 2, 1, 1], c["patches_out0"][:, 2, 1, 1], rtol=2e-3)


@pytest.mark.parametrize("mu", [2.0, 0.5])
@pytest.mark.parametrize("path", PATHS)
def test_closed_form_with_zero_weights(gold, path, mu):
    c = case_of(gold, "structure")
    # every fifth patch loses its edges: not referenced by kk
    keep = c["kk"] % 5 != 0
    edges = tuple(c[k][keep] for k in ("ii", "jj", "kk"))
    c = dict(c, target=c["target"][:, keep])
    weight = np.zeros_like(c["weight"][:, keep])
    est = c["patches_est"]
    d = c["patches"][:, 2, 1, 1]
    assert np.array_equal(c["patches"][:, 2], np.broadcast_to(d[:, None, None], (len(d), 3, 3)))
    _, gq = run(c, path, est=est, mu=mu, iters=1, weight=weight, edges=edges)
    e = est[:, 2, 1, 1]
    ref = np.zeros(len(d), bool)
    ref[np.unique(edges[2])] = True
    moved = ref & (e > 0)
    assert moved.sum() > 5 and (~ref & (e > 0)).sum() > 0 and (ref & (e == 0)).sum() > 5
    want = d.astype(np.float64) + mu / (mu + LMBDA) * (e.astype(np.float64) - d)
    got = gq[:, 2, 1, 1]
    assert np.all(np.abs(got[moved] - want[moved]) <= 1e-5 * np.abs(want[moved]))
    assert np.array_equal(gq[moved, 2], np.broadcast_to(got[moved, None, None], (moved.sum(), 3, 3)))
    # no prior, or not referenced by kk: the same bits
    assert np.array_equal(gq[~moved].view(np.uint32), c["patches"][~moved].view(np.uint32))
    assert np.array_equal(gq[:, :2], c["patches"][:, :2])


def test_neutral_inputs_equal_the_plain_call_bit_for_bit(gold):
    c = case_of(gold, "window")
    plain = run(c, est=None)
    est = c["patches_est"]
    assert not bits_equal(run(c), plain)                              # the prior does something
    assert bits_equal(run(c, mu=0.0), plain)                          # prior_mu = 0
    assert bits_equal(run(c, est=np.zeros_like(est)), plain)          # no patch has a prior
    # +inf, a negative value or NaN on a subset mean "no prior" there, like 0
    sub = np.flatnonzero(est[:, 2, 1, 1] > 0)[::2]
    zeroed = est.copy()
    zeroed[sub, 2] = 0.0
    want = run(c, est=zeroed)
    assert not bits_equal(want, plain) and not bits_equal(want, run(c))
    for bad in (np.inf, -0.5, np.nan):
        e = est.copy()
        e[sub, 2] = bad
        got = run(c, est=e)
        assert np.isfinite(got[1]).all()
        assert bits_equal(got, want), bad


@pytest.mark.parametrize("case", ["window", "structure"])
def test_repeatable_and_the_callers_csr(gold, case):
    c = case_of(gold, case)
    a = run(c)
    assert bits_equal(run(c), a)
    assert bits_equal(run(c, csr=True), a)


def test_shim_checks_patches_est():
    import cuda_ba
    g = case_of(dict(np.load(os.path.join(GOLDEN, "ba_prior_ref.npz"))), "structure")
    args = lambda: (T(g["poses"]), T(g["patches"])[None], T(g["intrinsics"]), T(g["target"]), T(g["weight"]),
                    torch.tensor([LMBDA], device="cuda:0"), T(g["ii"]), T(g["jj"]), T(g["kk"]), int(g["t0"]),
                    int(g["t1"]), 1)
    est = T(g["patches_est"])[None]
    for bad, msg in ((est.double(), "float32"), (est[:, :, :, :, :2], "contiguous"), (est[:, :-1], "element count"),
                     (est.cpu(), "GPU")):
        with pytest.raises(RuntimeError, match=msg):
            cuda_ba.forward(*args(), patches_est=bad)
    with pytest.raises(RuntimeError, match="prior_mu"):
        cuda_ba.forward(*args(), patches_est=est, prior_mu=-1.0)


# ---------------------------------------------------------------------------
# tracker: cfg.DEPTH_PRIOR_BA
# ---------------------------------------------------------------------------
MAX_FRAMES = 24   # test_gpu_tracker's stream: the warm-up's 10 keyframes arrive well inside it


def depth_map(t, ht=384, wd=512):
    """a smooth metric depth map (2 .. 4 m), drifting with the frame"""
    y, x = torch.meshgrid(torch.arange(ht, device="cuda"), torch.arange(wd, device="cuda"), indexing="ij")
    return 3.0 + torch.sin(x / 60.0 + 0.1 * t) * torch.cos(y / 45.0)


def fed_tracker(**overrides):
    """the frame-by-frame tracker of test_gpu_tracker.py with the prior on, fed
    images and depth maps until it has initialised (10 keyframes, 12 updates)
    and tracked two more frames -> (tracker, intrinsics, frames not yet fed)"""
    from dpvo.config import make_cfg
    from dpvo.dpvo import DPVO
    from dpvo.net import VONet
    from dpvo.synthetic import image_stream
    torch.manual_seed(0)
    net = VONet()
    with torch.no_grad():
        net.update.d[1].weight.mul_(40.0)  # random weights: make the motion probe pass
    cfg = make_cfg("fast", BUFFER_SIZE=64, DEPTH_PRIOR_BA=True, **overrides)
    intr = torch.tensor([320.0, 320.0, 320.0, 240.0], device="cuda")
    slam = DPVO(cfg, net, ht=384, wd=512)
    torch.manual_seed(1)
    stream = image_stream(MAX_FRAMES)
    tracked = 0
    for t, img in stream:
        tracked += slam.is_initialized
        slam(t, img, depth_map(t), None, intr)
        if tracked == 2:
            break
    assert slam.is_initialized and tracked == 2
    return slam, intr, stream


def rows_line_up(slam):
    """every stored patch's prior row is that patch's: same x, y"""
    n = slam.n
    return torch.equal(slam.pg.patches_est_[:n, :, :2], slam.pg.patches_[:n, :, :2])


@torch.no_grad()
def test_tracker_update_is_ba_with_the_prior_and_rows_survive_keyframe_removal():
    import cuda_ba
    slam, intr, stream = fed_tracker()
    cfg = slam.cfg
    assert rows_line_up(slam)
    assert (slam.patches_est[0, :slam.pg.m, 2, 1, 1] > 0).all()
    poses0, patches0 = slam.pg.poses_.clone(), slam.pg.patches_.clone()
    slam.update()
    slam.check_ba()
    # the same BA by hand, from the pre-BA state and update()'s targets / weights
    out = []
    for kw in (dict(patches_est=slam.patches_est, prior_mu=cfg.DEPTH_PRIOR_MU), {}):
        p, q = poses0.clone(), patches0.clone()
        cuda_ba.forward(p.view(1, slam.N, 7), q.view(1, slam.N * slam.M, 3, 3, 3), slam.intrinsics, slam.pg.target,
                        slam.pg.weight, slam._lmbda, slam.pg.ii, slam.pg.jj, slam.pg.kk,
                        max(slam.n - cfg.OPTIMIZATION_WINDOW, 1), slam.n, cfg.BA_ITERATIONS, **kw)
        out.append((p, q))
    same(slam.pg.poses_, out[0][0], "update() vs BA with the prior: poses")
    same(slam.pg.patches_, out[0][1], "update() vs BA with the prior: patches")
    assert not torch.equal(slam.pg.patches_, out[1][1])              # and not the plain BA
    # keyframe removal shifts patches_ and patches_est_ together
    orig_kf, calls = slam.keyframe, [0]

    def keyframe():
        slam.cfg.KEYFRAME_THRESH = float("inf") if calls[0] % 2 == 0 else -1.0
        calls[0] += 1
        orig_kf()
    slam.keyframe = keyframe
    for _ in range(4):
        t, img = next(stream)
        slam(t, img, depth_map(t), None, intr)
    slam.flush_keyframe()
    assert getattr(slam, "keyframes_dropped", 0) > 0
    assert rows_line_up(slam)
    assert torch.isfinite(slam.pg.poses_[:slam.n]).all()


@torch.no_grad()
def test_tracker_graph_replay_equals_eager_with_the_prior():
    a = fed_tracker()[0]
    b = fed_tracker()[0]
    same(a.pg.patches_, b.pg.patches_, "two identically fed trackers")
    for _ in range(3):
        a.update()
        b.update_graphed()
    torch.cuda.synchronize()
    assert b._ugraph is not None
    n, m = a.n, a.pg.m
    for name, x, y in (("poses", a.pg.poses_[:n], b.pg.poses_[:n]), ("patches", a.pg.patches_[:n], b.pg.patches_[:n]),
                       ("net", a.pg.net, b.pg.net), ("points", a.pg.points_[:m], b.pg.points_[:m]),
                       ("target", a.pg.target, b.pg.target), ("weight", a.pg.weight, b.pg.weight)):
        same(x, y, f"eager vs graph replay with the prior: {name}")
    a.check_ba()
    b.check_ba()


@torch.no_grad()
def test_tracker_global_ba_passes_the_prior(monkeypatch):
    """terminate()'s global BA hands BA the tracker's prior buffer and cfg.DEPTH_PRIOR_MU"""
    import dpvo.dpvo as D
    slam = fed_tracker(DEPTH_PRIOR_MU=0.5)[0]
    slam.enable_global_ba, slam.use_distance_edges = True, False
    seen = []
    real = D.fastba.BA

    def spy(*a, **k):
        seen.append(k)
        return real(*a, **k)
    monkeypatch.setattr(D.fastba, "BA", spy)
    d0 = slam.pg.patches_[:slam.n, :, 2, 1, 1].clone()
    slam.global_bundle_adjustment()
    assert len(seen) == 1 and seen[0]["prior_mu"] == 0.5
    assert seen[0]["patches_est"].data_ptr() == slam.pg.patches_est_.data_ptr()
    assert seen[0]["patches_est"].shape == slam.patches.shape
    d1 = slam.pg.patches_[:slam.n, :, 2, 1, 1]
    assert torch.isfinite(d1).all() and not torch.equal(d0, d1)
