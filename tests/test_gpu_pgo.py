"""Native Sim(3) pose-graph optimisation (csrc/pgo.hip through cuda_ba.pgo_residual
/ pgo_step / pgo, dpvo.loop_closure, PatchGraph.close_loop) against the fp64
numpy restatement of tests/pgo_helpers.py: the oracle's lietorch Sim3 for the
group operations, central differences for the Jacobians, oracle.solve_system
for the step.  pypose is not installed: parity with its own Exp / Log is
unpinned."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pgo_helpers as P
from oracle import oracle

pytestmark = pytest.mark.gpu

CASES = sorted(P.RANDOM_CASES)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _random(n, L):
    """the case, the kernel's residuals / Jacobians at its state g, shared by the tests below"""
    import cuda_ba
    poses, loops, ii, jj, g = P.random_case(n, L, seed=n + L)
    dev = cuda_ba.pgo_residual(T(g), T(poses), T(loops), T(ii), T(jj))
    return (poses, loops, ii, jj, g), tuple(x.cpu().numpy() for x in dev)


# ---------------------------------------------------------------------------
# residual and Jacobian
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", CASES)
def test_residual_and_jacobians(n, L):
    """res against the oracle's composition at 1e-9; Ji / Jj against fp64
    central differences of that composition, h = 1e-5: truncation ~ h^2,
    roundoff ~ 1e-11 / h, so rtol = atol = 1e-6.  Rotations up to 3 rad and
    translations up to 10 (a truncated-series Jacobian is off by O(1) there);
    nested loops, a shared endpoint, ii > jj (pgo_helpers.RANDOM_CASES).

    The state g is the initial state plus a perturbation whose scale
    coordinate sigma stays 0.05 away from zero.  At sigma = 0 +- h the
    composition evaluates (e^sigma - 1) / sigma with 11 digits lost, and its
    central differences carry ~5e-6 of noise (measured on the host against
    Richardson extrapolation): they cannot referee 1e-6 there."""
    (poses, loops, ii, jj, g), (res, Ji, Jj, iii, jjj) = _random(n, L)
    want = P.residual(g, poses, loops, ii, jj)
    fi, fj, wi, wj = P.jacobians_fd(g, poses, loops, ii, jj)
    assert res.shape == (n - 1 + L, 7) and Ji.shape == Jj.shape == (n - 1 + L, 7, 7)
    assert np.array_equal(iii, wi) and np.array_equal(jjj, wj)
    print("res err", np.abs(res - want).max(), "Ji err", np.abs(Ji - fi).max(), "Jj err", np.abs(Jj - fj).max())
    np.testing.assert_allclose(res, want, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(Ji, fi, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(Jj, fj, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n,L", CASES)
def test_residual_at_the_initial_state(n, L):
    """g = Log of the inverted input poses (sigma = 0): chain residuals vanish, all match the oracle"""
    import cuda_ba
    poses, loops, ii, jj, _ = _random(n, L)[0]
    g0 = P.initial_state(poses)
    res = cuda_ba.pgo_residual(T(g0), T(poses), T(loops), T(ii), T(jj))[0].cpu().numpy()
    np.testing.assert_allclose(res, P.residual(g0, poses, loops, ii, jj), rtol=1e-9, atol=1e-9)
    assert np.abs(res[:n - 1]).max() < 1e-9


# ---------------------------------------------------------------------------
# one damped step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ep,lm", [(0.0, 1e-6), (1e-4, 1e-3)])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,L", CASES)
def test_step_matches_solve_system(n, L, half, ep, lm):
    """the skyline solve against oracle.solve_system fed the kernel's own fp64
    res / Ji / Jj (the tolerance of test_gpu_solve_system.py: the oracle
    returns float32)"""
    import cuda_ba
    (poses, loops, ii, jj, g), (res, Ji, Jj, iii, jjj) = _random(n, L)
    freen = n // 2 if half else -1
    want = oracle.solve_system(Ji, Jj, iii, jjj, res, ep, lm, freen)
    got = cuda_ba.pgo_step(T(g), T(poses), T(loops), T(ii), T(jj), ep, lm, freen)
    assert got.shape == (n, 7) and got.dtype == torch.float64 and got.is_cuda
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-5)
    if freen >= 0:
        assert (got[freen:] == 0).all()


# ---------------------------------------------------------------------------
# status
# ---------------------------------------------------------------------------
def test_self_edge_and_bad_index_raise():
    import cuda_ba
    poses, loops, ii, jj, g = _random(6, 1)[0]
    for bad_ii, bad_jj, msg in (([3], [3], "ii == jj"), ([6], [1], "outside"), ([2], [-1], "outside")):
        a, b = T(np.array(bad_ii)), T(np.array(bad_jj))
        with pytest.raises(RuntimeError, match=msg):
            cuda_ba.pgo(T(poses), T(loops), a, b)
        with pytest.raises(RuntimeError, match=msg):
            cuda_ba.pgo_step(T(g), T(poses), T(loops), a, b, 0.0, 1e-6, -1)
        with pytest.raises(RuntimeError, match=msg):
            cuda_ba.pgo_residual(T(g), T(poses), T(loops), a, b)


def test_not_positive_definite_raises():
    """a non-positive pivot is reported (here: a negative ep), never clamped"""
    import cuda_ba
    poses, loops, ii, jj, g = _random(6, 1)[0]
    with pytest.raises(RuntimeError, match="not positive-definite"):
        cuda_ba.pgo_step(T(g), T(poses), T(loops), T(ii), T(jj), -1e6, 0.0, -1)


def test_synchronize_refuses_a_loop_on_the_last_pose():
    from dpvo.loop_closure import run_DPVO_PGO_sychronize
    poses, loops, _, _, _ = _random(6, 1)[0]
    with pytest.raises(RuntimeError, match="safe_i|max\\(loop_ii\\)"):
        run_DPVO_PGO_sychronize(T(poses), T(loops), T(np.array([5])), T(np.array([1])))


def test_global_ba_size_fits_64_mb_and_runs():
    """n = 4096, L = 16 (loops spanning ~4000 frames each: the skyline at its
    largest): the workspace is at most 64 MB -- the dense matrix would be
    6.6 GB -- and three iterations return finite values."""
    import cuda_ba
    n, L = 4096, 16
    assert cuda_ba.pgo_workspace_bytes(n, L) <= 64 << 20
    gt = P.circle_gt(n, turns=4.0)
    rng = np.random.default_rng(0)
    poses = gt.copy()
    poses[:, :3] += 1e-3 * rng.normal(size=(n, 3))
    ii, jj = (np.array(x, np.int64) for x in P.CIRCLE_LOOPS[(n, L)])
    loops = P.self_loops(gt, ii, jj)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, hist = cuda_ba.pgo(T(poses), T(loops), T(ii), T(jj), iters=3)
    assert torch.isfinite(out).all() and torch.isfinite(hist).all()
    assert hist[-1] <= hist[0]
    assert torch.cuda.max_memory_allocated() - base <= (64 << 20) + (4 << 20)   # workspace + inputs / outputs


# ---------------------------------------------------------------------------
# identity
# ---------------------------------------------------------------------------
def test_identity_for_consistent_loops():
    """loop constraints read off the input trajectory: output == input, scales == 1"""
    import cuda_ba
    rng = np.random.default_rng(3)
    poses = P.random_poses(30, rng)
    ii, jj = np.array([25, 3, 12]), np.array([2, 20, 13])
    out, hist = cuda_ba.pgo(T(poses), T(P.self_loops(poses, ii, jj)), T(ii), T(jj))
    out, hist = out.cpu().numpy(), hist.cpu().numpy()
    assert hist[0] < 1e-20
    want = P.se3_to_sim3(poses)
    sign = np.sign((out[:, 3:7] * want[:, 3:7]).sum(1, keepdims=True))   # q and -q are one rotation
    out[:, 3:7] *= sign
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-9)
    np.testing.assert_allclose(out[:, 7], 1.0, rtol=0, atol=1e-9)
    # the stop rule ends the run once five costs are in (cost < 1e-5, no progress)
    ran = int(np.isfinite(hist).sum())
    assert 5 <= ran < 30 and np.isnan(hist[ran:]).all()


# ---------------------------------------------------------------------------
# the Levenberg-Marquardt loop
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lm(n, L, iters, small_drift=False):
    """circle case -> device run, fp64 restatement, restatement on the float32 solve"""
    import cuda_ba
    kw = dict(scale_drift=0.002, rot_drift=0.001) if small_drift else {}
    gt, poses, loops, ii, jj = P.circle_case(n, L, P.LM_CASES[(n, L)]["seed"], **kw)
    out, hist = cuda_ba.pgo(T(poses), T(loops), T(ii), T(jj), iters=iters)
    ref = P.lm_restatement(poses, loops, ii, jj, iters=iters)
    r32 = P.lm_restatement(poses, loops, ii, jj, iters=iters, solver="f32")
    return (gt, poses, loops, ii, jj), out.cpu().numpy(), hist.cpu().numpy(), ref, r32


def _accepts(hist, ran):
    # an accepted step lowers the next iteration's cost; a rejected one repeats it bit for bit
    return [bool(hist[t + 1] < hist[t]) for t in range(ran - 1)]


@pytest.mark.parametrize("n,L", sorted(P.LM_CASES))
def test_lm_loop_matches_the_restatement(n, L):
    """Circle ground truth, input with 1 % scale drift per frame and rotation
    drift, loop constraints from the ground truth; iters = the leading steps
    of the restatement whose cost_new / cost_old lies outside [0.99, 1.01]
    (2 and 3: test_pgo_host.py checks it; the next step already has ratio
    0.9993 / 0.9996 and from then on 1 +- 1e-9, where rounding decides accept
    / reject).  Accept / reject sequence and iteration count equal, cost
    history at rtol 1e-6, final Sim3 within 10x the noise floor = the
    difference between the restatement solved in fp64 and with
    oracle.solve_system's float32 delta (measured on the host: floor 9.1e-8
    for (48, 1), 1.2e-6 for (96, 3); a host build of the kernels' code
    differed from the restatement by 5.6e-8 and 5.4e-7)."""
    iters = P.LM_CASES[(n, L)]["iters"]
    _, out, hist, ref, r32 = _lm(n, L, iters)
    ran = int(np.isfinite(hist).sum())
    floor = np.abs(ref["sim3"] - r32["sim3"]).max()
    print("iters", ran, "hist", hist, "ref", ref["hist"], "sim3 diff", np.abs(out - ref["sim3"]).max(), "floor", floor)
    assert ran == len(ref["hist"]) == iters
    np.testing.assert_allclose(hist[:ran], ref["hist"], rtol=1e-6, atol=0)
    assert _accepts(hist, ran) == ref["accepts"][:ran - 1]
    np.testing.assert_allclose(out, ref["sim3"], rtol=0, atol=10 * floor)


@pytest.mark.parametrize("n,L,small_drift", [(48, 1, False), (96, 3, False), (48, 1, True)])
def test_lm_loop_default_iterations_and_alignment(n, L, small_drift):
    """The default 30 iterations.  With 1 % drift per frame the converged cost
    stays above 1e-5 and all 30 run; with 0.2 % (small_drift) the stop rule
    ends the run after 6 (cost_1 / cost_5 = 1.15 < 1.5).  Iteration count
    equal, cost history at rtol 1e-6 (the plateau's accept / reject is decided
    by rounding and is not compared).  The pose graph has no fixed pose, so
    the raw estimate drifts along the gauge on the plateau: the comparison is
    on run_DPVO_PGO_sychronize's aligned output, within 10x the floor measured
    the same way (host, in the order of the cases: floor 1.1e-10, 4.2e-8,
    1.5e-9 on the aligned output -- 5.8e-6, 1.2e-3, 3.0e-7 on the raw estimates
    -- and a host build of the kernels' code 6.7e-11, 3.1e-9, 1.4e-9 from the
    restatement).  The
    aligned estimate equals the input pose at safe_i, and its last returned
    row keeps the estimate's relative pose to it."""
    from dpvo.loop_closure import run_DPVO_PGO_sychronize
    from dpvo.loop_closure.optim_utils import sim3_inv, sim3_mul
    (gt, poses, loops, ii, jj), out, hist, ref, r32 = _lm(n, L, 30, small_drift)
    ran = int(np.isfinite(hist).sum())
    assert ran == len(ref["hist"]) and (ran == 6 if small_drift else ran == 30)
    assert np.isnan(hist[ran:]).all()
    np.testing.assert_allclose(hist[:ran], ref["hist"], rtol=1e-6, atol=0)
    want, safe_i = P.synchronize(poses, ref["sim3"], ii)
    floor = np.abs(want - P.synchronize(poses, r32["sim3"], ii)[0]).max()
    got = run_DPVO_PGO_sychronize(T(poses), T(loops), T(ii), T(jj))
    assert got.shape == (safe_i, 8)
    print("aligned diff", np.abs(got.cpu().numpy() - want).max(), "floor", floor)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=10 * floor)
    # the same alignment of all rows of the device estimate
    est = torch.from_numpy(out)
    aligned = sim3_mul(sim3_mul(torch.from_numpy(P.se3_to_sim3(poses))[[safe_i]], sim3_inv(est[[safe_i]])), est)
    np.testing.assert_allclose(aligned[:safe_i].numpy(), got.cpu().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(aligned[safe_i].numpy(), P.se3_to_sim3(poses)[safe_i], rtol=0, atol=1e-9)
    rel = lambda x: sim3_mul(sim3_inv(x[[safe_i - 1]]), x[[safe_i]]).numpy()
    np.testing.assert_allclose(rel(aligned), rel(est), rtol=0, atol=1e-9)
    # the optimisation closed the loops: the cost fell by more than 100x
    assert hist[ran - 1] < 0.01 * hist[0]


def test_pgo_is_bitwise_repeatable(poisoned):
    """two calls on the same input give the same bits (fixed summation order,
    no float atomics), also with every workspace byte poisoned"""
    import _dpvo_hot as H
    import cuda_ba
    gt, poses, loops, ii, jj = P.circle_case(96, 3, 0)
    args = (T(poses), T(loops), T(ii), T(jj))
    a = cuda_ba.pgo(*args, iters=6)
    b = cuda_ba.pgo(*args, iters=6)
    H.set_poison(0x00)
    c = cuda_ba.pgo(*args, iters=6)
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0].view(torch.int64), y[0].view(torch.int64))
        assert torch.equal(x[1].view(torch.int64), y[1].view(torch.int64))
    d1 = cuda_ba.pgo_step(T(P.initial_state(poses)), *args, 0.0, 1e-6, -1)
    d2 = cuda_ba.pgo_step(T(P.initial_state(poses)), *args, 0.0, 1e-6, -1)
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64))


def test_fix_opt_window_keeps_the_tail():
    """fix_opt_window optimises the poses up to the largest loop index only"""
    import cuda_ba
    gt, poses, loops, ii, jj = P.circle_case(48, 1, 0)
    out, _ = cuda_ba.pgo(T(poses), T(loops), T(ii), T(jj), iters=3, fix_opt_window=True)
    keep = int(max(ii.max(), jj.max())) + 1
    want = P.se3_to_sim3(poses)
    out = out.cpu().numpy()
    out[:, 3:7] *= np.sign((out[:, 3:7] * want[:, 3:7]).sum(1, keepdims=True))
    np.testing.assert_allclose(out[keep:], want[keep:], rtol=0, atol=1e-9)
    assert np.abs(out[:keep] - want[:keep]).max() > 1e-3


# ---------------------------------------------------------------------------
# PatchGraph.close_loop
# ---------------------------------------------------------------------------
def _patch_graph(n=48, M=4):
    from dpvo.lietorch import SE3
    from dpvo.patchgraph import PatchGraph
    gt, poses, _, _, _ = P.circle_case(n, 1, 0)
    cfg = SimpleNamespace(BUFFER_SIZE=64)
    pg = PatchGraph(cfg, 3, 384, 36, M, 30, 40, 4, device="cuda")
    g = torch.Generator().manual_seed(0)
    pg.n, pg.m = n, n * M
    pg.poses_[:n] = T(P._se3_inv(poses)).float()            # world-to-camera
    pg.patches_[:n, :, :2] = (torch.rand(n, M, 2, 3, 3, generator=g) * 30).cuda()
    pg.patches_[:n, :, 2] = (0.2 + torch.rand(n, M, 1, 1, generator=g)).cuda()
    pg.intrinsics_[:n] = torch.tensor([40.0, 40.0, 20.0, 15.0], device="cuda")
    pg.index_[:n] = torch.arange(n, device="cuda")[:, None]
    pg.tstamps_[:n] = 2 * np.arange(n)                       # odd stamps: removed frames
    d = lambda: SE3(T(P.random_poses(1, np.random.default_rng(len(pg.delta)), rot=0.1, trans=0.5)[0]).float())
    pg.delta[5] = (4, d())       # removed frame 5 hangs on stamp 4 = keyframe 2
    pg.delta[7] = (5, d())       # chained: 7 -> 5 -> 4
    pg.delta[91] = (90, d())     # keyframe 45: above safe_i, scale 1
    return pg, gt, poses


def test_close_loop_writes_back_poses_depths_and_deltas():
    import cuda_ba
    from dpvo.loop_closure.optim_utils import sim3_inv, sim3_mul
    pg, gt, poses = _patch_graph()
    n = pg.n
    Tg = P.sim3_inv(P.se3_to_sim3(gt))
    far = lambda i, j: P.sim3_mul(Tg[[j]], P.sim3_inv(Tg[[i]]))   # measured T_j T_i^-1, from the ground truth
    before = dict(poses=pg.poses_.clone(), patches=pg.patches_.clone(),
                  delta={t: (t0, dP.data.clone()) for t, (t0, dP) in pg.delta.items()})
    i, j = 40, 2
    # what close_loop is to compute, from pgo's output on the torch CPU side
    from dpvo.lietorch import SE3
    c2w = SE3(pg.poses_[:n]).inv().data                           # the PGO input, as close_loop forms it
    est = cuda_ba.pgo(c2w, T(far(i, j)), T(np.array([i])), T(np.array([j])))[0].cpu()
    safe_i = i + 1
    a = torch.cat((c2w.double().cpu(), torch.ones(n, 1, dtype=torch.float64)), 1)
    aligned = sim3_mul(sim3_mul(a[[safe_i]], sim3_inv(est[[safe_i]])), est)[:safe_i]
    want_w2c = torch.from_numpy(P._se3_inv(aligned[:, :7].numpy()))   # SE3(res).inv(): the scale goes to the depths
    s = aligned[:, 7]

    assert pg.close_loop(i, j, T(far(i, j))) == safe_i
    got = pg.poses_[:safe_i].double().cpu()
    got[:, 3:7] *= torch.sign((got[:, 3:7] * want_w2c[:, 3:7]).sum(1, keepdim=True))
    # float32 storage: 6e-8 relative on translations up to ~10, a handful of operations
    np.testing.assert_allclose(got.numpy(), want_w2c.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(pg.patches_[:safe_i, :, 2].cpu().numpy(),
                               (before["patches"][:safe_i, :, 2].cpu() / s.float().view(-1, 1, 1, 1)).numpy(),
                               rtol=1e-6, atol=0)
    assert s.min() < 0.99 or s.max() > 1.01                       # the drifted scale was corrected
    # rows >= safe_i: bit-identical
    assert torch.equal(pg.poses_[safe_i:], before["poses"][safe_i:])
    assert torch.equal(pg.patches_[safe_i:], before["patches"][safe_i:])
    assert torch.equal(pg.patches_[:, :, :2], before["patches"][:, :, :2])
    # deltas: 5 and 7 end on stamp 4 (keyframe 2), 91 on keyframe 45 (scale 1)
    for t, k in ((5, 2), (7, 2), (91, None)):
        t0, dP = pg.delta[t]
        b0, bd = before["delta"][t]
        scale = 1.0 if k is None else float(s[k])
        assert t0 == b0
        np.testing.assert_allclose(dP.data[:3].cpu().numpy(), bd[:3].cpu().numpy() * np.float32(scale), rtol=1e-6)
        assert torch.equal(dP.data[3:], bd[3:])
    assert torch.isfinite(pg.points_[:pg.m]).all()
    assert pg.loop_ii.tolist() == [i] and pg.loop_jj.tolist() == [j]

    # a second loop carries the first one's indices, its constraint rebuilt from the corrected poses
    assert pg.close_loop(44, 10, T(far(44, 10))) == 45
    assert pg.loop_ii.tolist() == [40, 44] and pg.loop_jj.tolist() == [2, 10]
    assert torch.isfinite(pg.poses_).all() and torch.isfinite(pg.patches_).all()
