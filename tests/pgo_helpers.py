"""fp64 numpy restatement of the loop-closure pose-graph optimisation
(reference dpvo/loop_closure/optim_utils.py:158-255) and the fixtures of
test_pgo_host.py / test_gpu_pgo.py.

Group operations are the oracle's lietorch Sim3 (``oracle.lie_forward``,
pinned by tests/golden/lietorch_ref.npz); Jacobians are central differences;
the solve is ``np.linalg.solve`` on the dense normal equations (or the
float32 ``oracle.solve_system``).  Poses: camera-to-world SE3 ``[t, q]``;
state ``g``: tangent ``[tau, phi, sigma]`` of the world-to-camera Sim3.
"""
import numpy as np

from oracle import oracle

S = oracle.SIM3
FD_H = 1e-5


def sim3_exp(x):
    return oracle.lie_forward("exp", S, x)


def sim3_log(X):
    return oracle.lie_forward("log", S, X)


def sim3_inv(X):
    return oracle.lie_forward("inv", S, X)


def sim3_mul(X, Y):
    return oracle.lie_forward("mul", S, X, Y)


def se3_to_sim3(poses):
    poses = np.asarray(poses, np.float64)
    return np.concatenate([poses, np.ones_like(poses[:, :1])], 1)


def initial_state(poses):
    return sim3_log(sim3_inv(se3_to_sim3(poses)))


def edges(poses, loop_poses, loop_ii, loop_jj):
    """-> (C [E, 8], iii [E], jjj [E]): chain edges (k, k-1) then the loops"""
    T = sim3_inv(se3_to_sim3(poses))
    n = len(T)
    kk = np.arange(1, n)
    C = sim3_mul(T[kk - 1], sim3_inv(T[kk]))
    lp = np.asarray(loop_poses, np.float64).reshape(-1, 8)
    return (np.concatenate([C, lp], 0), np.concatenate([kk, np.asarray(loop_ii, np.int64)]),
            np.concatenate([kk - 1, np.asarray(loop_jj, np.int64)]))


def edge_residual(C, Gi, Gj):
    return sim3_log(sim3_mul(sim3_mul(C, sim3_exp(Gi)), sim3_inv(sim3_exp(Gj))))


def residual(g, poses, loop_poses, loop_ii, loop_jj):
    C, iii, jjj = edges(poses, loop_poses, loop_ii, loop_jj)
    return edge_residual(C, g[iii], g[jjj])


def jacobians_fd(g, poses, loop_poses, loop_ii, loop_jj, h=FD_H):
    """central differences of edge_residual in g_i and g_j: Ji, Jj [E, 7, 7]"""
    C, iii, jjj = edges(poses, loop_poses, loop_ii, loop_jj)
    Gi, Gj = g[iii].copy(), g[jjj].copy()
    Ji = np.zeros((len(iii), 7, 7))
    Jj = np.zeros((len(iii), 7, 7))
    for c in range(7):
        d = np.zeros(7)
        d[c] = h
        Ji[:, :, c] = (edge_residual(C, Gi + d, Gj) - edge_residual(C, Gi - d, Gj)) / (2 * h)
        Jj[:, :, c] = (edge_residual(C, Gi, Gj + d) - edge_residual(C, Gi, Gj - d)) / (2 * h)
    return Ji, Jj, iii, jjj


def solve_fp64(Ji, Jj, iii, jjj, res, ep, lm, freen):
    """oracle.solve_system without its final cast to float32"""
    r, n = len(iii), int(max(iii.max(), jjj.max())) + 1
    J = np.zeros((7 * r, 7 * n))
    for x in range(r):
        J[7 * x:7 * x + 7, 7 * iii[x]:7 * iii[x] + 7] += Ji[x]
        J[7 * x:7 * x + 7, 7 * jjj[x]:7 * jjj[x] + 7] += Jj[x]
    A = J.T @ J
    b = -(J.T @ res.reshape(-1))
    A[np.diag_indices_from(A)] += A.diagonal() * lm + ep
    m = 7 * n if freen < 0 else 7 * freen
    delta = np.zeros(7 * n)
    delta[:m] = np.linalg.solve(A[:m, :m], b[:m])
    return delta.reshape(n, 7)


def lm_restatement(poses, loop_poses, loop_ii, loop_jj, iters=30, ep=0.0, lmbda=1e-6, freen=-1, solver="fp64"):
    """perform_updates (optim_utils.py:222-255).  -> dict(sim3 [n, 8], hist,
    accepts, ratios = cost_new / cost_old of every step)"""
    g = initial_state(poses)
    hist, accepts, ratios = [], [], []
    for itr in range(iters):
        res = residual(g, poses, loop_poses, loop_ii, loop_jj)
        hist.append(float(np.mean(res ** 2)))
        Ji, Jj, iii, jjj = jacobians_fd(g, poses, loop_poses, loop_ii, loop_jj)
        if solver == "fp64":
            delta = solve_fp64(Ji, Jj, iii, jjj, res, ep, lmbda, freen)
        else:
            delta = oracle.solve_system(Ji, Jj, iii, jjj, res, ep, lmbda, freen).astype(np.float64)
        cand = g + delta
        new = float(np.mean(residual(cand, poses, loop_poses, loop_ii, loop_jj) ** 2))
        ratios.append(new / hist[-1] if hist[-1] > 0 else float("nan"))
        accepts.append(new < hist[-1])
        if accepts[-1]:
            g = cand
            lmbda /= 2
        else:
            lmbda *= 2
        if hist[-1] < 1e-5 and itr >= 4 and hist[-5] / hist[-1] < 1.5:
            break
    return dict(sim3=sim3_inv(sim3_exp(g)), hist=np.array(hist), accepts=accepts, ratios=np.array(ratios))


def synchronize(poses, est, loop_ii):
    """run_DPVO_PGO_sychronize's alignment (optim_utils.py:214-217):
    (Sim3(poses)[safe_i] est[safe_i]^-1) est, rows [:safe_i]"""
    safe_i = int(np.max(loop_ii)) + 1
    a = se3_to_sim3(poses)
    lead = sim3_mul(a[[safe_i]], sim3_inv(est[[safe_i]]))
    return sim3_mul(np.repeat(lead, len(est), 0), est)[:safe_i], safe_i


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
def _quat(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([axis * np.sin(angle / 2)[..., None], np.cos(angle / 2)[..., None]], -1)


def random_poses(n, rng, rot=3.0, trans=10.0):
    """SE3 [t, q]: rotation angles up to rot rad, translations up to trans"""
    t = rng.uniform(-trans, trans, (n, 3))
    q = _quat(rng.normal(size=(n, 3)), rng.uniform(0, rot, n))
    return np.concatenate([t, q], 1)


def random_loops(L, rng, rot=3.0, trans=10.0):
    """Sim3 [t, q, s] with scales in [0.5, 2]"""
    return np.concatenate([random_poses(L, rng, rot, trans), rng.uniform(0.5, 2.0, (L, 1))], 1)


# (n, L) -> loop index lists: (6, 1) a reversed loop (ii > jj); (40, 3) nested
# loops (one inside another) and one reversed; (200, 8) nested, overlapping,
# a shared endpoint (150 twice, 20 twice), reversed ones, one next to the chain
RANDOM_CASES = {
    (6, 1): ([4], [1]),
    (40, 3): ([2, 10, 35], [38, 30, 5]),
    (200, 8): ([5, 20, 150, 150, 199, 60, 20, 101], [120, 90, 30, 80, 0, 140, 170, 100]),
}


def random_case(n, L, seed):
    """poses, loop constraints and a generic state g (the initial state plus
    a perturbation whose sigma component is at least 0.05 from zero)"""
    rng = np.random.default_rng(seed)
    poses = random_poses(n, rng)
    ii, jj = (np.array(x, np.int64) for x in RANDOM_CASES[(n, L)])
    loops = random_loops(L, rng)
    g = initial_state(poses)
    g = g + rng.uniform(-0.05, 0.05, g.shape)
    g[:, 6] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.05, 0.3, n)
    return poses, loops, ii, jj, g


CIRCLE_LOOPS = {
    (48, 1): ([45], [1]),
    (96, 3): ([90, 60, 20], [3, 12, 75]),
    (4096, 16): (list(range(4000, 4080, 5)), list(range(10, 90, 5))),
}


# the Levenberg-Marquardt parity cases: seed of circle_case and the number of
# leading steps of the restatement whose cost_new / cost_old lies outside
# [0.99, 1.01] (test_pgo_host.py checks it).  Later steps sit on the converged
# plateau (ratio 1 +- 1e-9), where rounding decides accept / reject.
LM_CASES = {(48, 1): dict(seed=0, iters=2), (96, 3): dict(seed=0, iters=3)}


def circle_gt(n, radius=5.0, turns=1.0):
    th = 2 * np.pi * turns * np.arange(n) / n
    t = np.stack([radius * np.cos(th), radius * np.sin(th), 0.2 * np.sin(3 * th)], 1)
    q = _quat(np.tile([0.0, 0.0, 1.0], (n, 1)), th)
    return np.concatenate([t, q], 1)


def _se3_mul(a, b):
    return oracle.lie_forward("mul", oracle.SE3, a, b)


def _se3_inv(a):
    return oracle.lie_forward("inv", oracle.SE3, a)


def circle_case(n, L, seed, scale_drift=0.01, rot_drift=0.004):
    """ground truth on a circle; the input accumulates scale_drift per frame
    on the translation of every relative motion and a small rotation about a
    seeded axis; the loop constraints come from the ground truth."""
    rng = np.random.default_rng(seed)
    gt = circle_gt(n)
    rel = _se3_mul(_se3_inv(gt[:-1]), gt[1:])          # gt[k-1]^-1 gt[k]
    axis = rng.normal(size=3)
    noise = _quat(np.tile(axis, (n - 1, 1)), rot_drift * (1 + 0.5 * rng.uniform(-1, 1, n - 1)))
    rel[:, :3] *= (1.0 + scale_drift) ** np.arange(1, n)[:, None]
    rel = _se3_mul(rel, np.concatenate([np.zeros((n - 1, 3)), noise], 1))
    poses = [gt[0]]
    for k in range(n - 1):
        poses.append(_se3_mul(poses[-1][None], rel[[k]])[0])
    poses = np.array(poses)
    ii, jj = (np.array(x, np.int64) for x in CIRCLE_LOOPS[(n, L)])
    T = sim3_inv(se3_to_sim3(gt))
    loops = sim3_mul(T[jj], sim3_inv(T[ii]))             # zero residual at the ground truth
    return gt, poses, loops, ii, jj


def self_loops(poses, ii, jj):
    """loop constraints read off the trajectory itself (zero residual)"""
    T = sim3_inv(se3_to_sim3(poses))
    return sim3_mul(T[jj], sim3_inv(T[ii]))
