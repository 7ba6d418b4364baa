"""Loop-closure optimisation utilities (reference dpvo/loop_closure/optim_utils.py).

The names are the reference's; the work is not pypose's: the Sim(3)
pose-graph optimisation runs in ``cuda_ba.pgo_residual`` / ``pgo_step`` /
``pgo`` (csrc/pgo.hip, fp64 on the GPU); the point-cloud alignment is
``cuda_ba.ransac_sim3`` / ``umeyama`` (csrc/align.hip, fp64 on the GPU) behind
``ransac_umeyama_gpu``, with the plain-numpy functions of the reference's names
kept beside it.  Poses are camera-to-world SE3 ``[t, q]``, Sim3 data is ``[t, q, s]``;
arguments may be this package's ``lietorch`` groups or plain tensors.
"""
import numpy as np
import torch

import cuda_ba

from ..lietorch import SE3, Sim3


def _data(x):
    return x.data if isinstance(x, (SE3, Sim3)) else x


def SE3_to_Sim3(x):
    """[..., 7] SE3 -> [..., 8] Sim3 with scale 1 (an SE3 gives a Sim3, a tensor a tensor)"""
    d = _data(x)
    out = torch.cat((d, torch.ones_like(d[..., :1])), dim=-1)
    return Sim3(out) if isinstance(x, SE3) else out


def make_Sim3(rot, t, s, device=None):
    """rotation matrix, translation, scale (umeyama_alignment's result) -> Sim3 data [1, 8], fp64"""
    from ..utils import matrix_to_quaternion
    q = matrix_to_quaternion(torch.as_tensor(np.asarray(rot), dtype=torch.float64)[None])[:, [1, 2, 3, 0]]
    out = torch.cat((torch.as_tensor(np.asarray(t), dtype=torch.float64).view(1, 3), q,
                     torch.as_tensor(float(s), dtype=torch.float64).view(1, 1)), dim=1)
    return out.to(device) if device is not None else out


# ---- Sim3 on plain [..., 8] tensors (any dtype / device), for the alignment step
def _qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack((aw * bx + ax * bw + ay * bz - az * by,
                        aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx,
                        aw * bw - ax * bx - ay * by - az * bz), -1)


def _qrot(q, p):
    v = q[..., :3]
    uv = 2 * torch.cross(v, p, dim=-1)
    return p + q[..., 3:] * uv + torch.cross(v, uv, dim=-1)


def sim3_mul(a, b):
    ta, qa, sa = a.split([3, 4, 1], -1)
    tb, qb, sb = b.split([3, 4, 1], -1)
    q = _qmul(qa, qb)
    return torch.cat((ta + sa * _qrot(qa, tb), q / q.norm(dim=-1, keepdim=True), sa * sb), -1)


def sim3_inv(a):
    t, q, s = a.split([3, 4, 1], -1)
    qi = q * q.new_tensor([-1.0, -1.0, -1.0, 1.0])
    return torch.cat((-_qrot(qi, t) / s, qi, 1 / s), -1)


def residual(Ginv, input_poses, dSloop, ii, jj, jacobian=False):
    """residuals [E, 7] of the n - 1 chain edges and the loop edges at the
    state Ginv [n, 7] (tangent coordinates of the world-to-camera Sim3s);
    with jacobian: (resid, (J_Ginv_i, J_Ginv_j, iii, jjj))."""
    res, Ji, Jj, iii, jjj = cuda_ba.pgo_residual(_data(Ginv), _data(input_poses), _data(dSloop), ii, jj)
    return (res, (Ji, Jj, iii, jjj)) if jacobian else res


def perform_updates(input_poses, dSloop, ii_loop, jj_loop, iters, ep=0.0, lmbda=1e-6, fix_opt_window=False):
    """the Levenberg-Marquardt loop -> Sim3 data [n, 8] (fp64), camera-to-world"""
    return cuda_ba.pgo(_data(input_poses), _data(dSloop), ii_loop, jj_loop, iters=iters, ep=ep, lmbda=lmbda,
                       fix_opt_window=fix_opt_window)[0]


def run_DPVO_PGO_sychronize(pred_poses, loop_poses, loop_ii, loop_jj, iters=30):
    """optimise, then move the estimate onto the input trajectory at
    safe_i = max(loop_ii) + 1: (Sim3(poses)[safe_i] est[safe_i]^-1) est, rows
    [:safe_i] -> Sim3 data [safe_i, 8] (fp64)."""
    poses = _data(pred_poses)
    safe_i = int(torch.as_tensor(loop_ii).max().item()) + 1
    if safe_i >= poses.shape[0]:
        raise RuntimeError(f"run_DPVO_PGO_sychronize: max(loop_ii) + 1 = {safe_i} is not a pose index "
                           f"(n = {poses.shape[0]}); the newest loop frame needs a successor to align on")
    est = perform_updates(poses, loop_poses, loop_ii, loop_jj, iters=iters)
    aa = SE3_to_Sim3(poses.to(est.dtype))
    lead = sim3_mul(aa[[safe_i]], sim3_inv(est[[safe_i]]))
    return sim3_mul(lead, est[:safe_i])


# ---- Sim(3) between two matched point clouds, numpy
def umeyama_alignment(x, y):
    """least-squares similarity y ~ c r x + t between two m x n point sets
    (Umeyama, IEEE PAMI 1991) -> (r, t, c), or (None, None, None) when the
    covariance has rank below m - 1."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    m, n = x.shape
    mx, my = x.mean(axis=1), y.mean(axis=1)
    xc, yc = x - mx[:, None], y - my[:, None]
    var_x = (xc ** 2).sum() / n
    cov = yc @ xc.T / n
    u, d, vt = np.linalg.svd(cov)
    if np.count_nonzero(d > np.finfo(d.dtype).eps) < m - 1:
        return None, None, None
    sgn = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        sgn[m - 1, m - 1] = -1
    r = u @ sgn @ vt
    c = np.trace(np.diag(d) @ sgn) / var_x
    return r, my - c * (r @ mx), c


def ransac_umeyama(src_points, dst_points, iterations=1, threshold=0.1, rng=None):
    """RANSAC over 3-point samples -> (R, t, s, inliers) of the refit on the
    best sample's inliers ((None, None, None, 0) when no sample worked).  rng:
    a numpy Generator (or a seed) for the samples."""
    rng = np.random.default_rng(rng)
    src_points = np.asarray(src_points, np.float64)
    dst_points = np.asarray(dst_points, np.float64)
    best = (None, None, None)
    best_inliers = 0
    for _ in range(iterations):
        idx = rng.choice(src_points.shape[0], 3, replace=False)
        R, t, s = umeyama_alignment(src_points[idx].T, dst_points[idx].T)
        if t is None:
            continue
        moved = src_points @ (R * s).T + t
        mask = np.linalg.norm(moved - dst_points, axis=1) < threshold
        inliers = int(mask.sum())
        if inliers > best_inliers:
            best_inliers = inliers
            best = umeyama_alignment(src_points[mask].T, dst_points[mask].T)
        if inliers > 100:
            break
    return best[0], best[1], best[2], best_inliers


# ---- the same alignment on the device (csrc/align.hip)
def draw_samples(N, iterations, rng=None):
    """the 3-point samples ransac_umeyama draws from this Generator (or seed),
    in its order: `iterations` calls of rng.choice(N, 3, replace=False) ->
    int64 [iterations, 3]"""
    rng = np.random.default_rng(rng)
    return np.stack([rng.choice(N, 3, replace=False) for _ in range(iterations)]).astype(np.int64)


def ransac_umeyama_gpu(src_points, dst_points, iterations=400, threshold=0.5, rng=None, early_exit=100):
    """ransac_umeyama on the device: src_points / dst_points [N, 3] GPU tensors
    (fp32 or fp64), the samples of draw_samples(N, iterations, rng) -> (Sim3
    data [1, 8] fp64 on the device, inliers), or (None, 0) when no sample
    worked or the refit is degenerate.  With the same Generator it returns
    what ransac_umeyama returns (the reference stops at the first sample with
    more than early_exit = 100 inliers; early_exit < 0: the best of all).
    One host read, of the four status words."""
    N = src_points.shape[0]
    if N < 3:
        return None, 0
    samples = torch.from_numpy(draw_samples(N, iterations, rng)).to(src_points.device)
    sim3, _, _, info = cuda_ba.ransac_sim3(src_points, dst_points, samples, threshold, early_exit=early_exit)
    code, _, inliers, _ = info.tolist()
    if code != 0:
        return None, 0
    return sim3.view(1, 8), int(inliers)
