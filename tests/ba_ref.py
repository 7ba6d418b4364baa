"""fp64 restatement of ONE Gauss-Newton step of the bundle adjustment
(csrc/fastba.hpp, the header comment of csrc/fastba.hip) with the magnitude
companions its tests are held to.  Plain numpy, no GPU, nothing of the float
oracle: the normal equations are assembled from one sparse Jacobian row per
residual (a = [-Ji at pose i, +Jj at pose j], Jz at the patch), which shares no
statement order with any of the three solver paths.

    per edge (patch centre pixel):  G_ij = G_j G_i^-1, X = G_ij (x_n, y_n, 1, d),
        r = target - proj(X), mask, Jj = d proj / d xi_j, Ji = Jj Ad(G_ij)
        (d proj / d xi_i = -Ji), Jz = d proj / d d
    B = sum w a a^T    E_k = sum w Jz a    C_k = sum w Jz^2
    v = sum w r a      u_k = sum w r Jz    (prior: C_k += mu, u_k -= mu (d_k - est_k))
    Q = 1 / (C + lmbda),  S = B - E Q E^T,  y = v - E Q u,  S += diag(1e-4 S + 1)
    dX = S^-1 y,  dZ = Q (u - E^T dX),  poses <- Exp(dX) poses,
    depth <- clamp(depth[pixel 0] + dZ) on all P x P pixels.

The quaternions are used as stored (the kernels never normalise them): the
rotation is I + 2 w [q]x + 2 [q]x^2 of the raw (x, y, z, w).

Where the depth is read: the Jacobians, the residual and the prior's d use the
centre pixel ((P / 2) P + P / 2); the update reads pixel 0; the result goes to
all P x P pixels.

Magnitudes.  Every sum comes with the sum of the magnitudes of its terms, each
factor taken at the size its last fp32 rounding acts on:

    r      -> |r| for the roundings after it, and rmag = |target| + |x1| + |cx| for
              its own K_R (r = target - x1 cancels ~100 px to ~1 px)
    Ji     -> |Ad(G_ij)|^T |Jj|                    (the adjoint's sums cancel)
    Jz     -> fx (|t_ij,x| d + |t_ij,z| |X| d^2)   with |t_ij| = |t_j| + |R_ij| |t_i|
    Smag = sum w amag amag^T + Emag Q Emag^T (+ the damping's |1e-4 S| + 1)
    ymag = sum w |r| amag    + Emag Q umag        (yrmag, urmag: the same with rmag for |r|)

The bars (EPS = 2^-24), for the pose step xi = tangent(P_out, P_in) the GPU took:

    |S xi - y|_a <= k EPS ( sum_b M_ab |xi_b| + ymag_a ) + K_R EPS yrmag_a + q_a,
        M_ab = max(Smag_ab, sqrt(Sd_aa Sd_bb))   (Sd = the damped S: a Cholesky's
        backward error is gamma_(3n+1) |L| |L^T| <= gamma sqrt(S_aa S_bb), Higham
        10.3/10.4, so one matrix carries both the assembly and the solve)
        q_a = sum_b |S_ab| dxi_b, dxi = K_RETR EPS |d tangent / d P_out| Pmag:
        the retraction's roundings of the 7 stored numbers pushed through S
    |d_out - clamp(d[pixel 0] + dZ_ref(xi))|_k <= k_z EPS ( Q umag + Q Emag |xi| + |d| )_k
                                                   + K_R EPS Q urmag_k + Q |E_k| dxi

k is the count of fp32 roundings on the longest dependent path, per path:

    K_EDGE = 68   relSE3 (q_ij 4, t_ij +6 = 10), the ray 2, actSE3 +7 = 17,
                  d = 1 / Z 18, d^2 19, a Jj entry +4 = 23, adjSE3 (cross 2, the
                  rotation 5, the add) +8 = 31 for a Ji entry; a term w Ji Ji'
                  carries both factors' errors and three products: 31 + 31 + 3
                  = 65, and the mask / weight product and the sign +3
    accumulation  the adds a term passes through on its way into S / y:
        det     the wave sum (6) + the waves' LDS partial (patches per wave) +
                4 waves + the 512 partials (16 + 1 + 16)          = 43 + ceil(G / 2048)
        atomic  unordered: every edge that lands on the entry     = the most edges any
                one optimised pose has (as frame i or j) + 8 (the wave's
                pre-reduction, the workgroups' partials of the LDS variant)
        band    as atomic
    Schur         the products Q e e' (Q: a divide and an add: 4) and one add per
                  patch: det 4 + slots in order (G per workgroup round: <= G / 512
                  + 32); atomic and band 4 + the most patches any one pose sees
    solve         fp32 Cholesky + two substitutions: 3 n6 + 1 (det, every window;
                  atomic with n6 <= 64); fp64 factor (atomic n6 > 64, band): 2
                  (the roundings of S and dX to and from double)
    K_R = 22      the residual: X / Z at 18, fx *, + cx, target - x1
    K_RETR = 12   expSE3 (sin / cos, the divides, two crosses) and the
                  quaternion / rotation products of the retraction
    k_z           K_EDGE + the patch's accumulation (its edges) + the n6-term dot
                  product e . dX + 4 (Q, the multiply, the add, the clamp's add)

`k_pose(path, n6, edges, patches, G)` and `k_depth(n6, edges)` below are this table.
Observed ratios are recorded in profiles/ba_step_tests/NOTES.md.
"""
import numpy as np

EPS = 2.0 ** -24
K_EDGE = 68
K_R = 22
K_RETR = 12
REL_MARGIN = 1e-3


def k_pose(path, n6, edges, patches, G):
    """roundings on the longest path into one row of S xi = y (the table above);
    edges / patches: the most edges / unique patches on any one optimised pose,
    G: unique patches"""
    if path == "det":
        acc = 43 + -(-G // 2048)
        schur = 4 + G // 512 + 32
        solve = 3 * n6 + 1
    else:
        acc = edges + 8      # (+ the wave's pre-reduction and the workgroups' partials of the LDS variant)
        schur = 4 + patches
        solve = 3 * n6 + 1 if (path == "atomic" and n6 <= 64) else 2
    return K_EDGE + acc + schur + solve


def k_depth(n6, edges):
    return K_EDGE + edges + n6 + 4


# ---------------------------------------------------------------------------
# SE(3), generic over the dtype (float64: the reference; float32: float32_step)
def _c(x, dt):
    return np.asarray(x, dtype=dt)


def _act(q, X):
    """rotation of X [.., 3] by the raw quaternion q [.., 4] (x, y, z, w)"""
    two = _c(2, q.dtype)
    uv = two * np.cross(q[..., :3], X)
    return X + q[..., 3:4] * uv + np.cross(q[..., :3], uv)


def _rotmat(q):
    """I + 2 w [q]x + 2 [q]x^2 as a matrix [.., 3, 3]"""
    eye = np.eye(3, dtype=q.dtype)
    return np.stack([_act(q, np.broadcast_to(eye[c], q.shape[:-1] + (3,))) for c in range(3)], -1)


def _qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], -1)


def _qconj(q):
    return np.concatenate([-q[..., :3], q[..., 3:4]], -1)


def _exp_se3(xi):
    """[n, 6] (tau, phi) -> (t [n, 3], q [n, 4]) with the code's small-angle branches"""
    dt = xi.dtype
    tau, phi = xi[:, :3], xi[:, 3:]
    th2 = (phi * phi).sum(1)
    th = np.sqrt(th2)
    th4 = th2 * th2
    small = th2 < _c(1e-8, np.float32).astype(dt)
    ths = np.where(th > 0, th, _c(1, dt))
    imag = np.where(small, _c(0.5, dt) - _c(1.0 / 48.0, dt) * th2 + _c(1.0 / 3840.0, dt) * th4,
                    np.sin(_c(0.5, dt) * ths) / ths)
    real = np.where(small, _c(1, dt) - _c(1.0 / 8.0, dt) * th2 + _c(1.0 / 384.0, dt) * th4, np.cos(_c(0.5, dt) * th))
    q = np.concatenate([imag[:, None] * phi, real[:, None]], 1)
    big = th > _c(1e-4, np.float32).astype(dt)
    th2s = np.where(big, th2, _c(1, dt))
    a = np.where(big, (_c(1, dt) - np.cos(th)) / th2s, _c(0, dt))
    b = np.where(big, (ths - np.sin(ths)) / (ths * th2s), _c(0, dt))
    c1 = np.cross(phi, tau)
    c2 = np.cross(phi, c1)
    t = tau + a[:, None] * c1 + b[:, None] * c2
    return t, q


def retract(poses, xi):
    """left retraction Exp(xi) * (t, q) of [n, 7] poses"""
    dt_, dq = _exp_se3(xi)
    t, q = poses[:, :3], poses[:, 3:]
    return np.concatenate([_act(dq, t) + dt_, _qmul(dq, q)], 1)


def tangent(P1, P0):
    """Log(P1 * P0^-1) in fp64, [n, 7] x [n, 7] -> [n, 6] (tau, phi): the step a
    left retraction took, recovered from its in-place output"""
    P1, P0 = np.asarray(P1, np.float64), np.asarray(P0, np.float64)
    q0 = P0[:, 3:] / np.linalg.norm(P0[:, 3:], axis=1, keepdims=True)
    q1 = P1[:, 3:] / np.linalg.norm(P1[:, 3:], axis=1, keepdims=True)
    qr = _qmul(q1, _qconj(q0))
    tr = P1[:, :3] - _act(qr, P0[:, :3])
    qr = np.where(qr[:, 3:4] < 0, -qr, qr)
    nv = np.linalg.norm(qr[:, :3], axis=1)
    th = 2.0 * np.arctan2(nv, qr[:, 3])
    scale = np.where(nv > 1e-12, th / np.where(nv > 1e-12, nv, 1.0), 2.0)
    phi = qr[:, :3] * scale[:, None]
    out = np.zeros((len(P1), 6))
    for r in range(len(P1)):
        p, t = phi[r], th[r]
        K = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        c = 1.0 / 12.0 if t < 1e-6 else (1.0 - t * np.sin(t) / (2.0 * (1.0 - np.cos(t)))) / (t * t)
        out[r, :3] = (np.eye(3) - 0.5 * K + c * (K @ K)) @ tr[r]
        out[r, 3:] = p
    return out


def tangent_sensitivity(P1, P0, h=1e-6):
    """|d tangent / d P1| [n, 6, 7] by central differences"""
    P1 = np.asarray(P1, np.float64)
    J = np.zeros((len(P1), 6, 7))
    for s in range(7):
        d = np.zeros(7)
        d[s] = h
        J[:, :, s] = np.abs(tangent(P1 + d, P0) - tangent(P1 - d, P0)) / (2 * h)
    return J


# ---------------------------------------------------------------------------
# per edge
def centre_index(P):
    return (P // 2) * P + P // 2


def project(poses, px, py, d, intr, ii, jj):
    """fp64 reprojection of the points (px, py, inverse depth d) of frames ii into frames jj"""
    o = edge_terms(poses, np.stack([px, py, d], 1)[:, :, None, None], intr, np.zeros((len(ii), 2)),
                   np.ones((len(ii), 2)), ii, jj, np.arange(len(ii)), 0, 0)
    return -o["r"], o["Z"]


def edge_terms(poses, patches, intrinsics, target, weight, ii, jj, kk, t0, t1, dtype=np.float64):
    """Per edge: r [E, 2], mask [E], Ji / Jj [E, 2, 6], Jz [E, 2], ix, jx, iv, jv,
    self, the margins to every discontinuity and the magnitude companions."""
    dt = dtype
    poses = _c(poses, dt).reshape(-1, 7)
    P = patches.shape[-1]
    patches = _c(patches, dt).reshape(-1, 3, P * P)
    fx, fy, cx, cy = (_c(v, dt) for v in np.asarray(intrinsics, dtype=dt).reshape(-1, 4)[0])
    target = _c(target, dt).reshape(-1, 2)
    weight = _c(weight, dt).reshape(-1, 2)
    ii, jj, kk = (np.asarray(a, np.int64) for a in (ii, jj, kk))
    ce = centre_index(P)
    one = _c(1, dt)
    px, py, dk = patches[kk, 0, ce], patches[kk, 1, ce], patches[kk, 2, ce]
    ti, qi, tj, qj = poses[ii, :3], poses[ii, 3:], poses[jj, :3], poses[jj, 3:]
    qij = _qmul(qj, _qconj(qi))
    tij = tj - _act(qij, ti)
    a3 = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones_like(px)], 1)
    Xj = _act(qij, a3) + tij * dk[:, None]
    X, Y, Z, W = Xj[:, 0], Xj[:, 1], Xj[:, 2], dk
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(Z >= _c(0.2, np.float32).astype(dt), one / Z, _c(0, dt))
        x1, y1 = fx * (X / Z) + cx, fy * (Y / Z) + cy
    d2 = d * d
    r = np.stack([target[:, 0] - x1, target[:, 1] - y1], 1)
    rn = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    zlim = _c(0.2, np.float32).astype(dt)
    two = _c(2, dt)
    margins = {"Z": Z - zlim, "r": _c(128, dt) - rn, "x_lo": x1 + _c(64, dt), "y_lo": y1 + _c(64, dt),
               "x_hi": two * cx + _c(64, dt) - x1, "y_hi": two * cy + _c(64, dt) - y1}
    mask = np.ones(len(ii), bool)
    for m in margins.values():
        mask &= m > 0
    z = np.zeros_like(X)
    Jj = np.stack([np.stack([fx * W * d, z, fx * -X * W * d2, fx * -X * Y * d2, fx * (one + X * X * d2), fx * -Y * d], 1),
                   np.stack([z, fy * W * d, fy * -Y * W * d2, fy * (-one - Y * Y * d2), fy * (X * Y * d2), fy * X * d], 1)],
                  1)
    Jz = np.stack([fx * (tij[:, 0] * d - tij[:, 2] * (X * d2)), fy * (tij[:, 1] * d - tij[:, 2] * (Y * d2))], 1)
    # Ji = Jj Ad(G_ij): rows [a, b] -> [R^T a, R^T b + R^T (a x t)]
    qinv = _qconj(qij)[:, None, :]
    ja, jb = Jj[:, :, :3], Jj[:, :, 3:]
    Ji = np.concatenate([_act(qinv, ja), _act(qinv, jb) + _act(qinv, np.cross(ja, tij[:, None, :]))], 2)
    ix, jx = ii - t0, jj - t0
    N = t1 - t0
    iv, jv = (ix >= 0) & (ix < N), (jx >= 0) & (jx < N)
    out = dict(r=r, mask=mask, Ji=Ji, Jj=Jj, Jz=Jz, ix=ix, jx=jx, iv=iv, jv=jv, self=iv & jv & (ix == jx),
               margins=margins, Z=Z, x1=np.stack([x1, y1], 1), w=weight * mask[:, None].astype(dt), N=N)
    # magnitude companions
    Rt = np.abs(np.swapaxes(_rotmat(qij), -1, -2))          # |R_ij|^T
    tmag = np.abs(tj) + np.einsum("eba,eb->ea", Rt, np.abs(ti))
    at = np.abs(tij)
    ca = np.abs(ja)
    cr = np.stack([at[:, None, 1] * ca[:, :, 2] + at[:, None, 2] * ca[:, :, 1],
                   at[:, None, 2] * ca[:, :, 0] + at[:, None, 0] * ca[:, :, 2],
                   at[:, None, 0] * ca[:, :, 1] + at[:, None, 1] * ca[:, :, 0]], 2)
    out["Jimag"] = np.concatenate([np.einsum("eab,erb->era", Rt, ca),
                                   np.einsum("eab,erb->era", Rt, np.abs(jb) + cr)], 2)
    out["Jjmag"] = np.abs(Jj)
    out["Jzmag"] = np.stack([fx * (tmag[:, 0] * d + tmag[:, 2] * np.abs(X) * d2),
                             fy * (tmag[:, 1] * d + tmag[:, 2] * np.abs(Y) * d2)], 1)
    with np.errstate(invalid="ignore"):
        out["rmag"] = np.abs(target) + np.abs(out["x1"]) + np.stack([np.abs(cx) + z, np.abs(cy) + z], 1)
    return out


def min_relative_margin(et):
    """smallest margin of any edge to any mask discontinuity, relative to the threshold's scale"""
    m = et["margins"]
    x1 = np.abs(et["x1"])
    scale = {"Z": 0.2, "r": 128.0, "x_lo": np.maximum(x1[:, 0], 64), "y_lo": np.maximum(x1[:, 1], 64),
             "x_hi": np.maximum(x1[:, 0], 64), "y_hi": np.maximum(x1[:, 1], 64)}
    with np.errstate(invalid="ignore"):
        rel = np.stack([np.abs(m[k]) / scale[k] for k in m], 1)
    # behind the camera (Z <= 0) the projection is meaningless: Z alone decides there
    rel = np.where((et["Z"] <= 0.1)[:, None], np.abs(m["Z"])[:, None] / 0.2, rel)
    return rel.min(1)


# ---------------------------------------------------------------------------
# normal equations
def normal_equations(et, kk, lmbda, d_centre=None, est=None, mu=0.0, dtype=np.float64):
    """B, E [Mu, n6], C, v, u, Q, the damped S and y, and the magnitude sums
    Smag / ymag / Emag / umag.  d_centre / est: [num_patches] centre-pixel
    depth and prior (None: no prior).  ku: the sorted unique patches."""
    dt = dtype
    N = et["N"]
    n6 = 6 * N
    kk = np.asarray(kk, np.int64)
    ku, kinv = np.unique(kk, return_inverse=True)
    E_, Mu = len(kk), len(ku)
    a = np.zeros((E_, 2, n6), dt)
    am = np.zeros((E_, 2, n6), dt)
    for e in np.flatnonzero(et["iv"]):
        s = 6 * et["ix"][e]
        a[e, :, s:s + 6] -= et["Ji"][e]
        am[e, :, s:s + 6] += et["Jimag"][e].astype(dt)
    for e in np.flatnonzero(et["jv"]):
        s = 6 * et["jx"][e]
        a[e, :, s:s + 6] += et["Jj"][e]
        am[e, :, s:s + 6] += et["Jjmag"][e].astype(dt)
    w, r, Jz = et["w"], np.where(et["mask"][:, None], et["r"], _c(0, dt)), et["Jz"]
    rm, Jzm = np.where(et["mask"][:, None], et["rmag"], 0).astype(dt), et["Jzmag"].astype(dt)
    a2, am2, w2 = a.reshape(2 * E_, n6), am.reshape(2 * E_, n6), w.reshape(-1, 1)
    B = a2.T @ (a2 * w2)
    Bmag = am2.T @ (am2 * w2)
    v = np.einsum("er,er,era->a", w, r, a)
    vmag = np.einsum("er,er,era->a", w, np.abs(r), am)
    vrmag = np.einsum("er,er,era->a", w, rm, am)
    Em, Emag = np.zeros((Mu, n6), dt), np.zeros((Mu, n6), dt)
    C, u, umag, urmag = np.zeros(Mu, dt), np.zeros(Mu, dt), np.zeros(Mu, dt), np.zeros(Mu, dt)
    np.add.at(Em, kinv, np.einsum("er,er,era->ea", w, Jz, a))
    np.add.at(Emag, kinv, np.einsum("er,er,era->ea", w, Jzm, am))
    np.add.at(C, kinv, (w * Jz * Jz).sum(1))
    np.add.at(u, kinv, (w * r * Jz).sum(1))
    np.add.at(umag, kinv, (w * np.abs(r) * Jzm).sum(1))
    np.add.at(urmag, kinv, (w * rm * Jzm).sum(1))
    has_prior = np.zeros(Mu, bool)
    if est is not None and mu > 0:
        e_k, d_k = _c(est, dt)[ku], _c(d_centre, dt)[ku]
        with np.errstate(invalid="ignore"):
            has_prior = (e_k > 0) & (e_k < np.inf)
        m_ = _c(mu, dt)
        C = C + np.where(has_prior, m_, _c(0, dt))
        u = u - np.where(has_prior, m_ * (d_k - np.where(has_prior, e_k, 0)), _c(0, dt))
        umag = umag + np.where(has_prior, m_ * (np.abs(d_k) + np.abs(np.where(has_prior, e_k, 0))), _c(0, dt))
    Q = _c(1, dt) / (C + _c(lmbda, dt))
    EQ = Em * Q[:, None]
    S = B - EQ.T @ Em
    y = v - EQ.T @ u
    Smag = Bmag + (Emag * Q[:, None]).T @ Emag
    ymag = vmag + (Emag * Q[:, None]).T @ umag
    yrmag = vrmag + (Emag * Q[:, None]).T @ urmag
    dg = np.arange(n6)
    damp = _c(1e-4, np.float32).astype(dt) * S[dg, dg] + _c(1, dt)
    Smag[dg, dg] += np.abs(damp)
    S = S.copy()
    S[dg, dg] += damp
    return dict(B=B, E=Em, C=C, v=v, u=u, Q=Q, S=S, y=y, Smag=Smag, ymag=ymag, yrmag=yrmag, Emag=Emag, umag=umag, urmag=urmag,
                ku=ku,
                kinv=kinv, has_prior=has_prior, n6=n6)


def depth_update(d0, dZ, dtype=np.float64):
    d = d0 + dZ
    d = np.where(d > _c(20, dtype), _c(1, dtype), d)
    return np.maximum(d, _c(1e-4, np.float32).astype(dtype))


def step(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, est=None, mu=0.0,
         dtype=np.float64):
    """One Gauss-Newton step -> dict(dX [N, 6], dZ [Mu], poses, patches, et, ne, pre)
    (pre: depth[pixel 0] + dZ before the clamp)."""
    dt = dtype
    P = patches.shape[-1]
    poses = _c(poses, dt).reshape(-1, 7)
    patches = _c(patches, dt).reshape(-1, 3, P, P)
    et = edge_terms(poses, patches, intrinsics, target, weight, ii, jj, kk, t0, t1, dt)
    flat = patches.reshape(-1, 3, P * P)
    est_c = None if est is None else np.asarray(est).reshape(-1, 3, P * P)[:, 2, centre_index(P)]
    ne = normal_equations(et, kk, lmbda, flat[:, 2, centre_index(P)], est_c, mu, dt)
    N = t1 - t0
    if N > 0:
        dX = np.linalg.solve(ne["S"], ne["y"]).astype(dt)
        dZ = ne["Q"] * (ne["u"] - ne["E"] @ dX)
    else:
        dX = np.zeros(0, dt)
        dZ = ne["Q"] * ne["u"]
    new_poses = poses.copy()
    if N > 0:
        new_poses[t0:t1] = retract(poses[t0:t1], dX.reshape(N, 6))
    pre = flat[ne["ku"], 2, 0] + dZ
    new_patches = patches.copy()
    new_patches[ne["ku"], 2] = depth_update(flat[ne["ku"], 2, 0], dZ, dt)[:, None, None]
    return dict(dX=dX.reshape(N, 6), dZ=dZ, poses=new_poses, patches=new_patches, et=et, ne=ne, pre=pre)


def float32_step(*args, **kw):
    """`step` with every array and every operation in numpy float32: shows on
    the CPU that the bars leave room for honest fp32 arithmetic"""
    return step(*args, dtype=np.float32, **kw)


# ---------------------------------------------------------------------------
# the bars
def step_errors(sc, ref, poses_out, patches_out, path, t0, t1):
    """The worst ratios error / bar of a one-step result against `ref` =
    step(...) of the same inputs: dict(pose, depth, quat) plus the pieces."""
    ne = ref["ne"]
    N, n6, ku = t1 - t0, ne["n6"], ne["ku"]
    P = patches_out.shape[-1]
    p_in = np.asarray(sc["poses"], np.float64)
    p_out = np.asarray(poses_out, np.float64)
    G = len(ku)
    et = ref["et"]
    pose_of = np.concatenate([et["ix"][et["iv"]], et["jx"][et["jv"] & ~et["self"]]])
    patch_of = np.concatenate([ne["kinv"][et["iv"]], ne["kinv"][et["jv"] & ~et["self"]]])
    edges = int(np.bincount(pose_of, minlength=1).max()) if N > 0 else 0
    patches = int(np.bincount(np.unique(pose_of * G + patch_of) // G, minlength=1).max()) if N > 0 else 0
    out = dict(k=k_pose(path, n6, edges, patches, G))
    xi = np.zeros(0)
    dxi = np.zeros(0)
    if N > 0:
        xi = tangent(p_out[t0:t1], p_in[t0:t1]).reshape(-1)
        Jt = tangent_sensitivity(p_out[t0:t1], p_in[t0:t1])
        tm = np.abs(p_in[t0:t1, :3]).sum(1, keepdims=True) + np.abs(p_out[t0:t1, :3])
        pmag = np.concatenate([tm, np.ones((N, 4))], 1)
        dxi = (K_RETR * EPS * np.einsum("nas,ns->na", Jt, pmag)).reshape(-1)
        S, dg = ne["S"], np.sqrt(np.diag(ne["S"]))
        M = np.maximum(ne["Smag"], np.outer(dg, dg))
        res = np.abs(S @ xi - ne["y"])
        bar = out["k"] * EPS * (M @ np.abs(xi) + ne["ymag"]) + K_R * EPS * ne["yrmag"] + np.abs(S) @ dxi
        out.update(pose=float((res / bar).max()), pose_row=int((res / bar).argmax()), res=res, bar=bar)
        qn = np.abs(np.linalg.norm(p_out[t0:t1, 3:], axis=1) - 1.0)
        out["quat"] = float(qn.max() / (4 * EPS))
    else:
        out.update(pose=0.0, quat=0.0)
    flat_in = np.asarray(sc["patches"], np.float64).reshape(-1, 3, P * P)
    d0 = flat_in[ku, 2, 0]
    dZ = ne["Q"] * (ne["u"] - (ne["E"] @ xi if N > 0 else 0.0))
    want = depth_update(d0, dZ)
    got = np.asarray(patches_out, np.float64).reshape(-1, 3, P * P)[ku, 2, 0]
    cnt = np.bincount(ne["kinv"], minlength=G)
    kz = k_depth(n6, cnt)
    zbar = kz * EPS * (ne["Q"] * ne["umag"] + (ne["Q"][:, None] * ne["Emag"]) @ np.abs(xi) + np.abs(d0))
    zbar = zbar + K_R * EPS * ne["Q"] * ne["urmag"]
    if N > 0:
        zbar = zbar + (ne["Q"][:, None] * np.abs(ne["E"])) @ dxi
    zerr = np.abs(got - want)
    out.update(depth=float((zerr / zbar).max()), depth_patch=int(ku[(zerr / zbar).argmax()]), xi=xi, dZ=dZ,
               clamp_pre=d0 + dZ)
    return out


# ---------------------------------------------------------------------------
# the scene builder
def _patches_for(P, px, py, d0, dc, dr):
    """[n, 3, P, P]: integer-offset x / y around the centre; depth d0 at pixel
    0, dc at the centre, dr elsewhere (P = 1: the one pixel is both: dc)"""
    n = len(px)
    off = np.arange(P) - P // 2
    pa = np.zeros((n, 3, P, P))
    pa[:, 0] = px[:, None, None] + off[None, None, :]
    pa[:, 1] = py[:, None, None] + off[None, :, None]
    pa[:, 2] = dr[:, None, None]
    pa[:, 2, 0, 0] = d0
    pa[:, 2, P // 2, P // 2] = dc
    return pa


def _place(poses, intr, i, j, d, want, start=None):
    """patch centre (px, py) in frame i whose point at inverse depth d projects
    to `want` in frame j: X - u Z = 0, Y - v Z = 0 are linear in the ray"""
    fx, fy, cx, cy = intr
    qij = _qmul(poses[j, 3:], _qconj(poses[i, 3:]))
    R = _rotmat(qij)
    t = (poses[j, :3] - _act(qij, poses[i, :3])) * d
    u, v = (want[0] - cx) / fx, (want[1] - cy) / fy
    A = np.stack([R[0] - u * R[2], R[1] - v * R[2]])
    b = -np.array([t[0] - u * t[2], t[1] - v * t[2]])
    xn = np.linalg.solve(A[:, :2], b - A[:, 2])
    return np.array([xn[0] * fx + cx, xn[1] * fy + cy])


CLASSES = ("self", "i_fixed", "j_fixed", "both_fixed", "repeated", "single_edge", "all_masked", "zero_weight",
           "unreferenced")


def make_scene(seed, N, n=None, M=6, P=3, lmbda=1e-4, span=None, well_conditioned=False):
    """A seeded BA state over the window [n - N, n) on top of
    tests_helpers.dpvo_frames / with_edges: n frames (default max(14, N + 2)),
    M patches per frame, depth non-uniform inside every patch, stated numbers
    of every edge class and edges on both sides of every mask and clamp
    condition; every margin at least REL_MARGIN (closer base edges are re-drawn).
    span: the widest |i - j| of a base edge (None: 6).  well_conditioned: base
    edges only (the oracle comparison).  -> dict of float32 / int64 arrays plus
    `classes` (edge ids or patch ids per class) and `sides`."""
    from tests_helpers import dpvo_frames, with_edges
    n = n or max(14, N + 2)
    t0, t1 = n - N, n
    span = span or 6
    g, poses, patches, intrinsics = dpvo_frames(seed, n, M)
    intr = intrinsics[0]
    fx, fy, cx, cy = intr
    # frame 1 and the last frame relative to frame 0 by design: a sideways step
    # (the clamp patches' depth gradient) and a step towards the points (Z =
    # 0.1 / 0.4; the last frame is optimised in every window, so an edge the
    # mask should have dropped shows in the pose rows)
    q1 = np.array([0.005, -0.004, 0.003, 0.0]); q1[3] = np.sqrt(1 - (q1[:3] ** 2).sum())
    q2 = np.array([-0.004, 0.006, 0.002, 0.0]); q2[3] = np.sqrt(1 - (q2[:3] ** 2).sum())
    poses[0] = [0, 0, 0, 0, 0, 0, 1]
    poses[1] = np.concatenate([[0.05, 0.01, 0.0], q1])
    poses[n - 1] = np.concatenate([[0.02, 0.01, -0.15], q2])
    poses = poses.astype(np.float32).astype(np.float64)
    npat = n * M
    px, py = patches[:, 0, 1, 1].copy(), patches[:, 1, 1, 1].copy()
    dc = patches[:, 2, 1, 1].copy()
    # the patches' frame (patch k lives in frame k // M) and base edges
    frame = np.arange(npat) // M
    ii, jj, kk = [], [], []
    for k in range(npat):
        f = frame[k]
        js = [j for j in range(max(0, f - span // 2), min(n, f + span - span // 2 + 1)) if j != f]
        for j in js:
            ii.append(f); jj.append(j); kk.append(k)
    ii, jj, kk = (np.asarray(a, np.int64) for a in (ii, jj, kk))
    # reserved patches: the last frames' spare patches serve the special cases
    sign = np.where(g.random(npat) < 0.5, -1.0, 1.0)
    d0 = dc * (1 + sign * g.uniform(0.1, 0.3, npat))
    dr = dc * (1 - sign * g.uniform(0.1, 0.3, npat))
    classes = {c: [] for c in CLASSES}
    sides = {}
    spec = []   # (i, j, k, target xy or None, weight)

    def reserve(count):
        """patches taken out of the base edges, one per frame in turn"""
        nonlocal ii, jj, kk
        free = [k for k in sorted(range(npat), key=lambda k: (k % M, k)) if k not in reserved]
        take = free[:count]
        reserved.update(take)
        keep = ~np.isin(kk, take)
        ii, jj, kk = ii[keep], jj[keep], kk[keep]
        return take
    reserved = set()
    if not well_conditioned:
        need = 2 + 2 + 8 + 4 + 2
        assert need <= npat // 2, "scene too small for its special patches"
        # unreferenced
        classes["unreferenced"] = reserve(2)
        # Z = 0.1 / 0.4 along the designed approach 0 -> n - 1
        for zt, name in ((0.1, "Z_out"), (0.4, "Z_in")):
            k, = reserve(1)
            c0 = project(poses, np.array([cx]), np.array([cy]), np.array([0.0]), intr, [0], [n - 1])[1][0]
            tz = (project(poses, np.array([cx]), np.array([cy]), np.array([1.0]), intr, [0], [n - 1])[1][0] - c0)
            dc[k] = (zt - c0) / tz
            d0[k], dr[k] = dc[k] * 1.2, dc[k] * 0.85
            px[k], py[k] = _place(poses, intr, 0, n - 1, dc[k], (cx, cy), (cx, cy))
            dc[k] = (zt - project(poses, px[k:k + 1], py[k:k + 1], np.array([0.0]), intr, [0], [n - 1])[1][0]) / tz
            px[k], py[k] = _place(poses, intr, 0, n - 1, dc[k], (cx, cy), (px[k], py[k]))
            spec.append((0, n - 1, k, (cx + 0.7, cy - 0.4), (0.8, 0.6)))
            sides[name] = len(spec) - 1
        # projections 30 and 100 px outside every border, edge 0 -> 1
        W_, H_ = 2 * cx, 2 * cy
        for name, want in (("x_lo_in", (-30, cy)), ("x_lo_out", (-100, cy)), ("x_hi_in", (W_ + 30, cy)),
                           ("x_hi_out", (W_ + 100, cy)), ("y_lo_in", (cx, -30)), ("y_lo_out", (cx, -100)),
                           ("y_hi_in", (cx, H_ + 30)), ("y_hi_out", (cx, H_ + 100))):
            k, = reserve(1)
            dc[k] = 0.6; d0[k] = 0.72; dr[k] = 0.5
            px[k], py[k] = _place(poses, intr, 0, 1, dc[k], want, want)
            spec.append((0, 1, k, (want[0] + 0.6, want[1] - 0.8), (0.7, 0.9)))
            sides[name] = len(spec) - 1
        # clamp: single both-fixed edge 0 -> 1, the target set so that Q u lands the depth at `land`
        for name, start, land in (("hi_reset", 19.0, 21.5), ("hi_keep", 19.0, 19.5), ("lo_floor", 0.05, -0.05),
                                  ("lo_keep", 0.05, 0.03)):
            k, = reserve(1)
            d0[k] = start
            dc[k] = start / 1.2 if P > 1 else start
            dr[k] = dc[k] * 0.8
            px[k], py[k] = _place(poses, intr, 0, 1, dc[k], (cx, cy), (cx, cy))
            spec.append((0, 1, k, ("land", land - start), (1.0, 1.0)))
            sides[name] = len(spec) - 1
        # all edges masked: residual 200 px on both edges of two patches
        for _ in range(2):
            k, = reserve(1)
            classes["all_masked"].append(k)
            px[k], py[k] = cx + g.uniform(-10, 10), cy + g.uniform(-10, 10)
            for j in (1, 2):
                spec.append((0, j, k, ("off", 200.0), (0.5, 0.5)))
    # the base edges' targets and weights (tests_helpers.with_edges)
    base = _patches_for(3, px, py, d0, dc, dr)
    for attempt in range(20):
        sc = with_edges(g, n, M, poses, base, intrinsics, ii, jj, kk)
        tgt, wgt = sc["target"][0].astype(np.float64), sc["weight"][0].astype(np.float64)
        et = edge_terms(poses.astype(np.float32), base.astype(np.float32), intr.astype(np.float32), tgt, wgt, ii, jj,
                        kk, t0, t1)
        bad = (min_relative_margin(et) < REL_MARGIN) | ~et["mask"] | (et["Z"] < 0.45)
        if not bad.any():
            break
        ii, jj, kk = ii[~bad], jj[~bad], kk[~bad]   # re-drawn: the edge leaves, the rest get new noise
    else:
        raise AssertionError("no base edge set with the margins")
    if not well_conditioned:
        E0 = len(ii)
        pick = lambda cond, cnt: list(g.choice(np.flatnonzero(cond), cnt, replace=False))
        iv, jv = et["iv"], et["jv"]
        if N > 0:
            # residual 90 / 200 px on base edges inside the window
            both = np.flatnonzero(iv | jv)
            e90, e200 = g.choice(both, 4, replace=False).reshape(2, 2)
            for e, rr in [(e, 90.0) for e in e90] + [(e, 200.0) for e in e200]:
                ang = g.uniform(0, 2 * np.pi)
                tgt[e] = et["x1"][e] + rr * np.array([np.cos(ang), np.sin(ang)])
            sides["r_in"], sides["r_out"] = list(e90), list(e200)
        # zero weights: both rows on three edges, one row on two
        zw = pick(np.ones(E0, bool), 5)
        wgt[zw[:3]] = 0.0
        wgt[zw[3:], 0] = 0.0
        classes["zero_weight"] = zw
        # repeated (k, j): three base edges again, new noise
        rep = pick(np.ones(E0, bool), 3)
        # self edges: three patches of window frames (N = 0: of any frame)
        own = np.flatnonzero((frame >= t0) & ~np.isin(np.arange(npat), list(reserved))) if N > 0 else \
            np.flatnonzero(~np.isin(np.arange(npat), list(reserved)))
        selfk = list(g.choice(own, 3, replace=False))
        # edges whose frame i is not the patch's own: i fixed / j fixed / both fixed by construction
        add = [(int(ii[e]), int(jj[e]), int(kk[e])) for e in rep] + [(int(frame[k]), int(frame[k]), int(k)) for k in selfk]
        free = [k for k in range(npat) if k not in reserved]
        if N > 0:
            for _ in range(3):
                k = int(g.choice(free))
                add.append((int(g.integers(0, t0)), int(g.integers(t0, t1)), k))                   # i fixed
                add.append((int(g.integers(t0, t1)), int(g.integers(0, t0)), int(g.choice(free))))  # j fixed
                i_, j_ = g.choice(t0, 2, replace=False)
                add.append((int(i_), int(j_), int(g.choice(free))))                              # both fixed
        ai, aj, ak = (np.asarray([a[c] for a in add], np.int64) for c in range(3))
        if span < 6 and N > 0:
            # narrow band: keep every added edge within the patch's own span
            ok = (np.abs(ai - frame[ak]) <= 1) & (np.abs(aj - frame[ak]) <= 2) | (ai < t0) & (aj < t0)
            ok[:6] = True
            ai, aj, ak = ai[ok], aj[ok], ak[ok]
        si, sj, sk = (np.asarray([s[c] for s in spec], np.int64) for c in range(3))
        ii2 = np.concatenate([ii, ai, si])
        jj2 = np.concatenate([jj, aj, sj])
        kk2 = np.concatenate([kk, ak, sk])
        # targets of the added edges: the fp64 projection + noise
        pr, _ = project(poses, px[ak], py[ak], dc[ak], intr, ai, aj)
        tgt_a = pr + g.normal(0, 1.0, pr.shape)
        wgt_a = g.uniform(0.1, 1.0, pr.shape)
        prs, _ = project(poses, px[sk], py[sk], dc[sk], intr, si, sj)
        tgt_s, wgt_s = np.zeros_like(prs), np.zeros_like(prs)
        for x, s in enumerate(spec):
            wgt_s[x] = s[4]
            if s[3][0] == "off":
                ang = g.uniform(0, 2 * np.pi)
                tgt_s[x] = prs[x] + s[3][1] * np.array([np.cos(ang), np.sin(ang)])
            elif s[3][0] == "land":
                e1 = edge_terms(poses, _patches_for(3, px, py, d0, dc, dr), intr, np.zeros((1, 2)), np.ones((1, 2)),
                                [s[0]], [s[1]], [s[2]], t0, t1)
                Jz = e1["Jz"][0]
                C = (Jz * Jz).sum()
                tgt_s[x] = prs[x] + Jz * s[3][1] * (C + lmbda) / C
            else:
                tgt_s[x] = s[3]
        ii, jj, kk = ii2, jj2, kk2
        tgt = np.concatenate([tgt, tgt_a, tgt_s])
        wgt = np.concatenate([wgt, wgt_a, wgt_s])
        sides = {k_: (v + E0 + len(ai) if isinstance(v, int) else v) for k_, v in sides.items()}
        classes["repeated"] = list(range(E0, E0 + 3))
    out = dict(n=n, M=M, P=P, t0=t0, t1=t1, lmbda=lmbda, poses=poses.astype(np.float32),
               patches=_patches_for(P, px, py, d0, dc, dr).astype(np.float32),
               intrinsics=intrinsics.astype(np.float32), ii=ii, jj=jj, kk=kk,
               target=tgt.astype(np.float32)[None], weight=wgt.astype(np.float32)[None], sides=sides)
    # the classes as they stand in the final edge list
    et = edge_terms(out["poses"], out["patches"], out["intrinsics"], out["target"], out["weight"], ii, jj, kk, t0, t1)
    cnt = np.bincount(kk, minlength=npat)
    alive = np.bincount(kk, weights=et["mask"].astype(float), minlength=npat)
    classes.update(self=list(np.flatnonzero(ii == jj)), i_fixed=list(np.flatnonzero(~et["iv"] & et["jv"])),
                   j_fixed=list(np.flatnonzero(et["iv"] & ~et["jv"])),
                   both_fixed=list(np.flatnonzero(~et["iv"] & ~et["jv"])),
                   single_edge=list(np.flatnonzero(cnt == 1)),
                   all_masked=list(np.flatnonzero((cnt > 0) & (alive == 0))),
                   zero_weight=list(np.flatnonzero((out["weight"][0] == 0).any(1))),
                   unreferenced=list(np.flatnonzero(cnt == 0)))
    pairs = {}
    for e in range(len(kk)):
        pairs.setdefault((int(kk[e]), int(jj[e])), []).append(e)
    classes["repeated"] = [e for v in pairs.values() if len(v) > 1 for e in v]
    out["classes"] = classes
    out["min_margin"] = float(min_relative_margin(et).min())
    out["masked_share"] = float((~et["mask"]).mean())
    return out


def scene_args(sc):
    return (sc["poses"], sc["patches"], sc["intrinsics"], sc["target"], sc["weight"], sc["lmbda"], sc["ii"], sc["jj"],
            sc["kk"], sc["t0"], sc["t1"])


def make_prior(sc, seed=0):
    """A prior on every other referenced patch (centre depth x U[0.7, 1.3]) with
    the invalid values 0, -1, +inf and NaN mixed in -> (est like patches,
    the same with every invalid value replaced by 0)"""
    g = np.random.default_rng(seed)
    pa = sc["patches"]
    P = pa.shape[-1]
    est = np.zeros_like(pa)
    ku = np.unique(sc["kk"])
    on = ku[::2]
    est[on, 2] = (pa[on, 2, P // 2, P // 2] * g.uniform(0.7, 1.3, len(on)).astype(np.float32))[:, None, None]
    clean = est.copy()
    bad = ku[1::2][:8]
    for k, val in zip(bad, [0.0, -1.0, np.inf, np.nan] * 2):
        est[k, 2] = val
    return est, clean


def make_damping_scene(seed=0, n=14, M=6, P=3, delta=0.4):
    """One optimised pose (the last frame) seen from fixed frames only, the
    depths frozen by lmbda = 1e8, the targets the exact projections under that
    pose shifted by `delta` along x: r = Jj[:, 0] delta exactly, so y = B e_0
    delta and the step is e_0 delta up to the damping.  Row 0 of S xi = y is
    then S_00 xi_0 against y_0 alone -- no Schur cancellation, no other
    column -- and the damping's 1e-4 S_00 xi_0 stands several bars out."""
    from tests_helpers import dpvo_frames
    g, poses, patches, intrinsics = dpvo_frames(seed, n, M)
    poses = poses.astype(np.float32).astype(np.float64)
    intr = intrinsics[0]
    npat = n * M
    px, py = patches[:, 0, 1, 1].copy(), patches[:, 1, 1, 1].copy()
    dc = g.uniform(1.0, 2.0, npat)
    sign = np.where(g.random(npat) < 0.5, -1.0, 1.0)
    d0, dr = dc * (1 + sign * g.uniform(0.1, 0.3, npat)), dc * (1 - sign * g.uniform(0.1, 0.3, npat))
    kk = np.arange((n - 5) * M, (n - 1) * M, dtype=np.int64)
    ii, jj = kk // M, np.full(len(kk), n - 1, np.int64)
    moved = poses.copy()
    moved[n - 1] = retract(poses[n - 1:n], np.array([[delta, 0, 0, 0, 0, 0.0]]))[0]
    tgt, Z = project(moved, px[kk], py[kk], dc[kk], intr, ii, jj)
    wgt = g.uniform(0.5, 1.0, tgt.shape)
    out = dict(n=n, M=M, P=P, t0=n - 1, t1=n, lmbda=1e8, poses=poses.astype(np.float32),
               patches=_patches_for(P, px, py, d0, dc, dr).astype(np.float32), intrinsics=intrinsics.astype(np.float32),
               ii=ii, jj=jj, kk=kk, target=tgt.astype(np.float32)[None], weight=wgt.astype(np.float32)[None], sides={},
               classes={})
    et = edge_terms(out["poses"], out["patches"], out["intrinsics"], out["target"], out["weight"], ii, jj, kk, n - 1, n)
    out["min_margin"] = float(min_relative_margin(et).min())
    out["masked_share"] = float((~et["mask"]).mean())
    return out


# ---------------------------------------------------------------------------
# the cases of tests/test_gpu_ba_step.py, shared with the CPU proof of the bars
# (tests/test_ba_ref_host.py): (id, path, scene arguments, prior mu or 0)
PATH_FLAGS = {"det": 0, "band": 1, "atomic": 2}


def step_cases():
    c = []
    for N in range(0, 13):
        c.append((f"det-N{N}", "det", dict(seed=N, N=N), 0.0))
    for P in (1, 5):
        c.append((f"det-P{P}", "det", dict(seed=20 + P, N=4, P=P), 0.0))
    c.append(("det-2098-patches", "det", dict(seed=30, N=10, M=150), 0.0))
    for N in (1, 10, 11, 12, 13, 16, 17):
        c.append((f"atomic-N{N}", "atomic", dict(seed=40 + N, N=N), 0.0))
    c.append(("band-N10", "band", dict(seed=60, N=10), 0.0))
    c.append(("band-N16", "band", dict(seed=61, N=16), 0.0))
    c.append(("band-N40-narrow", "band", dict(seed=62, N=40, span=3), 0.0))
    for path, N in (("det", 7), ("atomic", 12), ("band", 16)):
        for lm in (1e-4, 0.5):
            c.append((f"{path}-lmbda{lm:g}", path, dict(seed=70 + N, N=N, lmbda=lm), 0.0))
        for mu in (0.5, 2.0):
            c.append((f"{path}-prior{mu:g}", path, dict(seed=80 + N, N=N), mu))
        c.append((f"{path}-damping", path, dict(damping=True), 0.0))
    return c


_SCENES = {}


def case_scene(kw):
    """the (cached, never modified) scene of a case and its fp64 step"""
    key = tuple(sorted(kw.items()))
    if key not in _SCENES:
        kw = dict(kw)
        sc = make_damping_scene() if kw.pop("damping", False) else make_scene(**kw)
        for v in sc.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SCENES[key] = sc
    return _SCENES[key]


def distance(a, b, sc):
    """(pose distance over the window, relative depth distance) of two (poses, patches) states"""
    t0, t1 = sc["t0"], sc["t1"]
    pa, pb = (np.asarray(x[0], np.float64)[t0:t1] for x in (a, b))
    qa, qb = (np.asarray(x[1], np.float64)[:, 2] for x in (a, b))
    return np.linalg.norm(pa - pb), np.linalg.norm(qa - qb) / np.linalg.norm(qb)


def two_steps(sc, dtype=np.float64):
    """`step` applied twice -> (poses, patches)"""
    args = list(scene_args(sc))
    for _ in range(2):
        s = step(*args, dtype=dtype)
        args[0], args[1] = s["poses"], s["patches"]
    return s["poses"], s["patches"]


# (path, scene): the atomic path's scene is the one of three measured whose
# iterations-2-against-two-calls distance, which varies from run to run with
# the order of the atomics, stays furthest below its bar (NOTES.md)
TWO_STEP_CASES = [("det", dict(seed=97, N=7)), ("atomic", dict(seed=5, N=12)), ("band", dict(seed=106, N=16))]
