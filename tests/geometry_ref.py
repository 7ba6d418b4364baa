"""fp64 restatement of the projective kernels (csrc/geometry.hip, the keyframe
distance matrix among them) with the error companions their tests are held
to.  Plain numpy, no GPU, no oracle: it follows dpvo/projective_ops.py and the
header comments of include/dpvo_hot.h, with rotation matrices instead of the
kernels' quaternion products, so it shares no statement order with the code
under test.

With unit quaternions (the inputs are normalised here, as on every load there):

    R_ij = R_j R_i^T              t_ij = t_j - R_ij t_i
    (tonly: R_ij := I for the rotation of the ray only; t_ij keeps the rotated form)
    a = ((px - cx_i) / fx_i, (py - cy_i) / fy_i, 1)
    X = R_ij a + t_ij d           Zc = max(Z, 0.1)
    x = fx_j X_x / Zc + cx_j      y likewise            depth = 1 / Zc

Every float output comes with a companion S: EPS = 2^-24 times the sum of the
magnitudes that one fp32 rounding can act on,

    A   = |R_ij| |a| + (|t_j| + |R_ij| |t_i|) d
    S_x = EPS [ fx_j (A_x + |X_x| A_z / Zc) / Zc + |x| + |cx_j| ]      (S_y likewise)
    S_d = EPS ( A_z / Zc^2 + 1 / Zc )

and the bar of an output is k S, k being the number of fp32 rounding steps on
the longest dependent path through the kernel's arithmetic.  Counted from
liegroups.hpp / geometry.hip (the file is built without fast-math: / and sqrtf
round correctly, FMA contraction only removes steps; doubling, negation and the
conjugate are exact):

    load + normalise q_i     x*x, three adds, sqrt, divide               6
    inverse                  conjugate, normalise again                 +6 = 12
      its translation        -R(q^-1) t: qact = uv (mul, sub), y*uv2,
                             sub, final add                             +5 = 17
    compose, rotation        qmul (mul, three adds) then normalise      +4 +6 = 22
    compose, translation     R(q_j) t_inv (qact, +5 on 17), t_j + ..    +1 = 23
    rotate the ray           qact with q_ij                             +5 = 27
    translate                t_ij * d is at 24; the add                 +1 = 28   -> Z:  K_Z  = 28
    divide                   1 / max(Z, 0.1)                            +1 = 29   -> d:  K_D  = 29
    scale                    d * X, fx *, + cx                          +3 = 32   -> xy: K_XY = 32

A count that let the errors of both factors of every product add up (the
quaternion enters its own sandwich twice) would come to about 52; the path
count is the tighter of the two and the one the tests use.  Observed ratios are
recorded in profiles/geometry_tests/NOTES.md.

The point cloud stops after the inverse:  X = R_i^T a + (-R_i^T t_i) d, w = d,
A_pc = |R_i^T| |a| + |R_i^T| |t_i| d, the rotation at 12 + 5, the translated
term at 17 + 1, the add: K_PC = 19, and the centre's division by w: K_PC + 1.

flow_mag = beta |x1 - x0| + (1 - beta) |x2 - x0| (x0 = transform(ii, ii),
x2 = tonly): each norm moves by at most the sum of its two coordinate
differences' bounds, so S_f = beta (S_x1 + S_x0 + S_y1 + S_y0) + (1 - beta)
(the same with x2); the norm's own steps (sub, square, add, sqrt, times beta,
add) act on values no larger than those magnitudes: K_FLOW = K_XY + 6.  A mean
of flows is held to K_FLOW mean(S_f) + steps EPS mean|f|, steps = the adds one
thread makes plus the tree's depth (`mean_steps`).
"""
import numpy as np

EPS = 2.0 ** -24
K_Z, K_D, K_XY = 28, 29, 32
K_PC = 19
K_FLOW = K_XY + 6


# ---------------------------------------------------------------------------
# groups
def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def rotmat(q):
    """[.., 4] (x, y, z, w) -> [.., 3, 3], normalising first."""
    x, y, z, w = np.moveaxis(_unit(q), -1, 0)
    R = np.empty(x.shape + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def se3_exp(xi):
    """[n, 6] tangents (tau, phi) -> [n, 7] poses (t, q)."""
    xi = np.asarray(xi, np.float64)
    tau, phi = xi[:, :3], xi[:, 3:]
    th = np.linalg.norm(phi, axis=1)
    out = np.zeros((len(xi), 7))
    for r in range(len(xi)):
        t, p = th[r], phi[r]
        K = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        if t < 1e-9:
            im, J = 0.5, np.eye(3) + 0.5 * K
        else:
            im = np.sin(0.5 * t) / t
            J = np.eye(3) + (1 - np.cos(t)) / t ** 2 * K + (t - np.sin(t)) / t ** 3 * (K @ K)
        out[r, :3] = J @ tau[r]
        out[r, 3:6] = im * p
        out[r, 6] = np.cos(0.5 * t)
    return out


# ---------------------------------------------------------------------------
# the scene
def make_scene(P, seed=0, n=12, M=8, E=3000):
    """Poses that put a fifth of the pixels behind or too close to the target
    camera, quaternions off unit norm, per-frame intrinsics, integer-offset
    patches; float32, as the kernels and the restatement both see it."""
    rng = np.random.default_rng(seed)
    xi = np.concatenate([0.4 * rng.standard_normal((n, 3)), 0.35 * rng.standard_normal((n, 3))], 1)
    xi[n - 2, 3:] = (0.0, 3.0, 0.0)
    poses = se3_exp(xi)
    poses[n - 1, 2] = -2.5
    scale = rng.uniform(0.5, 2.0, n)
    scale[::3] = 1.0
    poses[:, 3:] *= scale[:, None]
    intr = np.stack([rng.uniform(200, 500, n), rng.uniform(200, 500, n), rng.uniform(150, 330, n),
                     rng.uniform(100, 250, n)], 1)
    f = np.repeat(np.arange(n), M)
    cx = rng.uniform(0, 2 * intr[f, 2])
    cy = rng.uniform(0, 2 * intr[f, 3])
    d = np.exp(rng.uniform(np.log(0.02), np.log(4.0), n * M))
    off = np.arange(P) - P // 2
    patches = np.empty((n * M, 3, P, P))
    patches[:, 0] = cx[:, None, None] + off[None, None, :]
    patches[:, 1] = cy[:, None, None] + off[None, :, None]
    patches[:, 2] = d[:, None, None]
    kk = rng.integers(0, n * M, E)
    jj = rng.integers(0, n, E)
    return dict(poses=poses.astype(np.float32), patches=patches.astype(np.float32),
                intrinsics=intr.astype(np.float32), ii=(kk // M).astype(np.int64), jj=jj.astype(np.int64),
                kk=kk.astype(np.int64), ix=f.astype(np.int64), n=n, M=M, P=P)


# ---------------------------------------------------------------------------
# transform
def transform(poses, patches, intrinsics, ii, jj, kk, depth=False, tonly=False):
    """dict: coords [E, P, P, 2|3], Z [E, P, P] (before the clamp), valid,
    S [E, P, P, 2|3] (the coords' companions) and Az (Z's own magnitude sum)."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    P = patches.shape[-1]
    pa = np.asarray(patches, np.float64).reshape(-1, 3, P, P)[kk]
    K = np.asarray(intrinsics, np.float64).reshape(-1, 4)
    R = rotmat(poses[:, 3:])
    t = poses[:, :3]
    Rij = R[jj] @ np.swapaxes(R[ii], -1, -2)
    tij = t[jj] - np.einsum("erc,ec->er", Rij, t[ii])
    tmag = np.abs(t[jj]) + np.einsum("erc,ec->er", np.abs(Rij), np.abs(t[ii]))
    Rray = np.broadcast_to(np.eye(3), Rij.shape) if tonly else Rij
    ki, kj = K[ii][:, :, None, None], K[jj][:, :, None, None]
    a = np.stack([(pa[:, 0] - ki[:, 2]) / ki[:, 0], (pa[:, 1] - ki[:, 3]) / ki[:, 1], np.ones_like(pa[:, 2])], -1)
    d = pa[:, 2][..., None]
    X = np.einsum("erc,epqc->epqr", Rray, a) + tij[:, None, None, :] * d
    A = np.einsum("erc,epqc->epqr", np.abs(Rray), np.abs(a)) + tmag[:, None, None, :] * d
    Z = X[..., 2]
    Zc = np.maximum(Z, 0.1)
    x = kj[:, 0] * X[..., 0] / Zc + kj[:, 2]
    y = kj[:, 1] * X[..., 1] / Zc + kj[:, 3]
    Az = A[..., 2]
    Sx = EPS * (kj[:, 0] * (A[..., 0] + np.abs(X[..., 0]) * Az / Zc) / Zc + np.abs(x) + np.abs(kj[:, 2]))
    Sy = EPS * (kj[:, 1] * (A[..., 1] + np.abs(X[..., 1]) * Az / Zc) / Zc + np.abs(y) + np.abs(kj[:, 3]))
    coords, S = [x, y], [Sx, Sy]
    if depth:
        coords.append(1.0 / Zc)
        S.append(EPS * (Az / Zc ** 2 + 1.0 / Zc))
    return dict(coords=np.stack(coords, -1), S=np.stack(S, -1), Z=Z, Az=Az, valid=(Z > 0.2).astype(np.float64))


def coords_bar(r):
    """k S per output channel of transform()'s result"""
    k = np.array([K_XY, K_XY, K_D][:r["coords"].shape[-1]], np.float64)
    return k * r["S"]


def valid_undecided(r):
    """pixels whose Z is within its own bound of the 0.2 threshold: either flag is right"""
    return np.abs(r["Z"] - 0.2) <= K_Z * EPS * r["Az"]


# ---------------------------------------------------------------------------
# point cloud
def point_cloud(poses, patches, intrinsics, ix):
    """full [m, P, P, 4] with S [m, P, P, 4] (w is a copy: S = 0) -- bar K_PC S"""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    P = patches.shape[-1]
    m = len(ix)
    pa = np.asarray(patches, np.float64).reshape(-1, 3, P, P)[:m]
    K = np.asarray(intrinsics, np.float64).reshape(-1, 4)[ix][:, :, None, None]
    Rt = np.swapaxes(rotmat(poses[ix, 3:]), -1, -2)
    t = poses[ix, :3]
    a = np.stack([(pa[:, 0] - K[:, 2]) / K[:, 0], (pa[:, 1] - K[:, 3]) / K[:, 1], np.ones_like(pa[:, 2])], -1)
    d = pa[:, 2][..., None]
    tinv = -np.einsum("mrc,mc->mr", Rt, t)
    tmag = np.einsum("mrc,mc->mr", np.abs(Rt), np.abs(t))
    X = np.einsum("mrc,mpqc->mpqr", Rt, a) + tinv[:, None, None, :] * d
    A = np.einsum("mrc,mpqc->mpqr", np.abs(Rt), np.abs(a)) + tmag[:, None, None, :] * d
    return dict(full=np.concatenate([X, d], -1), S=np.concatenate([EPS * A, np.zeros_like(d)], -1))


def centre_index(P):
    return P // 2, P // 2     # (row, column) of the pixel dpvo.py:747-749 keeps


def point_cloud_centre(poses, patches, intrinsics, ix):
    """centre [m, 3] = xyz / w of the centre pixel, S [m, 3] -- bar (K_PC + 1) S"""
    r = point_cloud(poses, patches, intrinsics, ix)
    c = centre_index(patches.shape[-1])
    full, S = r["full"][:, c[0], c[1]], r["S"][:, c[0], c[1]]
    w = full[:, 3:]
    return dict(centre=full[:, :3] / w, S=S[:, :3] / w + EPS * np.abs(full[:, :3] / w))


# ---------------------------------------------------------------------------
# flow magnitude and its means
def flow_mag(poses, patches, intrinsics, ii, jj, kk, beta):
    """per pixel [E, P, P]: flow and its companion S (bar K_FLOW S)"""
    r0 = transform(poses, patches, intrinsics, ii, ii, kk)
    r1 = transform(poses, patches, intrinsics, ii, jj, kk)
    r2 = transform(poses, patches, intrinsics, ii, jj, kk, tonly=True)
    f1 = np.linalg.norm(r1["coords"] - r0["coords"], axis=-1)
    f2 = np.linalg.norm(r2["coords"] - r0["coords"], axis=-1)
    S1 = (r1["S"] + r0["S"]).sum(-1)
    S2 = (r2["S"] + r0["S"]).sum(-1)
    return dict(flow=beta * f1 + (1 - beta) * f2, S=beta * S1 + (1 - beta) * S2)


def mean_bar(fm, steps):
    """bar of the mean of the flows in fm (a flow_mag() result, any subset)"""
    return K_FLOW * fm["S"].mean() + steps * EPS * np.abs(fm["flow"]).mean()


def mean_steps(terms_per_thread, *tree_threads):
    """adds on the longest path of a mean: one thread's own terms, ceil(log2)
    per reduction tree, and the final division"""
    return terms_per_thread + sum(int(np.ceil(np.log2(max(t, 2)))) for t in tree_threads) + 1


def motion_mag(poses, patches, intrinsics, ii, jj, kk, i, j, beta):
    """the two means of DPVO.motionmag: [(mean, flow_mag result) or (nan, None)] for (i, j) and (j, i)"""
    out = []
    for a, b in ((i, j), (j, i)):
        sel = np.nonzero((ii == a) & (jj == b))[0]
        if len(sel) == 0:
            out.append((np.nan, None))
            continue
        fm = flow_mag(poses, patches, intrinsics, ii[sel], jj[sel], kk[sel], beta)
        out.append((fm["flow"].mean(), fm))
    return out


def keyframe_flow(poses, patches, intrinsics, n, M, beta):
    """dist [n, n] and bar [n, n]: frame a's M patches into frame b, 256 threads per pair"""
    P = patches.shape[-1]
    dist, bar = np.empty((n, n)), np.empty((n, n))
    kk = np.arange(n * M)
    steps = mean_steps(-(-M * P * P // 256), 256)
    for b in range(n):
        fm = flow_mag(poses, patches, intrinsics, kk // M, np.full(n * M, b), kk, beta)
        f, S = fm["flow"].reshape(n, -1), fm["S"].reshape(n, -1)
        dist[:, b] = f.mean(1)
        bar[:, b] = K_FLOW * S.mean(1) + steps * EPS * np.abs(f).mean(1)
    return dist, bar
