"""Drop-in replacement for the reference's ``cuda_ba`` extension.

Same module name, functions and argument meaning as dpvo/fastba/ba.cpp:236-241
(imported by dpvo/fastba/ba.py:2); the work runs in libdpvo_hot.so
(csrc/fastba.hip: entry points and dispatch; fastba_det.hip and
fastba_atomic.hip: the solver paths) on the current HIP stream.

``CHECK_CHOLESKY`` (default True) keeps the reference's behaviour of raising
when the Schur system is not positive definite (torch::linalg::cholesky in
ba_cuda.cu:521 raises); it costs one device->host read of a status word per
call.  Set it to False for fully asynchronous / graph-captured use; the
status is then left in ``last_status`` (a device tensor).  A caller may
instead pass ``status=`` (a device int32 tensor): the call then never reads
it, and the caller raises later (DPVO.update does, at keyframe()'s host read).

Windows of up to 12 optimised poses (DPVO's sliding window) take the
deterministic per-patch path: no float atomics, bitwise repeatable.  It
groups the edges by kk on the device, or reuses a caller's grouping
(``csr=(offs, perm, groups)`` from update_ops.group_by(kk), which
DPVO.update already computes for the update operator).  ``DETERMINISTIC =
False`` selects the atomic dense path instead (A/B tests).

Windows of more than 64 optimised poses (the global BA of dpvo.py:436-505)
take the sparse path automatically: per-edge Schur entries and a tiled band
Cholesky instead of the dense E / S (see include/dpvo_hot.h).  ``SPARSE =
True`` forces it for any window (used by the parity tests).

``patches_est=`` / ``prior_mu=`` (not in the reference's extension) add the
depth prior of the reference's Python BA (dpvo/ba.py:151-159) on all three
paths: a patch whose prior inverse depth (channel 2, centre pixel of
``patches_est``, laid out like ``patches``) is positive and finite is pulled
towards it with weight ``prior_mu``.  None (or ``prior_mu = 0``) is the plain
call, bit for bit.

``pgo_residual`` / ``pgo_step`` / ``pgo`` (not in the reference's extension)
are the loop-closure Sim(3) pose-graph optimisation of optim_utils.py:158-255
without pypose: exact fp64 Jacobians, a block-skyline Cholesky instead of the
dense 7n x 7n matrix, the Levenberg-Marquardt loop decided on the device.

``ransac_sim3`` / ``umeyama`` (not in the reference's extension) are the
point-cloud alignment of optim_utils.py:64-150 without numba or a host copy:
RANSAC over the caller's 3-point samples and the Umeyama refit, fp64, bitwise
repeatable (csrc/align.hip).
"""
import math

import torch

import _dpvo_hot as H

CHECK_CHOLESKY = True
SPARSE = False
DETERMINISTIC = True
last_status = None


def raise_for_status(s):
    """the reference's error for a BA status word (0: no error)."""
    s = int(s)
    if s > 0:
        raise RuntimeError(
            "linalg.cholesky: The factorization could not be completed because the input is not positive-"
            f"definite (the leading minor of order {s} is not positive-definite).")
    if s == -2:
        raise RuntimeError("DPVO.update: an edge lies outside the 64-frame key window "
                           "(REMOVAL_WINDOW / PATCH_LIFETIME invariant; set cfg.WINDOW_IJ_KEY = False)")
    if s < 0:
        raise RuntimeError("cuda_ba.forward: patch index out of range")


def forward(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, t0, t1, iterations, csr=None,
            status=None, keep_status=False, patches_est=None, prior_mu=2.0):
    """ba.cpp:31-43 -> ba_cuda.cu:422-540.  Updates poses and patches in place; returns [].
    csr (optional, not in the reference): (offs int32 [E+1], perm int32 [E],
    groups int64 [1]) of update_ops.group_by(kk) for these edges.
    status (optional, not in the reference): a device int32 [1] the call's
    status word is written to instead of being read here -- no host
    synchronisation; the caller checks it later (raise_for_status).
    keep_status (with status=): the word is not cleared first; if it already
    holds a failure (DPVO.update's window-key check) the call leaves poses and
    patches untouched (deterministic sliding-window path, DPVO_BA_KEEP_STATUS).
    patches_est, prior_mu (optional, not in the reference's extension): the
    depth prior of dpvo/ba.py:151-159 -- one prior inverse depth per patch, in
    the layout of patches (channel 2 at the centre pixel is read; <= 0, inf or
    NaN: no prior for that patch), and its weight mu."""
    global last_status
    if patches_est is not None and not patches_est.is_cuda:
        raise RuntimeError("patches_est must be a GPU (HIP) tensor; this library has no CPU backend")
    H.on_gpu(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk)
    for name, t in (("poses", poses), ("patches", patches), ("intrinsics", intrinsics), ("target", target),
                    ("weight", weight), ("patches_est", patches_est)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous (the reference views it, ba_cuda.cu:446-451)")
    P = patches.shape[3] if patches.dim() == 5 else patches.shape[-1]
    num_patches = patches.numel() // (3 * P * P)
    if patches_est is not None and (patches_est.numel() != patches.numel() or patches_est.device != patches.device):
        raise RuntimeError("patches_est must have the element count and device of patches")
    prior_mu = float(prior_mu)
    if not (math.isfinite(prior_mu) and prior_mu >= 0.0):
        raise RuntimeError("prior_mu must be finite and >= 0")
    ii, jj, kk = H.idx64(ii), H.idx64(jj), H.idx64(kk)
    lmbda = lmbda.to(device=poses.device, dtype=torch.float32).contiguous()
    E = ii.numel()
    N = int(t1) - int(t0)
    flags = (1 if SPARSE else 0) | (0 if DETERMINISTIC else 2) | (4 if keep_status and status is not None else 0)
    nbytes = H.lib().dpvo_ba_workspace_bytes_ex(E, num_patches, max(N, 0), flags)
    ws = H.empty(nbytes, dtype=torch.uint8, device=poses.device)
    deferred = status is not None
    if deferred:
        if status.dtype != torch.int32 or status.numel() < 1 or status.device != poses.device:
            raise RuntimeError("status must be a device int32 tensor of at least one element")
    else:
        status = torch.zeros(1, dtype=torch.int32, device=poses.device)
    offs = perm = groups = None
    if csr is not None:
        offs, perm, groups = csr
        H.on_gpu(offs, perm, groups)
        if (offs.dtype != torch.int32 or perm.dtype != torch.int32 or groups.dtype != torch.int64 or
                offs.numel() < E + 1 or perm.numel() < E):
            raise RuntimeError("csr must be update_ops.group_by(kk)'s (offs int32 [E+1], perm int32 [E], groups int64)")
    H.check(H.lib().dpvo_ba_forward_prior(
        H.ptr(poses), H.ptr(patches), num_patches, P, H.ptr(intrinsics), H.ptr(target), H.ptr(weight), H.ptr(lmbda),
        H.ptr(patches_est), prior_mu, H.ptr(ii), H.ptr(jj), H.ptr(kk), E, int(t0), int(t1), int(iterations), flags,
        H.ptr(offs), H.ptr(perm), H.ptr(groups), H.ptr(ws), nbytes, H.ptr(status), H.stream_of(poses)))
    last_status = status
    if CHECK_CHOLESKY and not deferred:
        raise_for_status(status.item())
    return []


def neighbors(ii, jj):
    """ba.cpp:113-158, GPU-resident: -> [ix, jx] (int64)."""
    H.on_gpu(ii, jj)
    ii, jj = H.idx64(ii), H.idx64(jj)
    E = ii.numel()
    ix = H.empty(E, dtype=torch.int64, device=ii.device)
    jx = H.empty(E, dtype=torch.int64, device=ii.device)
    if E:
        nbytes = H.lib().dpvo_neighbors_workspace_bytes(E)
        ws = H.empty(nbytes, dtype=torch.uint8, device=ii.device)
        H.check(H.lib().dpvo_neighbors(H.ptr(ii), H.ptr(jj), E, H.ptr(ix), H.ptr(jx), H.ptr(ws), nbytes,
                                       H.stream_of(ii)))
    return [ix, jx]


def reproject(poses, patches, intrinsics, ii, jj, kk):
    """ba.cpp:53-61 / ba_cuda.cu:543-575 -> coords [1, E, 2, P, P]."""
    H.on_gpu(poses, patches, intrinsics, ii, jj, kk)
    poses, patches, intrinsics = poses.contiguous(), patches.contiguous(), intrinsics.contiguous()
    P = patches.shape[-1]
    ii, jj, kk = H.idx64(ii), H.idx64(jj), H.idx64(kk)
    E = ii.numel()
    out = H.empty((E, 2, P, P), dtype=torch.float32, device=poses.device)
    H.check(H.lib().dpvo_reproject(H.ptr(poses), H.ptr(patches), P, H.ptr(intrinsics), H.ptr(ii), H.ptr(jj),
                                   H.ptr(kk), E, H.ptr(out), H.stream_of(poses)))
    return out.view(1, E, 2, P, P)


def solve_system(J_Ginv_i, J_Ginv_j, ii, jj, res, ep, lm, freen):
    """ba.cpp:174-234 (loop-closure PGO): -> [delta [n, 7]] on res.device.

    A = J^T J, b = -J^T res (fp64) are assembled on the device
    (dpvo_solve_system_assemble); the reference's Eigen SimplicialCholesky is a
    dense fp64 Cholesky here (rocSOLVER via torch.linalg).  freen >= 0 solves
    only the top-left 7*freen block (the rest of delta is zero), like the
    reference.  An edge with ii == jj raises (the reference calls exit(1)).

    Like the reference (which copies every input to the host itself), the
    inputs may live on any device -- PGO builds its Jacobians with pypose,
    possibly on the CPU (optim_utils.py:222-255).  The solve runs on the GPU
    (the current device when res is a CPU tensor) and delta comes back on
    res.device."""
    out_dev = res.device
    dev = res.device if res.is_cuda else torch.device("cuda", torch.cuda.current_device())
    Ji = J_Ginv_i.to(dev, torch.float32).contiguous()
    Jj = J_Ginv_j.to(dev, torch.float32).contiguous()
    rr = res.to(dev, torch.float32).contiguous().view(-1, 7)
    ii, jj = H.idx64(ii.to(dev)), H.idx64(jj.to(dev))
    r = rr.shape[0]
    if Ji.shape != (r, 7, 7) or Jj.shape != (r, 7, 7) or ii.numel() != r or jj.numel() != r:
        raise RuntimeError("solve_system: J_Ginv_i/J_Ginv_j must be [r, 7, 7], ii/jj [r], res [r, 7]")
    n = int(torch.maximum(ii.max(), jj.max()).item()) + 1 if r else 0
    m = 7 * n if int(freen) < 0 else min(7 * int(freen), 7 * n)
    A = H.empty(m, m, dtype=torch.float64, device=dev)
    b = H.empty(m, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    H.check(H.lib().dpvo_solve_system_assemble(H.ptr(Ji), H.ptr(Jj), H.ptr(ii), H.ptr(jj), H.ptr(rr), r, m,
                                               float(ep), float(lm), H.ptr(A), H.ptr(b), H.ptr(status),
                                               H.stream_of(rr)))
    if int(status.item()):
        raise RuntimeError("solve_system: an edge with ii == jj (the reference exits the process, ba.cpp:205)")
    delta = torch.zeros(7 * n, dtype=torch.float32, device=dev)
    if m:
        L = torch.linalg.cholesky(A)
        delta[:m] = torch.cholesky_solve(b[:, None], L)[:, 0].float()
    return [delta.view(n, 7).to(out_dev)]


# ---------------------------------------------------------------------------
# Loop-closure Sim(3) pose-graph optimisation (not in the reference's
# extension: there it is pypose autograd + solve_system, optim_utils.py:158-255).
# Native, fp64, device-resident (csrc/pgo.hip): no pypose, no dense 7n x 7n
# matrix.  poses [n, 7]: camera-to-world SE3 [t, q]; loop_poses [L, 8]: Sim3
# [t, q, s]; g [n, 7]: tangent coordinates [tau, phi, sigma] of the
# world-to-camera Sim3 of every pose.  Edge order: the n - 1 chain edges
# (k, k - 1), then the loops.
# ---------------------------------------------------------------------------
def raise_for_pgo_status(word):
    """the error for a PGO status word (include/dpvo_hot.h); returns the LM iterations run."""
    word = int(word)
    code, iters, pivot = word & 15, (word >> 4) & 255, word >> 12
    if code == 1:
        raise RuntimeError("pgo: a loop edge with ii == jj (the reference exits the process, ba.cpp:205)")
    if code == 2:
        raise RuntimeError("pgo: a loop index outside [0, n)")
    if code == 3:
        raise RuntimeError(
            "linalg.cholesky: The factorization could not be completed because the input is not positive-"
            f"definite (the leading minor of order {pivot} is not positive-definite).")
    return iters


def _pgo_operands(poses, loop_poses, loop_ii, loop_jj, g=None):
    H.on_gpu(poses, loop_poses, loop_ii, loop_jj, g)
    poses = poses.to(torch.float64).contiguous()
    loop_poses = loop_poses.to(torch.float64).contiguous()
    loop_ii, loop_jj = H.idx64(loop_ii).view(-1), H.idx64(loop_jj).view(-1)
    n, L = poses.shape[0], loop_ii.numel()
    if poses.dim() != 2 or poses.shape[1] != 7 or n < 2:
        raise RuntimeError("pgo: poses must be [n, 7] (SE3 [t, q]) with n >= 2")
    if loop_poses.numel() != 8 * L or loop_jj.numel() != L:
        raise RuntimeError("pgo: loop_poses must be [L, 8] (Sim3 [t, q, s]), loop_ii / loop_jj [L]")
    if g is not None:
        g = g.to(torch.float64).contiguous()
        if g.shape != (n, 7):
            raise RuntimeError("pgo: g must be [n, 7]")
    nbytes = H.lib().dpvo_pgo_workspace_bytes(n, L)
    if nbytes == 0:
        raise RuntimeError("pgo: n or L out of range (n <= 65536, L <= 65536)")
    ws = H.empty(nbytes, dtype=torch.uint8, device=poses.device)
    status = torch.zeros(1, dtype=torch.int32, device=poses.device)
    return poses, loop_poses, loop_ii, loop_jj, g, n, L, ws, nbytes, status


def pgo_workspace_bytes(n, L):
    """bytes of device workspace one PGO call over n poses and L loops takes"""
    return int(H.lib().dpvo_pgo_workspace_bytes(int(n), int(L)))


def pgo_residual(g, poses, loop_poses, loop_ii, loop_jj):
    """optim_utils.residual(..., jacobian=True): -> (res [E, 7], Ji [E, 7, 7],
    Jj [E, 7, 7], iii [E], jjj [E]) in fp64; Ji / Jj are the exact derivatives
    of res with respect to g[iii] / g[jjj]."""
    poses, loop_poses, loop_ii, loop_jj, g, n, L, ws, nbytes, status = _pgo_operands(poses, loop_poses, loop_ii,
                                                                                     loop_jj, g)
    if g is None:
        raise RuntimeError("pgo_residual: g missing")
    E = n - 1 + L
    res = H.empty((E, 7), dtype=torch.float64, device=poses.device)
    Ji = H.empty((E, 7, 7), dtype=torch.float64, device=poses.device)
    Jj = H.empty((E, 7, 7), dtype=torch.float64, device=poses.device)
    H.check(H.lib().dpvo_pgo_residual(H.ptr(g), H.ptr(poses), H.ptr(loop_poses), H.ptr(loop_ii), H.ptr(loop_jj), n, L,
                                      H.ptr(res), H.ptr(Ji), H.ptr(Jj), H.ptr(None), H.ptr(ws), nbytes, H.ptr(status),
                                      H.stream_of(poses)))
    raise_for_pgo_status(status.item())
    kk = torch.arange(1, n, device=poses.device)
    return res, Ji, Jj, torch.cat((kk, loop_ii)), torch.cat((kk - 1, loop_jj))


def pgo_step(g, poses, loop_poses, loop_ii, loop_jj, ep, lm, freen):
    """one damped step at g: the delta [n, 7] (fp64) solve_system gives for
    pgo_residual's Jacobians, from a block-skyline Cholesky instead of the
    dense matrix; freen >= 0 solves for the first freen poses only."""
    poses, loop_poses, loop_ii, loop_jj, g, n, L, ws, nbytes, status = _pgo_operands(poses, loop_poses, loop_ii,
                                                                                     loop_jj, g)
    if g is None:
        raise RuntimeError("pgo_step: g missing")
    delta = H.empty((n, 7), dtype=torch.float64, device=poses.device)
    H.check(H.lib().dpvo_pgo_step(H.ptr(g), H.ptr(poses), H.ptr(loop_poses), H.ptr(loop_ii), H.ptr(loop_jj), n, L,
                                  float(ep), float(lm), max(int(freen), -1), H.ptr(delta), H.ptr(ws), nbytes,
                                  H.ptr(status), H.stream_of(poses)))
    raise_for_pgo_status(status.item())
    return delta


def pgo(poses, loop_poses, loop_ii, loop_jj, iters=30, ep=0.0, lmbda=1e-6, fix_opt_window=False):
    """optim_utils.perform_updates: the whole Levenberg-Marquardt loop in one
    call -> (sim3 [n, 8] = Exp(g)^-1, cost_history [iters], NaN where an
    iteration did not run).  One host read (the status word) at the end."""
    poses, loop_poses, loop_ii, loop_jj, _, n, L, ws, nbytes, status = _pgo_operands(poses, loop_poses, loop_ii,
                                                                                     loop_jj)
    iters = int(iters)
    out = H.empty((n, 8), dtype=torch.float64, device=poses.device)
    hist = H.empty((iters,), dtype=torch.float64, device=poses.device)
    H.check(H.lib().dpvo_pgo(H.ptr(poses), H.ptr(loop_poses), H.ptr(loop_ii), H.ptr(loop_jj), n, L, iters, float(ep),
                             float(lmbda), -2 if fix_opt_window else -1, H.ptr(out), H.ptr(hist), H.ptr(ws), nbytes,
                             H.ptr(status), H.stream_of(poses)))
    raise_for_pgo_status(status.item())
    return out, hist


# ---------------------------------------------------------------------------
# Loop-closure alignment (not in the reference's extension: there it is numba
# on the host, optim_utils.py:64-150).  Native, fp64, device-resident
# (csrc/align.hip).  src, dst [N, 3]: matched points, y ~ s R x + t; sim3 [8]:
# [t, q (x y z w), s]; info [4] int32: {code, winner, winner's count, refit
# point count}, code 0 ok, 1 no valid hypothesis, 2 degenerate refit.
# ---------------------------------------------------------------------------
def _align_operands(name, src, dst):
    H.on_gpu(src, dst)
    src, dst = src.to(torch.float64).contiguous(), dst.to(torch.float64).contiguous()
    if src.dim() != 2 or src.shape[1] != 3 or dst.shape != src.shape or dst.device != src.device:
        raise RuntimeError(f"{name}: src and dst must be [N, 3] on one device")
    return src, dst, src.shape[0]


def ransac_sim3(src, dst, samples, threshold, early_exit=100):
    """optim_utils.ransac_umeyama on the caller's samples (any integer tensor
    [H, 3]; optim_utils.draw_samples gives the reference's sequence) ->
    (sim3 [8], counts [H] int32, mask [N] bool, info [4] int32), all on the
    device, no host read.  counts[h] = -1 for an invalid or degenerate sample;
    early_exit < 0 gives the first hypothesis with the largest count."""
    src, dst, N = _align_operands("ransac_sim3", src, dst)
    H.on_gpu(samples)
    if torch.is_floating_point(samples) or samples.dim() != 2 or samples.shape[1] != 3:
        raise RuntimeError("ransac_sim3: samples must be an integer tensor [H, 3]")
    samples = samples.to(device=src.device, dtype=torch.int32).contiguous()
    nh = samples.shape[0]
    dev = src.device
    sim3 = H.empty(8, dtype=torch.float64, device=dev)
    counts = H.empty(nh, dtype=torch.int32, device=dev)
    mask = H.empty(N, dtype=torch.bool, device=dev)
    info = H.empty(4, dtype=torch.int32, device=dev)
    nbytes = H.lib().dpvo_sim3_workspace_bytes(N, nh)
    ws = H.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    H.check(H.lib().dpvo_sim3_ransac(H.ptr(src), H.ptr(dst), N, H.ptr(samples), nh, float(threshold), int(early_exit),
                                     H.ptr(sim3), H.ptr(counts), H.ptr(mask), H.ptr(info), H.ptr(ws), nbytes,
                                     H.stream_of(src)))
    return sim3, counts, mask, info


def umeyama(src, dst, mask=None):
    """optim_utils.umeyama_alignment over the rows with mask (bool / uint8 [N];
    None: all) -> (sim3 [8], info [4] int32) on the device, no host read."""
    src, dst, N = _align_operands("umeyama", src, dst)
    if mask is not None:
        H.on_gpu(mask)
        if mask.numel() != N or mask.dtype not in (torch.bool, torch.uint8) or mask.device != src.device:
            raise RuntimeError("umeyama: mask must be a bool / uint8 tensor [N] on the points' device")
        mask = mask.contiguous().view(-1)
    dev = src.device
    sim3 = H.empty(8, dtype=torch.float64, device=dev)
    info = H.empty(4, dtype=torch.int32, device=dev)
    nbytes = H.lib().dpvo_sim3_workspace_bytes(N, 0)
    ws = H.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    H.check(H.lib().dpvo_sim3_umeyama(H.ptr(src), H.ptr(dst), N, H.ptr(mask), H.ptr(sim3), H.ptr(info), H.ptr(ws),
                                      nbytes, H.stream_of(src)))
    return sim3, info


# ---------------------------------------------------------------------------
# Loop-closure retrieval (the reference's query_online, netvlad_retrieval.py:
# 89-104, for Q queries in one call; csrc/retrieval.hip).  Scores are fp32
# dot products whose bits depend on the two rows alone: one query at a time
# and a batch give the same bits.
# ---------------------------------------------------------------------------
def retrieval_query(db, query_rows, skip_window, top_k=1, return_scores=False):
    """db [N, D] fp32 on the device (rows may be strided: db.stride(0) is the
    leading dimension); query_rows: Q row indices, as host integers (a
    sequence or a CPU tensor: checked against [0, N) with no device read) or
    as a device tensor (checked with one device->host copy).  Query n's
    candidates are the rows [0, n - skip_window).

    -> (val [Q, top_k] fp32, idx [Q, top_k] int64[, scores [Q, N] fp32]), on
    the device: the top_k largest <db[r], db[n]> in non-increasing order, ties
    by ascending row, the unused tail (-inf, -1); scores holds every
    candidate's score and -inf elsewhere."""
    H.on_gpu(db)
    if db.dtype != torch.float32:
        raise RuntimeError(f"retrieval_query: db must be float32, got {db.dtype}")
    if db.dim() != 2 or db.shape[0] < 1 or db.shape[1] < 1 or db.stride(1) != 1:
        raise RuntimeError("retrieval_query: db must be [N, D] with unit stride along D")
    N, D = db.shape
    ld = db.stride(0) if N > 1 else max(db.stride(0), D)
    dev = db.device
    if torch.is_tensor(query_rows):
        if torch.is_floating_point(query_rows) or query_rows.dim() != 1:
            raise RuntimeError("retrieval_query: query_rows must be a 1-D integer tensor or a sequence of integers")
        rows = [int(v) for v in query_rows.tolist()]
    else:
        rows = [int(v) for v in query_rows]
    Q = len(rows)
    bad = [n for n in rows if n < 0 or n >= N]
    if bad:
        raise RuntimeError(f"retrieval_query: query row {bad[0]} outside [0, {N})")
    top_k, skip_window = int(top_k), int(skip_window)
    val = H.empty(Q, max(top_k, 0), dtype=torch.float32, device=dev)
    idx = H.empty(Q, max(top_k, 0), dtype=torch.int64, device=dev)
    scores = H.empty(Q, N, dtype=torch.float32, device=dev) if return_scores else None
    if Q > 0:
        qr = torch.tensor(rows, dtype=torch.int64).to(dev)
        nbytes = H.lib().dpvo_retrieval_workspace_bytes(Q, N, top_k)
        ws = H.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        H.check(H.lib().dpvo_retrieval_query(H.ptr(db), ld, N, D, H.ptr(qr), Q, skip_window, top_k, H.ptr(val),
                                             H.ptr(idx), H.ptr(scores), H.ptr(ws), nbytes, H.stream_of(db)))
    return (val, idx, scores) if return_scores else (val, idx)
