"""Kernel-level tests of csrc/geometry.hip and csrc/keyframe.hip through the C
ABI: the projective kernels against the fp64 restatement of
tests/geometry_ref.py, each float output within k S of it (k counted from the
code, S the output's own magnitude sum -- see that module), and the keyframe
bookkeeping kernels of keyframe.hip (masks, frame shift, edge compaction)
bit-exact against torch / numpy.  Every output is a view between guard bytes
of a poisoned buffer; the guards must survive."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geometry_ref as G

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned")]

DEV = "cuda:0"
GUARD = 256            # bytes on either side of an output; keeps 16-byte alignment
WORST = {}             # entry point -> worst error / S seen (printed per test, -s)


def H():
    import _dpvo_hot
    return _dpvo_hot


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """nbytes of device memory between two guards, `offset` bytes off the
    16-byte grid; poisoned (0xFF) like everything _dpvo_hot.empty hands out"""

    def __init__(self, nbytes, offset=0, init=None):
        self.nbytes, self.lo = int(nbytes), GUARD + offset
        self.buf = H().empty(self.lo + self.nbytes + GUARD, dtype=torch.uint8, device=DEV)
        assert H().poison() == 0xFF and self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + self.nbytes]
        if init is not None:
            self.view.copy_(T(np.frombuffer(np.ascontiguousarray(init).tobytes(), np.uint8)))

    @classmethod
    def of(cls, shape, dtype=torch.float32):
        g = cls(int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size())
        g.t = g.view.view(dtype).view(*shape)
        return g

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo)

    def bytes(self):
        return self.view.cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == 0xFF).all() and (b[self.lo + self.nbytes:] == 0xFF).all(), "guard bytes overwritten"


def check(rc):
    H().check(rc)


def refused(rc, match):
    assert rc != 0
    with pytest.raises(RuntimeError, match=match):
        H().check(rc)


def within(name, got, want, S, k):
    """|got - want| <= k S everywhere; the worst ratio is kept for the notes"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{name}: output not fully written"
    err = np.abs(got - want)
    ratio = float(np.max(np.where(err > 0, err / np.maximum(S, 1e-300), 0.0))) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: worst error / S = {ratio:.2f} (bar {k}), max |error| = {err.max() if err.size else 0:.3g}")
    assert (err <= k * S).all(), f"{name}: error / S = {ratio:.2f} > k = {k}"


# ---------------------------------------------------------------------------
# scenes and references, computed once
@functools.lru_cache(maxsize=None)
def scene(P, M=8, n=12, seed=0):
    s = G.make_scene(P, seed=seed, n=n, M=M)
    s["dev"] = {k: T(s[k]) for k in ("poses", "patches", "intrinsics", "ii", "jj", "kk", "ix")}
    return s


@functools.lru_cache(maxsize=None)
def transform_ref(P, depth, tonly):
    s = scene(P)
    return G.transform(s["poses"], s["patches"], s["intrinsics"], s["ii"], s["jj"], s["kk"], depth=depth, tonly=tonly)


def run_transform(s, flags, with_valid, E=None, ii=None, jj=None, kk=None):
    d = s["dev"]
    ii, jj, kk = (d["ii"] if ii is None else ii), (d["jj"] if jj is None else jj), (d["kk"] if kk is None else kk)
    E = ii.numel() if E is None else E
    P, od = s["P"], 3 if flags & 1 else 2
    out = Guarded.of((E, od, P, P) if flags & 4 else (E, P, P, od))
    valid = Guarded.of((E, P, P)) if with_valid else None
    check(H().lib().dpvo_transform(H().ptr(d["poses"]), H().ptr(d["patches"]), P, H().ptr(d["intrinsics"]),
                                   H().ptr(ii), H().ptr(jj), H().ptr(kk), E, flags, out.ptr,
                                   valid.ptr if valid else None, H().stream_of(d["poses"])))
    torch.cuda.synchronize()
    out.intact()
    if valid:
        valid.intact()
    return out.t, (valid.t if valid else None)


# ---------------------------------------------------------------------------
# dpvo_transform
@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_transform_flags(P, flags, with_valid):
    """every flag combination at both template instances (P = 3 and run-time P,
    even P included): coords within k S of fp64, valid exact away from the
    threshold's own bound, CHW == HWC bitwise"""
    s = scene(P)
    r = transform_ref(P, bool(flags & 1), bool(flags & 2))
    out, valid = run_transform(s, flags, with_valid)
    hwc = out.permute(0, 2, 3, 1) if flags & 4 else out
    within("dpvo_transform", hwc.cpu().numpy(), r["coords"], r["S"], np.array([G.K_XY, G.K_XY, G.K_D][:hwc.shape[-1]]))
    if flags & 4:
        plain, _ = run_transform(s, flags & 3, False)
        assert torch.equal(hwc.contiguous().view(torch.int32), plain.view(torch.int32))
    if with_valid:
        v = valid.cpu().numpy()
        assert np.isin(v, (0.0, 1.0)).all()
        decided = ~G.valid_undecided(r)
        np.testing.assert_array_equal(v[decided], r["valid"][decided])


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_transform_tonly_self_is_identity(P):
    """tonly with ii == jj: R := I and t_ii = t_i - R_ii t_i = 0, the pixel comes back"""
    s = scene(P)
    d = s["dev"]
    r = G.transform(s["poses"], s["patches"], s["intrinsics"], s["ii"], s["ii"], s["kk"], depth=True, tonly=True)
    px = s["patches"][s["kk"]].astype(np.float64)
    want = np.stack([px[:, 0], px[:, 1], np.ones_like(px[:, 0])], -1)
    assert (np.abs(r["coords"] - want) <= r["S"]).all()      # the restatement itself, to fp64 noise
    out, _ = run_transform(s, 3, False, jj=d["ii"])
    within("dpvo_transform", out.cpu().numpy(), want, r["S"], np.array([G.K_XY, G.K_XY, G.K_D]))


@pytest.mark.parametrize("E", [1, 255, 256, 257])
@pytest.mark.parametrize("P", [2, 3])
def test_transform_edge_counts(P, E):
    s = scene(P)
    r = transform_ref(P, True, False)
    out, valid = run_transform(s, 1, True, E=E)
    within("dpvo_transform", out.cpu().numpy(), r["coords"][:E], r["S"][:E], np.array([G.K_XY, G.K_XY, G.K_D]))
    decided = ~G.valid_undecided(r)[:E]
    np.testing.assert_array_equal(valid.cpu().numpy()[decided], r["valid"][:E][decided])


def test_transform_empty_and_refusals():
    lib, d = H().lib(), scene(3)["dev"]
    assert lib.dpvo_transform(None, None, 3, None, None, None, None, 0, 0, None, None, None) == 0
    out = Guarded.of((4, 3, 3, 2))
    ops = [H().ptr(d[k]) for k in ("poses", "patches")], H().ptr(d["intrinsics"]), [H().ptr(d[k]) for k in ("ii", "jj", "kk")]
    refused(lib.dpvo_transform(*ops[0], 0, ops[1], *ops[2], 4, 0, out.ptr, None, None), "bad patch size")
    refused(lib.dpvo_transform(*ops[0], 3, None, *ops[2], 4, 0, out.ptr, None, None), "null operand")
    refused(lib.dpvo_transform(*ops[0], 3, ops[1], *ops[2], 4, 0, None, None, None), "null operand")
    torch.cuda.synchronize()
    out.intact()
    assert (out.bytes() == 0xFF).all()


# ---------------------------------------------------------------------------
# dpvo_point_cloud
@functools.lru_cache(maxsize=None)
def cloud_ref(P):
    s = scene(P, M=22, seed=1)     # 264 patches: m = 257 is a second workgroup of one thread
    a = (s["poses"], s["patches"], s["intrinsics"], s["ix"])
    return s, G.point_cloud(*a), G.point_cloud_centre(*a)


@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_point_cloud_full_and_centre(P, m):
    s, full_ref, centre_ref = cloud_ref(P)
    d = s["dev"]
    full, centre = Guarded.of((m, P, P, 4)), Guarded.of((m, 3))
    for out, c in ((full, 0), (centre, 1)):
        check(H().lib().dpvo_point_cloud(H().ptr(d["poses"]), H().ptr(d["patches"]), P, H().ptr(d["intrinsics"]),
                                         H().ptr(d["ix"]), m, c, out.ptr, H().stream_of(d["poses"])))
    torch.cuda.synchronize()
    full.intact()
    centre.intact()
    f, c = full.t.cpu().numpy(), centre.t.cpu().numpy()
    within("dpvo_point_cloud full", f[..., :3], full_ref["full"][:m, ..., :3], full_ref["S"][:m, ..., :3], G.K_PC)
    np.testing.assert_array_equal(f[..., 3], s["patches"][:m, 2])          # w is the inverse depth, copied
    within("dpvo_point_cloud centre", c, centre_ref["centre"][:m], centre_ref["S"][:m], G.K_PC + 1)
    # the centre is the full cloud's pixel (P/2, P/2) over w: the same chain,
    # then one division -- that division's rounding and one more for the chain
    row, col = G.centre_index(P)
    q = f[:, row, col, :3].astype(np.float64) / f[:, row, col, 3:].astype(np.float64)
    apart = float(np.max(np.abs(c - q) / np.abs(q)) / G.EPS)
    print(f"dpvo_point_cloud centre vs full[centre] / w: {apart:.2f} roundings apart (bar 2)")
    assert (np.abs(c - q) <= 2 * G.EPS * np.abs(q)).all(), apart


def test_point_cloud_empty_and_refusals():
    lib, d = H().lib(), scene(3)["dev"]
    assert lib.dpvo_point_cloud(None, None, 3, None, None, 0, 0, None, None) == 0
    refused(lib.dpvo_point_cloud(H().ptr(d["poses"]), H().ptr(d["patches"]), 0, H().ptr(d["intrinsics"]),
                                 H().ptr(d["ix"]), 4, 0, H().ptr(d["poses"]), None), "bad patch size")
    refused(lib.dpvo_point_cloud(H().ptr(d["poses"]), H().ptr(d["patches"]), 3, H().ptr(d["intrinsics"]),
                                 H().ptr(d["ix"]), 4, 0, None, None), "null operand")


# ---------------------------------------------------------------------------
# dpvo_motion_mag / dpvo_motion_mag_ws
def pair_edges(s, E, at, seed=5):
    """E edges between frames 0 / 1 / 2 only, then `at` = {(a, b): positions}
    overwrites single edges with direction a -> b (kk a patch of frame a)"""
    rng = np.random.default_rng(seed)
    M = s["M"]
    ii = rng.integers(0, 3, E)
    jj = rng.integers(0, 3, E)
    for (a, b), pos in at.items():
        ii[pos], jj[pos] = a, b
    kk = ii * M + rng.integers(0, M, E)
    return ii.astype(np.int64), jj.astype(np.int64), kk.astype(np.int64)


def run_motion_mag(s, ii, jj, kk, i, j, beta, ws_short=0):
    d, lib = s["dev"], H().lib()
    E = ii.numel()
    a = (H().ptr(d["poses"]), H().ptr(d["patches"]), s["P"], H().ptr(d["intrinsics"]), H().ptr(ii), H().ptr(jj),
         H().ptr(kk), E, i, j, beta)
    one, many = Guarded.of((2,)), Guarded.of((2,))
    nb = lib.dpvo_motion_mag_workspace_bytes(E)
    ws = Guarded(nb)
    check(lib.dpvo_motion_mag(*a, one.ptr, H().stream_of(ii)))
    check(lib.dpvo_motion_mag_ws(*a, many.ptr, ws.ptr, nb, H().stream_of(ii)))
    torch.cuda.synchronize()
    for g in (one, many, ws):
        g.intact()
    return one.t.cpu().numpy(), many.t.cpu().numpy()


def check_motion_mag(s, ii, jj, kk, i, j, beta):
    P, E = s["P"], len(ii)
    ref = G.motion_mag(s["poses"], s["patches"], s["intrinsics"], ii, jj, kk, i, j, beta)
    dii, djj, dkk = T(ii), T(jj), T(kk)
    one, many = run_motion_mag(s, dii, djj, dkk, i, j, beta)
    again = run_motion_mag(s, dii, djj, dkk, i, j, beta)
    assert one.tobytes() == again[0].tobytes() and many.tobytes() == again[1].tobytes()    # fixed reduction order
    nblk = min(-(-E // 256), 4096)
    for slot, ((a, b), (mean, fm)) in enumerate(zip(((i, j), (j, i)), ref)):
        if fm is None:
            assert np.isnan(one[slot]) and np.isnan(many[slot])
            continue
        pos = np.nonzero((ii == a) & (jj == b))[0]
        per_thread_one = np.bincount(pos % 1024).max()
        per_thread_ws = np.bincount(pos % (nblk * 256)).max()
        bar_one = G.mean_bar(fm, G.mean_steps(P * P * per_thread_one, 1024))
        bar_ws = G.mean_bar(fm, G.mean_steps(P * P + per_thread_ws + -(-nblk // 256), 256, 256))
        S = G.K_FLOW * fm["S"].mean()
        within("dpvo_motion_mag", one[slot], mean, bar_one / G.K_FLOW, G.K_FLOW)
        within("dpvo_motion_mag_ws", many[slot], mean, bar_ws / G.K_FLOW, G.K_FLOW)
        assert abs(float(one[slot]) - float(many[slot])) <= bar_one + bar_ws
        assert S > 0
    return ref


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("P", [2, 3])
def test_motion_mag_means(P, beta):
    """(4, 6) has edges in three workgroups, (6, 4) exactly one, (4, 9) some and (9, 4) none"""
    s = scene(P)
    at = {(4, 6): np.arange(7, 700, 37), (6, 4): [500], (4, 9): [3, 260, 699]}
    ii, jj, kk = pair_edges(s, 700, at)
    ref = check_motion_mag(s, ii, jj, kk, 4, 6, beta)
    assert all(fm is not None for _, fm in ref) and ref[1][1]["flow"].shape[0] == 1
    ref = check_motion_mag(s, ii, jj, kk, 4, 9, beta)
    assert ref[0][1] is not None and ref[1][1] is None            # NaN in the (9, 4) slot only


def test_motion_mag_grid_stride():
    """E past 4096 * 256: the partial kernel's grid-stride leg and the final
    kernel's strided loop over all 4096 partials"""
    s = scene(3)
    E = 1_048_576 + 77
    at = {(4, 6): [100, 70_001, 1_048_576 + 5, 1_048_576 + 40, E - 1], (6, 4): [1_048_576 + 60]}
    ii, jj, kk = pair_edges(s, E, at)
    check_motion_mag(s, ii, jj, kk, 4, 6, 0.5)


def test_motion_mag_refusals():
    s = scene(3)
    d, lib = s["dev"], H().lib()
    a = (H().ptr(d["poses"]), H().ptr(d["patches"]), 3, H().ptr(d["intrinsics"]), H().ptr(d["ii"]), H().ptr(d["jj"]),
         H().ptr(d["kk"]), 100, 4, 6, 0.5)
    out = Guarded.of((2,))
    nb = lib.dpvo_motion_mag_workspace_bytes(100)
    ws = Guarded(nb)
    refused(lib.dpvo_motion_mag_ws(*a, out.ptr, ws.ptr, nb - 1, None), "workspace too small")
    refused(lib.dpvo_motion_mag_ws(*a, out.ptr, None, nb, None), "workspace too small")
    refused(lib.dpvo_motion_mag(*a, None, None), "null operand")
    torch.cuda.synchronize()
    assert (out.bytes() == 0xFF).all() and (ws.bytes() == 0xFF).all()


# ---------------------------------------------------------------------------
# dpvo_keyframe_flow
def run_keyframe_flow(s, n, M, beta=0.5):
    d = s["dev"]
    out = Guarded.of((n, n))
    rc = H().lib().dpvo_keyframe_flow(H().ptr(d["poses"]), H().ptr(d["patches"]), s["P"], H().ptr(d["intrinsics"]), n,
                                      M, beta, out.ptr, H().stream_of(d["poses"]))
    torch.cuda.synchronize()
    out.intact()
    return rc, out


@pytest.mark.parametrize("n,M,P", [(1, 1, 1), (17, 3, 3), (5, 29, 3), (3, 8, 4)])
def test_keyframe_flow_matrix(n, M, P):
    """NPX = 1, 27, 261 and 128; n = 17 puts one frame in a second target
    block.  The diagonal is held to its own bound like every other entry."""
    s = scene(P, M=M, n=n, seed=2)
    dist, bar = G.keyframe_flow(s["poses"], s["patches"], s["intrinsics"], n, M, 0.5)
    rc, out = run_keyframe_flow(s, n, M)
    check(rc)
    within("dpvo_keyframe_flow", out.t.cpu().numpy(), dist, bar / G.K_FLOW, G.K_FLOW)


@pytest.mark.parametrize("M", [304, 753])
def test_keyframe_flow_large_lds(M):
    """65,664 B (just past 64 KiB) and 162,648 B + the 1 KiB reduction array
    (the most the guard admits): both must launch and compute"""
    s = scene(3, M=M, n=2, seed=3)
    assert H().lib().dpvo_keyframe_flow_lds_bytes(3, M) == 6 * 9 * M * 4
    dist, bar = G.keyframe_flow(s["poses"], s["patches"], s["intrinsics"], 2, M, 0.5)
    rc, out = run_keyframe_flow(s, 2, M)
    check(rc)
    within("dpvo_keyframe_flow", out.t.cpu().numpy(), dist, bar / G.K_FLOW, G.K_FLOW)


def test_keyframe_flow_refusals():
    s = scene(3, M=754, n=2, seed=3)
    rc, out = run_keyframe_flow(s, 2, 754)
    refused(rc, "do not fit in LDS")
    assert (out.bytes() == 0xFF).all()
    refused(H().lib().dpvo_keyframe_flow(None, None, 3, None, 2, 8, 0.5, out.ptr, None), "null operand")
    assert H().lib().dpvo_keyframe_flow(None, None, 3, None, 0, 8, 0.5, None, None) == 0


# ---------------------------------------------------------------------------
# dpvo_keyframe_masks
@pytest.mark.parametrize("E", [0, 1, 255, 131_072 + 300])
def test_keyframe_masks(E):
    """the torch expressions of test_gpu_tracker.py, with patch indices that
    fall outside ix (before or after the drop's shift): ix is a view inside a
    buffer whose neighbours would read as old, such edges count as not old"""
    g = torch.Generator().manual_seed(11 + E)
    M, n, RW, k = 8, 40, 6, 30
    ix_len = n * M
    big = torch.full((ix_len + 2 * M + 64,), -1000, dtype=torch.int64, device=DEV)     # -1000 < n - RW: "old"
    ix = big[M + 32:M + 32 + ix_len]
    ix.copy_(torch.arange(n, device=DEV).repeat_interleave(M))
    ii = torch.randint(n - 20, n, (E,), generator=g)
    kk = ii * M + torch.randint(0, M, (E,), generator=g)
    jj = torch.randint(n - 20, n, (E,), generator=g)
    # out-of-range patches: below 0, in [0, M) with ii > k (kk - M < 0), at and past ix_len
    odd = torch.tensor([-1, -M, 3, ix_len, ix_len + M - 1, ix_len + 5 * M])
    sel = torch.randperm(E, generator=g)[:E // 4]
    kk[sel] = odd[torch.randint(0, len(odd), (len(sel),), generator=g)]
    if E:
        ii[0], jj[0], kk[0] = k + 1, k, 3          # later edge, dropped, kk - M < 0
    ii, jj, kk = ii.to(DEV), jj.to(DEV), kk.to(DEV)
    mm = torch.tensor([0.25, float("nan")], device=DEV)
    fail = torch.tensor([-3], dtype=torch.int32, device=DEV)
    pose = torch.tensor([0, 0, float("nan") if E % 2 else 0.5, 0, 0, 0, 1], device=DEV)
    masks, idx, vals = Guarded.of((3, E), torch.uint8), Guarded.of((3, E), torch.int64), Guarded.of((7,), torch.float64)
    lib = H().lib()
    nb = lib.dpvo_keyframe_masks_workspace_bytes(E)
    ws = Guarded(nb)
    check(lib.dpvo_keyframe_masks(H().ptr(ii), H().ptr(jj), H().ptr(kk), E, H().ptr(ix), ix_len, k, M, n, RW,
                                  H().ptr(mm), H().ptr(fail), H().ptr(pose), masks.ptr, idx.ptr, vals.ptr, ws.ptr, nb,
                                  H().stream_of(ii)))
    torch.cuda.synchronize()
    for gd in (masks, idx, vals, ws):
        gd.intact()

    def old(p, bound):
        inside = (p >= 0) & (p < ix_len)
        return inside & (ix[p.clamp(0, ix_len - 1)] < bound)

    drop = (ii == k) | (jj == k)
    later = ii > k
    kk_d = torch.where(later, kk - M, kk)
    old_keep, old_d = old(kk, n - RW), old(kk_d, n - 1 - RW) & ~drop
    rm_d = old_d | drop
    assert torch.equal(masks.t, torch.stack([old_keep, old_d, rm_d]).to(torch.uint8))
    assert torch.equal(idx.t, torch.stack([torch.where(later, ii - 1, ii), torch.where(jj > k, jj - 1, jj), kk_d]))
    v = vals.t.cpu().tolist()
    assert v[0] == 0.25 and np.isnan(v[1]) and v[2] == -3.0 and v[3] == float(E % 2)
    assert v[4:] == [float(old_keep.sum()), float(old_d.sum()), float(rm_d.sum())]
    if E > 255:
        outside = (kk < 0) | (kk >= ix_len) | (kk_d < 0) | (kk_d >= ix_len)
        assert int(outside.sum()) > E // 8 and int(old_keep.sum()) > 0 and int(old_d.sum()) > 0


# ---------------------------------------------------------------------------
# dpvo_frame_shift
def run_frame_shift(segs, k, n):
    """segs: (Guarded, slot_bytes, ring)"""
    ns = len(segs)
    bases = (ctypes.c_void_p * ns)(*[g.ptr.value for g, _, _ in segs])
    sizes = (ctypes.c_int64 * ns)(*[sb for _, sb, _ in segs])
    rings = (ctypes.c_int64 * ns)(*[r for _, _, r in segs])
    rc = H().lib().dpvo_frame_shift(bases, sizes, rings, ns, k, n, None)
    torch.cuda.synchronize()
    return rc


def shifted(data, slot, ring, k, n):
    """the sequential move, frame after frame, on a [slots, slot_bytes] copy"""
    ref = data.copy().reshape(-1, slot)
    for f in range(k, n - 1):
        ref[f % ring if ring else f] = ref[(f + 1) % ring if ring else f + 1]
    return ref.reshape(-1)


def test_frame_shift_sixteen_segments():
    """16 buffers in one launch: 16-byte words (aligned base and slot), 4-byte
    words (28-byte and other slots), bytes (odd slots, or a base one byte off),
    plain buffers and rings -- ring 5 wraps with n - k == ring"""
    rng = np.random.default_rng(7)
    k, n = 9, 14
    spec = [(16, 0, 0), (48, 5, 0), (28, 0, 0), (4, 6, 0), (7, 0, 0), (16, 0, 1), (64, 5, 0), (1, 0, 0),
            (112, 0, 0), (28, 5, 0), (5, 6, 0), (32, 5, 1), (13, 0, 0), (256, 0, 0), (12, 7, 0), (33, 5, 0)]
    segs, datas = [], []
    for slot, ring, off in spec:
        data = rng.integers(0, 255, (ring or n + 2) * slot, dtype=np.uint8)
        segs.append((Guarded(len(data), offset=off, init=data), slot, ring))
        datas.append(data)
    check(run_frame_shift(segs, k, n))
    for (g, slot, ring), data in zip(segs, datas):
        g.intact()
        np.testing.assert_array_equal(g.bytes(), shifted(data, slot, ring, k, n), err_msg=f"slot {slot} ring {ring}")
        if not ring:   # slots outside [k, n) are part of the comparison; say so once
            assert (g.bytes().reshape(-1, slot)[[0, k - 1, n, n + 1]] == data.reshape(-1, slot)[[0, k - 1, n, n + 1]]).all()


def test_frame_shift_large_slot():
    """an 8 MiB + 48 B slot: 524,291 words, three past the 2048 x 256 grid"""
    slot, k, n = 8 * 1024 * 1024 + 48, 0, 4
    data = np.random.default_rng(8).integers(0, 255, 4 * slot, dtype=np.uint8)
    g = Guarded(len(data), init=data)
    check(run_frame_shift([(g, slot, 0)], k, n))
    g.intact()
    assert g.bytes().tobytes() == shifted(data, slot, 0, k, n).tobytes()


def test_frame_shift_noop_and_refusals():
    data = np.random.default_rng(9).integers(0, 255, 10 * 16, dtype=np.uint8)
    g = Guarded(len(data), init=data)
    for k, n in ((5, 6), (5, 5), (7, 3)):             # n - 1 <= k: nothing to move
        assert run_frame_shift([(g, 16, 0)], k, n) == 0
    refused(run_frame_shift([(g, 16, 0)] * 17, 2, 6), "at most 16 buffers")
    refused(run_frame_shift([(g, 16, 5)], 2, 8), "must fit in the ring")
    refused(run_frame_shift([(g, 16, 0)], -1, 6), "k must be >= 0")
    g.intact()
    np.testing.assert_array_equal(g.bytes(), data)


# ---------------------------------------------------------------------------
# dpvo_compact_edges
WT = {"16": (16, 0), "12": (12, 0), "8+4": (8, 4)}       # weight / target row bytes, offset off the 8-byte grid


def run_compact(E, density, mode, row_words, wt, seed=0):
    rng = np.random.default_rng(1000 * seed + E + row_words)
    wb, off = WT[wt]
    rb = 16 * row_words
    rm = (rng.random(E) < density) if 0 < density < 1 else np.full(E, bool(density))
    store = rm & (rng.random(E) < 0.5)
    ids = [rng.integers(-2 ** 62, 2 ** 62, E) for _ in range(3)]
    w, t = (rng.integers(0, 255, (E, wb), dtype=np.uint8) for _ in range(2))
    net = rng.integers(0, 255, (E, rb), dtype=np.uint8)
    keep = ~rm
    stored = {0: np.zeros(E, bool), 1: rm, 2: store}[mode]
    dev_in = [T(rm.astype(np.uint8)), T(store.astype(np.uint8))] + [T(a) for a in ids]
    gw, gt = Guarded(E * wb, offset=off, init=w), Guarded(E * wb, offset=off, init=t)
    gnet = Guarded(E * rb, init=net)
    # outputs sized for all E edges: the rows past the counts must keep the poison
    out_k = [Guarded(E * 8) for _ in range(3)] + [Guarded(E * wb, offset=off) for _ in range(2)] + [Guarded(E * rb)]
    out_s = [Guarded(E * 8) for _ in range(3)] + [Guarded(E * wb, offset=off) for _ in range(2)]
    lib = H().lib()
    nb = lib.dpvo_compact_edges_workspace_bytes(E)
    ws = Guarded(nb)
    sp = [g.ptr if mode else None for g in out_s]
    rc = lib.dpvo_compact_edges(E, H().ptr(dev_in[0]), H().ptr(dev_in[1]) if mode == 2 else None, mode,
                                H().ptr(dev_in[2]), H().ptr(dev_in[3]), H().ptr(dev_in[4]), gw.ptr, gt.ptr, wb, gnet.ptr,
                                rb, *[g.ptr for g in out_k], *sp, ws.ptr, nb, None)
    torch.cuda.synchronize()
    check(rc)

    def expect(rows, sel):
        full = np.full(rows.shape, 0xFF, np.uint8)
        full[:int(sel.sum())] = rows[sel]
        return full.reshape(-1)

    as_bytes = [a.astype(np.int64).view(np.uint8).reshape(E, 8) for a in ids] + [w, t]
    for g, rows, name in zip(out_k, as_bytes + [net], ("ii", "jj", "kk", "weight", "target", "net")):
        g.intact()
        np.testing.assert_array_equal(g.bytes(), expect(rows, keep), err_msg=f"kept {name}")
    for g, rows, name in zip(out_s, as_bytes, ("ii", "jj", "kk", "weight", "target")):
        g.intact()
        np.testing.assert_array_equal(g.bytes(), expect(rows, stored), err_msg=f"stored {name}")
    for g, src in ((gw, w), (gt, t), (gnet, net)):
        g.intact()
        np.testing.assert_array_equal(g.bytes(), src.reshape(-1))
    ws.intact()


ROWS = (1, 5, 96, 97, 200)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("density", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_compact_edges_sizes(E, density, mode):
    """every E x density x store_mode; the row width and the weight rows' size
    rotate through their values (each pair appears in the next test)"""
    i = [1, 255, 256, 257].index(E) + 4 * mode + int(density * 10)
    run_compact(E, density, mode, ROWS[i % 5], list(WT)[i % 3])


@pytest.mark.parametrize("wt", list(WT))
@pytest.mark.parametrize("row_words", ROWS)
def test_compact_edges_row_shapes(row_words, wt):
    """rows of 97 and 200 words reach the tail loop past the 12 unrolled words
    per lane; 12-byte rows and the 8-byte rows four bytes off the grid take
    ce_row's byte path, 16-byte rows the 8-byte one"""
    run_compact(257, 0.3, 2, row_words, wt, seed=1)
    run_compact(700, 0.3, 1, row_words, wt, seed=2)


@pytest.mark.parametrize("density", [0.0, 0.3, 1.0])
def test_compact_edges_many_blocks(density):
    """70,000 edges = 274 blocks: the prefix over earlier blocks runs its loop twice"""
    run_compact(70_000, density, 2, 5, "12", seed=3)
    run_compact(70_000, density, 1, 1, "16", seed=4)


def test_compact_edges_refusals():
    lib = H().lib()
    E = 8
    z = torch.zeros(E * 64 + 16, dtype=torch.uint8, device=DEV)
    p, q = H().ptr(z), ctypes.c_void_p(z.data_ptr() + 8)
    nb = lib.dpvo_compact_edges_workspace_bytes(E)

    def call(mode=1, store=p, net=p, net_k=p, rb=32):
        return lib.dpvo_compact_edges(E, p, store, mode, p, p, p, p, p, 8, net, rb, p, p, p, p, p, net_k, p, p, p, p, p,
                                      p, nb, None)

    refused(call(rb=24), "row sizes")
    refused(call(net=q), "16-byte aligned")
    refused(call(net_k=q), "16-byte aligned")
    refused(call(mode=2, store=None), "store_mode 2 needs the store mask")
    refused(call(mode=3), "store mode")
    torch.cuda.synchronize()
    assert int(z.sum()) == 0
