"""Native patch-centre selection (csrc/select.hip through encoder_ops, the
Patchifier and the tracker) against the numpy restatements of
tests/patch_select_ref.py and the Patchifier's torch branches.

Shapes are the smallest that still have a border, a partial 4x4 block (70x101)
and more candidates than a wave."""
import numpy as np
import pytest
import torch

import patch_select_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(64, 96), (70, 101)]


def dev(a):
    """a contiguous device tensor of exactly the array's bytes"""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def candidates(H, W, C, seed, dup=0):
    """C candidates on the whole stride-4 map (so some lie past the pooled map),
    the first two on its last column and last row; dup of them repeated"""
    h, w = R.map_size(H, W)
    rng = np.random.default_rng(seed)
    x, y = rng.integers(0, w, C), rng.integers(0, h, C)
    x[0], y[0] = w - 1, h // 2
    x[1], y[1] = w // 2, h - 1
    if dup:
        x[C - dup:], y[C - dup:] = x[2:2 + dup], y[2:2 + dup]
    return x.astype(np.int64), y.astype(np.int64)


# --------------------------------------------------------------------------- gradient scores and selection
@pytest.mark.parametrize("C", [48, 200])
@pytest.mark.parametrize("kind", ["noise", "blocky"])
@pytest.mark.parametrize("size", SIZES)
def test_gradient_scores_match_fp64(size, kind, C):
    import encoder_ops
    H, W = size
    img = R.frame(H, W, kind)
    x, y = candidates(H, W, C, seed=C)
    _, _, sc = encoder_ops.select_gradient(dev(img), dev(x), dev(y), C // 3, return_scores=True)
    sc = sc.cpu().numpy().astype(np.float64)
    ref = R.scores_at(img, x, y)
    err = np.abs(sc - ref)
    pos = ref > 0
    print(f"{kind} {H}x{W} C={C}: max relative {(err[pos] / ref[pos]).max():.3g} (bar {R.SCORE_RTOL:.3g}), "
          f"zeros {int((~pos).sum())}")
    assert (err <= R.SCORE_RTOL * ref).all()
    assert sc[0] == 0 and sc[1] == 0   # x = w - 1, y = h - 1: where the pooled map ends


@pytest.mark.parametrize("C,M", [(48, 16), (200, 67), (1152, 384)])
@pytest.mark.parametrize("size", SIZES)
def test_gradient_selection_is_the_stable_argsort_tail(size, C, M, poisoned):
    """a blocky frame (exact zeros and ties) and duplicated candidates: out is
    argsort(the kernel's own scores, stable)[-M:], candidate for candidate"""
    import encoder_ops
    H, W = size
    img = R.frame(H, W, "blocky")
    x, y = candidates(H, W, C, seed=3, dup=C // 6)
    ox, oy, sc = encoder_ops.select_gradient(dev(img), dev(x), dev(y), M, return_scores=True)
    top = torch.argsort(sc, stable=True)[-M:].cpu().numpy()
    assert top.tolist() == R.select_top(sc.cpu().numpy(), M).tolist()
    assert (sc == 0).sum().item() > 1
    assert ox.cpu().numpy().tolist() == x[top].tolist()
    assert oy.cpu().numpy().tolist() == y[top].tolist()
    ox2, oy2 = encoder_ops.select_gradient(dev(img), dev(x), dev(y), M)
    assert torch.equal(ox, ox2) and torch.equal(oy, oy2)


@pytest.mark.parametrize("kind", ["noise", "blocky"])
@pytest.mark.parametrize("size", SIZES)
def test_gradient_selection_against_the_torch_branch(size, kind):
    """the torch branch's scores (net.py:127-131) of the same candidates: every
    chosen candidate scores at least the torch cut minus the band, every
    candidate above the cut plus the band is chosen; the band is the score bar
    times the cut, and at most 5 % of the candidates may lie within it."""
    import encoder_ops
    from dpvo import altcorr
    from dpvo.net import Patchifier
    H, W = size
    M = 32
    img = dev(R.frame(H, W, kind))
    h, w = R.map_size(H, W)
    torch.manual_seed(5)
    x = torch.randint(1, w - 1, size=[1, 3 * M], device="cuda")
    y = torch.randint(1, h - 1, size=[1, 3 * M], device="cuda")
    with torch.no_grad():
        images = 2 * (img[None, None] / 255.0) - 0.5
        g = Patchifier._image_gradient(None, images)
        score = altcorr.patchify(g[0, :, None], torch.stack([x, y], -1).float(), 0).view(-1)
    score = score.double().cpu().numpy()
    cut = np.sort(score)[2 * M]
    band = R.SCORE_RTOL * cut
    near = int((np.abs(score - cut) <= band).sum())
    print(f"{kind} {H}x{W}: cut {cut:.6g}, {near} of {3 * M} candidates within the band")
    assert near <= 0.05 * 3 * M
    ox, oy = encoder_ops.select_gradient(img, x, y, M)
    xs, ys = x.view(-1).cpu().numpy(), y.view(-1).cpu().numpy()
    by_centre = {(int(a), int(b)): s for a, b, s in zip(xs, ys, score)}   # (duplicates share their score)
    chosen = set(zip(ox.cpu().numpy().tolist(), oy.cpu().numpy().tolist()))
    assert all(by_centre[c] >= cut - band for c in chosen)
    assert all((int(a), int(b)) in chosen for a, b, s in zip(xs, ys, score) if s > cut + band)


# --------------------------------------------------------------------------- mask
def mask_case(name):
    """(mask uint8 [H, W], keys int32 [h w], M)"""
    rng = np.random.default_rng(11)
    H, W = (70, 101) if name in ("pixels30_odd", "partial_rows", "ties_odd", "equal_keys") else (64, 96)
    if name == "hd_ties":
        H, W = 1080, 1920
    h, w = R.map_size(H, W)
    keys = rng.integers(0, 2 ** 31 - 1, h * w).astype(np.int32)
    mask = np.zeros((H, W), dtype=np.uint8)
    M = 16
    if name in ("pixels30", "pixels30_odd"):        # 30 % of the pixels: nearly every cell
        mask = (rng.random((H, W)) < 0.3).astype(np.uint8) * 255
    elif name == "cells30":                          # one pixel in 30 % of the cells
        cy, cx = np.nonzero(rng.random((h, w)) < 0.3)
        r = np.minimum(4 * cy + rng.integers(0, 4, cy.size), H - 1)
        c = np.minimum(4 * cx + rng.integers(0, 4, cx.size), W - 1)
        mask[r, c] = rng.integers(1, 256, cy.size)
        M = 40
    elif name == "last_cell":                        # the last full cell row and column: rejected
        mask[4 * (h - 1) + 1, 4 * (w - 1) + 2] = 1
    elif name == "cell00":                           # no lower bound: accepted
        mask[3, 3] = 1
    elif name == "partial_rows":                     # only the partial rows / column of 70x101
        mask[68:, :] = 1
        mask[:, 100:] = 1
    elif name in ("ties", "ties_odd"):
        mask = (rng.random((H, W)) < 0.1).astype(np.uint8)
        keys = rng.integers(0, 4, h * w).astype(np.int32)
        M = 100
    elif name == "equal_keys":                       # the order falls to the cell index alone
        mask[:] = 1
        keys[:] = 12345
        M = 50
    elif name == "hd_ties":                          # 129,600 cells, keys of 3 bits: the select runs into the cell bits
        mask = (rng.random((H, W)) < 0.05).astype(np.uint8)
        keys = rng.integers(0, 8, h * w).astype(np.int32)
        M = 384
    return mask, keys, M


MASK_CASES = ["pixels30", "pixels30_odd", "cells30", "last_cell", "cell00", "partial_rows", "ties", "ties_odd",
              "equal_keys", "hd_ties"]


def run_mask(mask, keys, M):
    import encoder_ops
    h, w = R.map_size(*mask.shape)
    x, y, count = encoder_ops.select_mask(dev(mask), dev(keys), M, h, w)
    return x.cpu().numpy(), y.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("name", MASK_CASES)
def test_mask_selection_matches_the_rule(name):
    mask, keys, M = mask_case(name)
    h, w = R.map_size(*mask.shape)
    rx, ry, rK = R.select_mask(mask, keys, M, h, w)
    x, y, K = run_mask(mask, keys, M)
    print(f"{name}: K = {K} of {h * w} cells, M = {M}")
    assert K == rK
    assert x.tolist() == rx.tolist() and y.tolist() == ry.tolist()
    assert {"last_cell": K == 0, "cell00": K == 1, "partial_rows": K == 0}.get(name, K > M)
    x2, y2, K2 = run_mask(mask, keys, M)     # the same bits on a second call
    assert (x2 == x).all() and (y2 == y).all() and K2 == K


@pytest.mark.parametrize("name", MASK_CASES)
def test_mask_selection_reads_nothing_unwritten(name, poisoned):
    mask, keys, M = mask_case(name)
    h, w = R.map_size(*mask.shape)
    rx, ry, rK = R.select_mask(mask, keys, M, h, w)
    x, y, K = run_mask(mask, keys, M)
    assert K == rK and x.tolist() == rx.tolist() and y.tolist() == ry.tolist()


def test_mask_with_fewer_cells_than_patches_repeats_cyclically():
    H, W = 64, 96
    h, w = R.map_size(H, W)
    mask = np.zeros((H, W), dtype=np.uint8)
    cells = [(2, 3), (5, 1), (0, 0), (14, 22), (7, 7)]
    for cy, cx in cells:
        mask[4 * cy + 1, 4 * cx + 2] = 9
    keys = np.random.default_rng(2).integers(0, 2 ** 31 - 1, h * w).astype(np.int32)
    x, y, K = run_mask(mask, keys, 16)
    assert K == 5
    order = sorted(cells, key=lambda c: (keys[c[0] * w + c[1]], c[0] * w + c[1]))
    assert list(zip(y.tolist(), x.tolist())) == [order[m % 5] for m in range(16)]
    x, y, K = run_mask(np.zeros((H, W), dtype=np.uint8), keys, 16)
    assert K == 0 and x.tolist() == [1] * 16 and y.tolist() == [1] * 16


def test_mask_selection_is_uniform():
    """8 valid cells, M = 4, 400 seeded key draws: each cell is chosen
    Binomial(400, 1/2) times, 200 +- 5 sigma = [150, 250]"""
    import encoder_ops
    H, W = 64, 96
    h, w = R.map_size(H, W)
    mask = np.zeros((H, W), dtype=np.uint8)
    cells = [(1, 1), (1, 20), (3, 9), (6, 0), (8, 15), (11, 4), (14, 22), (0, 12)]
    for cy, cx in cells:
        mask[4 * cy, 4 * cx] = 1
    m = dev(mask)
    torch.manual_seed(1234)
    picks = []
    for _ in range(400):
        keys = torch.randint(0, 2 ** 31 - 1, (h * w,), dtype=torch.int32, device="cuda")
        x, y, _ = encoder_ops.select_mask(m, keys, 4, h, w)
        picks.append(y * w + x)
    picks = torch.stack(picks).cpu().numpy()
    assert all(len(set(row)) == 4 for row in picks.tolist())
    times = {c: int((picks == c[0] * w + c[1]).sum()) for c in cells}
    print(times)
    assert sum(times.values()) == 1600
    assert all(150 <= t <= 250 for t in times.values())


# --------------------------------------------------------------------------- argument checks
def test_argument_checks():
    import _dpvo_hot as H
    lib = H.lib()
    st = H.stream_of(torch.zeros(1, device="cuda"))
    img = dev(R.frame(64, 96, "noise"))
    xs = torch.ones(8, dtype=torch.long, device="cuda")
    out = torch.zeros(8, dtype=torch.long, device="cuda")
    p = lambda t: t.data_ptr()
    err = lambda: lib.dpvo_hot_last_error().decode()
    assert lib.dpvo_select_gradient(None, 64, 96, p(xs), p(xs), 8, 4, p(out), p(out), None, st) == -1
    assert "dpvo_select_gradient" in err() and "null" in err()
    assert lib.dpvo_select_gradient(p(img), 64, 96, p(xs), p(xs), 8, 4, None, p(out), None, st) == -1
    assert lib.dpvo_select_gradient(p(img), 64, 96, p(xs), p(xs), 4, 8, p(out), p(out), None, st) == -1
    assert "M > C" in err()
    assert lib.dpvo_select_gradient(p(img), 7, 96, p(xs), p(xs), 8, 4, p(out), p(out), None, st) == -1
    assert lib.dpvo_select_gradient(p(img), 64, 7, p(xs), p(xs), 8, 4, p(out), p(out), None, st) == -1
    assert "8 x 8" in err()
    # M == 0 launches nothing (no operand is looked at)
    assert lib.dpvo_select_gradient(None, 64, 96, None, None, 8, 0, None, None, None, st) == 0
    mask = torch.ones(64, 96, dtype=torch.uint8, device="cuda")
    keys = torch.zeros(16 * 24, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.dpvo_select_mask_workspace_bytes(16, 24), dtype=torch.uint8, device="cuda")
    assert lib.dpvo_select_mask(None, 64, 96, 16, 24, p(keys), 8, p(out), p(out), p(cnt), p(ws), st) == -1
    assert "dpvo_select_mask" in err() and "null" in err()
    assert lib.dpvo_select_mask(p(mask), 64, 96, 16, 24, p(keys), 8, p(out), p(out), None, p(ws), st) == -1
    assert lib.dpvo_select_mask(p(mask), 64, 96, 16, 24, p(keys), 8, p(out), p(out), p(cnt), None, st) == -1
    assert lib.dpvo_select_mask(p(mask), 64, 96, 0, 24, p(keys), 8, p(out), p(out), p(cnt), p(ws), st) == -1
    assert lib.dpvo_select_mask(p(mask), 64, 96, 16, 24, p(keys), 4097, p(out), p(out), p(cnt), p(ws), st) == -1
    assert lib.dpvo_select_mask(None, 64, 96, 16, 24, None, 0, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert out.abs().sum().item() == 0 and cnt.item() == 0   # nothing ran
    import encoder_ops
    with pytest.raises(RuntimeError, match="stride-4 map"):   # a grid that is not the mask's
        encoder_ops.select_mask(mask, torch.zeros(15 * 24, dtype=torch.int32, device="cuda"), 8, 15, 24)


# --------------------------------------------------------------------------- Patchifier
NAMES = ("fmap", "gmap", "imap", "patches", "index", "clr")


def _patchifier(seed=0):
    from dpvo.net import Patchifier
    torch.manual_seed(seed)
    return Patchifier(3).cuda().eval()


def _half_mask(H, W, left, dtype=torch.bool):
    m = torch.zeros(H, W, device="cuda")
    if left:
        m[:, :W // 2] = 1
    else:
        m[:, W // 2:] = 1
    return m.to(dtype)


def _run(pf, img, mode, seed=11, mask=None, M=32):
    kw = dict(gradient_bias=True) if mode == "gradient" else dict(mask=mask)
    with torch.no_grad(), torch.autocast("cuda", enabled=True):
        torch.manual_seed(seed)
        return pf(img, patches_per_image=M, return_color=True, **kw)


def _centres(out):
    p = out[3]
    return p[0, :, 0, 1, 1].long(), p[0, :, 1, 1, 1].long()


@pytest.mark.parametrize("mode", ["gradient", "mask"])
def test_patchifier_graphed_and_eager_agree(mode):
    H, W = 128, 160
    pf = _patchifier()
    img = dev(R.frame(H, W, "noise"))
    mask = _half_mask(H, W, True) if mode == "mask" else None
    out = {}
    for graphed in (False, True):
        pf.graphed = graphed
        out[graphed] = _run(pf, img, mode, mask=mask)
    assert pf._graph is not None and pf._graph_key[-1] == mode
    for name, a, b in zip(NAMES, out[False], out[True]):
        assert torch.equal(a, b), name


def test_patchifier_gradient_native_matches_the_torch_branch():
    """the same candidates (same seed) and the same choice: centres, patches
    and colours bit for bit, the maps within the encoders' fp16 bar"""
    H, W = 128, 160
    pf = _patchifier()
    img = dev(R.frame(H, W, "noise"))
    pf.graphed = False
    out = {}
    try:
        for native in (False, True):
            type(pf).NATIVE_SELECT = native
            out[native] = _run(pf, img, "gradient")
    finally:
        type(pf).NATIVE_SELECT = True
    ax, ay = _centres(out[False])
    bx, by = _centres(out[True])
    assert torch.equal(ax, bx) and torch.equal(ay, by)
    for name, a, b in zip(NAMES, out[False], out[True]):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if name in ("patches", "index", "clr"):
            assert torch.equal(a, b), name
        else:
            d = (a.float() - b.float()).abs().max().item()
            assert d <= 2e-2 * a.float().abs().max().item(), (name, d)


@pytest.mark.parametrize("graphed", [False, True])
def test_patchifier_mask_follows_the_rule(graphed):
    """mask mode draws one int32 key per cell, then the rule; a float mask's
    0.5 entries count as set; the torch branch (other cells: another random
    stream) sees the same valid set and gives the same fmap.  Bit-equal
    patches and clr against the torch branch are asked of gradient mode only:
    here the two paths choose different centres by design, so only what does
    not depend on the centres (fmap, shapes, dtypes) is compared across them;
    gmap / imap / patches / clr at the native centres are covered by the rule
    check below and by the eager / graphed equality test."""
    H, W, M = 128, 160, 32
    h, w = R.map_size(H, W)
    pf = _patchifier()
    pf.graphed = graphed
    img = dev(R.frame(H, W, "noise"))
    mask = torch.zeros(H, W, device="cuda")
    mask[20:60, 30:100] = 0.5
    mask[100, 8] = 2.0
    out = _run(pf, img, "mask", seed=7, mask=mask, M=M)
    torch.manual_seed(7)
    keys = torch.randint(0, 2 ** 31 - 1, (h * w,), dtype=torch.int32, device="cuda").cpu().numpy()
    rx, ry, K = R.select_mask(mask.cpu().numpy(), keys, M, h, w)
    x, y = _centres(out)
    assert int(pf.last_mask_cells.item()) == K and K > M
    assert x.cpu().numpy().tolist() == rx.tolist() and y.cpu().numpy().tolist() == ry.tolist()
    try:
        type(pf).NATIVE_SELECT = False
        ref = _run(pf, img, "mask", seed=7, mask=mask, M=M)
    finally:
        type(pf).NATIVE_SELECT = True
    assert pf.last_mask_cells is None
    valid = R.valid_cells(mask.cpu().numpy(), h, w)
    tx, ty = _centres(ref)
    assert valid[ty.cpu().numpy(), tx.cpu().numpy()].all() and valid[ry, rx].all()
    for name, a, b in zip(NAMES, ref, out):
        assert a.shape == b.shape and a.dtype == b.dtype, name
    d = (ref[0].float() - out[0].float()).abs().max().item()
    assert d <= 2e-2 * ref[0].float().abs().max().item()


def test_patchifier_replay_follows_a_changed_mask():
    """no centre is baked into the graph: the second replay returns the new mask's cells"""
    H, W = 128, 160
    h, w = R.map_size(H, W)
    pf = _patchifier()
    pf.graphed = True
    img = dev(R.frame(H, W, "noise"))
    a = _run(pf, img, "mask", mask=_half_mask(H, W, True))
    graph = pf._graph
    b = _run(pf, img, "mask", mask=_half_mask(H, W, False, dtype=torch.uint8))
    assert pf._graph is graph
    assert (_centres(a)[0] < w // 2).all() and (_centres(b)[0] >= w // 2).all()
    assert int(pf.last_mask_cells.item()) == (h - 1) * (w // 2 - 1)


# --------------------------------------------------------------------------- tracker
def _tracker(**cfg_kw):
    from dpvo.config import make_cfg
    from dpvo.dpvo import DPVO
    from dpvo.net import VONet
    torch.manual_seed(0)
    net = VONet()
    with torch.no_grad():
        net.update.d[1].weight.mul_(40.0)  # random weights: make the motion probe pass
    return DPVO(make_cfg("fast", BUFFER_SIZE=64, **cfg_kw), net, ht=384, wd=512)


INTR = (320.0, 320.0, 320.0, 240.0)


@pytest.mark.parametrize("mode", ["gradient", "mask"])
def test_tracker_runs_on_the_native_selection(mode):
    from dpvo.synthetic import image_stream
    intr = torch.tensor(INTR, device="cuda")
    yy, xx = torch.meshgrid(torch.arange(384, device="cuda"), torch.arange(512, device="cuda"), indexing="ij")
    mask = ((xx // 8 + yy // 8) % 2 == 0) if mode == "mask" else None
    with torch.no_grad():
        slam = _tracker(GRADIENT_BIAS=mode == "gradient")
        for t, img in image_stream(18):
            slam(t, img, None, mask, intr)
        assert slam.is_initialized
        poses, _ = slam.terminate()
    assert np.isfinite(poses).all() and len(poses) == 18
    pf = slam.network.patchify
    assert pf._graph is not None and pf._graph_key[-1] == mode   # the frames took the replay


@pytest.mark.parametrize("defer", [False, True])
def test_tracker_refuses_a_mask_with_too_few_cells(defer):
    from dpvo.synthetic import image_stream
    intr = torch.tensor(INTR, device="cuda")
    good = torch.ones(384, 512, dtype=torch.bool, device="cuda")
    bad = torch.zeros(384, 512, dtype=torch.bool, device="cuda")
    for cy, cx in [(3, 4), (10, 50), (40, 7), (60, 100), (90, 20)]:
        bad[4 * cy, 4 * cx] = True
    calls = 0
    with torch.no_grad():
        slam = _tracker(DEFER_KEYFRAME=defer)
        with pytest.raises(RuntimeError, match=r"5 valid cells.*PATCHES_PER_FRAME = 48"):
            for t, img in image_stream(21):
                if t >= 18:
                    assert slam.is_initialized
                    calls += 1
                slam(t, img, None, good if t < 18 else bad, intr)
            slam.terminate()
    assert 1 <= calls <= 3   # the bad frame's own call or one of the two that follow (else terminate())
