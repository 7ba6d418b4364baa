"""The patch-selection rules' numpy restatements (tests/patch_select_ref.py)
against the reference's own torch expression, and the host side of the native
selection (exports, shims) -- no GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_select_ref as R

SIZES = [(64, 96), (70, 101), (128, 160)]


def frame(H, W, kind, seed=1):
    return torch.from_numpy(R.frame(H, W, kind, seed))


def reference_gradient(image):
    """the reference's data flow (net.py:116 then :103-109) in fp32 torch"""
    images = 2 * (image[None, None] / 255.0) - 0.5
    gray = ((images + 0.5) * (255.0 / 2)).sum(dim=2)
    dx = gray[..., :-1, 1:] - gray[..., :-1, :-1]
    dy = gray[..., 1:, :-1] - gray[..., :-1, :-1]
    return F.avg_pool2d(torch.sqrt(dx ** 2 + dy ** 2), 4, 4)[0, 0]


@pytest.mark.parametrize("kind", ["noise", "blocky"])
@pytest.mark.parametrize("size", SIZES)
def test_score_restatement_matches_the_reference_expression(size, kind):
    H, W = size
    img = frame(H, W, kind)
    ref = reference_gradient(img).double().numpy()
    mine = R.score_map(img.numpy())
    assert mine.shape == ref.shape == ((H - 1) // 4, (W - 1) // 4)
    err = np.abs(ref - mine)
    rel = (err[mine > 0] / mine[mine > 0]).max()
    print(f"{kind} {H}x{W}: max relative {rel:.3g} (bar {R.SCORE_RTOL:.3g}), zeros {int((mine == 0).sum())}")
    assert (err <= R.SCORE_RTOL * mine).all()
    if kind == "blocky":
        assert (mine == 0).any()


def test_scores_at_is_zero_outside_the_pooled_map():
    img = frame(64, 96, "noise").numpy()
    h, w = R.map_size(64, 96)
    m = R.score_map(img)
    assert m.shape == (15, 23) and (h, w) == (16, 24)
    s = R.scores_at(img, [3, w - 1, 22, 0, -1], [2, 5, h - 1, 0, 3])
    assert s[0] == m[2, 3] and s[3] == m[0, 0] and s[1] == 0 and s[2] == 0 and s[4] == 0


def test_select_top_is_the_stable_argsort_tail():
    s = np.array([2.0, 0.0, 2.0, 1.0, 0.0, 2.0])
    assert R.select_top(s, 4).tolist() == [3, 0, 2, 5]
    assert R.select_top(s, 6).tolist() == [1, 4, 3, 0, 2, 5]
    assert R.select_top(s, 0).tolist() == []
    t = torch.argsort(torch.from_numpy(s), stable=True)[-4:]
    assert t.tolist() == R.select_top(s, 4).tolist()


def test_mask_rule():
    H, W = 70, 101
    h, w = R.map_size(H, W)
    assert (h, w) == (18, 26)
    mask = np.zeros((H, W), dtype=np.uint8)
    mask[0, 0] = 1                      # cell (0, 0): no lower bound
    mask[4 * (h - 2) + 3, 4 * (w - 2)] = 7    # the last admitted row and column
    mask[4 * (h - 1), 8] = 1            # partial last row: rejected
    mask[9, 4 * (w - 1)] = 1            # partial last column: rejected
    cells = R.valid_cells(mask, h, w)
    assert sorted(map(tuple, np.argwhere(cells))) == [(0, 0), (h - 2, w - 2)]
    keys = np.zeros(h * w, dtype=np.int32)
    x, y, K = R.select_mask(mask, keys, 5, h, w)      # tied keys: cell order, cyclic
    assert K == 2 and x.tolist() == [0, w - 2, 0, w - 2, 0] and y.tolist() == [0, h - 2, 0, h - 2, 0]
    keys[0] = 9
    x, y, K = R.select_mask(mask, keys, 1, h, w)
    assert (x[0], y[0]) == (w - 2, h - 2)
    x, y, K = R.select_mask(np.zeros((H, W)), keys, 3, h, w)
    assert K == 0 and x.tolist() == [1, 1, 1] and y.tolist() == [1, 1, 1]


def test_library_exports_the_selection_entry_points():
    import _dpvo_hot as H
    lib = H.lib()
    for name in ("dpvo_select_gradient", "dpvo_select_mask", "dpvo_select_mask_workspace_bytes"):
        assert name in H.EXPORTED and hasattr(lib, name)
    assert lib.dpvo_hot_abi_version() == 2
    assert lib.dpvo_select_mask_workspace_bytes(96, 128) >= 96 * 128 * 4
    assert lib.dpvo_select_mask_workspace_bytes(18, 26) % 16 == 0


def test_selection_shims_refuse_cpu_tensors():
    import encoder_ops
    img = frame(64, 96, "noise")
    xs = torch.ones(8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder_ops.select_gradient(img, xs, xs, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        encoder_ops.select_mask(torch.ones(64, 96, dtype=torch.uint8), torch.zeros(16 * 24, dtype=torch.int32), 4,
                                16, 24)


def test_patchifier_has_the_native_select_switch():
    from dpvo.net import Patchifier
    assert Patchifier.NATIVE_SELECT is True
