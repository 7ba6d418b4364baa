"""numpy restatements of the Patchifier's two non-uniform centre choices
(reference dpvo/net.py:103-109,129-134 and :141-144), the rules
csrc/select.hip implements: fp64 gradient scores from the integer gray image,
the stable (lexsort) selections, the mask's cell validity.

SCORE_RTOL is the bar of an fp32 score against the fp64 one: one correctly
rounded square root of an exact integer (2^-24 relative) per term, fifteen
additions of non-negative terms (2^-24 of the running sum each, which the total
bounds), an exact scaling by 1/16 -- 16 roundings, taken with a factor of two
in hand; nothing absolute (a zero score is exactly zero)."""
import numpy as np

SCORE_RTOL = 32 * 2.0 ** -24


def frame(H, W, kind, seed=1):
    """uint8 [3, H, W] test frame: uniform noise, or ("blocky") 8x8 blocks of
    one colour each -- exact zero scores inside the blocks, exact ties"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    blocks = rng.integers(0, 256, (3, (H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
    return np.ascontiguousarray(blocks.repeat(8, axis=1).repeat(8, axis=2)[:, :H, :W])


def map_size(H, W):
    """the stride-4 feature map (conv1 s2, layer2 s2)"""
    return ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2


def gray(image):
    """uint8 [3, H, W] -> int64 [H, W], R + G + B"""
    return np.asarray(image).astype(np.int64).sum(axis=0)


def score_map(image):
    """fp64 [(H-1)//4, (W-1)//4]: 4x4 means of sqrt(dx^2 + dy^2) (net.py:103-109)"""
    g = gray(image)
    dx = g[:-1, 1:] - g[:-1, :-1]
    dy = g[1:, :-1] - g[:-1, :-1]
    mag = np.sqrt((dx * dx + dy * dy).astype(np.float64))
    ph, pw = mag.shape[0] // 4, mag.shape[1] // 4
    return mag[:4 * ph, :4 * pw].reshape(ph, 4, pw, 4).mean(axis=(1, 3))


def scores_at(image, x, y):
    """fp64 [C]: the score map at the candidates, 0 outside it"""
    m = score_map(image)
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    inside = (x >= 0) & (x < m.shape[1]) & (y >= 0) & (y < m.shape[0])
    out = np.zeros(x.shape, dtype=np.float64)
    out[inside] = m[y[inside], x[inside]]
    return out


def select_top(scores, M):
    """indices of the M last candidates in ascending (score, index) order"""
    scores = np.asarray(scores)
    order = np.lexsort((np.arange(scores.size), scores))
    return order[scores.size - M:]


def valid_cells(mask, h, w):
    """bool [h, w]: some set mask pixel falls in the cell, cx < w - 1, cy < h - 1"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    cells = np.zeros((h, w), dtype=bool)
    rr, cc = np.nonzero(mask)
    ok = (rr // 4 < h) & (cc // 4 < w)
    cells[rr[ok] // 4, cc[ok] // 4] = True
    cells[h - 1:, :] = False
    cells[:, w - 1:] = False
    return cells


def select_mask(mask, keys, M, h, w):
    """x, y int64 [M] and K: the valid cells in ascending (key, cell) order,
    repeated cyclically when K < M, all (1, 1) when K == 0"""
    cell = np.nonzero(valid_cells(mask, h, w).reshape(-1))[0]
    K = cell.size
    if K == 0:
        return np.ones(M, dtype=np.int64), np.ones(M, dtype=np.int64), 0
    keys = np.asarray(keys).astype(np.int64)
    cell = cell[np.lexsort((cell, keys[cell]))]
    pick = cell[np.arange(M) % K]
    return pick % w, pick // w, K
