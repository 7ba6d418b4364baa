"""CPU pins of tests/rowops_ref.py, the fp64 restatement the GPU row-GEMM /
SoftAgg kernel tests compare against: it agrees with a torch fp64 composition
and with the oracle's SoftAgg at 1e-12, `exact_inputs` is exact at every K the
GPU tests use, `random_inputs` holds its small-variance class, and an fp32
numpy restatement of each stage (accumulating in a shuffled order, reducing
LayerNorm by a tree, running the online softmax in batches of 8 with
rescaling) stays inside its own counted bar.  The last measures the
reference's bars, not the code under test: they are neither vacuous nor too
tight.  The printed worst ratios are recorded in profiles/rowops_tests/NOTES.md."""
import numpy as np
import pytest
import torch

import rowops_ref as R
from oracle import oracle

KS = (64, 128, 192, 256, 384, 896)
F = torch.nn.functional


def t64(x):
    return torch.from_numpy(np.asarray(x, np.float64))


def h(x):
    """fp16 rounding (through fp32) of an fp64 torch tensor"""
    return x.float().half().double()


def close(got, want, tol=1e-12):
    want = want.numpy() if isinstance(want, torch.Tensor) else want
    err = np.abs(got - want) / (1 + np.abs(want))
    assert err.max() <= tol, float(err.max())


@pytest.mark.parametrize("flags", [0, R.RELU, R.SIGMOID, R.LN | R.LN_RELU, R.RES, R.RES | R.LN, R.GATE, R.GATE | R.LN,
                                   R.GATE | R.HEADS])
def test_epilogue_matches_torch_fp64(flags):
    d = R.random_inputs(65, 128, seed=3)
    A, W, b = t64(d["A"]), t64(d["W1"]), t64(d["b1"])
    act = flags & 3
    lin = R.linear(d["A"], d["W1"], d["b1"], act=act)
    y = h(A @ W.T + b)
    if act == R.RELU:
        y = y.clamp_min(0)
    if act == R.SIGMOID:
        y = h(torch.sigmoid(y))
    close(lin["y"], y, 0)
    kw = dict(res32=d["res32"], res16=d["res16"], res16_idx=d["res16_idx"]) if flags & R.RES else {}
    if flags & R.GATE:
        kw = dict(res32=d["res32"], gate16=d["gate16"])
    r = R.epilogue(lin, flags & ~3, ln=d["ln"], heads=d["heads"], **kw)
    v = y
    if flags & R.RES:
        idx = torch.from_numpy(d["res16_idx"])
        add = torch.where((idx >= 0)[:, None], t64(d["res16"])[idx.clamp_min(0)], torch.zeros(1, dtype=torch.float64))
        v = t64(d["res32"]) + add + y
    if flags & R.GATE:
        v = t64(d["res32"]) + h(t64(d["gate16"]) * y)
    if flags & R.LN:
        v = F.layer_norm(v, (384,), t64(d["ln"][0]), t64(d["ln"][1]), d["ln"][2])
        if flags & R.LN_RELU:
            v = v.clamp_min(0)
    close(r["v"], v)
    if flags & R.HEADS:
        z = h(h(v.clamp_min(0)) @ t64(d["heads"][0]).T + t64(d["heads"][1]))
        # (hx is the value before the last fp16 rounding: d = z's exact sum, w = sigmoid(fp16 z))
        close(R.f16(r["hx"][:, :2]), z[:, :2], 0)
        close(r["hx"][:, 2:], torch.sigmoid(z[:, 2:]))


def test_rowadd_and_pair_pre_match_torch_fp64():
    d = R.exact_inputs(65, 384, seed=1)
    a, b16, c16 = t64(d["a32"]), t64(d["b16"]), t64(d["c16"])
    bi, ci = torch.from_numpy(d["b_idx"]), torch.from_numpy(d["c_idx"])
    z = torch.zeros(1, dtype=torch.float64)
    vb = torch.where(((bi >= 0) & (bi < 53))[:, None], b16[bi.clamp(0, 52)], z)
    vc = torch.where(((ci >= 0) & (ci < 31))[:, None], c16[ci.clamp(0, 30)], z)
    close(R.rowadd_ln(d["a32"], d["b16"], d["b_idx"])["v"], a + vb)
    r = R.rowadd_ln(d["a32"], d["b16"], d["b_idx"], d["c16"], d["c_idx"], ln=d["ln"])
    close(r["v"], F.layer_norm(a + vb + vc, (384,), t64(d["ln"][0]), t64(d["ln"][1]), d["ln"][2]))
    vb40 = torch.where(((bi >= 0) & (bi < 40))[:, None], b16[bi.clamp(0, 39)], z)
    close(R.pair_pre_rows(d["a32"], d["b16"], d["b_idx"], b_rows=40), h(a + vb40), 0)


@pytest.mark.parametrize("kind", ["normal", "ascending", "descending", "wide"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_softagg_restatement_matches_oracle(kind, dtype):
    rng = np.random.default_rng(5)
    lab, G = R.group_labels(rng, empty=(3,))
    D = 6
    s = R.softagg_logits(rng, lab, D, kind, dtype)
    f = (2 * rng.standard_normal((len(lab), D))).astype(dtype)
    y, bar = R.softagg(f, s, lab, G)
    want = oracle.softagg(f.astype(np.float64), s.astype(np.float64), lab, G)
    close(y, want)
    assert (y[3] == 0).all() and np.isfinite(bar).all()
    sizes = np.bincount(lab, minlength=G)
    assert set(sizes) >= {0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 67, R.SA_CAP, R.SA_CAP + 1}
    assert (np.diff(lab) < 0).any()      # not sorted by group
    if kind == "ascending":
        m = np.nonzero(lab == G - 1)[0]
        assert (np.diff(s[m].astype(np.float64), axis=0) >= 0).all()


@pytest.mark.parametrize("K", KS)
def test_exact_inputs_are_exact(K):
    """the generator's own assertions, at every K the GPU tests use (it raises otherwise)"""
    d = R.exact_inputs(257, K, seed=0)
    assert 0.3 < d["y_std"] < 1.5 and d["y_absmax"] < 8
    l1 = R.linear(d["A"], d["W1"], d["b1"], act=R.RELU, exact=True)
    assert (l1["ey"] == 0).all() and (l1["x"] == l1["y"]).all()
    l2 = R.linear(l1["y"], d["W2"], d["b2"], exact=True)
    assert (l2["x"] == l2["y"]).all() and (l2["ey"] == 0).all()


def test_random_inputs_class_shares():
    d = R.random_inputs(257, 384, seed=0)
    assert d["small"].mean() >= 0.05
    v = R.epilogue(R.linear(d["A"], d["W1"], d["b1"]), R.RES, res32=d["res32"])["v"]
    spread = v.max(1) - v.min(1)
    assert (spread[d["small"]] <= 2e-2).all() and (spread[~d["small"]] > 1).all()
    # there ln_eps = 1e-3 is most of var + eps
    assert (v[d["small"]].var(1) < 1e-4).all()
    assert d["ln"][0].min() >= 0.5


# ---------------------------------------------------------------------------
# fp32 restatements inside their own bars
def tree_sum32(x):
    """pairwise fp32 tree over the last axis (384 = 3 * 128: 3 sequential adds, then a binary tree)"""
    x = x.astype(np.float32)
    x = (x[..., 0::3] + x[..., 1::3]) + x[..., 2::3]
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def ln32(v, g, b, eps, relu=False):
    v = v.astype(np.float32)
    mean = tree_sum32(v) * np.float32(1.0 / 384)
    dd = v - mean[:, None]
    var = tree_sum32(dd * dd) * np.float32(1.0 / 384)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    out = dd * rstd[:, None] * g.astype(np.float32) + b.astype(np.float32)
    return np.maximum(out, 0) if relu else out


def test_fp32_gemm_in_shuffled_order_is_inside_its_bar(capsys):
    M, K = 257, 896
    d = R.random_inputs(M, K, seed=2)
    lin = R.linear(d["A"], d["W1"], d["b1"])
    A, W = d["A"].astype(np.float32), d["W1"].astype(np.float32)
    acc = np.zeros((M, 384), np.float32)
    for k in np.random.default_rng(0).permutation(K):
        acc = acc + A[:, k:k + 1] * W[None, :, k]
    got = acc + d["b1"].astype(np.float32)
    ratio = np.abs(got - lin["x"]) / (R.U * lin["S"])
    with capsys.disabled():
        print(f"\n[rowops host] fp32 GEMM, shuffled k, M={M} K={K}: worst {ratio.max():.2f} u S_acc, bar {R.k_acc(K)}")
    assert ratio.max() <= R.k_acc(K)
    assert ratio.max() > 0.5      # the bar is not vacuous by orders of magnitude for this order
    assert R.ok16(got.astype(np.float16), lin["x"], lin["e"]).all()


def test_fp32_epilogues_are_inside_their_bars(capsys):
    M, K = 257, 384
    d = R.random_inputs(M, K, seed=4)
    lin = R.linear(d["A"], d["W1"], d["b1"])
    y32 = lin["y"].astype(np.float32)
    out = []
    # RES | LN on the kernel's own y (no intermediate flips: the bar is the fp32 one alone)
    r = R.epilogue(dict(lin, ey=np.zeros_like(lin["ey"])), R.RES | R.LN, res32=d["res32"], ln=d["ln"])
    v32 = d["res32"] + y32
    got = ln32(v32, *d["ln"])
    ratio = np.abs(got - r["v"]) / r["E"]
    out.append(("RES|LN out32", ratio.max(), ratio[d["small"]].max()))
    assert ratio.max() <= 1
    # GATE | HEADS
    r = R.epilogue(dict(lin, ey=np.zeros_like(lin["ey"])), R.GATE | R.HEADS, res32=d["res32"], gate16=d["gate16"],
                   heads=d["heads"])
    t = (d["gate16"].astype(np.float32) * y32).astype(np.float16).astype(np.float32)
    v32 = d["res32"] + t
    ratio = np.abs(v32 - r["v"]) / r["E"]
    out.append(("GATE out32", ratio.max(), 0))
    assert ratio.max() <= 1
    x = np.maximum(v32, 0).astype(np.float16).astype(np.float32)
    hw, hb = d["heads"][0].astype(np.float32), d["heads"][1].astype(np.float32)
    z = np.zeros((M, 4), np.float32)
    for k in np.random.default_rng(1).permutation(384):
        z = z + x[:, k:k + 1] * hw[None, :, k]
    z = z + hb
    ratio = np.abs(z[:, :2] - r["hx"][:, :2]) / r["hE"][:, :2]
    out.append(("head dot", ratio.max(), 0))
    assert ratio.max() <= 1
    assert R.ok16(z[:, :2].astype(np.float16), r["hx"][:, :2], r["hE"][:, :2]).all()
    with capsys.disabled():
        for name, a, b in out:
            print(f"[rowops host] fp32 {name}: worst error / bar {a:.3f}" + (f" (small-variance rows {b:.3f})" if b else ""))


def online32(f, s, batch=8):
    f, s = f.astype(np.float32), s.astype(np.float32)
    m = np.full(f.shape[1], -np.inf, np.float32)
    l = np.zeros(f.shape[1], np.float32)
    acc = np.zeros(f.shape[1], np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(0, len(f), batch):
            mb = np.maximum(m, s[i:i + batch].max(0))
            a = np.where(np.isneginf(m), np.float32(0), np.exp(m - mb)).astype(np.float32)
            l, acc = l * a, acc * a
            for e in range(i, min(i + batch, len(f))):
                p = np.exp(s[e] - mb).astype(np.float32)
                l = l + p
                acc = acc + p * f[e]
            m = mb
    return acc / (l + np.float32(1e-12))


@pytest.mark.parametrize("kind", ["normal", "ascending", "descending", "wide"])
def test_fp32_online_softmax_is_inside_its_bar(kind, capsys):
    rng = np.random.default_rng(7)
    lab, G = R.group_labels(rng)
    D = 8
    s = R.softagg_logits(rng, lab, D, kind, np.float32)
    f = (2 * rng.standard_normal((len(lab), D))).astype(np.float32)
    y, bar = R.softagg(f, s, lab, G)
    worst = 0.0
    for g in range(G):
        m = np.nonzero(lab == g)[0]
        got = online32(f[m], s[m])
        ratio = np.abs(got - y[g]) / bar[g]
        assert ratio.max() <= 1, (g, len(m), float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    with capsys.disabled():
        print(f"[rowops host] fp32 online softmax ({kind}): worst error / bar {worst:.3f}")
