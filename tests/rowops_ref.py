"""fp64 restatement of the row-GEMM epilogues (csrc/rowgemm.hip) and of SoftAgg
(csrc/updateop.hip) with the error companions their tests are held to.  Plain
numpy: no GPU, no torch, no oracle.  It follows the header comment of
rowgemm.hip and include/dpvo_hot.h, not the kernel bodies:

    acc = A W^T                      (exact values of the fp16 operands)
    y   = fp16(acc + b)  [-> relu | fp16(sigmoid)]
    v   = y | (res32 + res16[idx]) + y | res32 + fp16(gate16 * y)
    v   = LayerNorm_384(v) [-> relu]      (biased variance, eps inside the root)
    heads: z_q = fp16(sum fp16(relu(v)) hw_q + hb_q); d = z_0, z_1; w = fp16(sigmoid(z_2, z_3))
    out32 = v, out16 = fp16(v)
    rows with a_idx < 0 (or past A) are zero rows; res16_idx < 0 adds nothing
    rowadd_ln: v = (a + b16[b_idx]) + c16[c_idx] (indices outside [0, rows) add nothing) [-> LayerNorm]
    rowgemm_pair_pre's A rows: fp16(a32 + b16[idx])

fp16 roundings are np.float16 casts of the fp64 value rounded through
np.float32 first (`f16`), as the kernels round an fp32 register.

Every output comes with a companion.  u = 2^-24; S is the sum of magnitudes
one fp32 rounding can act on; the bar of an fp32 value is k u S, k counted from
the code (rowgemm.hip is built without fast-math: +, *, / round correctly and
FMA contraction only removes steps):

    stage                k                 S                       counted as
    GEMM acc + b         K/32 + 33         |A| |W|^T + |b|         K/32 chained 16x16x32 MFMAs, at most 32 adds
                                                                   inside one, the bias add.  No kernel splits K
                                                                   over accumulators: every one of them chains
                                                                   all K/32 blocks into one accumulator per
                                                                   output (rowgemm3: 2 per 64-wide stage;
                                                                   rowgemm5 / rowpair6 / rowchain5 / narrow:
                                                                   1 per 32-wide stage)
    sigmoid              9                 sigmoid(y)              __expf 4, the add 1, rcpf 4
    RES                  2                 |res32 + r16|, |v|      (res32 + res16) + y
    GATE                 1                 |v|                     gate16 * y is exact in fp32 (two 11-bit
                                                                   significands), fp16 of it is the reference's
                                                                   own rounding, then res32 + . rounds once
    LN mean              19                mean |v|                12 per-lane adds, 4 DPP adds, the lane swap's
                                                                   add, the constant 1/384 and its product
    LN variance          24                var + eps               v - mean 1 and its square 1 (both on d^2: 2),
                                                                   the same 17 adds, 1/384 and product 2,
                                                                   + eps 1, and 2 spare
    LN rsqrtf            4                 rstd                    allowance (nobody has measured it)
    LN output            3 on |g d rstd|, 1 on |out|               v - mean, two products; the add of the bias
    head dot             30                |x| |hw| + |hb|         12 products and 12 adds per lane, 5 reduce adds,
                                                                   the bias
    SoftAgg edge e       see softagg()

LayerNorm's propagation, out_i = g_i d_i r + b_i with d = v - mean, r = (var + eps)^-1/2, q = var + eps:
    d out_i / d mean = -g_i r            d out_i / d var = -g_i d_i r / (2 q)
    E_mean = 19 u mean|v| + mean(E_v)
    E_var  = 2 mean(|d| (E_v + E_mean)) + 24 u q
    E_out  = |g| r (E_v + E_mean) + |g d| r (E_var / (2 q) + 4 u + 3 u) + u |out|
E_v being the bar the rows arrive with.

An fp16 output o of an exact value x whose fp32 register has bar e passes when
    |o - x| <= 2^-11 |x| + e + 2^-25
(half an fp16 ulp, the fp32 bar, half the smallest subnormal): `ok16`.

Where an fp16 rounding is an *intermediate* (y as the next stage's operand,
fp16(relu(v)) in the heads, the on-chip gate), the kernel's value equals the
reference's unless an fp16 rounding boundary lies within the register's bar;
`undecided16` gives |fp16(x + e) - fp16(x - e)| (0 almost everywhere) and the
next stage carries it on as E.  With `exact_inputs` the GEMM stage has no
rounding at all (asserted there), so flags 0 / RELU outputs are compared bit
for bit and every later stage at pure fp32 bars.
"""
import numpy as np

U = 2.0 ** -24
WIDTH = 384
RELU, SIGMOID, RES, GATE, LN, LN_RELU, HEADS = 1, 2, 4, 8, 16, 32, 64
K_SIGMOID, K_MEAN, K_VAR, K_RSQRT, K_HEAD = 9, 19, 24, 4, 30
SA_UNROLL, SA_SPLIT, SA_CAP = 8, 64, 1024


def k_acc(K):
    return K // 32 + 33


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def bar16(x, e):
    """the bar of an fp16 output of the exact value x whose fp32 register has bar e"""
    return 2.0 ** -11 * np.abs(x) + e + 2.0 ** -25


def ok16(o, x, e):
    return np.abs(np.asarray(o, np.float64) - x) <= bar16(x, e)


def undecided16(x, e, relu=False):
    """|fp16(x + e) - fp16(x - e)|: what an intermediate fp16 rounding can differ by"""
    lo, hi = f16(x - e), f16(x + e)
    if relu:
        lo, hi = np.maximum(lo, 0), np.maximum(hi, 0)
    return np.abs(hi - lo)


# ---------------------------------------------------------------------------
# the Linear
def gather_rows(A, a_idx=None, M=None):
    A = np.asarray(A, np.float64)
    if a_idx is None:
        return A if M is None else A[:M]
    a_idx = np.asarray(a_idx)
    ok = (a_idx >= 0) & (a_idx < A.shape[0])
    return np.where(ok[:, None], A[np.clip(a_idx, 0, A.shape[0] - 1)], 0.0)


def linear(A, W, b, act=0, a_idx=None, M=None, eA=None, exact=False):
    """dict: x (the exact value before the last fp16 rounding), e (its fp32 bar),
    y (the reference's fp16 output) and ey (what y can differ by as an operand).
    eA: the bar the A rows arrive with (an earlier stage's ey).  exact: the
    operands are exact_inputs' (every partial sum is exact in fp32: e = 0)."""
    A = gather_rows(A, a_idx, M)
    W = np.asarray(W, np.float64)
    b = np.asarray(b, np.float64)
    K = W.shape[1]
    x = A[:, :K] @ W.T + b
    S = np.abs(A[:, :K]) @ np.abs(W).T + np.abs(b)
    e = (0.0 if exact else k_acc(K)) * U * S
    if eA is not None:
        e = e + gather_rows(eA, a_idx, M)[:, :K] @ np.abs(W).T
    y = f16(x)
    if act == RELU:
        return dict(x=np.maximum(x, 0), e=e, y=np.maximum(y, 0), ey=undecided16(x, e, relu=True), S=S, K=K)
    if act == SIGMOID:
        xs = sigmoid(y)
        es = 0.25 * undecided16(x, e) + K_SIGMOID * U * xs
        return dict(x=xs, e=es, y=f16(xs), ey=undecided16(xs, es), S=S, K=K)
    return dict(x=x, e=e, y=y, ey=undecided16(x, e), S=S, K=K)


# ---------------------------------------------------------------------------
# the row epilogue
def layernorm(v, Ev, g, b, eps, relu=False):
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    mean = v.mean(1, keepdims=True)
    d = v - mean
    var = (d * d).mean(1, keepdims=True)
    q = var + eps
    r = 1.0 / np.sqrt(q)
    out = d * r * g + b
    Em = K_MEAN * U * np.abs(v).mean(1, keepdims=True) + Ev.mean(1, keepdims=True)
    Evar = 2 * (np.abs(d) * (Ev + Em)).mean(1, keepdims=True) + K_VAR * U * q
    E = np.abs(g) * r * (Ev + Em) + np.abs(g * d) * r * (Evar / (2 * q) + (K_RSQRT + 3) * U) + U * np.abs(out)
    if relu:
        out = np.maximum(out, 0)
    return out, E


def epilogue(lin, flags=0, res32=None, res16=None, res16_idx=None, gate16=None, egate=None, ln=None, heads=None,
             eres=None):
    """the row epilogue on linear()'s result: dict v (out32's exact value), E (its
    fp32 bar; out16 is held to bar16(v, E)), and with HEADS: hx [M, 4] (the exact
    values before the heads' last fp16 rounding), hE (their bars).
    egate: what gate16 can differ by (the on-chip gate); eres: res32's own bar."""
    y, ey = lin["y"], lin["ey"]
    M = y.shape[0]
    if flags & (RES | GATE) == 0:
        # out16 / out32 of the plain Linear (or the LayerNorm of it): v is the fp16 y
        v, Ev = y, ey
        pre = dict(x=lin["x"], e=lin["e"])
    else:
        pre = None
        r32 = np.asarray(res32, np.float64)[:M]
        er = np.zeros_like(r32) if eres is None else eres[:M]
        if flags & GATE:
            gt = np.asarray(gate16, np.float64)[:M]
            p = gt * y
            t = f16(p)
            eg = np.zeros_like(p) if egate is None else egate[:M]
            moved = (ey > 0) | (eg > 0)
            Et = np.where(moved, np.abs(gt) * ey + np.abs(y) * eg + ey * eg + undecided16(p, np.abs(gt) * ey + np.abs(y) * eg + U * np.abs(p)), 0.0)
            v = r32 + t
            Ev = Et + er + U * np.abs(v)
        else:
            add = np.zeros_like(r32)
            if res16 is not None:
                r16 = np.asarray(res16, np.float64)
                if res16_idx is None:
                    add = r16[:M]
                else:
                    idx = np.asarray(res16_idx)[:M]
                    add = np.where((idx >= 0)[:, None], r16[np.clip(idx, 0, None)], 0.0)
            v = (r32 + add) + y
            Ev = ey + er + U * np.abs(r32 + add) + U * np.abs(v)
    out = dict(pre=pre)
    if flags & LN:
        v, Ev = layernorm(v, Ev, ln[0], ln[1], ln[2], relu=bool(flags & LN_RELU))
        out["pre"] = None
    if flags & HEADS:
        hw, hb = np.asarray(heads[0], np.float64), np.asarray(heads[1], np.float64)
        x = np.maximum(f16(v), 0)
        Ex = undecided16(v, Ev, relu=True)
        z = x @ hw.T + hb
        Ez = Ex @ np.abs(hw).T + K_HEAD * U * (np.abs(x) @ np.abs(hw).T + np.abs(hb))
        zs = sigmoid(f16(z[:, 2:]))
        Es = 0.25 * undecided16(z[:, 2:], Ez[:, 2:]) + K_SIGMOID * U * zs
        out["hx"] = np.concatenate([z[:, :2], zs], 1)
        out["hE"] = np.concatenate([Ez[:, :2], Es], 1)
    out["v"], out["E"] = v, Ev
    return out


def rowadd_ln(a, b16=None, b_idx=None, c16=None, c_idx=None, ln=None):
    """v = (a + b16[b_idx]) + c16[c_idx] [-> LayerNorm]: dict v, E"""
    a = np.asarray(a, np.float64)
    M = a.shape[0]

    def addend(t, idx):
        if t is None:
            return np.zeros_like(a), np.zeros((M, 1), bool)
        t = np.asarray(t, np.float64)
        idx = np.arange(M) if idx is None else np.asarray(idx)
        ok = ((idx >= 0) & (idx < t.shape[0]))[:, None]
        return np.where(ok, t[np.clip(idx, 0, t.shape[0] - 1)], 0.0), ok

    (vb, okb), (vc, okc) = addend(b16, b_idx), addend(c16, c_idx)
    v = (a + vb) + vc
    Ev = U * np.abs(a + vb) * okb + U * np.abs(v) * okc
    if ln is not None:
        v, Ev = layernorm(v, Ev, ln[0], ln[1], ln[2])
    return dict(v=v, E=Ev)


def pair_pre_rows(a32, b16, b_idx, b_rows=None):
    """rowgemm_pair_pre's A rows: fp16(a32 + b16[idx]); indices outside [0, b_rows) add nothing"""
    b16 = np.asarray(b16, np.float64)
    return f16(rowadd_ln(a32, b16[:b_rows], b_idx)["v"])


# ---------------------------------------------------------------------------
# SoftAgg
def softagg(f, s, group, G, eps=1e-12, long_groups=False, f64_in=False):
    """y[g] = sum_e p_e f_e / (sum_e p_e + eps), p_e = exp(s_e - max_g s): (y, bar).
    The kernels run an online softmax in fp32 in batches of 8.  Roundings the
    weight of edge e passes through, relative to p_e |f_e| (d_e = max - s_e):

        2 d_e      the subtraction s_e - m before its own __expf (u |s_e - m|, a relative u |s_e - m| of p_e)
                   and the subtractions of the later rescales, whose rises telescope to at most d_e
        4 + 1      its own __expf, the product with f_e
        5 (nb - 1) one rescale per later batch: __expf 4, the product 1  (nb = batches of the chain)
        n          the adds after it, n = the chain's length (each acts on a partial sum <= the whole)
        8          dpvo_softagg_csr_long's merge: __expf 4, product 1, 3 adds
        2          l + eps and the division, on |y|
        1, 2 |s|   fp64 inputs: f and s rounded to fp32 first (f64_in)

    The chain is the whole group, or its longest quarter when long_groups and
    the group has >= 64 edges.  The denominator has the same weights with
    f = 1, so bar = u (sum p_e k_e |f_e| / L + |y| (sum p_e k_e / L + 2)).
    Terms with d_e > 104 are zero in fp32: they add their whole magnitude."""
    f, s = np.asarray(f, np.float64), np.asarray(s, np.float64)
    group = np.asarray(group)
    D = f.shape[1]
    y, bar = np.zeros((G, D)), np.zeros((G, D))
    for g in range(G):
        m = np.nonzero(group == g)[0]
        S = len(m)
        if S == 0:
            continue
        fe, se = f[m], s[m]
        mx = se.max(0)
        d = mx - se
        p = np.exp(-d)
        L = p.sum(0)
        n = -(-S // 4) if (long_groups and S >= SA_SPLIT) else S
        nb = -(-n // SA_UNROLL)
        k = 2 * d + 5 + 5 * (nb - 1) + n + (8 if (long_groups and S >= SA_SPLIT) else 0)
        if f64_in:
            k = k + 1 + 2 * (np.abs(se) + np.abs(mx))
        gone = d > 104
        k = np.where(gone, 1.0 / U, k)      # the whole term
        yy = (p * fe).sum(0) / (L + eps)
        y[g] = yy
        bar[g] = U * ((p * k * np.abs(fe)).sum(0) / L + np.abs(yy) * ((p * k).sum(0) / L + 2))
    return y, bar


def group_labels(rng, sizes=(1, 7, 8, 9, 16, 17, 63, 64, 65, 67, SA_CAP, SA_CAP + 1), empty=()):
    """one label vector holding a group of each size, interleaved (edges not
    sorted by group); `empty` group ids are left without edges"""
    ids = [i for i in range(len(sizes) + len(empty)) if i not in empty]
    lab = np.concatenate([np.full(n, i) for i, n in zip(ids, sizes)])
    return lab[rng.permutation(len(lab))].astype(np.int64), len(sizes) + len(empty)


def softagg_logits(rng, lab, D, kind, dtype):
    """N(0, 3) | ascending within a group (the maximum rises in every batch) |
    descending | wide (one group spans the dtype's range: the maximum is subtracted exactly)"""
    E = len(lab)
    s = rng.standard_normal((E, D)) * 3
    if kind in ("ascending", "descending"):
        for g in np.unique(lab):
            m = np.nonzero(lab == g)[0]
            o = np.sort(s[m], 0)
            s[m] = o if kind == "ascending" else o[::-1]
    elif kind == "wide":
        big = 6e4 if dtype == np.float16 else 1e4
        s = s + rng.choice([-big, 0.0, big], size=(E, 1)) * (rng.random((E, D)) < 0.5)
        s = np.clip(s, -big, big)
    elif kind != "normal":
        raise ValueError(kind)
    return s.astype(dtype)


# ---------------------------------------------------------------------------
# inputs
def _ln_params(rng):
    return (rng.uniform(0.5, 1.5, WIDTH).astype(np.float32), (0.1 * rng.standard_normal(WIDTH)).astype(np.float32),
            1e-3)


def _heads(rng):
    return ((0.05 * rng.standard_normal((4, WIDTH))).astype(np.float16), (0.1 * rng.standard_normal(4)).astype(np.float16))


def _is16(x):
    return bool(np.all(f16(x) == x))


def exact_inputs(M, K, seed=0, rows=None):
    """Inputs for which every fp16 rounding point of the GEMM stage is exact:
    A in {-1, 0, 1}, W1 in {-1, 0, 1} / 16, biases multiples of 1/16 in
    [-1/2, 1/2], the second Linear 8 nonzeros of +-1/2 per output row; the
    rowadd / pair_pre operands multiples of 1/4 in [-2, 2].  Asserts it (no
    case is left out): y1, relu(y1), y2 (after both), the formed A rows, and
    gate16 * y in fp32.  All partial sums are multiples of 2^-6 below 2^11
    times that, so the fp32 accumulation is exact in any order too, and the
    double rounding fp64 -> fp32 -> fp16 of `f16` cannot differ from one."""
    rng = np.random.default_rng([seed, M, K])
    rows = rows or M
    d = {}
    d["A"] = rng.integers(-1, 2, (rows, K)).astype(np.float16)
    d["W1"] = (rng.integers(-1, 2, (WIDTH, K)) / 16).astype(np.float16)
    d["b1"] = (rng.integers(-8, 9, WIDTH) / 16).astype(np.float16)
    d["Wb"] = (rng.integers(-1, 2, (WIDTH, K)) / 16).astype(np.float16)      # the pair's / gate's second W
    d["bb"] = (rng.integers(-8, 9, WIDTH) / 16).astype(np.float16)
    W2 = np.zeros((WIDTH, WIDTH))
    for r in range(WIDTH):
        W2[r, rng.choice(WIDTH, 8, replace=False)] = rng.choice([-0.5, 0.5], 8)
    d["W2"] = W2.astype(np.float16)
    d["b2"] = (rng.integers(-8, 9, WIDTH) / 16).astype(np.float16)
    d["a_idx"] = rng.integers(-1, rows, M).astype(np.int64)
    d["a_idx"][:: 5] = d["a_idx"][1 % M]                    # repeated rows
    d["a_idx"][M // 2] = -1
    d["res32"] = rng.standard_normal((M, WIDTH)).astype(np.float32)
    d["res16"] = rng.standard_normal((97, WIDTH)).astype(np.float16)
    d["res16_idx"] = rng.integers(-1, 97, M).astype(np.int64)
    d["res16_idx"][0] = -1
    d["gate16"] = rng.random((M, WIDTH)).astype(np.float16)
    d["ln"] = _ln_params(rng)
    d["heads"] = _heads(rng)
    # rowadd_ln / pair_pre
    d["a32"] = (rng.integers(-8, 9, (M, WIDTH)) / 4).astype(np.float32)
    d["b16"] = (rng.integers(-8, 9, (53, WIDTH)) / 4).astype(np.float16)
    d["c16"] = (rng.integers(-8, 9, (31, WIDTH)) / 4).astype(np.float16)
    d["b_idx"] = rng.integers(-2, 53 + 3, M).astype(np.int64)
    d["c_idx"] = rng.integers(-2, 31 + 3, M).astype(np.int64)
    d["b_idx"][0], d["c_idx"][0] = -1, 31
    # ---- the exactness assertions
    y1 = gather_rows(d["A"], None) @ d["W1"].astype(np.float64).T + d["b1"].astype(np.float64)
    assert _is16(y1) and _is16(np.maximum(y1, 0)), "y1 not exact in fp16"
    assert np.all(f32(np.abs(d["A"].astype(np.float64)) @ np.abs(d["W1"].astype(np.float64)).T * 64) < 2 ** 24)
    for h in (y1, np.maximum(y1, 0)):
        y2 = h @ d["W2"].astype(np.float64).T + d["b2"].astype(np.float64)
        assert _is16(y2), "y2 not exact in fp16"
    yb = d["A"].astype(np.float64) @ d["Wb"].astype(np.float64).T + d["bb"].astype(np.float64)
    assert _is16(yb)
    if K == WIDTH:
        rows16 = rowadd_ln(d["a32"], d["b16"], d["b_idx"])["v"]
        assert _is16(rows16), "pair_pre rows not exact in fp16"
        ya = rows16 @ d["W1"].astype(np.float64).T + d["b1"].astype(np.float64)
        yc = rows16 @ d["Wb"].astype(np.float64).T + d["bb"].astype(np.float64)
        assert _is16(ya) and _is16(yc), "pair_pre outputs not exact in fp16"
        v3 = rowadd_ln(d["a32"], d["b16"], d["b_idx"], d["c16"], d["c_idx"])["v"]
        assert np.all(f32(v3) == v3) and _is16(v3)
    p = d["gate16"].astype(np.float64)[: min(M, rows)] * y1[: min(M, rows)]
    assert np.all(f32(p) == p), "gate16 * y not exact in fp32"
    d["y_absmax"], d["y_std"] = float(np.abs(y1).max()), float(y1.std())
    return d


def random_inputs(M, K, seed=0, small_share=0.08):
    """The existing tests' style: normal A, uniform W / sqrt(K), LN weights in
    [0.5, 1.5] (the lower bound a choice: |g| never hides an error), plus rows
    whose v = res32 + y lies within 1e-2 of one value (`small`: their
    variance is ~3e-5, so ln_eps = 1e-3 carries the result)."""
    rng = np.random.default_rng([seed, M, K, 1])
    d = {}
    d["A"] = rng.standard_normal((M, K)).astype(np.float16)
    d["W1"] = (rng.uniform(-1, 1, (WIDTH, K)) / np.sqrt(K)).astype(np.float16)
    d["b1"] = (rng.uniform(-1, 1, WIDTH) / np.sqrt(K)).astype(np.float16)
    d["ln"] = _ln_params(rng)
    d["heads"] = _heads(rng)
    d["res32"] = rng.standard_normal((M, WIDTH)).astype(np.float32)
    d["res16"] = rng.standard_normal((97, WIDTH)).astype(np.float16)
    d["res16_idx"] = rng.integers(-1, 97, M).astype(np.int64)
    d["gate16"] = sigmoid(rng.standard_normal((M, WIDTH))).astype(np.float16)
    small = rng.random(M) < small_share
    small[:: 9] = True
    y = linear(d["A"], d["W1"], d["b1"])["y"]
    c = rng.uniform(-2, 2, (M, 1))
    flat = (c + rng.uniform(-5e-3, 5e-3, (M, WIDTH)) - y).astype(np.float32)
    d["res32"][small] = flat[small]
    d["small"] = small
    return d
