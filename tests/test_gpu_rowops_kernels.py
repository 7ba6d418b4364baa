"""Every entry point of csrc/rowgemm.hip and the three SoftAgg entry points of
csrc/updateop.hip against the fp64 restatement of tests/rowops_ref.py, at the
tiling's edges: bit for bit where `exact_inputs` makes every fp16 rounding
point exact, at the counted bars of rowops_ref's tables everywhere else.  No
tolerance here is a chosen number: each bar is k u S from the module's
docstring, and an fp16 output is held to half an ulp plus its fp32 bar.

Anchors that stay elsewhere: dpvo_rowchain3 has a LayerNorm -> fp16 in the
middle, so no input makes its second intermediate exact; it stays anchored by
test_gpu_rowgemm.test_rowchain3_is_chain_plus_rowgemm (bit-identity to
rowchain + rowgemm), both of which are anchored here.

Every `[rowops] name: worst error / bar` line printed here is recorded in
profiles/rowops_tests/NOTES.md."""
import functools

import numpy as np
import pytest
import torch

import rowops_ref as R
from tests_helpers import same

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned")]

MS = (1, 63, 64, 65, 127, 128, 129, 257)
ROWS = 257
PAD = 3                      # sentinel rows past M
S16, S32 = 7.0, -77.0
K_ROW = (64, 128, 192, 384, 896)      # [384][K] W
K_KB = (64, 128, 256, 384, 896)       # k-blocked W


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def held(name, got, x, bar):
    """|got - x| <= bar elementwise; prints the worst ratio"""
    err = np.abs(host(got) - x)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    w = float(ratio.max()) if ratio.size else 0.0
    print(f"[rowops] {name}: worst error / bar {w:.3f}")
    assert w <= 1, f"{name}: {int((ratio > 1).sum())} of {ratio.size} outside the bar, worst {w:.3f} at " \
                   f"{np.unravel_index(int(ratio.argmax()), ratio.shape)}"
    return w


def held16(name, got, x, e):
    return held(name, got, x, R.bar16(x, e))


def bits16(got, want, what):
    assert same(got, dev(np.asarray(want).astype(np.float16)), what)


def bits32(got, want, what):
    assert same(got, dev(np.asarray(want).astype(np.float32)), what)


def full16(rows, ld=R.WIDTH):
    return torch.full((rows, ld), S16, dtype=torch.float16, device="cuda")


def full32(rows):
    return torch.full((rows, R.WIDTH), S32, dtype=torch.float32, device="cuda")


def untouched(t, sentinel, what):
    assert bool((t == sentinel).all()), f"{what}: rows past the row count were written"


def poison_rows(t, what):
    """rows the shim allocated (0xff-filled by `poisoned`) and the kernel must not write"""
    ib = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    assert bool((t.contiguous().view(ib) == -1).all()), f"{what}: rows past the row count were written"


@functools.lru_cache(maxsize=None)
def EX(K):
    d = R.exact_inputs(ROWS, K, seed=0)
    t = {k: dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    t["ln"] = (dev(d["ln"][0]), dev(d["ln"][1]), d["ln"][2])
    t["heads"] = (dev(d["heads"][0]), dev(d["heads"][1]))
    return d, t


@functools.lru_cache(maxsize=None)
def RND(K):
    d = R.random_inputs(ROWS, K, seed=0)
    t = {k: dev(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    t["ln"] = (dev(d["ln"][0]), dev(d["ln"][1]), d["ln"][2])
    t["heads"] = (dev(d["heads"][0]), dev(d["heads"][1]))
    return d, t


@functools.lru_cache(maxsize=None)
def LIN(K, act, which="W1", gathered=False):
    d, _ = EX(K)
    W, b = (d["W1"], d["b1"]) if which == "W1" else (d["Wb"], d["bb"])
    return R.linear(d["A"], W, b, act=act, a_idx=d["a_idx"] if gathered else None, exact=True)


def check_y(out, lin, act, what):
    """the plain Linear's fp16 output: bit for bit, or (sigmoid) half an ulp + 9 u"""
    M = out.shape[0]
    if act == R.SIGMOID:
        held16(what, out, lin["x"][:M], lin["e"][:M])
    else:
        bits16(out, lin["y"][:M], what)


def weight(t, layout, name="W1"):
    import update_ops as U
    return U.kblock(t[name]) if layout == "kb" else t[name]


# ---------------------------------------------------------------------------
# dpvo_rowgemm, flags 0 / RELU / SIGMOID
@pytest.mark.parametrize("flags", [0, R.RELU, R.SIGMOID])
@pytest.mark.parametrize("layout,K", [("row", k) for k in K_ROW] + [("kb", k) for k in K_KB])
def test_linear(layout, K, flags):
    """rowgemm3_kernel ([384][K]: the 64-row epilogue halves at +-1 row, the A
    ring at K/64 = 1, 2, 3) and rowgemm5_kernel (k-blocked), every M of the
    grid; then a gathered A (negative and repeated rows), lda > K, and a device
    row count on the [384][K] kernel."""
    import update_ops as U
    d, t = EX(K)
    W = weight(t, layout)
    lin = LIN(K, flags)
    for M in MS:
        out = full16(M + PAD)
        U.rowgemm(t["A"][:M], W, t["b1"], flags=flags, out16=out)
        check_y(out[:M], lin, flags, f"rowgemm {layout} K={K} flags={flags} M={M}")
        untouched(out[M:], S16, f"rowgemm {layout} K={K} M={M}")
    for M in (65, 129):
        g = R.linear(d["A"], d["W1"], d["b1"], act=flags, a_idx=d["a_idx"][:M], exact=True)
        out = full16(M + PAD)
        U.rowgemm(t["A"], W, t["b1"], flags=flags, a_idx=t["a_idx"][:M], out16=out)
        check_y(out[:M], g, flags, f"rowgemm {layout} K={K} flags={flags} a_idx M={M}")
        untouched(out[M:], S16, "a_idx")
    wide = torch.full((ROWS, K + 8), 3.0, dtype=torch.float16, device="cuda")
    wide[:, :K] = t["A"]
    out = full16(ROWS + PAD, R.WIDTH + 4)           # ldo16 > 384 too
    U.rowgemm(wide[:, :K], W, t["b1"], flags=flags, out16=out[:, :R.WIDTH])
    check_y(out[:ROWS, :R.WIDTH], lin, flags, f"rowgemm {layout} K={K} lda > K")
    untouched(out[ROWS:], S16, "lda")
    untouched(out[:, R.WIDTH:], S16, "ldo16 padding")
    if layout == "row":
        for Md in (0, 100):
            out = full16(ROWS)
            U.rowgemm(t["A"], W, t["b1"], flags=flags, out16=out, M_dev=torch.tensor([Md], device="cuda"))
            check_y(out[:Md], lin, flags, f"rowgemm row K={K} M_dev={Md}")
            untouched(out[Md:], S16, "M_dev")


@pytest.mark.parametrize("flags", [0, R.RELU, R.SIGMOID])
@pytest.mark.parametrize("K", [384, 896])
def test_linear_narrow_device_row_count(K, flags):
    """rowgemm_narrow_kernel<6> / <14> (k-blocked W with a device row count):
    32-row tiles at +-1 row under M = 4096; *M_dev = 0 writes nothing."""
    import update_ops as U
    d, t = EX(K)
    W = weight(t, "kb")
    lin = LIN(K, flags)
    for Md in (0, 1, 31, 32, 33, 100):
        out = full16(4096)
        U.rowgemm(t["A"], W, t["b1"], flags=flags, M=4096, out16=out, M_dev=torch.tensor([Md], device="cuda"))
        check_y(out[:Md], lin, flags, f"narrow K={K} flags={flags} M_dev={Md}")
        untouched(out[Md:], S16, f"narrow M_dev={Md}")
    idx = t["a_idx"].repeat(16)[:4096]
    g = R.linear(d["A"], d["W1"], d["b1"], act=flags, a_idx=d["a_idx"][:100], exact=True)
    out = full16(4096)
    U.rowgemm(t["A"], W, t["b1"], flags=flags, a_idx=idx, out16=out, M_dev=torch.tensor([100], device="cuda"))
    check_y(out[:100], g, flags, f"narrow K={K} a_idx")
    untouched(out[100:], S16, "narrow a_idx")


# ---------------------------------------------------------------------------
# dpvo_rowgemm, every dispatched epilogue
EPI = {
    "ln_relu": (R.LN | R.LN_RELU, ()),
    "res": (R.RES, ("res32",)),
    "res_r16": (R.RES, ("res32", "res16rows")),
    "res_r16_idx": (R.RES, ("res32", "res16", "res16_idx")),
    "res_ln": (R.RES | R.LN, ("res32",)),
    "res_ln_idx": (R.RES | R.LN, ("res32", "res16", "res16_idx")),
    "gate": (R.GATE, ("res32", "gate16")),
    "gate_ln": (R.GATE | R.LN, ("res32", "gate16")),
    "gate_heads": (R.GATE | R.HEADS, ("res32", "gate16")),
}


def epi_kwargs(case, d, t, M=None):
    """(reference kwargs, kernel kwargs) of an EPI case; res16rows: res16 without an index (row m)"""
    flags, names = EPI[case]
    kr, kk = {}, {}
    for n in names:
        src = "gate16" if n == "res16rows" else n
        dst = "res16" if n == "res16rows" else n
        kr[dst] = d[src]
        kk[dst] = t[src] if (M is None or n == "res16") else t[src][:M]
    if flags & R.LN:
        kr["ln"], kk["ln"] = d["ln"], t["ln"]
    if flags & R.HEADS:
        kr["heads"], kk["heads"] = d["heads"], t["heads"]
    return flags, kr, kk


def check_epilogue(what, r, M, o32, o16, ho):
    if o32 is not None:
        held(what + " out32", o32[:M], r["v"][:M], r["E"][:M])
    if o16 is not None:
        held16(what + " out16", o16[:M], r["v"][:M], r["E"][:M])
    if ho is not None:
        held16(what + " heads", ho[:M], r["hx"][:M], r["hE"][:M])


@pytest.mark.parametrize("case", list(EPI))
@pytest.mark.parametrize("inputs,K", [("exact", 64), ("exact", 192), ("exact", 384), ("random", 128),
                                      ("random", 384), ("random", 896)])
def test_epilogues(inputs, K, case):
    """out32, out16 and head_out of every epilogue rowgemm3 is dispatched for,
    each against the reference at its counted bar; the bare GATE case
    (compiled in, called by nothing else) included."""
    import update_ops as U
    d, t = EX(K) if inputs == "exact" else RND(K)
    flags, kr, _ = epi_kwargs(case, d, t)
    lin = R.linear(d["A"], d["W1"], d["b1"], exact=inputs == "exact")
    r = R.epilogue(lin, flags, **kr)
    for M in MS:
        _, _, kk = epi_kwargs(case, d, t, M)
        o32, o16 = full32(M + PAD), full16(M + PAD)
        _, _, ho = U.rowgemm(t["A"][:M], t["W1"], t["b1"], flags=flags, out32=o32, out16=o16, **kk)
        check_epilogue(f"rowgemm {case} {inputs} K={K} M={M}", r, M, o32, o16, ho)
        untouched(o32[M:], S32, f"{case} out32 M={M}")
        untouched(o16[M:], S16, f"{case} out16 M={M}")
        if ho is not None:
            assert ho.shape == (M, 4)


@pytest.mark.parametrize("flags", [0, R.RELU, R.SIGMOID])
@pytest.mark.parametrize("K", [128, 384, 896])
def test_linear_random_inputs(K, flags):
    """the [384][K] kernel on normal A / uniform W: y within half an fp16 ulp
    plus (K/32 + 33) u S_acc of the exact sum -- where `bias after the fp16
    rounding` shows."""
    import update_ops as U
    d, t = RND(K)
    lin = R.linear(d["A"], d["W1"], d["b1"], act=flags)
    out = full16(ROWS + PAD)
    U.rowgemm(t["A"], t["W1"], t["b1"], flags=flags, out16=out)
    held16(f"rowgemm row random K={K} flags={flags}", out[:ROWS], lin["x"], lin["e"])
    untouched(out[ROWS:], S16, "random")


# ---------------------------------------------------------------------------
# the pair kernels
@pytest.mark.parametrize("layout,K", [("row", k) for k in K_ROW] + [("kb", k) for k in K_KB])
def test_rowgemm_pair(layout, K):
    """dpvo_rowgemm_pair: rowgemm3 DUAL ([384][K]), rowpair6 (k-blocked, the A
    tile resident: K = 128 .. 384) and rowgemm5 DUAL (K = 64: shorter than the
    staging depth; K = 896: the tile does not fit); then a device row count."""
    import update_ops as U
    d, t = EX(K)
    Wa, Wb = weight(t, layout, "W1"), weight(t, layout, "Wb")
    la, lb = LIN(K, 0, "W1"), LIN(K, 0, "Wb")
    for M in MS:
        f, g = U.rowgemm_pair(t["A"][:M], Wa, t["b1"], Wb, t["bb"])
        bits16(f, la["y"][:M], f"pair {layout} K={K} M={M} f")
        bits16(g, lb["y"][:M], f"pair {layout} K={K} M={M} g")
    for Md in (0, 100, 129):
        f, g = U.rowgemm_pair(t["A"], Wa, t["b1"], Wb, t["bb"], M_dev=torch.tensor([Md], device="cuda"))
        bits16(f[:Md], la["y"][:Md], f"pair {layout} K={K} M_dev={Md} f")
        bits16(g[:Md], lb["y"][:Md], f"pair {layout} K={K} M_dev={Md} g")
        poison_rows(f[Md:], "pair M_dev f")
        poison_rows(g[Md:], "pair M_dev g")


@pytest.mark.parametrize("b_rows", [None, 40])
def test_rowgemm_pair_pre(b_rows):
    """dpvo_rowgemm_pair_pre: the A rows fp16(a32 + b16[idx]) with negative
    indices, indices past b_rows (inside the buffer when b_rows = 40 < 53) and
    past the buffer: bit for bit (the sums are exact in fp16)."""
    import update_ops as U
    d, t = EX(384)
    rows = R.pair_pre_rows(d["a32"], d["b16"], d["b_idx"], b_rows)
    assert ((d["b_idx"] < 0).any() and (d["b_idx"] >= 53).any() and ((d["b_idx"] >= 40) & (d["b_idx"] < 53)).any())
    la = R.linear(rows, d["W1"], d["b1"], exact=True)
    lb = R.linear(rows, d["Wb"], d["bb"], exact=True)
    assert (la["x"] == la["y"]).all() and (lb["x"] == lb["y"]).all()
    Wa, Wb = weight(t, "kb", "W1"), weight(t, "kb", "Wb")
    for M in MS:
        f, g = U.rowgemm_pair_pre(t["a32"][:M], t["b16"], t["b_idx"][:M], Wa, t["b1"], Wb, t["bb"], b_rows=b_rows)
        bits16(f, la["y"][:M], f"pair_pre M={M} f")
        bits16(g, lb["y"][:M], f"pair_pre M={M} g")


# ---------------------------------------------------------------------------
# dpvo_rowadd_ln
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("addends", [1, 2])
@pytest.mark.parametrize("a_dtype", ["fp32", "fp16_padded"])
def test_rowadd_ln(a_dtype, addends, with_ln):
    """a + b16[b_idx] (+ c16[c_idx]) [-> LayerNorm]: the sums are exact (dyadic
    operands), so without LN out32 / out16 are compared bit for bit; with LN at
    the LayerNorm bars.  want32 / want16 separately and together."""
    import update_ops as U
    d, t = EX(384)
    if a_dtype == "fp32":
        a = t["a32"]
    else:
        buf = torch.full((ROWS, R.WIDTH + 4), 5.0, dtype=torch.float16, device="cuda")
        buf[:, :R.WIDTH] = t["a32"].half()
        a = buf[:, :R.WIDTH]
    c = dict(c16=d["c16"], c_idx=d["c_idx"]) if addends == 2 else {}
    r = R.rowadd_ln(d["a32"], d["b16"], d["b_idx"], ln=d["ln"] if with_ln else None, **c)
    if not with_ln:
        assert (R.f16(r["v"]) == r["v"]).all()
    for M in MS:
        kw = dict(ln=t["ln"] if with_ln else None)
        if addends == 2:
            kw.update(c16=t["c16"], c_idx=t["c_idx"][:M])
        both = U.rowadd_ln(a[:M], t["b16"], t["b_idx"][:M], **kw)
        only32 = U.rowadd_ln(a[:M], t["b16"], t["b_idx"][:M], want16=False, **kw)
        only16 = U.rowadd_ln(a[:M], t["b16"], t["b_idx"][:M], want32=False, **kw)
        assert only32[1] is None and only16[0] is None
        assert same(only32[0], both[0]) and same(only16[1], both[1])
        what = f"rowadd_ln {a_dtype} addends={addends} ln={with_ln} M={M}"
        if with_ln:
            held(what + " out32", both[0], r["v"][:M], r["E"][:M])
            held16(what + " out16", both[1], r["v"][:M], r["E"][:M])
        else:
            bits32(both[0], r["v"][:M], what + " out32")
            bits16(both[1], r["v"][:M], what + " out16")


# ---------------------------------------------------------------------------
# the chains
@pytest.mark.parametrize("case", ["ln_relu", "res", "res_r16_idx", "gate_ln", "gate_heads"])
@pytest.mark.parametrize("act1,K", [(R.RELU, 64), (R.RELU, 384), (R.RELU, 896), (R.SIGMOID, 384), (0, 384)])
def test_rowchain(act1, K, case):
    """dpvo_rowchain against the reference of the whole chain.  With a ReLU (or
    no) first activation the intermediate is exact, so the second GEMM's
    output is too and the epilogue meets the single-launch bars; a sigmoid
    first activation carries its `undecided16` into the second GEMM's bar.
    The RES cases gather their A rows (negative and repeated indices)."""
    import update_ops as U
    d, t = EX(K)
    gathered = case.startswith("res")
    flags, kr, _ = epi_kwargs(case, d, t)
    l1 = R.linear(d["A"], d["W1"], d["b1"], act=act1, a_idx=d["a_idx"] if gathered else None, exact=True)
    l2 = R.linear(l1["y"], d["W2"], d["b2"], eA=l1["ey"], exact=act1 != R.SIGMOID)
    if act1 != R.SIGMOID:
        assert (l1["ey"] == 0).all() and (l2["x"] == l2["y"]).all()
    r = R.epilogue(l2, flags, **kr)
    for M in MS:
        _, _, kk = epi_kwargs(case, d, t, M)
        a = dict(a_idx=t["a_idx"][:M]) if gathered else dict(M=M)
        o32, o16, ho = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=act1, flags=flags, want32=True,
                                  **a, **kk)
        assert o32.shape == (M, R.WIDTH) and o16.shape == (M, R.WIDTH)
        check_epilogue(f"rowchain {case} act1={act1} K={K} M={M}", r, M, o32, o16, ho)


@pytest.mark.parametrize("K", [384, 896])
def test_rowchain_plain_outputs_are_bit_exact(K):
    """the chain's GEMM outputs themselves: RES with res32 = 0 leaves
    out32 = (0 + 0) + y2 and out16 = y2, exact with `exact_inputs` -- compared
    bit for bit."""
    import update_ops as U
    d, t = EX(K)
    l1 = R.linear(d["A"], d["W1"], d["b1"], act=R.RELU, exact=True)
    l2 = R.linear(l1["y"], d["W2"], d["b2"], exact=True)
    zero = torch.zeros(ROWS, R.WIDTH, device="cuda")
    for M in MS:
        o32, o16, _ = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=R.RELU, flags=R.RES, M=M,
                                 res32=zero[:M], want32=True)
        bits32(o32, l2["y"][:M], f"rowchain y2 K={K} M={M} out32")
        bits16(o16, l2["y"][:M], f"rowchain y2 K={K} M={M} out16")


@pytest.mark.parametrize("case", ["gate_ln", "gate_heads"])
def test_rowchain_gated(case):
    """dpvo_rowchain_gated: the on-chip gate is an approximate sigmoid rounded
    to fp16, so it can differ from the reference's gate by `undecided16` of
    its 9-rounding bar, and fp16(gate * y) can flip with it: the chain is held
    to the bar propagated from the gate's (|y| times the gate's, plus the fp16
    step of the product where either moved).  The sharp anchor of this path is
    the explicit-gate16 case (test_rowchain / test_epilogues) plus
    test_gpu_rowgemm.test_rowchain_gated_is_gate_gemm_plus_chain (bit-identity)."""
    import update_ops as U
    d, t = EX(384)
    flags, kr, _ = epi_kwargs(case, d, t)
    gt = R.linear(d["A"], d["Wb"], d["bb"], act=R.SIGMOID, exact=True)
    l1 = R.linear(d["A"], d["W1"], d["b1"], act=R.RELU, exact=True)
    l2 = R.linear(l1["y"], d["W2"], d["b2"], exact=True)
    kr.update(gate16=gt["y"], egate=gt["ey"])
    r = R.epilogue(l2, flags, **kr)
    print(f"[rowops] rowchain_gated {case}: gate undecided at {(gt['ey'] > 0).mean():.2e} of the elements")
    for M in MS:
        _, _, kk = epi_kwargs(case, d, t, M)
        kk.pop("gate16")
        o32, o16, ho = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=R.RELU, flags=flags, M=M,
                                  want32=True, gate=(t["Wb"], t["bb"]), **kk)
        check_epilogue(f"rowchain_gated {case} M={M}", r, M, o32, o16, ho)


def test_rowchain_gated_pre():
    """dpvo_rowchain_gated_pre: the residual rows LayerNorm(a32 + b16[b_idx] +
    c16[c_idx]) formed in the epilogue (negative and out-of-range indices add
    nothing), then the gated chain's GATE | LN on them: the first LayerNorm's
    bar arrives as the residual's."""
    import update_ops as U
    d, t = EX(384)
    rng = np.random.default_rng(11)
    ln0 = (rng.uniform(0.5, 1.5, R.WIDTH).astype(np.float32), (0.1 * rng.standard_normal(R.WIDTH)).astype(np.float32),
           1e-3)
    pre = R.rowadd_ln(d["a32"], d["b16"], d["b_idx"], d["c16"], d["c_idx"], ln=ln0)
    gt = R.linear(d["A"], d["Wb"], d["bb"], act=R.SIGMOID, exact=True)
    l1 = R.linear(d["A"], d["W1"], d["b1"], act=R.RELU, exact=True)
    l2 = R.linear(l1["y"], d["W2"], d["b2"], exact=True)
    r = R.epilogue(l2, R.GATE | R.LN, res32=pre["v"], eres=pre["E"], gate16=gt["y"], egate=gt["ey"], ln=d["ln"])
    tln0 = (dev(ln0[0]), dev(ln0[1]), ln0[2])
    for M in MS:
        o32, o16, _ = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=R.RELU, flags=R.GATE | R.LN, M=M,
                                 want32=True, ln=t["ln"], gate=(t["Wb"], t["bb"]),
                                 pre=(t["a32"][:M], t["b16"], t["b_idx"][:M], t["c16"], t["c_idx"][:M], tln0))
        check_epilogue(f"rowchain_gated_pre M={M}", r, M, o32, o16, None)


def same_outputs(ref, got, what):
    for name, r, g in zip(("out32", "out16", "head_out"), ref, got):
        assert (r is None) == (g is None)
        if r is not None:
            assert same(g, r, f"{what} {name}")


@pytest.mark.parametrize("act1", [R.SIGMOID, 0])
def test_rowchain3_run_time_first_activation(act1):
    """dpvo_rowchain3 with a first activation that is not ReLU (K1 = 64): the
    three-GEMM kernel that reads the activation from the flags at run time,
    bit for bit the composition test_gpu_rowgemm uses for ReLU -- rowchain
    (LN | LN_RELU) writing fp16 rows, then rowgemm (RES | LN) with the gather."""
    import update_ops as U
    _, t = EX(64)
    W3, b3 = EX(384)[1]["W1"], EX(384)[1]["b1"]
    kw = dict(flags=R.RES | R.LN, res32=t["res32"], res16=t["res16"], res16_idx=t["res16_idx"], ln=t["ln"], want32=True)
    _, h, _ = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=act1, flags=R.LN | R.LN_RELU, ln=t["ln"])
    ref = U.rowgemm(h, W3, b3, **kw)
    got = U.rowchain(t["A"], t["W1"], t["b1"], W3, b3, flags1=act1, mid=(t["W2"], t["b2"], t["ln"]), **kw)
    same_outputs(ref, got, f"rowchain3 act1={act1}")


@pytest.mark.parametrize("case", ["gate_ln", "gate_heads"])
@pytest.mark.parametrize("act1", [R.SIGMOID, 0])
def test_rowchain_gated_run_time_first_activation(act1, case):
    """dpvo_rowchain_gated with a first activation that is not ReLU (K1 = 64):
    the gated kernels that read it from the flags at run time, bit for bit the
    gate rowgemm (SIGMOID) followed by rowchain(gate16 = its output)."""
    import update_ops as U
    d, t = EX(64)
    flags, _, kk = epi_kwargs(case, d, t)
    kk.pop("gate16")
    chain = functools.partial(U.rowchain, t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=act1, flags=flags,
                              want32=True, **kk)
    _, g16, _ = U.rowgemm(t["A"], t["Wb"], t["bb"], flags=R.SIGMOID)
    same_outputs(chain(gate16=g16), chain(gate=(t["Wb"], t["bb"])), f"rowchain_gated {case} act1={act1}")


@pytest.mark.parametrize("K", [128, 64])
def test_rowgemm_pair_rows_8_byte_aligned(K):
    """dpvo_rowgemm_pair writing out16 rows that are only 8-byte aligned
    (ldo16 = 388): the two-rows-per-pass store path of rowpair6 (K = 128) and
    rowgemm5 DUAL (K = 64), which the shim's 384-wide outputs never take.
    Bit for bit the shim's outputs; padding columns and rows past M untouched."""
    import ctypes

    import _dpvo_hot as H
    import update_ops as U
    _, t = EX(K)
    A = t["A"]
    ops = ((weight(t, "kb", "W1"), t["b1"]), (weight(t, "kb", "Wb"), t["bb"]))
    want = U.rowgemm_pair(A, ops[0][0], ops[0][1], ops[1][0], ops[1][1])
    outs, args = [], []
    for W, b in ops:
        o = full16(ROWS + PAD, R.WIDTH + 4)
        a = U.RowGemmArgs()
        a.A, a.lda, a.a_rows, a.W, a.K, a.N, a.bias = A.data_ptr(), A.stride(0), ROWS, W.data_ptr(), K, R.WIDTH, b.data_ptr()
        a.zero_row, a.M, a.flags, a.out16, a.ldo16 = U.zero_row(A.device, K).data_ptr(), ROWS, U.WKB, o.data_ptr(), o.stride(0)
        outs.append(o)
        args.append(a)
    assert outs[0].stride(0) == 388 and outs[0].data_ptr() % 16 == 0
    H.check(H.lib().dpvo_rowgemm_pair(ctypes.byref(args[0]), ctypes.byref(args[1]), H.stream_of(A)))
    for o, w, name in zip(outs, want, "fg"):
        assert same(o[:ROWS, :R.WIDTH], w, f"pair K={K} ldo16=388 {name}")
        untouched(o[ROWS:], S16, f"pair ldo16=388 {name} rows past M")
        untouched(o[:, R.WIDTH:], S16, f"pair ldo16=388 {name} padding")


# ---------------------------------------------------------------------------
# more 128-row tiles than twice the compute units: once per kernel, K <= 384
@pytest.mark.parametrize("kernel", ["rowgemm3", "rowgemm5", "narrow", "pair3", "pair5", "pair6", "pair_pre",
                                    "rowchain5", "rowadd_ln"])
def test_more_tiles_than_twice_the_compute_units(kernel):
    """every persistent kernel with blocks that walk several tiles: row m of
    the launch is row m mod 257 of the small reference (exact inputs, so the
    comparison stays bit for bit; the chain's RES out32 at its 2 roundings)."""
    import update_ops as U
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = (2 * cus + 1) * 128 + 1
    idx = torch.arange(M, device="cuda") % ROWS
    hidx = idx.cpu().numpy()

    def rows16(got, ref, what):
        assert same(got, dev(ref.astype(np.float16))[idx], what)

    if kernel in ("rowgemm3", "rowgemm5"):
        d, t = EX(64)
        out = full16(M + PAD)
        U.rowgemm(t["A"], weight(t, "kb" if kernel == "rowgemm5" else "row"), t["b1"], flags=R.RELU, a_idx=idx, out16=out)
        rows16(out[:M], LIN(64, R.RELU)["y"], kernel)
        untouched(out[M:], S16, kernel)
    elif kernel == "narrow":       # 32-row tiles: 4 per 128 rows, a device row count just below M
        d, t = EX(384)
        out = full16(M)
        U.rowgemm(t["A"], weight(t, "kb"), t["b1"], flags=R.RELU, a_idx=idx, out16=out,
                  M_dev=torch.tensor([M - 33], device="cuda"))
        assert same(out[:M - 33], dev(LIN(384, R.RELU)["y"].astype(np.float16))[idx[:M - 33]], kernel)
        untouched(out[M - 33:], S16, kernel)
    elif kernel in ("pair3", "pair5", "pair6"):
        K = 128 if kernel == "pair6" else 64
        layout = "row" if kernel == "pair3" else "kb"
        d, t = EX(K)
        f, g = U.rowgemm_pair(t["A"][idx], weight(t, layout, "W1"), t["b1"], weight(t, layout, "Wb"), t["bb"])
        rows16(f, LIN(K, 0, "W1")["y"], kernel + " f")
        rows16(g, LIN(K, 0, "Wb")["y"], kernel + " g")
    elif kernel == "pair_pre":
        d, t = EX(384)
        rows = R.pair_pre_rows(d["a32"], d["b16"], d["b_idx"])
        f, g = U.rowgemm_pair_pre(t["a32"][idx], t["b16"], t["b_idx"][idx], weight(t, "kb", "W1"), t["b1"],
                                  weight(t, "kb", "Wb"), t["bb"])
        rows16(f, R.linear(rows, d["W1"], d["b1"], exact=True)["y"], "pair_pre f")
        rows16(g, R.linear(rows, d["Wb"], d["bb"], exact=True)["y"], "pair_pre g")
    elif kernel == "rowchain5":
        d, t = EX(64)
        l1 = R.linear(d["A"], d["W1"], d["b1"], act=R.RELU, exact=True)
        l2 = R.linear(l1["y"], d["W2"], d["b2"], exact=True)
        r = R.epilogue(l2, R.RES, res32=d["res32"])
        o32, o16, _ = U.rowchain(t["A"], t["W1"], t["b1"], t["W2"], t["b2"], flags1=R.RELU, flags=R.RES, a_idx=idx,
                                 res32=t["res32"][idx], want32=True)
        held("rowchain5 many tiles out32", o32, r["v"][hidx], r["E"][hidx])
        held16("rowchain5 many tiles out16", o16, r["v"][hidx], r["E"][hidx])
    else:
        d, t = EX(384)
        r = R.rowadd_ln(d["a32"], d["b16"], d["b_idx"], d["c16"], d["c_idx"])
        o32, o16 = U.rowadd_ln(t["a32"][idx], t["b16"], t["b_idx"][idx], c16=t["c16"], c_idx=t["c_idx"][idx])
        assert same(o32, dev(r["v"].astype(np.float32))[idx]) and same(o16, dev(r["v"].astype(np.float16))[idx])


# ---------------------------------------------------------------------------
# refusals, by message (arguments only: nothing runs on the device)
def test_refusals_by_message():
    import _dpvo_hot as H
    import update_ops as U
    d, t = EX(384)
    A, W, b = t["A"], t["W1"], t["b1"]

    def args(**over):
        out = torch.empty(ROWS, R.WIDTH, dtype=torch.float16, device="cuda")
        a = U.RowGemmArgs()
        a.A, a.lda, a.a_rows, a.W, a.K, a.N, a.bias = A.data_ptr(), 384, ROWS, W.data_ptr(), 384, 384, b.data_ptr()
        a.zero_row, a.M, a.out16, a.ldo16 = U.zero_row(A.device, 384).data_ptr(), ROWS, out.data_ptr(), 384
        for k, v in over.items():
            setattr(a, k, v)
        return a, out

    import ctypes
    st = H.stream_of(A)
    for over, msg in ((dict(K=96), "multiple of 64"), (dict(K=32), "multiple of 64"), (dict(N=256), "must be 384"),
                      (dict(ldo16=386), r"ldo16 % 4"), (dict(flags=R.RES), "residual input missing"),
                      (dict(flags=R.GATE, res32=A.data_ptr()), "gate input missing"),
                      (dict(flags=R.LN | R.LN_RELU), "LayerNorm weights missing"),
                      (dict(flags=R.GATE | R.HEADS, res32=A.data_ptr(), gate16=A.data_ptr()), "head weights missing"),
                      (dict(flags=R.RELU | R.LN, ln_g=A.data_ptr(), ln_b=A.data_ptr()),
                       "unsupported epilogue flag combination")):
        a, keep = args(**over)
        with pytest.raises(RuntimeError, match=msg):
            H.check(H.lib().dpvo_rowgemm(ctypes.byref(a), st))
    # the pair with unequal K (past the shim's own shape check: straight to the C ABI)
    a, k1 = args()
    b2, k2 = args(K=320)
    with pytest.raises(RuntimeError, match="must share A, K and M"):
        H.check(H.lib().dpvo_rowgemm_pair(ctypes.byref(a), ctypes.byref(b2), st))
    with pytest.raises(RuntimeError, match="of one shape"):
        U.rowgemm_pair(A, W, b, EX(64)[1]["W1"], b)
    # the chain: a first flag that is no activation; a missing residual / gate / LN / heads; K1
    with pytest.raises(RuntimeError, match="takes only an activation"):
        U.rowchain(A, W, b, t["W2"], t["b2"], flags1=R.LN, flags=R.RES, res32=t["res32"])
    with pytest.raises(RuntimeError, match="residual input missing"):
        U.rowchain(A, W, b, t["W2"], t["b2"], flags=R.RES)
    with pytest.raises(RuntimeError, match="gate input missing"):
        U.rowchain(A, W, b, t["W2"], t["b2"], flags=R.GATE | R.LN, res32=t["res32"], ln=t["ln"])
    with pytest.raises(RuntimeError, match="LayerNorm weights missing"):
        U.rowchain(A, W, b, t["W2"], t["b2"], flags=R.LN | R.LN_RELU)
    with pytest.raises(RuntimeError, match="head weights missing"):
        U.rowchain(A, W, b, t["W2"], t["b2"], flags=R.GATE | R.HEADS, res32=t["res32"], gate16=t["gate16"])
    with pytest.raises(RuntimeError, match="multiple of 64"):
        U.rowchain(A[:, :96], U.kblock(W[:, :96].contiguous()), b, t["W2"], t["b2"], flags=R.RES, res32=t["res32"])


# ---------------------------------------------------------------------------
# SoftAgg
DS = (2, 126, 128, 130, 384)
TDT = {np.float16: torch.float16, np.float32: torch.float32, np.float64: torch.float64}


def sa_check(what, got, y, bar, dtype):
    if dtype == np.float16:
        return held16(what, got, y, bar)
    return held(what, got, y, bar)


@pytest.mark.parametrize("kind", ["normal", "ascending", "descending", "wide"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_softagg(dtype, kind):
    """dpvo_softagg_forward (with an empty group), dpvo_softagg_csr and
    dpvo_softagg_csr_long on one label vector with groups of 1, 7, 8, 9, 16,
    17, 63, 64, 65, 67, SA_CAP and SA_CAP + 1 edges, interleaved; f | s as the
    strided halves of one [E, 2D] buffer; csr == dense bit for bit (groups up
    to SA_CAP: the dense path takes larger ones in arrival order)."""
    import update_ops as U
    rng = np.random.default_rng([3, ["normal", "ascending", "descending", "wide"].index(kind)])
    lab, G = R.group_labels(rng)
    lab_e, G_e = np.where(lab >= 3, lab + 1, lab), G + 1           # group 3 left empty (dense path only)
    sizes = np.bincount(lab, minlength=G)
    capped = dev(np.nonzero(sizes <= R.SA_CAP)[0])
    short = dev(np.nonzero(sizes < R.SA_SPLIT)[0])
    tlab = dev(lab)
    gid, offs, perm, groups = U.group_by(tlab, key_bits=8)
    assert int(groups.item()) == G
    for D in DS:
        s = R.softagg_logits(rng, lab, D, kind, np.float32 if dtype == np.float64 else dtype)
        f = (2 * rng.standard_normal((len(lab), D)))
        if dtype == np.float64:
            s = s.astype(np.float64) + 1e-9 * rng.standard_normal(s.shape)     # not fp32 values
        f = f.astype(dtype)
        fs = dev(np.concatenate([f, s], 1))
        tf, ts = fs[:, :D], fs[:, D:]
        what = f"softagg {np.dtype(dtype).name} {kind} D={D}"
        y, bar = R.softagg(f, s, lab, G, f64_in=dtype == np.float64)
        dense = U.softagg(tf, ts, dev(lab_e), G_e)
        keep = [g for g in range(G_e) if g != 3]
        assert bool((dense[3] == 0).all())
        sa_check(what + " dense", dense[keep], y, bar, dtype)
        csr = U.softagg_csr(tf, ts, offs, perm, groups, G + 2)
        sa_check(what + " csr", csr[:G], y, bar, dtype)
        poison_rows(csr[G:], "softagg_csr rows >= groups")
        assert same(csr[capped], dense[keep][capped], what + " csr == dense")     # one online pass: every dtype
        if dtype != np.float64:                                                   # (the long path: fp16 / fp32)
            yl, barl = R.softagg(f, s, lab, G, long_groups=True)
            lng = U.softagg_csr(tf, ts, offs, perm, groups, G + 2, long_groups=True)
            sa_check(what + " csr_long", lng[:G], yl, barl, dtype)
            poison_rows(lng[G:], "softagg_csr_long rows >= groups")
            assert same(lng[short], csr[short], what + " csr_long == csr below the split")


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_softagg_plumbing_equal_logits(dtype):
    """all logits of a group equal and f dyadic: p = 1 exactly, sum f is exact
    in fp32, y is the rounding of the group mean -- one rounding (fp16: the
    fp16 rounding of that fp32 value).  A dropped, duplicated or foreign edge
    moves it by far more."""
    import update_ops as U
    rng = np.random.default_rng(9)
    lab, G = R.group_labels(rng)
    D = 130
    f = (rng.integers(-8, 9, (len(lab), D)) / 4).astype(dtype)
    s = np.broadcast_to(rng.integers(-3, 4, (G, 1))[lab] / 2, (len(lab), D)).astype(dtype)
    mean = np.stack([f[lab == g].astype(np.float64).sum(0) / (lab == g).sum() for g in range(G)])
    tf, ts, tlab = dev(f), dev(s), dev(lab)
    gid, offs, perm, groups = U.group_by(tlab, key_bits=8)
    outs = {"dense": U.softagg(tf, ts, tlab, G), "csr": U.softagg_csr(tf, ts, offs, perm, groups, G)[:G],
            "csr_long": U.softagg_csr(tf, ts, offs, perm, groups, G, long_groups=True)[:G]}
    for name, got in outs.items():
        what = f"softagg plumbing {np.dtype(dtype).name} {name}"
        if dtype == np.float16:
            held16(what, got, mean, R.U * np.abs(mean))
        else:
            held(what, got, mean, R.U * np.abs(mean))
