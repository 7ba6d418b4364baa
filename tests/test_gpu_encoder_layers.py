"""Every frame-ingest encoder kernel (csrc/encoder.hip) on its own, through the
C ABI exactly as encoder_ops calls it, against tests/encoder_layers_ref.py: the
fp64 restatement of that one layer.

a. Crafted inputs make x = xform(a, r) known bit for bit (activations on
   multiples of 2^-5, instance-norm partials that reduce to power-of-two rstd
   and eighths for the mean), so xout is compared bitwise and the only freedom
   left in `out` is the fp32 accumulation:
       |float(h) - v64| <= spacing16(v64) / 2 + (K + 2) 2^-24 conv(|x|, |w|)
   (encoder_layers_ref.out_excess).  The weights reach the kernels through
   encoder_ops._Packed, the reference convolves the module's own tensors.
b. The partials a launch writes against fp64 sums of its own fp16 output per
   8 x 16 tile (valid pixels only), within 128 * 2^-24 of the absolute sums.
c. Real statistics, producer -> consumer, with the producer's |mean| / std
   raised through its bias: what reduce_stats makes of the one-pass fp32 tile
   sums against fp64 statistics of the same fp16 map, within a quarter of an
   fp16 spacing of a normalised value (2^-13).

Every output view sits between poisoned guard rows (and columns where the
pixel stride exceeds the channel count); the guards must keep their bits.
"""
import copy
import ctypes as ct
import dataclasses
import functools
import zlib

import numpy as np
import pytest
import torch

import encoder_layers_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned")]

G = 3   # guard rows before and after every output view

# (ks, stride, cin, cout, xmode) of the six dpvo_encoder_conv instantiations
CONV = {
    "c32m1": (3, 1, 32, 32, 1),
    "c32m2": (3, 1, 32, 32, 2),
    "down": (3, 2, 32, 128, 2),     # conv1 | 1x1 downsample as the centre tap
    "c64m1": (3, 1, 64, 64, 1),
    "c64m2": (3, 1, 64, 64, 2),
    "head": (1, 1, 64, 128, 2),
}
STEM = (7, 2, 3, 32, 0)
SIZES = {"s1": [(1, 1), (8, 16), (9, 17), (5, 40)], "down": [(2, 2), (15, 31), (16, 32), (17, 33)],
         "stem": [(7, 13), (16, 32), (17, 33), (31, 61)]}


def _products(layer):
    """accumulated products per output channel"""
    if layer == "stem":
        return 147
    if layer == "down":
        return [288] * 64 + [32] * 64
    ks, _, cin, _, _ = CONV[layer]
    return ks * ks * cin


@dataclasses.dataclass(frozen=True)
class Case:
    layer: str
    hw: tuple
    tiles: int = 17            # rows of the crafted a_st / r_st
    y5d: bool = False          # input on 128-wide pixel rows at channel 64, statistics rows 256 wide
    norms: tuple = (True,)     # per encoder: instance-norm statistics given / NULL
    oview: bool = False        # o_ps = cout + 64, o_co = 32 (and x_ps = cin + 8)
    scale: float = 1.0
    part: bool = True

    @property
    def id(self):
        return (f"{self.layer}-{self.hw[0]}x{self.hw[1]}" + (f"-tiles{self.tiles}" if self.tiles != 17 else "") +
                ("-y5d" if self.y5d else "") + (f"-enc{len(self.norms)}" if len(self.norms) > 1 else "") +
                ("-oview" if self.oview else "") + (f"-scale{self.scale}" if self.scale != 1.0 else "") +
                ("" if self.part else "-nopart"))


def _cases():
    """one axis at a time around a base case per layer"""
    out = []
    for layer in list(CONV) + ["stem"]:
        sizes = SIZES.get(layer, SIZES["s1"])
        base = sizes[2]
        out += [Case(layer, hw) for hw in sizes]
        if layer != "stem":
            out += [Case(layer, base, tiles=1), Case(layer, base, tiles=130), Case(layer, base, y5d=True)]
        out += [Case(layer, base, norms=(True, False)), Case(layer, base, oview=True),
                Case(layer, base, scale=0.25), Case(layer, base, part=False)]
    return out


@dataclasses.dataclass(frozen=True)
class HeadCase:
    cout: int = 384
    M: int = 300
    norm: bool = True
    tiles: int = 17
    y5d: bool = False
    oview: bool = False
    scale: float = 0.25
    hw: tuple = (9, 17)

    @property
    def id(self):
        return (f"head_at-{self.cout}-M{self.M}" + ("" if self.norm else "-nostats") + f"-tiles{self.tiles}" +
                ("-y5d" if self.y5d else "") + ("-oview" if self.oview else "") + f"-scale{self.scale}")


HEAD_CASES = [HeadCase(), HeadCase(cout=128), HeadCase(M=0), HeadCase(M=1), HeadCase(norm=False),
              HeadCase(tiles=1), HeadCase(tiles=130), HeadCase(y5d=True), HeadCase(oview=True), HeadCase(scale=1.0)]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def crafted_stat_cases():
    """(channels, pixels, rows, seed) of every crafted statistics buffer below
    (tests/test_encoder_layers_host.py checks each on the CPU)"""
    for c in _cases():
        if c.layer == "stem":
            continue
        _, _, cin, _, xmode = CONV[c.layer]
        for i, norm in enumerate(c.norms):
            for which in ("a", "r")[:xmode]:
                if norm:
                    yield cin, c.hw[0] * c.hw[1], c.tiles, _seed(c.id, i, which)
    for c in HEAD_CASES:
        for which in ("a", "r"):
            if c.norm:
                yield 64, c.hw[0] * c.hw[1], c.tiles, _seed(c.id, 0, which)


# ------------------------------------------------------------------ plumbing

@functools.lru_cache(maxsize=None)
def _encoder(i, out_dim=128):
    """(the CPU module, its weights as encoder_ops packs them, on the GPU)"""
    import encoder_ops
    from dpvo.extractor import BasicEncoder4
    torch.manual_seed(100 + i)
    enc = BasicEncoder4(out_dim, "instance" if i == 0 else "none").eval()
    return enc, encoder_ops._Packed(copy.deepcopy(enc).cuda())


def _layer(enc, pk, layer):
    """(the layer's nn.Conv2d modules, its packed (weights, bias))"""
    l1, l2 = enc.layer1, enc.layer2
    return {"stem": ([enc.conv1], pk.stem),
            "c32m1": ([l1[0].conv1], pk.l1[0]),
            "c32m2": ([l1[1].conv1], pk.l1[2]),
            "down": ([l2[0].conv1, l2[0].downsample[0]], pk.l2_down),
            "c64m1": ([l2[0].conv2], pk.l2[0]),
            "c64m2": ([l2[1].conv1], pk.l2[1]),
            "head": ([enc.conv2], pk.head)}[layer]


def conv_args(a=None, a_ps=0, a_co=0, a_st=None, a_st_tiles=0, a_st_ld=0, r=None, r_ps=0, r_co=0, r_st=None,
              r_st_tiles=0, r_st_ld=0, xout=None, x_ps=0, w=None, bias=None, out=None, o_ps=0, o_co=0, scale=1.0,
              part=None, eps=R.EPS):
    from encoder_ops import ConvArgs
    p = lambda t: t.data_ptr() if t is not None else None
    return ConvArgs(p(a), a_ps, a_co, p(a_st), a_st_tiles, a_st_ld, p(r), r_ps, r_co, p(r_st), r_st_tiles, r_st_ld,
                    p(xout), x_ps, p(w), p(bias), p(out), o_ps, o_co, scale, p(part), eps)


def _guarded(rows, cols, dtype):
    """[G + rows + G][cols] through _dpvo_hot.empty: NaN everywhere under the poisoned fixture"""
    import _dpvo_hot as H
    assert H.poison() == 0xFF
    return H.empty(rows + 2 * G, cols, dtype=dtype, device="cuda")


def _guards_intact(buf, rows, c0, c1):
    """every element outside rows [G, G + rows) x columns [c0, c1) still holds the poison bits"""
    raw = buf.view(torch.int16 if buf.dtype == torch.float16 else torch.int32)
    view = torch.zeros_like(raw, dtype=torch.bool)
    view[G:G + rows, c0:c1] = True
    return bool((raw[~view] == -1).all())


def _grid(rows, cols, gen):
    """fp64 multiples of 2^-5 in [-2, 2]"""
    return torch.randint(-64, 65, (rows, cols), generator=gen).double() / 32.0


def _crafted(C, n, tiles, y5d, seed):
    """(mean, rstd) per channel and the partial rows [tiles][ld] that reduce to
    them; the statistics of the channels beside them are junk"""
    gen = torch.Generator().manual_seed(seed)
    mean, rstd, part = R.crafted_stats(C, n, tiles, gen)
    ld, co = (256, 64) if y5d else (2 * C, 0)
    buf = (torch.rand(tiles, ld, generator=gen) * 100.0).float()
    buf[:, 2 * co:2 * (co + C)] = torch.from_numpy(part)
    return (mean, rstd), buf.cuda(), ld


def _operand(n, C, y5d, gen):
    """activations on the grid: (the [n][ps] buffer, ps, co); channels [co, co + C) are the operand"""
    ps, co = (128, 64) if y5d else (C, 0)
    return _grid(n, ps, gen), ps, co


def _chw(buf, co, C, Hi, Wi):
    return buf[:, co:co + C].T.reshape(C, Hi, Wi)


def _stream():
    import _dpvo_hot as H
    return H._vp(torch.cuda.current_stream().cuda_stream)


def _check_part(pbuf, T, h, cout):
    """b. row `tile` of part against fp64 sums of the kernel's own output over the tile's valid pixels"""
    assert _guards_intact(pbuf, T, 0, 2 * cout)
    got = pbuf[G:G + T].double().cpu()
    S, Q, A = R.tile_sums(h)
    assert S.shape == (T, cout)
    assert ((got[:, 0::2] - S).abs() <= 128 * R.U * A).all()
    assert ((got[:, 1::2] - Q).abs() <= 128 * R.U * Q).all()


def _run_conv(case, norms):
    """one launch of `case` with the given per-encoder statistics switches; checks a. and b."""
    import _dpvo_hot as H
    import encoder_ops
    lib = H.lib()
    stem = case.layer == "stem"
    ks, s, cin, cout, xmode = STEM if stem else CONV[case.layer]
    Hi, Wi = case.hw
    n_in = Hi * Wi
    Ho, Wo = encoder_ops.conv_out(Hi, ks, s), encoder_ops.conv_out(Wi, ks, s)
    n_out = Ho * Wo
    T = lib.dpvo_encoder_tiles(Hi, Wi, ks, s)
    assert T == -(-Ho // 8) * -(-Wo // 16)
    o_ps, o_co = (cout + 64, 32) if case.oview else (cout, 0)
    x_ps = cin + 8 if case.oview else cin
    want_x = ks == 3 and s == 1
    image = None
    if stem:
        img = torch.randint(0, 256, (3, Hi, Wi), generator=torch.Generator().manual_seed(_seed(case.id)),
                            dtype=torch.uint8)
        image = img.cuda()
    encs, keep = [], []
    for i, norm in enumerate(norms):
        enc, pk = _encoder(i)
        convs, (w, b) = _layer(enc, pk, case.layer)
        kw = dict(w=w, bias=b)
        if stem:
            x = R.stem_input(img)
        else:
            gen = torch.Generator().manual_seed(_seed(case.id, i))
            abuf, a_ps, a_co = _operand(n_in, cin, case.y5d, gen)
            a_st = r_st = rr = None
            kw.update(a=abuf.half().cuda(), a_ps=a_ps, a_co=a_co)
            if norm:
                a_st, kw["a_st"], kw["a_st_ld"] = _crafted(cin, n_in, case.tiles, case.y5d, _seed(case.id, i, "a"))
                kw["a_st_tiles"] = case.tiles
            if xmode == 2:
                rbuf, r_ps, r_co = _operand(n_in, cin, case.y5d, gen)
                rr = _chw(rbuf, r_co, cin, Hi, Wi)
                kw.update(r=rbuf.half().cuda(), r_ps=r_ps, r_co=r_co)
                if norm:
                    r_st, kw["r_st"], kw["r_st_ld"] = _crafted(cin, n_in, case.tiles, case.y5d,
                                                                _seed(case.id, i, "r"))
                    kw["r_st_tiles"] = case.tiles
            x = R.xform(_chw(abuf, a_co, cin, Hi, Wi), xmode, a_st, rr, r_st)
        v, absv = R.conv_layer(x, convs)
        assert v.shape == (cout, Ho, Wo)
        obuf = _guarded(n_out, o_ps, torch.float16)
        xbuf = _guarded(n_in, x_ps, torch.float16) if want_x else None
        pbuf = _guarded(T, 2 * cout, torch.float32) if case.part else None
        kw.update(out=obuf[G:], o_ps=o_ps, o_co=o_co, scale=case.scale)
        if want_x:
            kw.update(xout=xbuf[G:], x_ps=x_ps)
        if case.part:
            kw.update(part=pbuf[G:])
        keep.append(kw)
        encs.append((conv_args(**kw), x, v, absv, obuf, xbuf, pbuf))
    arr = (encoder_ops.ConvArgs * len(encs))(*[e[0] for e in encs])
    if stem:
        H.check(lib.dpvo_encoder_stem(image.data_ptr(), Hi, Wi, arr, len(encs), _stream()))
    else:
        H.check(lib.dpvo_encoder_conv(ks, s, cin, cout, xmode, Hi, Wi, arr, len(encs), _stream()))
    torch.cuda.synchronize()
    worst = 0.0
    for i, (_, x, v, absv, obuf, xbuf, pbuf) in enumerate(encs):
        assert _guards_intact(obuf, n_out, o_co, o_co + cout), f"encoder {i}: out guard"
        h = obuf[G:G + n_out, o_co:o_co + cout].double().cpu().T.reshape(cout, Ho, Wo)
        ex = R.out_excess(h, v, absv, _products(case.layer), case.scale)
        print(f"delta-usage {case.id} enc{i} norm={int(norms[i])} {ex.max().item():.4f}")
        assert (ex <= 1.0).all(), f"encoder {i}: out off by {ex.max().item():.3f} of the bound"
        worst = max(worst, ex.max().item())
        if want_x:
            assert _guards_intact(xbuf, n_in, 0, cin), f"encoder {i}: xout guard"
            got = xbuf[G:G + n_in, :cin].cpu()
            want = x.reshape(cin, n_in).T.to(torch.float16)
            assert torch.equal(want.double(), x.reshape(cin, n_in).T)            # x is exact in fp16
            assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), f"encoder {i}: xout"
        if case.part:
            _check_part(pbuf, T, h, cout)
    return worst


# ------------------------------------------------- a / b: each kernel, x bit-exact

@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.id)
def test_layer_against_fp64(case):
    """the launch with crafted statistics, then the same operands with a_st =
    r_st = NULL (the inet path: x = relu(a), x = relu(relu(a) + r))"""
    _run_conv(case, case.norms)
    if case.layer != "stem":
        _run_conv(case, (False,) * len(case.norms))


def _head_points(Hi, Wi, M, gen):
    """inside the map, on each border, outside it on each side"""
    edge = [(0, 0), (Wi - 1, 0), (0, Hi - 1), (Wi - 1, Hi - 1), (Wi // 2, 0), (0, Hi // 2), (Wi - 1, Hi // 2),
            (Wi // 2, Hi - 1), (-1, 3), (Wi, 3), (3, -1), (3, Hi), (-1, -1), (Wi, Hi), (-(2 ** 40), 2), (2, 2 ** 40)]
    if M == 1:
        return torch.tensor([Wi // 2]), torch.tensor([Hi // 2])
    xs = torch.cat([torch.tensor([p[0] for p in edge]), torch.randint(0, Wi, (M - len(edge),), generator=gen)])
    ys = torch.cat([torch.tensor([p[1] for p in edge]), torch.randint(0, Hi, (M - len(edge),), generator=gen)])
    return xs[:M], ys[:M]


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: c.id)
def test_head_at_against_fp64(case):
    import _dpvo_hot as H
    lib = H.lib()
    Hi, Wi = case.hw
    n_in, cout, M = Hi * Wi, case.cout, case.M
    enc, pk = _encoder(1, cout)
    w, b = pk.head_rows
    gen = torch.Generator().manual_seed(_seed(case.id, 0))
    abuf, a_ps, a_co = _operand(n_in, 64, case.y5d, gen)
    rbuf, r_ps, r_co = _operand(n_in, 64, case.y5d, gen)
    kw = dict(a=abuf.half().cuda(), a_ps=a_ps, a_co=a_co, r=rbuf.half().cuda(), r_ps=r_ps, r_co=r_co, w=w, bias=b)
    a_st = r_st = None
    if case.norm:
        a_st, kw["a_st"], kw["a_st_ld"] = _crafted(64, n_in, case.tiles, case.y5d, _seed(case.id, 0, "a"))
        r_st, kw["r_st"], kw["r_st_ld"] = _crafted(64, n_in, case.tiles, case.y5d, _seed(case.id, 0, "r"))
        kw["a_st_tiles"] = kw["r_st_tiles"] = case.tiles
    x = R.xform(_chw(abuf, a_co, 64, Hi, Wi), 2, a_st, _chw(rbuf, r_co, 64, Hi, Wi), r_st)
    xs, ys = _head_points(Hi, Wi, max(M, 1), gen)
    v, absv = R.head_at(x, enc.conv2, xs, ys)
    o_ps, o_co = (cout + 64, 32) if case.oview else (cout, 0)
    obuf = _guarded(M, o_ps, torch.float16)
    kw.update(out=obuf[G:] if M else obuf, o_ps=o_ps, o_co=o_co, scale=case.scale)
    xd, yd = xs.cuda(), ys.cuda()
    e = conv_args(**kw)
    H.check(lib.dpvo_encoder_head_at(ct.byref(e), cout, Hi, Wi, xd.data_ptr(), yd.data_ptr(), M, _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(obuf, M, o_co, o_co + cout)
    if M == 0:
        return
    h = obuf[G:G + M, o_co:o_co + cout].double().cpu()
    ex = R.out_excess(h, v, absv, 64, case.scale)
    print(f"delta-usage {case.id} {ex.max().item():.4f}")
    assert (ex <= 1.0).all(), f"head_at off by {ex.max().item():.3f} of the bound"
    outside = (xs < 0) | (xs >= Wi) | (ys < 0) | (ys >= Hi)
    assert outside.sum() == (8 if M > 1 else 0)
    bias = (b.cpu().float() * case.scale).to(torch.float16)
    assert torch.equal(obuf[G:G + M, o_co:o_co + cout].cpu()[outside], bias[None].expand(int(outside.sum()), -1))


def test_entry_points_refuse_what_they_do_not_support():
    """error return only: nothing is launched"""
    import _dpvo_hot as H
    import encoder_ops
    lib = H.lib()
    enc, pk = _encoder(0)
    a = torch.zeros(16 * 32, 128, dtype=torch.float16, device="cuda")
    out = _guarded(16 * 32, 128, torch.float16)
    xo = _guarded(16 * 32, 64, torch.float16)
    img = torch.zeros(3, 16, 32, dtype=torch.uint8, device="cuda")
    w, b = pk.l1[0]
    ok = dict(a=a, a_ps=32, r=a, r_ps=32, w=w, bias=b, out=out[G:], o_ps=32)
    one = lambda **kw: (encoder_ops.ConvArgs * 3)(*[conv_args(**{**ok, **kw})] * 3)
    s = _stream()
    assert lib.dpvo_encoder_conv(3, 1, 32, 64, 1, 16, 32, one(), 1, s) == -1          # no such layer shape
    assert "unsupported layer shape" in lib.dpvo_hot_last_error().decode()
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 0, 16, 32, one(), 1, s) == -1          # xmode 0 has no instantiation
    assert lib.dpvo_encoder_conv(5, 1, 32, 32, 1, 16, 32, one(), 1, s) == -1
    w2, b2 = pk.l2_down
    assert lib.dpvo_encoder_conv(3, 2, 32, 128, 2, 16, 32, one(w=w2, bias=b2, o_ps=128, xout=xo[G:], x_ps=32), 1,
                                 s) == -1                                             # xout on a stride-2 layer
    wh, bh = pk.head
    assert lib.dpvo_encoder_conv(1, 1, 64, 128, 2, 16, 32, one(w=wh, bias=bh, a_ps=64, r_ps=64, o_ps=128,
                                                               xout=xo[G:], x_ps=64), 1, s) == -1   # ... or a 1x1
    for n_enc in (0, 3):
        assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 16, 32, one(), n_enc, s) == -1
        assert lib.dpvo_encoder_stem(img.data_ptr(), 16, 32, one(), n_enc, s) == -1
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 0, 32, one(), 1, s) == -1           # empty input
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 16, 32, one(a_ps=36), 1, s) == -1   # 16-byte loads
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 16, 32, one(o_co=2), 1, s) == -1    # 8-byte stores
    st = torch.zeros(4, 64, device="cuda")
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 16, 32, one(a_st=st, a_st_tiles=0, a_st_ld=64), 1, s) == -1
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 1, 16, 32, one(a_st=st, a_st_tiles=4, a_st_ld=66), 1, s) == -1
    assert lib.dpvo_encoder_conv(3, 1, 32, 32, 2, 16, 32, one(r=None), 1, s) == -1    # xmode 2 without a residual
    assert lib.dpvo_encoder_stem(None, 16, 32, one(), 1, s) == -1
    e = conv_args(**{**ok, "r": None})
    xs = torch.zeros(1, dtype=torch.long, device="cuda")
    assert lib.dpvo_encoder_head_at(ct.byref(e), 128, 16, 32, xs.data_ptr(), xs.data_ptr(), 1, s) == -1
    e = conv_args(**ok)
    assert lib.dpvo_encoder_head_at(ct.byref(e), 128, 16, 32, xs.data_ptr(), xs.data_ptr(), -1, s) == -1
    torch.cuda.synchronize()
    assert _guards_intact(out, 0, 0, 0) and _guards_intact(xo, 0, 0, 0)


# ------------------------------------------------- c: real statistics, producer -> consumer

# |mean| / std of the producing layer's output.  Asserted up to STATS_R_ASSERTED
# = twice the largest R any fnet layer shows on textured, noise and flat frames
# (25.94, scripts/encoder_layer_R.py; include/dpvo_hot.h states the range next
# to a_st); beyond it the figures are printed only.  Measured on an MI355X
# (profiles/encoder_layers/NOTES.md), worst |rstd / rstd64 - 1| over the two
# chains and frames: 2.4e-6 at R = 10, 1.5e-5 at 25, 7.2e-5 at 52, 5.2e-4 at 150.
STATS_R = [0.2, 4.0, 10.0, 25.0, 52.0, 150.0]
STATS_R_ASSERTED = 52.0
QUARTER = 2.0 ** -13   # a quarter of the fp16 spacing of a normalised value in [1, 2)


@pytest.mark.parametrize("Rt", STATS_R)
@pytest.mark.parametrize("frame", [(33, 65), (96, 128)], ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("chain", ["stem-c32", "c64-c64"])
def test_real_statistics_producer_to_consumer(chain, frame, Rt):
    """stem -> layer1's first convolution, and a 64-channel 3x3 launch -> the
    next one: the consumer normalises with what reduce_stats makes of the
    producer's partials.  The producer's bias is shifted per channel so that its
    output has |mean| / std = Rt."""
    import _dpvo_hot as H
    import encoder_ops
    lib = H.lib()
    enc = copy.deepcopy(_encoder(0)[0])
    H1, W1 = encoder_ops.conv_out(frame[0], 7, 2), encoder_ops.conv_out(frame[1], 7, 2)
    gen = torch.Generator().manual_seed(_seed(chain, frame))
    if chain == "stem-c32":
        C, Hi, Wi = 32, H1, W1
        img = torch.randint(0, 256, (3,) + frame, generator=gen, dtype=torch.uint8)
        px, pconv, cconv = R.stem_input(img), enc.conv1, enc.layer1[0].conv1
    else:
        C, Hi, Wi = 64, encoder_ops.conv_out(H1, 3, 2), encoder_ops.conv_out(W1, 3, 2)
        abuf = _grid(Hi * Wi, 64, gen)
        px, pconv, cconv = R.xform(_chw(abuf, 0, 64, Hi, Wi), 1), enc.layer2[1].conv2, enc.layer2[0].conv2
    n = Hi * Wi
    with torch.no_grad():
        m0, r0 = R.stats64(R.conv_layer(px, [pconv])[0], 0.0)
        sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
        pconv.bias += (sign * Rt / r0 - m0).float()
    pk = encoder_ops._Packed(copy.deepcopy(enc).cuda())
    T = lib.dpvo_encoder_tiles(Hi, Wi, 3, 1)
    ybuf, pbuf = _guarded(n, C, torch.float16), _guarded(T, 2 * C, torch.float32)
    xbuf, obuf = _guarded(n, C, torch.float16), _guarded(n, C, torch.float16)
    if chain == "stem-c32":
        assert T == lib.dpvo_encoder_tiles(frame[0], frame[1], 7, 2)
        image = img.cuda()
        p = conv_args(w=pk.stem[0], bias=pk.stem[1], out=ybuf[G:], o_ps=C, part=pbuf[G:])
        H.check(lib.dpvo_encoder_stem(image.data_ptr(), frame[0], frame[1], ct.byref(p), 1, _stream()))
        cw = pk.l1[0]
    else:
        ad = abuf.half().cuda()
        p = conv_args(a=ad, a_ps=64, w=pk.l2[2][0], bias=pk.l2[2][1], out=ybuf[G:], o_ps=C, part=pbuf[G:])
        H.check(lib.dpvo_encoder_conv(3, 1, 64, 64, 1, Hi, Wi, ct.byref(p), 1, _stream()))
        cw = pk.l2[0]
    c = conv_args(a=ybuf[G:], a_ps=C, a_st=pbuf[G:], a_st_tiles=T, a_st_ld=2 * C, xout=xbuf[G:], x_ps=C,
                  w=cw[0], bias=cw[1], out=obuf[G:], o_ps=C)
    H.check(lib.dpvo_encoder_conv(3, 1, C, C, 1, Hi, Wi, ct.byref(c), 1, _stream()))
    torch.cuda.synchronize()
    for buf, cols in ((ybuf, C), (xbuf, C), (obuf, C)):
        assert _guards_intact(buf, n, 0, cols)
    assert _guards_intact(pbuf, T, 0, 2 * C)
    y = _chw(ybuf[G:G + n].double().cpu(), 0, C, Hi, Wi)
    _check_part(pbuf, T, y, C)
    # the statistics: reduce_stats' arithmetic on the kernel's partials against fp64 ones of the same map
    mean64, rstd64 = R.stats64(y)
    mean, rstd, shift = R.reduce_stats_np(pbuf[G:G + T].cpu().numpy(), 0, C, n)
    e_rstd = np.abs(rstd.astype(np.float64) / rstd64.numpy() - 1).max()
    e_mean = (np.abs(mean - mean64.numpy()) * rstd64.numpy()).max()
    R_seen = R.channel_R(y)
    # x as the consumer built it
    xk = _chw(xbuf[G:G + n].double().cpu(), 0, C, Hi, Wi)
    n64 = (y - mean64[:, None, None]) * rstd64[:, None, None]
    x64 = R.relu(n64)
    bound = (R.spacing16(x64) / 2 + 4 * R.U * (y.abs() + mean64.abs()[:, None, None]) * rstd64[:, None, None] +
             QUARTER * x64.abs())
    e_x = ((xk - x64).abs() / bound).max().item()
    print(f"real-stats {chain} {frame[0]}x{frame[1]} R target {Rt} seen {R_seen.min().item():.3g}.."
          f"{R_seen.max().item():.3g}: |rstd/rstd64-1| {e_rstd:.3g} |dmean| rstd64 {e_mean:.3g} "
          f"(bar {QUARTER:.3g}); x excess {e_x:.3f}")
    # the consumer's own convolution of the x it wrote
    v, absv = R.conv_layer(xk, [cconv])
    h = _chw(obuf[G:G + n].double().cpu(), 0, C, Hi, Wi)
    ex = R.out_excess(h, v, absv, 9 * C)
    assert (ex <= 1.0).all()
    if Rt <= STATS_R_ASSERTED:
        assert e_rstd <= QUARTER and e_mean <= QUARTER
        assert e_x <= 1.0
