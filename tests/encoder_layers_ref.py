"""fp64 restatement of ONE layer of the native frame-ingest encoders
(csrc/encoder.hip), for tests/test_encoder_layers_host.py and
tests/test_gpu_encoder_layers.py.  Plain torch / numpy on the CPU.

A layer is  out = fp16(fp16(conv(x, fp16 w) + fp16 b) * out_scale)  with
x = xform(a, r) built on load (include/dpvo_hot.h, "Frame ingest"):
  xmode 1: x = relu(fp16(IN(a)));  2: x = relu(fp16(relu(fp16(IN(a))) + fp16(IN'(r))))
IN(a) = (a - mean) * rstd per channel (skipped without statistics), x = 0
outside the image.  The functions here return the convolution value BEFORE
its rounding (v64) and absv = conv(|x|, |w|) + |b|, the scale of the fp32
accumulation error; out_excess() is the derived output criterion.

Weights are taken from the torch module (cast to fp16 as autocast does) and
convolved by torch.nn.functional.conv2d; nothing here packs or swizzles --
the kernels get encoder_ops._Packed's tensors, so the packing is under test.
Test infrastructure only.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
U = 2.0 ** -24        # half an fp32 spacing, relative


def r16(t, on=True):
    """round to fp16 (values kept in fp64); identity with the roundings off"""
    return t.to(torch.float16).double() if on else t


def relu(t):
    return torch.where(t > 0, t, torch.zeros_like(t))   # +0 for -0, as the kernels' n > 0 ? n : 0


def spacing16(v):
    """fp16 spacing at |v| (2^-24 in the subnormal range)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -14))   # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 11)


def stats64(a, eps=EPS):
    """instance-norm (mean, rstd) per channel of a [C, H, W], biased variance"""
    mean = a.mean(dim=(1, 2))
    var = (a - mean[:, None, None]).pow(2).mean(dim=(1, 2))
    return mean, 1.0 / torch.sqrt(var + eps)


def _norm(t, st, round16, eps):
    if st is None:
        return t
    mean, rstd = stats64(t, eps) if isinstance(st, str) else st
    return r16((t - mean[:, None, None]) * rstd[:, None, None], round16)


def xform(a, xmode, a_stats=None, r=None, r_stats=None, round16=True, eps=EPS):
    """x of one layer.  a, r: [C, Hi, Wi] fp64.  *_stats: None (no norm),
    "fp64" (computed over all Hi x Wi pixels) or (mean [C], rstd [C])."""
    if xmode == 0:
        return a
    n = relu(_norm(a, a_stats, round16, eps))
    if xmode == 2:
        n = relu(r16(n + _norm(r, r_stats, round16, eps), round16))
    return n


def conv_layer(x, convs, round16=True):
    """(v64, absv) of the layer whose output channels are the concatenation of
    `convs` (nn.Conv2d modules with their own kernel size, stride, padding):
    one module for a plain layer, (conv1, downsample[0]) for the stride-2 block."""
    vs, av = [], []
    for c in convs:
        w = r16(c.weight.detach().double(), round16)
        b = r16(c.bias.detach().double(), round16)
        vs.append(F.conv2d(x[None], w, b, stride=c.stride, padding=c.padding)[0])
        av.append(F.conv2d(x.abs()[None], w.abs(), b.abs(), stride=c.stride, padding=c.padding)[0])
    return torch.cat(vs), torch.cat(av)


def stem_input(u8, round16=True):
    """the frame as conv1 sees it: fp16(2 (u8 / 255) - 0.5), evaluated in fp32
    as the stem kernel does; uint8 [3, H, W] -> fp64 [3, H, W]"""
    if not round16:
        return 2 * (u8.double() / 255.0) - 0.5
    f = np.float32(2) * (u8.numpy().astype(np.float32) / np.float32(255)) - np.float32(0.5)
    return torch.from_numpy(f.astype(np.float16).astype(np.float64))


def head_at(x, conv, xs, ys, round16=True):
    """the 1x1 head at points only: (v64, absv) [M, cout]; a point outside
    the map sees x = 0, i.e. the bias"""
    C, Hi, Wi = x.shape
    w = r16(conv.weight.detach().double(), round16)[:, :, 0, 0]
    b = r16(conv.bias.detach().double(), round16)
    inside = (xs >= 0) & (xs < Wi) & (ys >= 0) & (ys < Hi)
    px = x[:, ys.clamp(0, Hi - 1), xs.clamp(0, Wi - 1)].T * inside[:, None].double()   # [M, C]
    return px @ w.T + b, px.abs() @ w.abs().T + b.abs()


def out_excess(h, v64, absv, K, scale=1.0):
    """|float(h) / scale - v64| as a fraction of the allowed spacing16(v64) / 2 +
    (K + 2) 2^-24 absv (the final fp16 rounding plus K fp32 accumulations, the
    bias add and slack for the MFMA's internal order); <= 1 passes.  K: the
    number of accumulated products, scalar or per output channel [cout] (h
    channel-first).  scale 0.25 is exact except in the subnormal range: one
    subnormal spacing more where |h| < 2^-12."""
    K = torch.as_tensor(K, dtype=torch.float64)
    if K.dim() == 1:
        K = K.reshape(-1, *([1] * (h.dim() - 1)))
    bound = spacing16(v64) / 2 + (K + 2) * U * absv
    if scale != 1.0:
        bound = bound + (h.abs() < 2.0 ** -12).double() * (2.0 ** -24 / scale)
    return (h / scale - v64).abs() / bound


def reduce_stats_np(part, co, C, n, eps=EPS):
    """numpy restatement of encoder.hip reduce_stats: part [tiles][ld] float32
    with (sum, sumsq) of channel c at 2 (co + c); fp64 sums, var = Q / n -
    mean^2 clamped at 0, rstd = 1 / sqrtf((float) var + eps), shift = (float)(-mean) rstd.
    -> mean fp64 [C], rstd fp32 [C], shift fp32 [C]"""
    p = np.asarray(part, np.float32)[:, 2 * co:2 * (co + C)].astype(np.float64)
    S, Q = p[:, 0::2].sum(0), p[:, 1::2].sum(0)
    mean = S / n
    var = np.maximum(Q / n - mean * mean, 0.0)
    rstd = np.float32(1) / np.sqrt(var.astype(np.float32) + np.float32(eps))
    shift = (-mean).astype(np.float32) * rstd
    return mean, rstd.astype(np.float32), shift.astype(np.float32)


def crafted_channels(C, gen):
    """per-channel target statistics on a grid that keeps a * rstd - mean * rstd
    exact in fp16 for a on multiples of 2^-5, |a| <= 2: rstd in {0.5, 1, 2, 4},
    mean a multiple of 1/8 with |mean| <= min(1, 2 / rstd) (|mean rstd| <= 2
    keeps the fp32 rounding of the crafted sum of squares within two spacings of
    rstd, see crafted_partials)."""
    rstd = torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=gen)]
    lim = torch.clamp(16.0 / rstd, max=8.0).long()                       # in eighths
    mean = (torch.randint(0, 1 << 30, (C,), generator=gen) % (2 * lim + 1) - lim).double() / 8.0
    return mean, rstd


def tile_counts(n, tiles, gen):
    """`tiles` uneven non-negative integers that sum to n"""
    cuts = torch.sort(torch.randint(0, n + 1, (tiles - 1,), generator=gen)).values
    edges = torch.cat([torch.zeros(1, dtype=torch.long), cuts, torch.tensor([n])])
    return edges[1:] - edges[:-1]


def crafted_partials(mean, rstd, nt, eps=EPS):
    """float32 [tiles][2 C] partial rows of nt[t] pixels each whose reduction
    gives (mean, rstd): S_t = mean n_t, Q_t = (1 / rstd^2 - eps + mean^2) n_t.
    Q_t is not representable in fp32 (eps); each row is rounded so that the
    running fp64 sum of the stored values follows the exact one, which leaves
    one rounding of one row in the total."""
    nt = nt.double().numpy()
    m, q = mean.numpy(), (1.0 / rstd.numpy() ** 2 - eps + mean.numpy() ** 2)
    out = np.zeros((len(nt), 2 * len(m)), np.float32)
    out[:, 0::2] = nt[:, None] * m[None]
    want = np.cumsum(nt[:, None] * q[None], axis=0)
    have = np.zeros(len(m))
    for t in range(len(nt)):
        out[t, 1::2] = (want[t] - have).astype(np.float32)
        have += out[t, 1::2].astype(np.float64)
    return out


def reduces_exactly(part, mean, rstd, n, eps=EPS):
    """per channel: reduce_stats' arithmetic on `part` returns exactly mean,
    fp32(rstd) and fp32(-mean rstd)"""
    m, r, sh = reduce_stats_np(part, 0, len(mean), n, eps)
    mn, rn = mean.numpy(), rstd.numpy()
    return (m == mn) & (r == rn.astype(np.float32)) & (sh == (-mn * rn).astype(np.float32))


def crafted_stats(C, n, tiles, gen, eps=EPS):
    """(mean [C], rstd [C], part float32 [tiles][2 C]): statistics on
    crafted_channels' grid and partial rows over `tiles` uneven pixel counts
    summing to n that reduce_stats reduces to them EXACTLY, so that x = a rstd -
    mean rstd has no rounding at all.  The one rounding crafted_partials leaves
    can put (float) var + eps one spacing off 1 / rstd^2 (always possible with a
    single row): the last row's sum of squares is then moved by up to 3
    spacings, and a channel that still misses draws other statistics."""
    nt = tile_counts(n, tiles, gen)
    last = int(torch.nonzero(nt)[-1])
    mean, rstd = crafted_channels(C, gen)
    for _ in range(64):
        part = crafted_partials(mean, rstd, nt, eps)
        good = reduces_exactly(part, mean, rstd, n, eps)
        for k in (1, -1, 2, -2, 3, -3):
            if good.all():
                break
            trial = part.copy()
            q = trial[last, 1::2].copy()
            trial[last, 1::2] = (q.view(np.int32) + k).view(np.float32)     # k spacings (q > 0)
            ok = reduces_exactly(trial, mean, rstd, n, eps) & ~good
            part[last, 1::2] = np.where(ok, trial[last, 1::2], part[last, 1::2])
            good |= ok
        if good.all():
            return mean, rstd, part
        m2, r2 = crafted_channels(C, gen)
        bad = torch.from_numpy(~good)
        mean, rstd = torch.where(bad, m2, mean), torch.where(bad, r2, rstd)
    raise AssertionError("no exactly reducing statistics found")


def tile_sums(h, th=8, tw=16):
    """per-tile fp64 (S, Q, sum |h|) of h [C, Ho, Wo] over each 8 x 16 tile's
    valid pixels, tiles row-major -> three [tiles, C] tensors"""
    C, Ho, Wo = h.shape
    ty, tx = -(-Ho // th), -(-Wo // tw)
    p = torch.zeros(C, ty * th, tx * tw, dtype=torch.float64)
    p[:, :Ho, :Wo] = h
    p = p.reshape(C, ty, th, tx, tw).permute(1, 3, 0, 2, 4).reshape(ty * tx, C, th * tw)
    return p.sum(-1), p.pow(2).sum(-1), p.abs().sum(-1)


# ---- the whole network as a chain of the layers above (NativeEncoders.run's order) ----

def encoder_chain(enc, u8, round16=True, on_layer=None):
    """BasicEncoder4 `enc` on the uint8 frame [3, H, W] as NativeEncoders.run
    chains the layers; -> the head's v64 [cout, h, w].  on_layer(name, y): called
    with every convolution's output (pre-norm)."""
    st = "fp64" if enc.norm_fn == "instance" else None
    l1, l2 = enc.layer1, enc.layer2
    eps = EPS
    for m in enc.modules():
        if isinstance(m, torch.nn.InstanceNorm2d):
            eps = m.eps
    rec = on_layer or (lambda name, y: None)

    def conv(name, x, *convs):
        y = r16(conv_layer(x, convs, round16)[0], round16)
        rec(name, y)
        return y

    xf = lambda a, xmode, r=None, r_st=None: xform(a, xmode, st, r, r_st, round16, eps)
    y0 = conv("conv1", stem_input(u8, round16), enc.conv1)
    x0 = xf(y0, 1)
    y1 = conv("layer1.0.conv1", x0, l1[0].conv1)
    y2 = conv("layer1.0.conv2", xf(y1, 1), l1[0].conv2)
    x1 = xf(y2, 2, x0)
    y3 = conv("layer1.1.conv1", x1, l1[1].conv1)
    y4 = conv("layer1.1.conv2", xf(y3, 1), l1[1].conv2)
    x2 = xf(y4, 2, x1)
    y5d = conv("layer2.0.conv1|downsample", x2, l2[0].conv1, l2[0].downsample[0])
    y6 = conv("layer2.0.conv2", xf(y5d[:64], 1), l2[0].conv2)
    x3 = xf(y6, 2, y5d[64:], st)
    y7 = conv("layer2.1.conv1", x3, l2[1].conv1)
    y8 = conv("layer2.1.conv2", xf(y7, 1), l2[1].conv2)
    x4 = xf(y8, 2, x3)
    return conv_layer(x4, [enc.conv2], round16)[0]


def channel_R(y, eps=EPS):
    """|mean| / std per channel of y [C, H, W]"""
    mean, rstd = stats64(y, eps)
    return mean.abs() * rstd
