"""CPU checks of tests/encoder_layers_ref.py, the fp64 restatement the GPU
layer tests (tests/test_gpu_encoder_layers.py) compare the encoder kernels
with: chained with its roundings off it is BasicEncoder4.forward, and the
crafted instance-norm partials reduce to the statistics they were made for.
"""
import numpy as np
import pytest
import torch

import encoder_layers_ref as R


@pytest.mark.parametrize("norm", ["instance", "none"])
def test_chained_layers_are_the_module(norm):
    """the helper's layers in NativeEncoders.run's order, fp16 roundings off ==
    BasicEncoder4.forward in fp64 (20 x 36 frame)"""
    from dpvo.extractor import BasicEncoder4
    torch.manual_seed(3)
    enc = BasicEncoder4(128 if norm == "instance" else 384, norm).double().eval()
    u8 = torch.randint(0, 256, (3, 20, 36), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    with torch.no_grad():
        want = enc((2 * (u8.double() / 255.0) - 0.5)[None, None])[0, 0]
        seen = []
        got = R.encoder_chain(enc, u8, round16=False, on_layer=lambda name, y: seen.append(name))
    assert got.shape == want.shape == (enc.conv2.out_channels, 5, 9)
    assert len(seen) == 9        # the nine convolutions whose outputs are normalised
    assert (got - want).abs().max().item() <= 1e-12


def test_spacing16():
    v = torch.tensor([0.0, 2.0 ** -30, 2.0 ** -14, 0.75, 1.0, 1.5, 2.0, -3.0, 1000.0], dtype=torch.float64)
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 0.5]
    assert R.spacing16(v).tolist() == want


def _crafted_cases():
    """(C, n, tiles, seed) of every crafted statistics buffer the GPU tests build"""
    import test_gpu_encoder_layers as T
    return sorted(set(T.crafted_stat_cases()))


def test_crafted_partials_reduce_to_their_statistics():
    """reduce_stats' arithmetic on the crafted partial rows returns the
    intended rstd and shift = -mean rstd within 2 fp32 spacings, for every
    (channels, pixels, rows, seed) the GPU tests use"""
    cases = _crafted_cases()
    assert len(cases) > 20
    for C, n, tiles, seed in cases:
        gen = torch.Generator().manual_seed(seed)
        mean, rstd, part = R.crafted_stats(C, n, tiles, gen)
        assert part.shape == (tiles, 2 * C) and part.dtype == np.float32
        m, s, sh = R.reduce_stats_np(part, 0, C, n)
        np.testing.assert_array_equal(m, mean.numpy())            # the sums are exact
        want_r = rstd.numpy().astype(np.float32)
        want_s = (-mean.numpy() * rstd.numpy()).astype(np.float32)
        assert (np.abs(s - want_r) <= 2 * np.spacing(want_r)).all(), (C, n, tiles, seed)
        assert (np.abs(sh - want_s) <= 2 * np.spacing(np.abs(want_s))).all(), (C, n, tiles, seed)
        # ... and in fact exactly, which is what makes xout comparable bit for bit
        assert R.reduces_exactly(part, mean, rstd, n).all(), (C, n, tiles, seed)
        # the grid keeps x exact: a * rstd + shift on multiples of 2^-6, at most 12
        assert (np.abs(mean.numpy() * rstd.numpy()) <= 2).all() and len(set(zip(m.tolist(), want_r.tolist()))) > 1


def test_tile_counts_are_uneven_and_sum_to_n():
    for n, tiles in ((1, 17), (153, 1), (153, 17), (153, 130), (200, 130)):
        gen = torch.Generator().manual_seed(n + tiles)
        mean, rstd, part = R.crafted_stats(8, n, tiles, gen)
        assert set(rstd.tolist()) <= {0.5, 1.0, 2.0, 4.0} and (mean * 8 == (mean * 8).round()).all()
        assert (mean.abs() <= 1).all()
        nt = R.tile_counts(n, tiles, gen)
        assert nt.shape == (tiles,) and int(nt.sum()) == n and int(nt.min()) >= 0
        if tiles > 1 and n > 1:
            assert len(set(nt.tolist())) > 1


def test_tile_sums_count_valid_pixels_only():
    h = torch.ones(2, 9, 17, dtype=torch.float64)
    S, Q, A = R.tile_sums(h)
    assert S.shape == (4, 2)
    assert S[:, 0].tolist() == [128.0, 8.0, 16.0, 1.0] and torch.equal(S, Q) and torch.equal(S, A)
