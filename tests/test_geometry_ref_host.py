"""CPU pins of tests/geometry_ref.py, the fp64 restatement the GPU geometry
tests compare against: it agrees with the oracle on the edge-reaching scene,
with the reference Python's recorded outputs on the golden scene, and the scene
reaches the clamp, the back of the camera and the validity threshold often
enough that the GPU tests cannot pass vacuously."""
import os

import numpy as np
import pytest

import geometry_ref as G
from conftest import GOLDEN
from oracle import oracle

PS = (1, 2, 3, 4)
SEEDS = (0, 1, 2, 3, 4)


def close_rel(got, want, scale, rel=1e-12):
    """|got - want| <= rel * (the magnitudes the value was summed from)"""
    err = np.abs(got - want)
    assert (err <= rel * scale).all(), float((err / scale).max())


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("depth,tonly", [(False, False), (True, False), (False, True), (True, True)])
def test_transform_restatement_matches_oracle(P, depth, tonly):
    s = G.make_scene(P)
    args = (s["poses"], s["patches"], s["intrinsics"], s["ii"], s["jj"], s["kk"])
    r = G.transform(*args, depth=depth, tonly=tonly)
    want, v = oracle.transform(*args, depth=depth, valid=True, tonly=tonly)
    # relative to the sum of magnitudes behind each value (S / EPS): x and y are
    # differences of terms up to 1e4 px, a bar relative to |x| alone would
    # measure the cancellation, not the restatement
    close_rel(r["coords"], want[0], r["S"] / G.EPS)
    near = np.abs(r["Z"] - 0.2) < 1e-12 * r["Az"]
    assert not near.any()
    np.testing.assert_array_equal(r["valid"], v[0])


@pytest.mark.parametrize("P", PS)
def test_point_cloud_centre_restatement_matches_oracle(P):
    s = G.make_scene(P)
    args = (s["poses"], s["patches"], s["intrinsics"], s["ix"])
    r = G.point_cloud_centre(*args)
    close_rel(r["centre"], oracle.point_cloud_centre(*args), r["S"] / G.EPS)
    c = G.centre_index(P)
    full = G.point_cloud(*args)["full"]
    np.testing.assert_array_equal(r["centre"], full[:, c[0], c[1], :3] / full[:, c[0], c[1], 3:])


def test_restatement_matches_reference_python_golden():
    """the bars are those the golden file's fp32 outputs are held to in test_gpu_geometry.py"""
    g = np.load(os.path.join(GOLDEN, "pops_ref.npz"))
    args = (g["poses"], g["patches"], g["intrinsics"], g["ii"], g["jj"], g["kk"])
    r = G.transform(*args)
    np.testing.assert_allclose(r["coords"][None], g["coords"], rtol=1e-5, atol=2e-4)
    r = G.transform(*args, depth=True)
    np.testing.assert_allclose(r["coords"][None], g["coords_depth"], rtol=1e-5, atol=2e-4)
    np.testing.assert_array_equal(r["valid"][None], g["valid"])
    r = G.transform(*args, tonly=True)
    np.testing.assert_allclose(r["coords"][None], g["coords_tonly"], rtol=1e-5, atol=2e-4)
    pc = G.point_cloud(g["poses"], g["patches"], g["intrinsics"], g["ix"])
    np.testing.assert_allclose(pc["full"][None], g["point_cloud"], rtol=1e-5, atol=1e-5)
    # flow_mag has no bar of its own in that file's tests: each norm moves by at
    # most its two coordinate differences' bars, 2 x 2e-4
    fm = G.flow_mag(g["poses"], g["patches"], g["intrinsics"], g["ii"][:40], g["jj"][:40], g["kk"][:40], 0.5)
    np.testing.assert_allclose(fm["flow"][None], g["flow_mag"], rtol=1e-5, atol=4e-4)


def test_fp32_chain_stays_within_counted_bar():
    """S has the right shape: the same chain in fp32 numpy (matrix form, its
    own statement order) stays inside K S on the scene, with room to spare"""
    worst = 0.0
    for P in PS:
        s = G.make_scene(P)
        f = np.float32
        q = s["poses"][:, 3:]
        q = q / np.sqrt((q * q).sum(1, dtype=f))[:, None]
        R = G.rotmat(q).astype(f)
        t = s["poses"][:, :3]
        ii, jj = s["ii"], s["jj"]
        Rij = np.einsum("erk,eck->erc", R[jj], R[ii])
        tij = t[jj] - np.einsum("erc,ec->er", Rij, t[ii])
        pa, Ki, Kj = s["patches"][s["kk"]], s["intrinsics"][ii][:, :, None, None], s["intrinsics"][jj][:, :, None, None]
        a = np.stack([(pa[:, 0] - Ki[:, 2]) / Ki[:, 0], (pa[:, 1] - Ki[:, 3]) / Ki[:, 1], np.ones_like(pa[:, 2])], -1)
        X = np.einsum("erc,epqc->epqr", Rij, a) + tij[:, None, None, :] * pa[:, 2][..., None]
        assert X.dtype == np.float32
        d = f(1) / np.maximum(X[..., 2], f(0.1))
        xy = np.stack([Kj[:, 0] * (d * X[..., 0]) + Kj[:, 2], Kj[:, 1] * (d * X[..., 1]) + Kj[:, 3], d], -1)
        r = G.transform(s["poses"], s["patches"], s["intrinsics"], ii, jj, s["kk"], depth=True)
        ratio = np.abs(xy.astype(np.float64) - r["coords"]) / r["S"]
        worst = max(worst, float(ratio.max()))
    print(f"fp32 numpy chain: worst error / S = {worst:.2f}")
    assert worst <= G.K_D


def test_scene_reaches_the_edges():
    """class shares and the cap on undecided valid flags, on the reference alone"""
    tot = clamped = behind = band = undecided = 0
    for P in PS:
        for seed in SEEDS:
            s = G.make_scene(P, seed)
            r = G.transform(s["poses"], s["patches"], s["intrinsics"], s["ii"], s["jj"], s["kk"])
            Z = r["Z"]
            share = lambda m: m.mean()
            # every scene on its own: a GPU test on any of them meets each class
            assert share(Z < 0.1) >= 0.01 and share(Z < 0) >= 0.01 and share((Z >= 0.1) & (Z <= 0.2)) >= 0.01, (P, seed)
            assert share(G.valid_undecided(r)) <= 0.005, (P, seed)
            tot += Z.size
            clamped += (Z < 0.1).sum(); behind += (Z < 0).sum(); band += ((Z >= 0.1) & (Z <= 0.2)).sum()
            undecided += G.valid_undecided(r).sum()
    print(f"{tot} pixels: Z<0.1 {clamped / tot:.3%}, Z<0 {behind / tot:.3%}, 0.1<=Z<=0.2 {band / tot:.3%}, "
          f"undecided valid {undecided / tot:.4%}")
    # quaternions off unit norm and |x| far outside the image, as the scene promises
    s = G.make_scene(3)
    qn = np.linalg.norm(s["poses"][:, 3:].astype(np.float64), axis=1)
    assert (np.abs(qn[::3] - 1) < 1e-6).all() and (np.abs(np.delete(qn, np.s_[::3]) - 1) > 1e-3).any()
    assert np.abs(G.transform(s["poses"], s["patches"], s["intrinsics"], s["ii"], s["jj"], s["kk"])["coords"]).max() > 5e3
