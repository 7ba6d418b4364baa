"""Host side of the loop-closure alignment and triangulation: the fixture
conditions that let test_gpu_loop_align.py ask for exact counts and masks, the
winner rule against the numpy ransac_umeyama, the new C-ABI signatures and the
fp64 triangulation restatement (loop_align_ref.py).  No GPU."""
import numpy as np
import pytest
import torch

import loop_align_ref as L


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_fixture_has_no_undecided_point(name):
    """no residual of any hypothesis lies within 1e-9 max(1, threshold) of the
    threshold: two fp64 implementations of the 3-point model (they differ by
    ~1e-15 times the sample's condition number) count the same inliers"""
    r = L.restated(name)
    print(name, "undecided", int(r["undecided"].sum()), "counts max", int(r["counts"].max()))
    assert int(r["undecided"].sum()) == 0
    assert (r["counts"] >= 0).all()        # seeded samples are valid (a least-squares fit through an outlier may have no inlier)


def test_fixtures_cover_both_sides_of_the_early_exit():
    k = L.restated("exit")["counts"]
    above = k[k > L.EARLY_EXIT]
    assert len(above) >= 3 and len(set(above.tolist())) >= 2
    # the early exit does not return the best hypothesis there, nor in the largest case
    for name in ("exit", "big"):
        k = L.restated(name)["counts"]
        first, best = L.pick_winner(k, L.EARLY_EXIT), L.pick_winner(k, -1)
        assert first != best and k[first] < k[best]
    for name in ("n3", "n4", "n63", "n64", "n65"):
        assert L.restated(name)["counts"].max() <= L.EARLY_EXIT


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_winner_rule_is_the_sequential_loop(name):
    """first count > 100, else first maximum == what numpy's ransac_umeyama
    (break at inliers > 100, strict improvement) returns on the same Generator"""
    from dpvo.loop_closure import ransac_umeyama
    c, r = L.case(name), L.restated(name)
    R, t, s, inliers = ransac_umeyama(c["src"], c["dst"], iterations=len(c["samples"]), threshold=c["threshold"],
                                      rng=c["seed"])
    assert inliers == r["info"][2] == int(r["mask"].sum())
    np.testing.assert_allclose(R, r["refit"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(t, r["refit"][1], rtol=0, atol=1e-12)
    assert abs(s - r["refit"][2]) < 1e-12


@pytest.mark.parametrize("name", sorted(L.CASES))
@pytest.mark.parametrize("early_exit", [L.EARLY_EXIT, -1])
def test_winner_inliers_are_well_conditioned(name, early_exit):
    """sigma3 / sigma1 of the winner's inlier covariance >= 1e-3: the refit is
    held to 1e-9 on these fixtures"""
    c, r = L.case(name), L.restated(name, early_exit)
    x, y = c["src"][r["mask"]], c["dst"][r["mask"]]
    d = np.linalg.svd((y - y.mean(0)).T @ (x - x.mean(0)) / len(x), compute_uv=False)
    print(name, early_exit, "sigma3/sigma1", d[2] / d[0])
    assert d[2] / d[0] >= 1e-3 or len(x) == 3    # three points span a plane: rank 2, by construction
    assert d[1] / d[0] >= 1e-3


def test_crafted_samples():
    c = L.crafted()
    r = L.restate(c["src"], c["dst"], c["samples"], c["threshold"])
    assert [h for h in range(len(c["samples"])) if r["counts"][h] == -1] == c["bad"]
    assert r["undecided"].sum() == 0 and r["winner"] == 4
    # the collinear triple's covariance has one non-zero entry: rank 1 exactly
    x, y = c["src"][:3], c["dst"][:3]
    cov = (y - y.mean(0)).T @ (x - x.mean(0)) / 3
    assert np.count_nonzero(cov) == 1
    only_bad = L.restate(c["src"], c["dst"], c["samples"][c["bad"]], c["threshold"])
    assert only_bad["info"] == [1, -1, 0, 0]
    line = L.restate(c["src"][:10], c["dst"][:10], np.array([[0, 1, 2]]), c["threshold"])
    assert line["info"][0] == 1


def test_draw_samples_is_the_numpy_sequence():
    from dpvo.loop_closure import draw_samples
    rng = np.random.default_rng(3)
    want = np.stack([rng.choice(50, 3, replace=False) for _ in range(7)])
    assert np.array_equal(draw_samples(50, 7, 3), want)
    assert np.array_equal(draw_samples(50, 7, np.random.default_rng(3)), want)


def test_align_signatures_match_the_header():
    import ctypes
    import _dpvo_hot as H
    from test_capi import prototypes
    cls = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_size_t: "size", ctypes.c_int: "int",
           ctypes.c_double: "double"}
    protos = prototypes()
    for name in ["dpvo_sim3_workspace_bytes", "dpvo_sim3_ransac", "dpvo_sim3_umeyama"]:
        assert name in protos, name
        assert [cls[a] for a in H._SIGNATURES[name][1]] == protos[name], name
    lib = H.lib()
    assert 0 < lib.dpvo_sim3_workspace_bytes(6000, 400) <= 4096
    assert lib.dpvo_sim3_workspace_bytes(2, 1) == 0


def test_align_entries_refuse_cpu_tensors():
    import cuda_ba
    from dpvo.loop_closure import ransac_umeyama_gpu
    src, dst = torch.zeros(5, 3), torch.ones(5, 3)
    samples = torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.ransac_sim3(src, dst, samples, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.umeyama(src, dst)
    with pytest.raises(RuntimeError, match="GPU"):
        ransac_umeyama_gpu(src, dst, iterations=2, rng=0)


@pytest.mark.parametrize("n", [1, 65, 300])
def test_triangulation_scene(n):
    """in the fp64 restatement (oracle.transform + oracle.ba_forward, structure
    only) no track's larger residual lies in [1.9, 2.1] px, every shifted
    track is rejected and every clean one kept; the depths come out right"""
    sc = L.scene(n)
    for frame in (L.SCENE_I, L.SCENE_J):
        r = L.triangulate_ref(n, frame)
        sh = sc["shifted"][frame]
        print(n, frame, "worst clean", r["worst"][~sh].max(), "least shifted", r["worst"][sh].min() if sh.any() else None)
        assert not ((r["worst"] >= 1.9) & (r["worst"] <= 2.1)).any()
        assert np.array_equal(r["keep"], ~sh)
        scale = L.SCENE_SCALE if frame == L.SCENE_J else 1.0
        # 0.2 px of noise on 160 px of parallax per unit of inverse depth: a few percent in depth at z = 10
        np.testing.assert_allclose(r["points"][~sh, 2], scale * sc["depth"][frame][~sh], rtol=0.1)


def test_tracks_restatement_recovers_the_scene_sim3():
    R, t, s, inliers = L.tracks_far_ref(300)
    far = L.scene(300)["far"]
    assert inliers > L.EARLY_EXIT       # of ~240 matched pairs; depth noise at z = 10 is ~0.2 units
    err = L.far_error((R, t, s), far)
    print("restatement's far_rel_pose error", err)
    assert err < 0.05
