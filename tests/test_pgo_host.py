"""Host side of the loop-closure pose-graph optimisation: the numpy
point-cloud alignment, the ctypes signatures of the new C-ABI entries, and the
fp64 restatement of the Levenberg-Marquardt loop (pgo_helpers.py) that
test_gpu_pgo.py compares the device against.  No GPU."""
import numpy as np
import pytest
import torch

import pgo_helpers as P


def _similarity(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.uniform(-3, 3, 3), float(rng.uniform(0.5, 2.0))


def test_umeyama_recovers_a_known_similarity():
    from dpvo.loop_closure import umeyama_alignment
    rng = np.random.default_rng(0)
    R, t, s = _similarity(rng)
    x = rng.normal(size=(3, 10))
    y = s * (R @ x) + t[:, None]
    r, tt, c = umeyama_alignment(x, y)
    np.testing.assert_allclose(r, R, atol=1e-9)
    np.testing.assert_allclose(tt, t, atol=1e-9)
    assert abs(c - s) < 1e-9


def test_umeyama_refuses_collinear_points():
    from dpvo.loop_closure import umeyama_alignment
    # points on one axis: the covariance has rank 1 exactly (the rule is the
    # reference's absolute one, singular values > machine epsilon)
    x = np.outer([1.0, 0.0, 0.0], np.arange(10.0))
    y = 2.0 * x + 1.0
    r, t, c = umeyama_alignment(x, y)
    assert r is None and t is None and c is None


def test_ransac_umeyama_with_gross_outliers():
    from dpvo.loop_closure import ransac_umeyama
    rng = np.random.default_rng(1)
    R, t, s = _similarity(rng)
    src = rng.normal(size=(60, 3)) * 2
    dst = s * src @ R.T + t
    bad = rng.choice(60, 18, replace=False)            # 30 % gross outliers
    dst[bad] += rng.choice([-1.0, 1.0], (18, 3)) * rng.uniform(5, 10, (18, 3))
    r, tt, c, inliers = ransac_umeyama(src, dst, iterations=200, threshold=0.1, rng=np.random.default_rng(7))
    assert inliers == 42
    np.testing.assert_allclose(r, R, atol=1e-9)
    np.testing.assert_allclose(tt, t, atol=1e-9)
    assert abs(c - s) < 1e-9
    # the same seed gives the same samples
    again = ransac_umeyama(src, dst, iterations=200, threshold=0.1, rng=np.random.default_rng(7))
    assert again[3] == inliers and np.array_equal(again[0], r)


def test_pgo_signatures_match_the_header():
    import ctypes
    import _dpvo_hot as H
    from test_capi import prototypes
    cls = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_size_t: "size", ctypes.c_int: "int",
           ctypes.c_double: "double"}
    protos = prototypes()
    names = ["dpvo_pgo_workspace_bytes", "dpvo_pgo_residual", "dpvo_pgo_step", "dpvo_pgo"]
    for name in names:
        assert name in protos, name
        assert [cls[a] for a in H._SIGNATURES[name][1]] == protos[name], name
    lib = H.lib()
    # the skyline, not the dense matrix: at most 64 MB at the global-BA size
    assert 0 < lib.dpvo_pgo_workspace_bytes(4096, 16) <= 64 << 20
    assert lib.dpvo_pgo_workspace_bytes(1, 0) == 0


def test_pgo_entries_refuse_cpu_tensors():
    import cuda_ba
    poses = torch.zeros(4, 7)
    poses[:, 6] = 1
    loops = torch.tensor([[0.0, 0, 0, 0, 0, 0, 1, 1]])
    ii, jj = torch.tensor([2]), torch.tensor([0])
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.pgo(poses, loops, ii, jj)
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.pgo_step(torch.zeros(4, 7), poses, loops, ii, jj, 0.0, 1e-6, -1)
    with pytest.raises(RuntimeError, match="GPU"):
        cuda_ba.pgo_residual(torch.zeros(4, 7), poses, loops, ii, jj)


def test_sim3_tensor_helpers_match_the_oracle():
    from dpvo.loop_closure.optim_utils import sim3_inv, sim3_mul
    rng = np.random.default_rng(2)
    a, b = P.random_loops(5, rng), P.random_loops(5, rng)
    np.testing.assert_allclose(sim3_mul(torch.from_numpy(a), torch.from_numpy(b)).numpy(), P.sim3_mul(a, b),
                               atol=1e-12)
    np.testing.assert_allclose(sim3_inv(torch.from_numpy(a)).numpy(), P.sim3_inv(a), atol=1e-12)


@pytest.mark.parametrize("n,L", sorted(P.LM_CASES))
def test_lm_restatement_fixture_condition(n, L):
    """The restatement's leading LM_CASES[..]['iters'] steps have
    cost_new / cost_old outside [0.99, 1.01] (so accept / reject cannot flip
    between two fp64 implementations), they are all accepted, and the loop
    constraints pull the drifted trajectory back: the cost falls by 100x."""
    case = P.LM_CASES[(n, L)]
    gt, poses, loops, ii, jj = P.circle_case(n, L, case["seed"])
    ref = P.lm_restatement(poses, loops, ii, jj, iters=case["iters"] + 1)
    ratios = ref["ratios"]
    print("ratios", ratios, "hist", ref["hist"])
    lead = ratios[:case["iters"]]
    assert ((lead < 0.99) | (lead > 1.01)).all()
    assert ref["accepts"][:case["iters"]] == [True] * case["iters"]
    assert ref["hist"][case["iters"]] < 0.01 * ref["hist"][0]
    # zero residual at the ground truth: the loop constraints are consistent with it
    assert np.abs(P.residual(P.initial_state(gt), gt, loops, ii, jj)).max() < 1e-9
    # the float32 solve of oracle.solve_system takes the same decisions
    r32 = P.lm_restatement(poses, loops, ii, jj, iters=case["iters"], solver="f32")
    assert r32["accepts"] == ref["accepts"][:case["iters"]]
