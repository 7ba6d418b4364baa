"""The depth-prior BA fixture (tests/golden/ba_prior_ref.npz, written by
make_golden_ba_prior.py from the reference's own dpvo/ba.py) is fit to pin
the native prior term, and the host-side argument checks (no GPU work).

The GPU parity test (test_gpu_ba_prior.py) compares with assert_close_rel at
rtol 2e-3, the project's bar for GPU fastba against ba.py.  A BA that ignores
the prior must miss that bar by a wide margin: here, by a factor of 10.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CASES = ["window", "full", "structure"]
RTOL, FLOOR = 2e-3, 1e-5   # test_gpu_ba_prior.py's bar (assert_close_rel)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "ba_prior_ref.npz"))


def optimised(gold, case):
    return np.unique(gold[f"{case}_kk"])


def excess(a, b):
    """how many times over assert_close_rel's per-element bar a is off b (max)"""
    big = np.abs(b) > 1e-3
    return float((np.abs(a[big] - b[big]) / (RTOL * np.abs(b[big]) + FLOOR)).max())


@pytest.mark.parametrize("case", CASES)
def test_fixture_loads_and_depths_are_far_from_the_clamps(gold, case):
    f = lambda k: gold[f"{case}_{k}"]
    n_patch = f("patches").shape[0]
    assert f("patches_est").shape == f("patches").shape == f("patches_out").shape == (n_patch, 3, 3, 3)
    assert f("poses_out").shape == f("poses").shape
    est = f("patches_est")[:, 2, 1, 1]
    assert np.isfinite(est).all() and (est >= 0).all()
    k = optimised(gold, case)
    assert 0 < (est[k] > 0).sum() < len(k)          # patches with and without a prior
    # away from the reference's clamp (1e-3, 10) and from fastba's reset rule
    # (d > 20 -> 1, max(d, 1e-4)): the differing retraction rules never fire
    d = f("patches_out")[k, 2]
    assert d.min() > 1e-2 and d.max() < 5
    d0 = f("patches_out0")[k, 2]
    assert d0.min() > 1e-2 and d0.max() < 5


@pytest.mark.parametrize("case", CASES)
def test_a_ba_without_the_prior_cannot_pass(gold, case):
    f = lambda k: gold[f"{case}_{k}"]
    k = optimised(gold, case)
    assert excess(f("patches_out0")[k, 2, 1, 1], f("patches_out")[k, 2, 1, 1]) >= 10
    if case != "structure":
        assert excess(f("poses_out0"), f("poses_out")) >= 10
    else:
        assert np.array_equal(f("poses_out"), f("poses")) and np.array_equal(f("poses_out0"), f("poses"))


def _cpu_args(gold):
    f = lambda k: torch.from_numpy(np.ascontiguousarray(gold[f"structure_{k}"]))
    return (f("poses"), f("patches")[None], f("intrinsics"), f("target"), f("weight"), torch.tensor([1e-4]),
            f("ii"), f("jj"), f("kk"), int(gold["structure_t0"]), int(gold["structure_t1"]), 1)


def test_forward_refuses_a_cpu_patches_est(gold):
    import cuda_ba
    args = _cpu_args(gold)
    with pytest.raises(RuntimeError, match="patches_est"):
        cuda_ba.forward(*args, patches_est=torch.zeros_like(args[1]), prior_mu=2.0)


@pytest.mark.parametrize("mu", [-1.0, float("nan"), float("inf")])
def test_a_negative_or_non_finite_mu_is_an_error(mu):
    """through the C ABI (checked before any GPU work) and in the Python shim"""
    import _dpvo_hot as H
    lib = H.lib()
    null = ctypes.c_void_p(0)
    rc = lib.dpvo_ba_forward_prior(null, null, 0, 3, null, null, null, null, null, mu, null, null, null, 0, 0, 0, 0, 0,
                                   null, null, null, null, 0, null, null)
    assert rc != 0
    assert b"prior_mu" in lib.dpvo_hot_last_error()


def test_config_defaults_leave_the_tracker_as_it_was():
    from dpvo.config import cfg, make_cfg
    assert cfg.DEPTH_PRIOR_BA is False and cfg.DEPTH_PRIOR_MU == 2.0
    c = make_cfg("fast", DEPTH_PRIOR_BA=True, DEPTH_PRIOR_MU=1)
    assert c.DEPTH_PRIOR_BA is True and c.DEPTH_PRIOR_MU == 1.0 and isinstance(c.DEPTH_PRIOR_MU, float)
