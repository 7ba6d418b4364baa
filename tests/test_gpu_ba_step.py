"""One Gauss-Newton step of the bundle adjustment on the GPU, through the C ABI
(dpvo_ba_forward_prior), on all three solver paths, against the fp64
restatement tests/ba_ref.py with its counted error bars:

  a. the pose step the GPU took solves the reference's normal equations to
     within the backward-error bar (independent of the system's conditioning);
  b. the written depth is clamp(d[pixel 0] + Q (u - E^T xi)) for the GPU's own
     xi, the same bits on all P x P pixels;
  c. nothing else moves (poses outside the window, x / y, unreferenced patches,
     the guards around poses, patches and workspace), status 0;
  d. the output quaternions are unit within 4 u.

The bars, their derivation and the cases are in ba_ref.py (`step_cases`);
tests/test_ba_ref_host.py shows on the CPU that honest fp32 arithmetic stays
below half of every bar.  Observed ratios: profiles/ba_step_tests/NOTES.md.
"""
import numpy as np
import pytest
import torch

import ba_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096          # floats on either side of poses / patches
WS_GUARD = 1 << 16    # bytes behind the workspace (test_ba_workspace_guard_untouched)
KEEP_STATUS = 4


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def guarded(a):
    """a float32 array between two poisoned guards -> (whole buffer, the view BA gets)"""
    n = a.size
    buf = torch.full((2 * GUARD + n,), -1, dtype=torch.int32, device=DEV).view(torch.float32)
    view = buf[GUARD:GUARD + n].view(a.shape)
    view.copy_(T(a))
    return buf, view


def guards_intact(buf, n):
    g = buf.view(torch.int32)
    return bool((g[:GUARD] == -1).all()) and bool((g[GUARD + n:] == -1).all())


def run_gpu(sc, path, iters=1, csr=False, est=None, mu=0.0, kk=None, state=None, status_init=0, flags=0):
    """one dpvo_ba_forward_prior call -> (poses, patches, status) as numpy / int;
    asserts the guards.  state: (poses, patches) to start from instead of the scene's."""
    import _dpvo_hot as H
    import update_ops
    poses, patches = state if state is not None else (sc["poses"], sc["patches"])
    pbuf, p = guarded(np.asarray(poses, np.float32))
    qbuf, q = guarded(np.asarray(patches, np.float32))
    P = patches.shape[-1]
    num_patches = patches.shape[0]
    ii, jj, kk = T(sc["ii"]), T(sc["jj"]), T(sc["kk"] if kk is None else kk)
    E, N = ii.numel(), sc["t1"] - sc["t0"]
    intr, tgt, wgt = T(sc["intrinsics"]), T(sc["target"]), T(sc["weight"])
    lm = torch.tensor([sc["lmbda"]], dtype=torch.float32, device=DEV)
    e = None if est is None else T(est)
    flags |= R.PATH_FLAGS[path]
    offs = perm = groups = None
    if csr:
        _, offs, perm, groups = update_ops.group_by(kk)
    nbytes = H.lib().dpvo_ba_workspace_bytes_ex(E, num_patches, N, flags)
    ws = torch.full((nbytes + WS_GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), status_init, dtype=torch.int32, device=DEV)
    H.check(H.lib().dpvo_ba_forward_prior(
        H.ptr(p), H.ptr(q), num_patches, P, H.ptr(intr), H.ptr(tgt), H.ptr(wgt), H.ptr(lm), H.ptr(e), float(mu),
        H.ptr(ii), H.ptr(jj), H.ptr(kk), E, sc["t0"], sc["t1"], iters, flags, H.ptr(offs), H.ptr(perm), H.ptr(groups),
        H.ptr(ws), nbytes, H.ptr(status), H.stream_of(p)))
    torch.cuda.synchronize()
    assert guards_intact(pbuf, p.numel()), "poses guard"
    assert guards_intact(qbuf, q.numel()), "patches guard"
    assert bool((ws[nbytes:] == 0xAB).all()), "workspace guard"
    return p.cpu().numpy(), q.cpu().numpy(), int(status.item())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_step(name, sc, path, got, est=None, mu=0.0):
    """assertions a - d on one one-step result"""
    gp, gq, status = got
    assert status == 0, name
    t0, t1, P = sc["t0"], sc["t1"], sc["P"]
    ref = R.step(*R.scene_args(sc), est=est, mu=mu)
    e = R.step_errors(sc, ref, gp, gq, path, t0, t1)
    print(f"{name}: k = {e['k']}, pose residual {e['pose']:.3g} of its bar, depth {e['depth']:.3g} "
          f"(patch {e['depth_patch']}), |q| - 1 {e['quat']:.3g} of 4 u")
    assert np.isfinite(gp).all() and np.isfinite(gq).all(), name
    assert e["pose"] <= 1.0, (name, "a: pose step", e["pose"], e.get("pose_row"))
    assert e["depth"] <= 1.0, (name, "b: depth step", e["depth"], e["depth_patch"])
    ku = ref["ne"]["ku"]
    d = bits(gq[ku, 2].reshape(len(ku), -1))
    assert (d == d[:, :1]).all(), (name, "b: the P x P pixels differ")
    # c. nothing else moves
    out = np.ones(len(gp), bool)
    out[t0:t1] = False
    assert np.array_equal(bits(gp[out]), bits(sc["poses"][out])), (name, "c: a pose outside the window")
    assert np.array_equal(bits(gq[:, :2]), bits(sc["patches"][:, :2])), (name, "c: x / y")
    idle = np.ones(len(gq), bool)
    idle[ku] = False
    assert idle.sum() >= (0 if "damping" in name else 2)
    assert np.array_equal(bits(gq[idle]), bits(sc["patches"][idle])), (name, "c: an unreferenced patch")
    if t1 > t0:
        assert e["quat"] <= 1.0, (name, "d: quaternion norm", e["quat"])
    return e


CASES = R.step_cases()


@pytest.mark.parametrize("name,path,kw,mu", CASES, ids=[c[0] for c in CASES])
def test_one_step(name, path, kw, mu):
    sc = R.case_scene(kw)
    est = clean = None
    if mu:
        est, clean = R.make_prior(sc)
    got = run_gpu(sc, path, est=est, mu=mu)
    check_step(name, sc, path, got, est=est, mu=mu)
    if mu:
        # 0, -1, +inf and NaN are "no prior": the same bits as a prior of 0 there
        g2 = run_gpu(sc, path, est=clean, mu=mu)
        if path == "det":
            assert np.array_equal(bits(got[0]), bits(g2[0])) and np.array_equal(bits(got[1]), bits(g2[1])), name
        else:       # (unordered sums: held to the bars instead)
            check_step(name + "/clean", sc, path, g2, est=clean, mu=mu)
        plain = run_gpu(sc, path)
        assert not np.array_equal(bits(plain[1]), bits(got[1])), (name, "the prior did nothing")
    if path == "det":
        # the caller's CSR (update_ops.group_by) gives the bits of BA's own grouping, and so does a rerun
        for kwargs in (dict(csr=True), dict()):
            g2 = run_gpu(sc, path, est=est, mu=mu, **kwargs)
            assert np.array_equal(bits(got[0]), bits(g2[0])) and np.array_equal(bits(got[1]), bits(g2[1])), \
                (name, kwargs)


# The deterministic path's fused second iteration (bd_patch_kernel<true, true>:
# iteration 1's depth step and iteration 2's Hessian in one pass) against two
# one-iteration calls (<false, true> then the closing <true, false>, twice).
# Recorded on an MI355X: see profiles/ba_step_tests/NOTES.md.
DET_TWO_ITERATIONS_BIT_IDENTICAL = True


@pytest.mark.parametrize("path,kw", R.TWO_STEP_CASES, ids=[c[0] for c in R.TWO_STEP_CASES])
def test_two_iterations_equal_two_calls(path, kw):
    sc = R.case_scene(kw)
    two = run_gpu(sc, path, iters=2)
    first = run_gpu(sc, path, iters=1)
    twice = run_gpu(sc, path, iters=1, state=first[:2])
    assert two[2] == 0 and twice[2] == 0
    same = np.array_equal(bits(two[0]), bits(twice[0])) and np.array_equal(bits(two[1]), bits(twice[1]))
    dp, dq = R.distance(two, twice, sc)
    cp, cq = R.distance(R.two_steps(sc, np.float32), R.two_steps(sc), sc)
    print(f"{path} N={kw['N']}: iterations = 2 vs two calls: bit-identical {same}; poses {dp:.3g} (float32_step twice vs "
          f"step twice: {cp:.3g}), depths {dq:.3g} ({cq:.3g})")
    if path == "det" and DET_TWO_ITERATIONS_BIT_IDENTICAL:
        assert same
    else:
        assert dp <= 4 * cp and dq <= 4 * cq


@pytest.mark.parametrize("path", ["det", "atomic", "band"])
def test_bad_patch_index_gives_a_negative_status_and_an_untouched_state(path):
    sc = R.case_scene(dict(seed=5, N=5))
    npat = sc["patches"].shape[0]
    bits_ = 1
    while (1 << bits_) < npat:
        bits_ += 1
    # below 0, just past the end, and past the end by the group-by's bin count
    # (the same low bits as a valid patch that other edges reference)
    for bad in (-1, npat, int(sc["kk"][3]) + (1 << bits_)):
        kk = sc["kk"].copy()
        kk[len(kk) // 2] = bad
        gp, gq, status = run_gpu(sc, path, kk=kk)
        assert status < 0, (path, bad, status)
        assert np.array_equal(bits(gp), bits(sc["poses"])) and np.array_equal(bits(gq), bits(sc["patches"])), (path, bad)


def test_keep_status_with_a_failure_in_the_word_leaves_the_state():
    sc = R.case_scene(dict(seed=5, N=5))
    for word in (7, -2):
        gp, gq, status = run_gpu(sc, "det", status_init=word, flags=KEEP_STATUS)
        assert status == word
        assert np.array_equal(bits(gp), bits(sc["poses"])) and np.array_equal(bits(gq), bits(sc["patches"]))
    gp, gq, status = run_gpu(sc, "det", status_init=0, flags=KEEP_STATUS)
    assert status == 0 and not np.array_equal(bits(gp), bits(sc["poses"]))
    # without the flag the word is cleared and the step is taken
    gp2, gq2, status = run_gpu(sc, "det", status_init=7)
    assert status == 0 and np.array_equal(bits(gp2), bits(gp)) and np.array_equal(bits(gq2), bits(gq))
