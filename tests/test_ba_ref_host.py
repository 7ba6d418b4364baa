"""tests/ba_ref.py (the fp64 one-step restatement of the bundle adjustment)
pinned on the CPU, independently of any kernel: against the float oracle, the
reference's own Python BA (golden), central differences of its own
reprojection, its scene builder's stated contents, and the proof that the bars
of tests/test_gpu_ba_step.py leave a factor 2 for honest fp32 arithmetic."""
import os

import numpy as np
import pytest

import ba_ref as R
from conftest import GOLDEN
from oracle import oracle


def test_one_step_agrees_with_the_float_oracle():
    """The oracle differs from the fp64 step by its own fp32 arithmetic: no
    more than 4 times what the float32 restatement differs by (the two fp32
    computations differ in summation order)."""
    sc = R.make_scene(3, 10, well_conditioned=True)
    args = R.scene_args(sc)
    ref, f32 = R.step(*args), R.float32_step(*args)
    op, oq, st = oracle.ba_forward(*args, 1)
    assert st == 0
    dp, dq = R.distance((op, oq), (ref["poses"], ref["patches"]), sc)
    fp, fq = R.distance((f32["poses"], f32["patches"]), (ref["poses"], ref["patches"]), sc)
    print(f"oracle vs fp64: poses {dp:.3g} depths {dq:.3g}; float32_step vs fp64: {fp:.3g} {fq:.3g}")
    assert np.abs(ref["dX"]).max() > 1e-3          # the window moved
    assert dp <= 4 * fp and dq <= 4 * fq


def assert_close_rel(got, ref, rtol, floor=1e-5):
    """test_gpu_fastba.assert_close_rel: norm-wise per tensor, and per element where |ref| > 1e-3."""
    assert np.linalg.norm(got - ref) <= rtol * max(np.linalg.norm(ref), floor)
    big = np.abs(ref) > 1e-3
    assert np.all(np.abs(got[big] - ref[big]) <= rtol * np.abs(ref[big]) + floor)


def repeated_step(c, est=None, mu=0.0, lmbda=1e-4):
    p, q = c["poses"], c["patches"]
    for _ in range(int(c["iters"])):
        s = R.step(p, q, c["intrinsics"], c["target"], c["weight"], lmbda, c["ii"], c["jj"], c["kk"], int(c["t0"]),
                   int(c["t1"]), est=est, mu=mu)
        p, q = s["poses"], s["patches"]
    return p, q


@pytest.mark.parametrize("case", ["window", "full", "structure"])
def test_agrees_with_the_reference_python_ba(case):
    """the golden outputs of the reference's Python BA (2 iterations, fp32) at
    the project's bar for that reference, 2e-3 relative"""
    g = dict(np.load(os.path.join(GOLDEN, "ba_python_ref.npz")))
    c = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + "_")}
    p, q = repeated_step(c)
    assert_close_rel(p, c["poses_out"].reshape(-1, 7).astype(np.float64), 2e-3)
    assert_close_rel(q[:, 2, 1, 1], c["patches_out"][:, 2, 1, 1].astype(np.float64), 2e-3)


@pytest.mark.parametrize("case", ["window", "full", "structure"])
def test_agrees_with_the_reference_python_ba_with_the_prior(case):
    g = dict(np.load(os.path.join(GOLDEN, "ba_prior_ref.npz")))
    c = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + "_")}
    p, q = repeated_step(c, est=c["patches_est"], mu=2.0)
    assert_close_rel(p, c["poses_out"].reshape(-1, 7).astype(np.float64), 2e-3)
    assert_close_rel(q[:, 2, 1, 1], c["patches_out"][:, 2, 1, 1].astype(np.float64), 2e-3)
    p, q = repeated_step(c)
    assert_close_rel(p, c["poses_out0"].reshape(-1, 7).astype(np.float64), 2e-3)
    assert_close_rel(q[:, 2, 1, 1], c["patches_out0"][:, 2, 1, 1].astype(np.float64), 2e-3)


@pytest.mark.parametrize("mu", [2.0, 0.5])
def test_closed_form_with_zero_weights(mu):
    """test_gpu_ba_prior's closed form: all weights zero, one step moves a patch
    with a prior to d + mu / (mu + lmbda) (est - d); d is the centre pixel's in
    the prior term and pixel 0's in the update"""
    sc = R.make_scene(5, 6)
    est, _ = R.make_prior(sc)
    s = R.step(sc["poses"], sc["patches"], sc["intrinsics"], sc["target"], np.zeros_like(sc["weight"]), 1e-4,
               sc["ii"], sc["jj"], sc["kk"], sc["t0"], sc["t1"], est=est, mu=mu)
    ku = s["ne"]["ku"]
    d0, dc, e = (np.asarray(x, np.float64) for x in (sc["patches"][ku, 2, 0, 0], sc["patches"][ku, 2, 1, 1],
                                                      est[ku, 2, 1, 1]))
    on = s["ne"]["has_prior"]
    assert on.sum() > 5 and (~on).sum() > 5
    want = np.where(on, d0 + mu / (mu + 1e-4) * (np.where(on, e, 0) - dc), d0)
    np.testing.assert_allclose(s["patches"][ku, 2, 1, 1], R.depth_update(want, 0.0), rtol=1e-12)
    assert np.abs(s["dX"]).max() < 1e-12


def test_jacobians_are_central_differences_of_the_reprojection():
    sc = R.make_scene(7, 8)
    # (unit quaternions in fp64: the analytic Jacobians assume them; the float32
    # ones are off by 1e-7, which is what the difference would then measure)
    poses = sc["poses"].astype(np.float64)
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    et = R.edge_terms(poses, *R.scene_args(sc)[1:5], sc["ii"], sc["jj"], sc["kk"], sc["t0"], sc["t1"])
    ok = et["Z"] > 0.25          # (below 0.2 the Jacobians are zero by definition)
    ii, jj, kk = sc["ii"][ok], sc["jj"][ok], sc["kk"][ok]
    px, py, d = (sc["patches"][kk, c, 1, 1].astype(np.float64) for c in range(3))
    intr = sc["intrinsics"][0].astype(np.float64)
    h = 1e-6
    # every edge gets its own copy of its two poses, so each role moves alone
    E = len(ii)
    poses = np.concatenate([poses[ii], poses[jj]])
    I, J_ = np.arange(E), E + np.arange(E)

    def proj(P, dd=d):
        return R.project(P, px, py, dd, intr, I, J_)[0]
    worst = 0.0
    for t in range(6):
        xi = np.zeros((E, 6))
        xi[:, t] = h
        for rows, J, sign in ((I, et["Ji"][ok], -1.0), (J_, et["Jj"][ok], 1.0)):
            plus, minus = poses.copy(), poses.copy()
            plus[rows], minus[rows] = R.retract(poses[rows], xi), R.retract(poses[rows], -xi)
            num = (proj(plus) - proj(minus)) / (2 * h)
            err = np.abs(num - sign * J[:, :, t]) / (1 + np.abs(J[:, :, t]))
            worst = max(worst, err.max())
    num = (proj(poses, d + h) - proj(poses, d - h)) / (2 * h)
    worst = max(worst, (np.abs(num - et["Jz"][ok]) / (1 + np.abs(et["Jz"][ok]))).max())
    print(f"worst relative difference to central differences: {worst:.3g}")
    assert worst < 1e-6   # h^2 |f'''| + 1e-16 |f| / h with h = 1e-6 on values of 1e2


def all_scenes():
    seen = {}
    for name, path, kw, mu in R.step_cases():
        seen.setdefault(tuple(sorted(kw.items())), (name, kw))
    return list(seen.values())


def test_scene_builder_contents():
    for name, kw in all_scenes():
        sc = R.case_scene(kw)
        assert sc["min_margin"] >= R.REL_MARGIN, (name, sc["min_margin"])
        assert sc["masked_share"] <= 0.25, name
        if kw.get("damping"):
            continue
        assert 14 <= sc["n"] <= max(24, sc["t1"] - sc["t0"] + 2) and 3 <= sc["M"] <= 6 or kw.get("M") == 150
        N = sc["t1"] - sc["t0"]
        for cls in R.CLASSES:
            if N == 0 and cls in ("i_fixed", "j_fixed"):
                continue          # no window: every edge has both poses fixed
            assert len(sc["classes"][cls]) >= 2, (name, cls)
        # both sides of every mask condition, as the fp64 edge terms see them
        et = R.edge_terms(*R.scene_args(sc)[:5], sc["ii"], sc["jj"], sc["kk"], sc["t0"], sc["t1"])
        s = sc["sides"]
        assert abs(et["Z"][s["Z_out"]] - 0.1) < 1e-3 and abs(et["Z"][s["Z_in"]] - 0.4) < 1e-3
        assert not et["mask"][s["Z_out"]] and et["mask"][s["Z_in"]]
        W, H = 2 * sc["intrinsics"][0, 2], 2 * sc["intrinsics"][0, 3]
        for key, axis, want in (("x_lo", 0, -30), ("x_hi", 0, W + 30), ("y_lo", 1, -30), ("y_hi", 1, H + 30)):
            out = want - 70 if want < 0 else want + 70
            assert abs(et["x1"][s[key + "_in"], axis] - want) < 1e-2 and et["mask"][s[key + "_in"]]
            assert abs(et["x1"][s[key + "_out"], axis] - out) < 1e-2 and not et["mask"][s[key + "_out"]]
        if N > 0:
            rn = np.linalg.norm(et["r"], axis=1)
            assert np.allclose(rn[s["r_in"]], 90, atol=1e-3) and et["mask"][s["r_in"]].all()
            assert np.allclose(rn[s["r_out"]], 200, atol=1e-3) and not et["mask"][s["r_out"]].any()
        # non-uniform depth: pixel 0, the centre and the rest differ by 10 to 30 %
        P = sc["P"]
        if P > 1:
            d = sc["patches"][:, 2].astype(np.float64)
            d0, dc, dr = d[:, 0, 0], d[:, P // 2, P // 2], d[:, 0, 1]
            for a, b in ((d0, dc), (dr, dc), (d0, dr)):
                rel = np.abs(a / b - 1)
                assert (rel > 0.099).all(), name
            assert (np.abs(d0 / dc - 1) < 0.301).all() and (np.abs(dr / dc - 1) < 0.301).all(), name


def clamp_margins(sc, ref):
    """both sides of both clamp limits, as the fp64 step lands them"""
    ku, pre = ref["ne"]["ku"], ref["pre"]
    at = lambda key: pre[np.searchsorted(ku, sc["kk"][sc["sides"][key]])]
    return at("hi_reset"), at("hi_keep"), at("lo_floor"), at("lo_keep")


def test_bars_leave_a_factor_two_for_honest_fp32():
    """float32_step, held to every bar of test_gpu_ba_step.py on every scene and
    parameter set used there, stays below half of it; and no decision (mask,
    clamp, small-angle branch) sits within REL_MARGIN of its threshold."""
    worst = {}
    for name, path, kw, mu in R.step_cases():
        sc = R.case_scene(kw)
        est = R.make_prior(sc)[0] if mu else None
        args = R.scene_args(sc)
        ref, f32 = R.step(*args, est=est, mu=mu), R.float32_step(*args, est=est, mu=mu)
        e = R.step_errors(sc, ref, f32["poses"], f32["patches"], path, sc["t0"], sc["t1"])
        for key in ("pose", "depth"):
            worst[key] = max(worst.get(key, (0, ""))[0], e[key]), name
            assert e[key] <= 0.5, (name, key, e[key])
        assert np.array_equal(ref["et"]["mask"], f32["et"]["mask"]), name
        pre = ref["pre"]
        mag = np.abs(pre - ref["dZ"]) + np.abs(ref["dZ"])
        assert (np.abs(pre - 20) >= R.REL_MARGIN * 20).all() and (np.abs(pre - 1e-4) >= R.REL_MARGIN * mag).all(), name
        if not kw.get("damping") and not mu:
            hr, hk, lf, lk = clamp_margins(sc, ref)
            assert hr > 20.5 and 19 < hk < 19.9 and lf < -0.01 and 1e-3 < lk < 0.05, (name, hr, hk, lf, lk)
        if sc["t1"] > sc["t0"]:
            th = np.linalg.norm(ref["dX"][:, 3:], axis=1)
            assert (th > 2e-4).all(), name     # clear of both small-angle branches (1e-4; theta^2 < 1e-8)
    print("worst float32_step error in units of the bar:", worst)


@pytest.mark.parametrize("path,kw", R.TWO_STEP_CASES, ids=[c[0] for c in R.TWO_STEP_CASES])
def test_two_steps_distance(path, kw):
    """the CPU distance the two-iteration GPU test is held to (4 times it)"""
    sc = R.case_scene(kw)
    dp, dq = R.distance(R.two_steps(sc, np.float32), R.two_steps(sc), sc)
    print(f"{path} N={kw['N']}: float32_step twice vs step twice: poses {dp:.3g}, depths {dq:.3g} relative")
    assert 0 < dp < 1e-4 and 0 < dq < 1e-4
