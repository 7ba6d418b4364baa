"""Generate tests/golden/ba_prior_ref.npz: the depth-prior bundle adjustment
of the reference's OWN Python (``dpvo/ba.py:151-159``), executed as imported
code.

Runs only where the read-only reference checkout is mounted (see
make_golden.py, whose stand-ins for the reference's native modules, synthetic
state and edge rules this imports).  The fixture is data: seeded inputs, the
prior, and the expected outputs with and without it.

The cases and arguments are those of make_golden.ba_fixtures, which make
``ba.BA`` the Gauss-Newton step of fastba: ep=1.0, lmbda=1e-4,
bounds=[-64,-64,2cx+64,2cy+64], fixedp=t0, one call per iteration.  The prior
is drawn from default_rng(seed + 200): every patch has one with probability
0.5, its depth the patch's depth times U(0.6, 1.6); the rest hold 0 (none).

Usage:  python tests/golden/make_golden_ba_prior.py
"""
import os

import numpy as np
import torch

from make_golden import HERE, dpvo_edges, import_reference, oracle, synth_state

CASES = {   # seed, n, M, t0, iterations, structure only
    "window": (3, 12, 8, 2, 2, False),
    "full": (4, 10, 6, 1, 3, False),
    "structure": (5, 8, 6, 8, 2, True),
}


def main():
    _, ba, lie = import_reference()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    for case, (seed, n, M, t0, iters, structure_only) in CASES.items():
        poses, patches, intr = synth_state(seed, n=n, M=M)
        ii, jj, kk = dpvo_edges(n, M)
        g = np.random.default_rng(seed + 100)
        coords = oracle.transform(poses, patches, intr, ii, jj, kk)[0]  # [E,P,P,2]
        target = (coords[:, 1, 1, :] + g.normal(0, 0.5, size=(len(ii), 2))).astype(np.float32)[None]
        weight = g.uniform(0.2, 1.0, size=(len(ii), 2)).astype(np.float32)[None]
        g = np.random.default_rng(seed + 200)
        scale = g.uniform(0.6, 1.6, n * M)
        has = g.random(n * M) < 0.5
        patches_est = patches.copy()
        patches_est[:, 2] = np.where(has, patches[:, 2, 1, 1] * scale, 0.0).astype(np.float32)[:, None, None]
        cx, cy = float(intr[0, 2]), float(intr[0, 3])
        bounds = [-64, -64, 2 * cx + 64, 2 * cy + 64]

        def run(est):
            Gs, pt = lie.SE3(T(poses.copy())[None]), T(patches.copy())[None]
            for _ in range(iters):
                Gs, pt = ba.BA(Gs, pt, T(intr)[None], T(target), T(weight), 1e-4, T(ii), T(jj), T(kk), bounds,
                               ep=1.0, fixedp=t0, structure_only=structure_only, patches_est=est)
            return Gs.data[0].numpy(), pt[0].numpy()

        poses_out, patches_out = run(T(patches_est)[None])
        poses_out0, patches_out0 = run(torch.zeros_like(T(patches))[None])
        t1 = t0 if structure_only else int(max(ii.max(), jj.max())) + 1
        out.update({f"{case}_poses": poses, f"{case}_patches": patches, f"{case}_intrinsics": intr,
                    f"{case}_target": target, f"{case}_weight": weight, f"{case}_ii": ii, f"{case}_jj": jj,
                    f"{case}_kk": kk, f"{case}_t0": np.int64(t0), f"{case}_t1": np.int64(t1),
                    f"{case}_iters": np.int64(iters), f"{case}_patches_est": patches_est,
                    f"{case}_poses_out": poses_out, f"{case}_patches_out": patches_out,
                    f"{case}_poses_out0": poses_out0, f"{case}_patches_out0": patches_out0})
        opt = np.unique(kk)
        d1, d0 = patches_out[opt, 2, 1, 1], patches_out0[opt, 2, 1, 1]
        print(f"{case}: {int((patches_est[opt, 2, 1, 1] > 0).sum())}/{len(opt)} optimised patches carry a prior; "
              f"depths {d1.min():.3f}..{d1.max():.3f}; the prior moves depths by up to "
              f"{np.abs(d1 / d0 - 1).max():.3f} relative, poses by up to {np.abs(poses_out - poses_out0).max():.2e}")
    np.savez_compressed(os.path.join(HERE, "ba_prior_ref.npz"), **out)
    print("ba prior: reference Python BA vectors saved")


if __name__ == "__main__":
    main()
