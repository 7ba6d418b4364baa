"""Time the loop-closure alignment at the reference's largest size (N = 6000
matched points, H = 400 hypotheses, threshold 0.5, early exit off so that all
hypotheses are scored): cuda_ba.ransac_sim3 with HIP events against the numpy
ransac_umeyama loop on the host plus the device->host copy it needs.  Prints
one JSON line.  python scripts/bench_loop_align.py [--runs 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "wild-video-3d-reconstruction_amd")):
    sys.path.insert(0, p)


def host_loop(src, dst, samples, threshold):
    """optim_utils.ransac_umeyama with its break at inliers > 100 removed"""
    from dpvo.loop_closure import umeyama_alignment
    best, best_inliers = (None, None, None), 0
    for idx in samples:
        R, t, s = umeyama_alignment(src[idx].T, dst[idx].T)
        if t is None:
            continue
        mask = np.linalg.norm(src @ (R * s).T + t - dst, axis=1) < threshold
        inliers = int(mask.sum())
        if inliers > best_inliers:
            best_inliers = inliers
            best = umeyama_alignment(src[mask].T, dst[mask].T)
    return best, best_inliers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--hypotheses", type=int, default=400)
    a = ap.parse_args()
    import cuda_ba
    from dpvo.loop_closure import draw_samples
    rng = np.random.default_rng(0)
    N, H = a.points, a.hypotheses
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    src = rng.normal(size=(N, 3)) * 2
    dst = 1.3 * src @ q.T + rng.uniform(-3, 3, 3) + 0.02 * rng.normal(size=(N, 3))
    bad = rng.choice(N, N // 2, replace=False)
    dst[bad] += rng.uniform(5, 10, (len(bad), 3))
    samples = draw_samples(N, H, 1)
    dsrc, ddst, dsmp = (torch.from_numpy(x).cuda() for x in (src, dst, samples))
    for _ in range(3):
        out = cuda_ba.ransac_sim3(dsrc, ddst, dsmp, 0.5, early_exit=-1)
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = cuda_ba.ransac_sim3(dsrc, ddst, dsmp, 0.5, early_exit=-1)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host_ms, copy_ms = [], []
    for _ in range(max(a.runs // 4, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hs, hd = dsrc.cpu().numpy(), ddst.cpu().numpy()
        t1 = time.perf_counter()
        best, inl = host_loop(hs, hd, samples, 0.5)
        t2 = time.perf_counter()
        copy_ms.append(1e3 * (t1 - t0))
        host_ms.append(1e3 * (t2 - t1))
    info = out[3].tolist()
    assert info[2] == inl, (info, inl)
    print(json.dumps(dict(points=N, hypotheses=H, runs=a.runs, device=torch.cuda.get_device_name(0),
                          device_ms_median=float(np.median(dev_ms)), device_ms_min=float(np.min(dev_ms)),
                          device_ms_max=float(np.max(dev_ms)), host_loop_ms_median=float(np.median(host_ms)),
                          host_copy_ms_median=float(np.median(copy_ms)), inliers=inl, winner=info[1])))


if __name__ == "__main__":
    main()
