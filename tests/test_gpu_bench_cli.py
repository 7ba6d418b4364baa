"""bench.main() as a plain run (no --full) with --dump-outputs, on a small
buffer: the line holds the headline figure and nothing that takes runs of its
own, --steps sets the number of timed updates, and the dump is the state the
last timed update() left."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "roofline_update_op", "breakdown_ms", "fastba_us_per_iteration", "host_calibration",
             "cpu_baseline", "end_to_end")


def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys):
    import bench
    from dpvo.dpvo import DPVO
    out = tmp_path / "dump"
    calls = []
    update = DPVO.update
    monkeypatch.setattr(DPVO, "update", lambda self, *a, **k: (calls.append(self), update(self, *a, **k))[1])
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--buffer", "72",
                                     "--dump-outputs", str(out)])
    bench.main()
    torch.cuda.synchronize()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert len(calls) == 2 + 3                      # the warmup and the timed steps, nothing else
    assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "keyframes/s" and line["higher_is_better"] is True and line["dtype"] == "f16+f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]

    slam = calls[-1]
    n, m, M, E = slam.n, slam.pg.m, slam.M, slam.pg.ii.numel()
    shapes = {"poses": (n, 7), "patches": (n * M, 27), "points": (m, 3), "net": (E, 384), "target": (E, 2),
              "weight": (E, 2)}
    assert sorted(os.listdir(out)) == sorted(f"{k}.npy" for k in shapes)
    got = {k: np.load(out / f"{k}.npy") for k in shapes}
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    # the edge state (E x 384 floats) is above the per-array bound: a fixed sample of its rows
    # (seed = its position among the arrays); the others are written whole
    rows = bench.sample_rows(E, 4 * 384, seed=3)
    assert rows is not None and len(rows) == bench.DUMP_ARRAY_BYTES // (4 * 384)
    shapes["net"] = (len(rows), 384)
    for k, a in got.items():
        assert a.dtype == np.float32 and a.shape == shapes[k], k
        assert np.isfinite(a).all(), k
    # main() ran nothing after the last timed step: the tracker still holds what was written
    assert np.array_equal(got["poses"], slam.pg.poses_[:n].cpu().numpy())
    assert np.array_equal(got["patches"], slam.pg.patches_[:n].reshape(n * M, 27).cpu().numpy())
    assert np.array_equal(got["points"], slam.pg.points_[:m].cpu().numpy())
    assert np.array_equal(got["net"], slam.pg.net[0].float().cpu().numpy()[rows])
    assert np.array_equal(got["target"], slam.pg.target[0].cpu().numpy())
    assert np.array_equal(got["weight"], slam.pg.weight[0].cpu().numpy())
