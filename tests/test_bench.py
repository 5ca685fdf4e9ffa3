"""bench.py's plain run and --dump-outputs: exactly --steps timed steps in one region, nothing of --full, and the arrays of the
last timed step written the same way from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 64 * 10 ** 6


def test_dump_sample_fits_the_budget_and_is_fixed():
    """CPU: last_step_outputs at the headline's shapes (2 x 400k agents, 13 x 13 x 7 views, 34 features): every reward, the same
    seeded rows of views and features, ascending and distinct, within the byte budget -- and the same rows on a second call"""
    sys.path.insert(0, ROOT)
    import bench
    import torch
    n = 400000
    ids = torch.arange(n, dtype=torch.float32)
    last = {g: (ids.view(n, 1, 1, 1).expand(n, 13, 13, 7), ids.view(n, 1).expand(n, 34), ids + g, n - 1000 * g) for g in (0, 1)}
    out = bench.last_step_outputs(torch, last)
    again = bench.last_step_outputs(torch, last)
    assert sorted(out) == sorted(again) == ["g%d_%s" % (g, k) for g in (0, 1) for k in ("feature_rows", "reward", "view_rows")]
    assert LIMIT * 0.8 < sum(a.nbytes for a in out.values()) <= bench.DUMP_BYTES <= LIMIT
    for g in (0, 1):
        rows = out["g%d_feature_rows" % g][:, 0]
        assert out["g%d_view_rows" % g].shape == (len(rows), 13, 13, 7) and len(rows) > 1000
        assert np.all(np.diff(rows) > 0) and rows[-1] < n - 1000 * g
        assert np.array_equal(out["g%d_view_rows" % g][:, 6, 6, 3], rows)
        assert np.array_equal(out["g%d_reward" % g], np.arange(n - 1000 * g, dtype=np.float32) + g)
        for k in out:
            assert out[k].dtype == np.float32 and np.array_equal(out[k], again[k])


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    """a plain run (no --full) on a small battle world: one JSON line, one region of exactly --steps timed steps, none of what --full
    adds; --dump-outputs writes float32 arrays within 64 MB, bit-identical between two runs with the same arguments"""
    recs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--map-size", "200",
                            "--agents", "2000", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
        assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
        rec = json.loads(lines[0])
        assert rec["steps"] == 7 and rec["repeats"] == 1 and len(rec["repeats_ms_per_step"]) == 1 and rec["ms_per_step"] > 0
        assert rec["unit"] == "agent-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["no_preheat"] is None and "extra" not in rec
        assert abs(rec["value"] * rec["ms_per_step"] * 1e-3 / sum(rec["config"]["agents_at_start"]) - 1) < 0.25
        recs.append({f: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    a, b = recs
    assert sorted(a) == sorted(b) == ["g%d_%s.npy" % (g, k) for g in (0, 1) for k in ("feature_rows", "reward", "view_rows")]
    assert sum(x.nbytes for x in a.values()) <= LIMIT
    for f in a:
        assert a[f].dtype == np.float32 and a[f].size > 0 and np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f
    assert a["g0_view_rows.npy"].shape[1:] == (13, 13, 7) and len(a["g0_view_rows.npy"]) == len(a["g0_reward.npy"])    # a small world: every row
