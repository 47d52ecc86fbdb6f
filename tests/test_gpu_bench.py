"""bench.py's command line: a plain run prints the headline line only and `--dump-outputs`
writes what the last timed step computed; `--full` adds the measurements with runs of their
own (CPU baseline, instrumented per-phase steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_options_parse():
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 2
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(libfia_path, tmp_path):
    """One plain run (ml-1m-ex MF k=16, 12,074 queries in one batch, two batches in flight; an odd
    step count, so the last step is the first lane's): the line carries the headline fields and
    none of the `--full` ones, and the dumped arrays are the caller's view of that step."""
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--spinup-seconds", "0", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["value"] > 0
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 12074) < 1e-6 * 12074
    assert out["roofline"]["phase"] == "score" and out["roofline"]["kernel_ms"] > 0
    for key in ("cpu_baseline", "phases_ms_per_step", "phases_ms_per_launch"):
        assert key not in out

    import bench
    Q, D = 12074, 2 * (16 + 1)
    total = out["config"]["related_ratings_rank0_step"]
    arrs = {n[:-4]: np.load(str(out_dir / n)) for n in os.listdir(str(out_dir))}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64e6
    assert total > bench.DUMP_MAX_ELEMS                      # the sampled path
    assert sorted(arrs) == ["influence", "influence_pos", "inverse_hvp", "offsets", "rel_idx", "topk_idx",
                            "topk_pos", "topk_val"]
    off = arrs["offsets"]
    assert off.shape == (Q + 1,) and off[0] == 0 and off[-1] == total and np.all(np.diff(off) >= 0)
    pos = arrs["influence_pos"].astype(np.int64)
    want = np.sort(np.random.default_rng(0).choice(total, bench.DUMP_MAX_ELEMS, replace=False))
    assert np.array_equal(pos, want)
    assert arrs["influence"].shape == arrs["rel_idx"].shape == pos.shape
    assert np.all(np.isfinite(arrs["influence"])) and np.any(arrs["influence"] != 0)
    rel = arrs["rel_idx"]
    assert np.all(rel == np.floor(rel)) and rel.min() >= 0 and rel.max() < out["config"]["n_train"]
    assert arrs["inverse_hvp"].shape == (Q * D,) and np.all(np.isfinite(arrs["inverse_hvp"]))
    # top-1 of each query: the position inside its related set, that rating's train row and value
    tp, tix, tv = arrs["topk_pos"].astype(np.int64), arrs["topk_idx"].astype(np.int64), arrs["topk_val"]
    assert tp.shape == tix.shape == tv.shape == (Q,)
    n_q = np.diff(off).astype(np.int64)
    has = n_q > 0
    assert np.all(tp[has] >= 0) and np.all(tp[has] < n_q[has])
    # where a sampled rating is its query's top-1, the two dumps agree
    q_of = np.searchsorted(off, pos, side="right") - 1
    hit = pos == (off[q_of].astype(np.int64) + tp[q_of])
    assert hit.any()
    assert np.array_equal(arrs["influence"][hit], tv[q_of[hit]])
    assert np.array_equal(rel[hit].astype(np.int64), tix[q_of[hit]])
