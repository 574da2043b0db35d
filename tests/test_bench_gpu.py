"""bench.py's plain run on the GPU (small table): the result line's headline fields, nothing of the
--full legs in it, and --dump-outputs writing the same float arrays on every run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--keys", "30000", "--workers", "48", *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    runs = []
    for name in ("a", "b"):
        d = _bench("--dump-outputs", str(tmp_path / name))
        assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "ops/s"
        assert d["higher_is_better"] is True and d["dtype"] == "u8" and d["detail"]["error_flags"] == 0
        # the legs of a --full run are not in a plain one
        assert "cpu_baseline" not in d and not {"policies", "host_api", "commit_breakdown"} & set(d["detail"])
        assert list(d["roofline"]["launches"]) == ["local"]
        runs.append({f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = runs
    assert set(a) == {f"{n}.npy" for n in ("op_states", "ops", "table_entries", "inv_count", "counters")}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64), f
        assert np.array_equal(x, b[f]), f"{f} differs between two runs with the same arguments"
    # three timed steps and a warm-up step of 48 x 250 ops: commits counted, ops answered, INVs sent
    assert a["op_states.npy"].shape == (48, 250) and a["ops.npy"].shape[0] == 48 * 250
    assert a["table_entries.npy"].shape[0] == 30000
    assert 0 < a["counters.npy"][0] <= 4 * 48 * 250 and a["inv_count.npy"].sum() > 0
