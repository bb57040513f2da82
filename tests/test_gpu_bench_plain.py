"""A plain `bench.py --gpus 1` run on a short context: the result line carries the headline
fields and none of the `--full` measurements, `--steps` sets the number of timed steps, and
`--dump-outputs` writes the last step's tokens / logits / hidden state as float arrays that a
second run on the same inputs reproduces bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEQ = 64


def _plain(dump, steps=3):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "1", "--max-seq", str(MAX_SEQ), "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    out, err = _plain(tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "tokens/s" and out["higher_is_better"] is True and out["dtype"] == "fp16"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    gen = out["config"]["generated_per_step"]
    assert abs(out["value"] - gen / (out["ms_per_step"] * 1e-3)) <= 1e-2 * out["value"]
    for k in ("roofline", "kernels_us", "kernels_GBps", "graph_timeline", "prefill", "int8_13b", "cpu_baseline"):
        assert k not in out, k
    assert "kernel timings" not in err and "cpu baseline" not in err

    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("tokens", "logits", "hidden")}
    assert a["tokens"].dtype == np.float64 and a["tokens"].shape == (MAX_SEQ + 1,)
    assert a["logits"].dtype == np.float32 and a["logits"].shape == (32000,)
    assert a["hidden"].dtype == np.float32 and a["hidden"].shape == (4096,)
    assert all(np.isfinite(v).all() for v in a.values())
    # greedy: the last token is the argmax of the last forward's logits
    assert int(a["tokens"][-1]) == int(np.argmax(a["logits"]))

    # the same arguments but one timed step: the outputs are those of any step, and a step
    # takes the time it took above. A timed loop that ignored --steps would report a per-step
    # time 3x off in one of the two runs; the same work on the same device repeats well within 2x.
    one, _ = _plain(tmp_path / "b", steps=1)
    assert one["steps"] == 1
    ratio = one["ms_per_step"] / out["ms_per_step"]
    print(f"ms_per_step: {out['ms_per_step']} at --steps 3, {one['ms_per_step']} at --steps 1, ratio {ratio:.3f}")
    assert 0.5 < ratio < 2.0, ratio
    for n, v in a.items():
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / f"{n}.npy"), err_msg=n)
