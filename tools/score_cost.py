#!/usr/bin/env python3
"""What the scored prefill costs, and what it saves: same-process A/B on Llama-2-7B synthetic
(fp16 weights and KV), the modes alternating pass by pass so box drift hits all of them alike.

  prefill:  prefill(512) against prefill(512, score=True) at n_top 0 and 8 -- the cost of the
            final norm + lm_head GEMM over 512 rows + the logits slab + one logprob launch;
  score:    Engine.score(ids) stepping (len - 1 graph-replayed token steps) against
            Engine.score(ids, prefill=True) for a text of --text ids.

    python tools/score_cost.py [--passes 3] [--text 2048] [--out profiles/score_cost.jsonl]

Prints one JSON line per (pass, part, mode) and a summary line (medians, each mode's spread over
the passes); --out writes the same lines.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import numpy as np  # noqa: E402

import llmi  # noqa: E402
from llmi.engine import Engine, preset, synth_prompt  # noqa: E402

PREFILL_MODES = {"plain": None, "scored_n_top0": 0, "scored_n_top8": 8}


def timed(e, fn):
    e.sync()
    t0 = time.perf_counter()
    out = fn()
    e.sync()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--text", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--preset", default="llama2-7b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = preset(a.preset, layers=a.layers, max_seq=max(a.text, a.rows))
    cfg.kv_dtype = llmi.F16
    prompt = synth_prompt(0, a.rows, cfg.vocab)
    text = synth_prompt(1, a.text, cfg.vocab)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def prefill_once(e, n_top):
        e.set_logprobs(-1 if n_top is None else n_top)
        e.set_prompt(prompt)
        return timed(e, lambda: e.prefill(a.rows, score=n_top is not None))[0]

    ms = {m: [] for m in PREFILL_MODES}
    sc = {"stepping": [], "prefill": []}
    with Engine(cfg) as e:
        e.load_synthetic(0)
        for m, n_top in PREFILL_MODES.items():  # scratch, slab and kernels loaded outside the timed region
            prefill_once(e, n_top)
        for p in range(a.passes):
            for m, n_top in PREFILL_MODES.items():
                ms[m].append(prefill_once(e, n_top))
                emit({"pass": p, "part": "prefill", "mode": m, "ms": round(ms[m][-1], 3)})
        e.set_logprobs(0)
        e.score(text)  # every split count's graph captured outside the timed region
        got = {}
        for p in range(a.passes):
            for m in sc:
                dt, got[m] = timed(e, lambda: e.score(text, prefill=(m == "prefill")))
                sc[m].append(dt)
                emit({"pass": p, "part": "score", "mode": m, "ms": round(dt, 3)})
    d = np.abs(got["prefill"].astype(np.float64) - got["stepping"])

    def med(v):
        return round(statistics.median(v), 3)

    def spread(v):
        return round((max(v) / min(v) - 1) * 100, 2)

    base = statistics.median(ms["plain"])
    emit({"workload": f"{a.preset} synthetic fp16, fp16 KV, layers {a.layers}; prefill of {a.rows} rows; "
                      f"score of a {a.text}-id text; {a.passes} alternating passes, wall clock around a stream sync",
          "prefill_ms_median": {m: med(v) for m, v in ms.items()},
          "prefill_spread_pct": {m: spread(v) for m, v in ms.items()},
          "scoring_cost_ms": {m: round(statistics.median(v) - base, 3) for m, v in ms.items() if m != "plain"},
          "scoring_cost_pct": {m: round((statistics.median(v) / base - 1) * 100, 2) for m, v in ms.items()
                               if m != "plain"},
          "logits_slab_mb": round(min(a.rows, 512) * cfg.vocab * 4 / 1e6, 1),
          "score_ms_median": {m: med(v) for m, v in sc.items()},
          "score_spread_pct": {m: spread(v) for m, v in sc.items()},
          "score_us_per_token": {m: round(statistics.median(v) * 1e3 / (a.text - 1), 2) for m, v in sc.items()},
          "score_speedup": round(statistics.median(sc["stepping"]) / statistics.median(sc["prefill"]), 1),
          "score_max_abs_dlp": float(d.max()), "score_mean_abs_dlp": float(d.mean())})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
