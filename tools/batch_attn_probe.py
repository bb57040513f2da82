#!/usr/bin/env python3
"""Batch option "batch_attn" (csrc/attn_batch.hip) against the per-slot attention + o_proj launches,
same process, alternating (Llama-2-7B fp16 synthetic weights, fp16 and int8 KV, graph-replayed steps).

    python tools/batch_attn_probe.py [--pairs 3] [--layers 32] [--n-seq 2,4,8] [--caches F16,I8]
                                     [--out profiles/batch_attn_probe.jsonl]

Two windows per (cache, n_seq): "short", 256 steps from position 0 (8 prompt ids per slot), and
"long", 128 steps from position 1984 (the slots are prefilled once to 1984 rows and rewound there by
Batch.edit before every window), crossing the split boundary at 2048. Every pair times option 0 and
then option 1 on the same slots; set_option drops the captured steps, so each timed window follows an
untimed run of the same window that captures every graph it replays and warms the code objects. A
timed window ends in a stream synchronise. One JSON line per (cache, window, n_seq, pair, option):

  us_per_step   host clock over the window / steps
  tok_s         aggregate: n_seq * steps / window
  tb_s          (llmi_batch_bytes' weight bytes + n_seq * kv_bytes_per_pos * mean cached positions)
                / step time / 1e12 -- option 1 counts W_o once, so its bytes are fewer
  tokens_equal  slot 0's ids after the window equal option 0's of the same pair

and one summary line per (cache, window, n_seq): the medians, the on / off ratio of each pair, the
run-to-run spread (max - min) / median of each arm, and `inside_spread`: whether the median gain is
smaller than the larger of the two spreads. The yardstick is the option-0 arm of the same process.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import llmi  # noqa: E402
from llmi.engine import Batch, preset, synth_prompt  # noqa: E402

LONG_P0, LONG_STEPS, SHORT_STEPS = 1984, 128, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--n-seq", default="2,4,8")
    ap.add_argument("--caches", default="F16,I8")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_attn_probe.jsonl"))
    a = ap.parse_args()
    ns = sorted((int(v) for v in a.n_seq.split(",")), reverse=True)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for cache in a.caches.split(","):
        cfg = preset("llama2-7b", layers=a.layers, max_seq=LONG_P0 + LONG_STEPS, kv_dtype=getattr(llmi, cache))
        short = [synth_prompt(i, 8, cfg.vocab) for i in range(max(ns))]
        long_ = [synth_prompt(100 + i, LONG_P0 + 1, cfg.vocab) for i in range(max(ns))]
        with Batch(cfg, max(ns)) as b:
            b.load_synthetic(0)

            def start(window, n):
                for i in range(n, max(ns)):  # (n_seq runs downwards: an idle slot cannot be rewound)
                    b.reset(i)
                for i in range(n):
                    if window == "short":
                        b.set_prompt(i, short[i])
                    else:  # the cache rows 0 .. 1983 of the one prefill, the last prompt id forced next
                        b.edit(i, LONG_P0, long_[i][LONG_P0:])

            for window, steps, p0 in (("short", SHORT_STEPS, 0), ("long", LONG_STEPS, LONG_P0)):
                if window == "long":
                    for i in range(max(ns)):
                        b.reset(i)
                        b.set_prompt(i, long_[i])
                        b.prefill(i, LONG_P0)
                    b.sync()
                mean_pos = p0 + (steps + 1) / 2.0
                for n in ns:
                    for pair in range(a.pairs):
                        want = None
                        for on in (0, 1):
                            b.set_option("batch_attn", on)
                            start(window, n)
                            b.decode(steps)  # untimed: captures the graphs, warms the code objects
                            b.sync()
                            start(window, n)
                            t0 = time.perf_counter()
                            b.decode(steps)
                            b.sync()
                            dt = (time.perf_counter() - t0) / steps
                            w, kv_pos = b.bytes_per_step()
                            toks = b.tokens(0, p0 + steps + 1).tolist()
                            want = toks if on == 0 else want
                            emit({"cache": cache, "window": window, "n_seq": n, "pair": pair, "batch_attn": on,
                                  "us_per_step": round(dt * 1e6, 2), "tok_s": round(n / dt, 2),
                                  "tb_s": round((w + n * kv_pos * mean_pos) / dt / 1e12, 4), "tokens_equal": toks == want})
                    arm = {on: [r["us_per_step"] for r in lines if (r.get("cache"), r.get("window"), r.get("n_seq"),
                                                                    r.get("batch_attn")) == (cache, window, n, on)]
                           for on in (0, 1)}
                    med = {on: statistics.median(v) for on, v in arm.items()}
                    spread = {on: round((max(v) - min(v)) / med[on], 4) for on, v in arm.items()}
                    emit({"summary": True, "cache": cache, "window": window, "n_seq": n,
                          "us_off_median": med[0], "us_on_median": med[1], "speedup_median": round(med[0] / med[1], 4),
                          "speedup_pairs": [round(x / y, 4) for x, y in zip(arm[0], arm[1])],
                          "spread_off": spread[0], "spread_on": spread[1],
                          "inside_spread": abs(med[0] / med[1] - 1.0) < max(spread.values())})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
