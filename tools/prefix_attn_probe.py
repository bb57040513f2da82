#!/usr/bin/env python3
"""Batch option "prefix_attn" (csrc/attn_prefix.hip) against "batch_attn" 1, same process, alternating
(Llama-2-7B fp16 synthetic weights, fp16 and int8 KV, 32 and 8 kv heads, graph-replayed steps).

    python tools/prefix_attn_probe.py [--pairs 3] [--layers 32] [--n-seq 2,4,8] [--caches F16,I8]
                                      [--kv-heads 32,8] [--prompts 2048,8192] [--steps 64]
                                      [--out profiles/prefix_attn_probe.jsonl]

Per (cache, kv heads): slot 0 prefills the longest prompt once. A window at prompt length L rewinds
slot 0 to L (Batch.edit), forks it into slots 1 .. n - 1 at L (one fork group sharing L rows) and
decodes `steps` steps. Every pair times batch_attn 1 / prefix_attn 0 and then prefix_attn 1 on the same
slots; set_option drops the captured steps, so each timed window follows an untimed run of the same
window that captures every graph it replays and warms the code objects. A timed window ends in a
stream synchronise. One JSON line per (cache, kv_heads, prompt, n_seq, pair, option):

  us_per_step   host clock over the window / steps
  tok_s         aggregate: n_seq * steps / window
  kv_gb_off     cache bytes a step reads without sharing: n_seq * kv_bytes_per_pos * mean positions
  kv_gb_on      ... with the prompt's whole 64-row splits read once for the group
  tokens_equal  slot 1's ids after the window equal option 0's of the same pair (the option is
                faithful to fp32, not bitwise: a late id may differ)

and one summary line per (cache, kv_heads, prompt, n_seq): the medians, the off / on ratio of each
pair, the run-to-run spread (max - min) / median of each arm, and `inside_spread`: whether the median
gain is smaller than the larger of the two spreads. The yardstick is the option-0 arm of the same process.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--n-seq", default="2,4,8")
    ap.add_argument("--caches", default="F16,I8")
    ap.add_argument("--kv-heads", default="32,8")
    ap.add_argument("--prompts", default="2048,8192")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prefix_attn_probe.jsonl"))
    a = ap.parse_args()
    ns = [int(v) for v in a.n_seq.split(",")]
    # (longest first: a window decodes over the prefilled rows behind its prompt length)
    prompts = sorted((int(v) for v in a.prompts.split(",")), reverse=True)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for cache in a.caches.split(","):
        for kvh in (int(v) for v in a.kv_heads.split(",")):
            cfg = preset("llama2-7b", layers=a.layers, kv_heads=kvh, max_seq=max(prompts) + a.steps,
                         kv_dtype=getattr(llmi, cache))
            ids = synth_prompt(100, max(prompts) + 1, cfg.vocab)
            with Batch(cfg, max(ns)) as b:
                b.load_synthetic(0)
                b.set_option("batch_attn", 1)
                b.set_prompt(0, ids)
                b.prefill(0, max(prompts))
                b.sync()

                def start(L, n):  # n slots at position L, one fork group of L shared rows
                    for i in range(1, max(ns)):
                        b.reset(i)
                    b.edit(0, L, ids[L:L + 1])
                    b.fork(0, range(1, n), keep=L, ids=ids[L:L + 1])

                for L in prompts:
                    for n in ns:
                        for pair in range(a.pairs):
                            want = None
                            for on in (0, 1):
                                b.set_option("prefix_attn", on)
                                start(L, n)
                                b.decode(a.steps)  # untimed: captures the graphs, warms the code objects
                                b.sync()
                                start(L, n)
                                t0 = time.perf_counter()
                                b.decode(a.steps)
                                b.sync()
                                dt = (time.perf_counter() - t0) / a.steps
                                kv_pos = b.bytes_per_step()[1]
                                toks = b.tokens(1, L + a.steps + 1).tolist()
                                want = toks if on == 0 else want
                                mean = L + (a.steps + 1) / 2.0
                                emit({"cache": cache, "kv_heads": kvh, "prompt": L, "n_seq": n, "pair": pair,
                                      "prefix_attn": on, "us_per_step": round(dt * 1e6, 2), "tok_s": round(n / dt, 2),
                                      "kv_gb_off": round(n * kv_pos * mean / 1e9, 3),
                                      "kv_gb_on": round(kv_pos * (n * (mean - L // 64 * 64) + L // 64 * 64) / 1e9, 3),
                                      "tokens_equal": toks == want})
                        key = (cache, kvh, L, n)
                        arm = {on: [r["us_per_step"] for r in lines if not r.get("summary") and
                                    (r["cache"], r["kv_heads"], r["prompt"], r["n_seq"], r["prefix_attn"]) == key + (on,)]
                               for on in (0, 1)}
                        med = {on: statistics.median(v) for on, v in arm.items()}
                        spread = {on: round((max(v) - min(v)) / med[on], 4) for on, v in arm.items()}
                        emit({"summary": True, "cache": cache, "kv_heads": kvh, "prompt": L, "n_seq": n,
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
