#!/usr/bin/env python3
"""Batched decode against the plain engine, same process, alternating (Llama-2-7B fp16 synthetic
weights, fp16 KV, 8 prompt ids, graph-replayed forwards at positions 0 .. ctx-1, ctx 256).

    python tools/batch_probe.py [--passes 3] [--ctx 256] [--layers 32] [--n-seq 1,2,4,8] [--out profiles/batch_probe.jsonl]

Every pass times the plain Engine and then a Batch at each n_seq (every slot active, its own
prompt), so drift of the box hits all of them alike; the Engine is the yardstick of its own
pass. Each timed window is ctx forwards ending in a stream synchronise, after an untimed run of
the same window that captured every graph it replays. One JSON line per (pass, variant):

  us_per_step     host clock over the window / ctx
  tok_s           aggregate: n_seq * ctx / window (forwards of all sequences per second)
  weight_bytes    llmi_batch_bytes: the weights once + W_o once more per further active slot
  kv_bytes        n_seq * kv_bytes_per_pos * mean cached positions of the window
  bytes_s         (weight_bytes + kv_bytes) / step time: achieved algorithmic bytes per second
  model_bytes_per_token   the byte model (W - W_o) / n + W_o + KV for one token of one sequence

and a last line with the medians, each n_seq's speed-up over the Engine of the same pass, and
the spread of the Engine's own passes (the margin a speed-up has to clear). On the MI355X this
was measured on ("Batched decode") aggregate tokens/s rises at every n_seq up to 8
-- 8 is not slower than 4 -- so n_seq is not capped below the kernel's limit of 8.
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
from llmi.engine import Batch, Engine, preset, synth_prompt  # noqa: E402


def window(run, reset, ctx):
    reset()
    run(ctx)          # untimed: captures every graph the window replays, warms the code objects
    reset()
    t0 = time.perf_counter()
    run(ctx)          # ends in a stream synchronise
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--n-seq", default="1,2,4,8")
    ap.add_argument("--int8", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_probe.jsonl"))
    a = ap.parse_args()
    ns = [int(v) for v in a.n_seq.split(",")]
    cfg = preset("llama2-7b", layers=a.layers, max_seq=a.ctx)
    cfg.kv_dtype = llmi.F16
    if a.int8:
        cfg.weight_dtype = llmi.I8
    prompts = [synth_prompt(i, 8, cfg.vocab) for i in range(max(ns))]
    mean_pos = (a.ctx + 1) / 2.0  # positions 1 .. ctx are cached over the window
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    with Engine(cfg) as e, Batch(cfg, max(ns)) as b:
        e.load_synthetic(0)
        b.load_synthetic(0)
        w_engine, kv_pos = e.bytes_per_token()
        c = cfg
        w_o = c.layers * c.hidden * c.hidden * (1 if a.int8 else 2) + (c.layers * c.hidden * 2 if a.int8 else 0)

        def run_e(n):
            e.decode(n)
            e.sync()

        def run_b(n):
            b.decode(n)
            b.sync()

        def reset_b(n_seq):
            for i in range(max(ns)):
                b.reset(i)
            for i in range(n_seq):
                b.set_prompt(i, prompts[i])

        # the batch decodes what the engine decodes (slot 0 holds the engine's prompt)
        reset_b(max(ns))
        run_b(32)
        e.set_prompt(prompts[0])
        run_e(32)
        same = b.tokens(0, 33).tolist() == e.tokens(33).tolist()

        for p in range(a.passes):
            dt = window(run_e, lambda: e.set_prompt(prompts[0]), a.ctx)
            kv = kv_pos * mean_pos
            emit({"pass": p, "variant": "engine", "n_seq": 1, "us_per_step": round(dt / a.ctx * 1e6, 2),
                  "tok_s": round(a.ctx / dt, 2), "weight_bytes": w_engine, "kv_bytes": int(kv),
                  "bytes_s": round((w_engine + kv) / (dt / a.ctx), 0),
                  "model_bytes_per_token": int(w_engine + kv), "tokens_equal": same})
            for n in ns:
                dt = window(run_b, lambda n=n: reset_b(n), a.ctx)
                w, _ = b.bytes_per_step()
                kv = n * kv_pos * mean_pos
                emit({"pass": p, "variant": "batch", "n_seq": n, "us_per_step": round(dt / a.ctx * 1e6, 2),
                      "tok_s": round(n * a.ctx / dt, 2), "weight_bytes": w, "kv_bytes": int(kv),
                      "bytes_s": round((w + kv) / (dt / a.ctx), 0),
                      "model_bytes_per_token": int((w_engine - w_o) / n + w_o + kv_pos * mean_pos),
                      "tokens_equal": same})

    eng = [r["tok_s"] for r in lines if r["variant"] == "engine"]
    summary = {"summary": True, "engine_tok_s_median": statistics.median(eng),
               "engine_spread": round((max(eng) - min(eng)) / statistics.median(eng), 4), "batch": {}}
    for n in ns:
        t = [r["tok_s"] for r in lines if r["variant"] == "batch" and r["n_seq"] == n]
        # per-pass ratio against the Engine of the same pass
        ratios = [x / y for x, y in zip(t, eng)]
        summary["batch"][str(n)] = {"tok_s_median": statistics.median(t), "speedup_min": round(min(ratios), 4),
                                    "speedup_median": round(statistics.median(ratios), 4),
                                    "spread": round((max(t) - min(t)) / statistics.median(t), 4)}
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
