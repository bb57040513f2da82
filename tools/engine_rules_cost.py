#!/usr/bin/env python3
"""What the logit rules cost per token inside the engine's token step: same-process A/B on the
bench workload (Llama-2-7B synthetic, fp16 weights and KV, 8 prompt ids, graph-replayed forwards
at positions 0..max_seq-1), alternating the modes pass by pass so box drift hits all of them
alike.

    python tools/engine_rules_cost.py [--passes 5] [--max-seq 2048] [--tail 48] [--out profiles/engine_rules_cost.json]

modes: off (no rules: the step is the step without this feature), bias_mask (a bias on 128 ids,
8 of them banned, and an allowed set of every odd id), full (the same plus presence / frequency
penalties with count_prompt, so the history is every id so far). Each pass times the whole run
and, separately, its last --tail positions, where the history of `full` holds max_seq - tail
ids or more (2000 at the defaults). Prints one JSON line per (pass, mode) and a summary
(medians, run-to-run spread) at the end; --out writes the summary.
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

MODES = ("off", "bias_mask", "full")


def set_mode(e, mode, vocab):
    e.clear_logit_rules()
    if mode == "off":
        return
    rng = np.random.default_rng(1)
    ids = rng.choice(vocab, 128, replace=False)
    bias = {int(i): (-np.inf if k < 8 else float(rng.normal() * 2)) for k, i in enumerate(ids)}
    if mode == "bias_mask":
        e.set_logit_rules(bias=bias)
    else:
        e.set_logit_rules(bias=bias, presence_penalty=0.4, frequency_penalty=0.2, count_prompt=True)
    e.set_allowed(np.arange(1, vocab, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-seq", type=int, default=2048)
    ap.add_argument("--tail", type=int, default=48)
    ap.add_argument("--preset", default="llama2-7b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = preset(a.preset, layers=a.layers, max_seq=a.max_seq)
    cfg.kv_dtype = llmi.F16
    prompt = synth_prompt(0, 8, cfg.vocab)
    head = a.max_seq - a.tail
    whole = {m: [] for m in MODES}
    tail = {m: [] for m in MODES}
    with Engine(cfg) as e:
        e.load_synthetic(0)
        for p in range(a.passes):
            for m in MODES:
                set_mode(e, m, cfg.vocab)  # drops the captured graphs
                e.set_prompt(prompt)
                e.decode(a.max_seq)  # every split count's graph captured outside the timed region
                e.set_prompt(prompt)
                e.sync()
                t0 = time.perf_counter()
                e.decode(head)
                e.sync()
                t1 = time.perf_counter()
                e.decode(a.tail)
                e.sync()
                t2 = time.perf_counter()
                whole[m].append((t2 - t0) / a.max_seq * 1e6)
                tail[m].append((t2 - t1) / a.tail * 1e6)
                print(json.dumps({"pass": p, "mode": m, "us_per_token": round(whole[m][-1], 2),
                                  "tail_us_per_token": round(tail[m][-1], 2)}), flush=True)

    def stats(runs):
        med = statistics.median(runs)
        return {"us_median": round(med, 2), "tokens_per_s": round(1e6 / med, 1),
                "us_runs": [round(x, 2) for x in runs], "spread_pct": round((max(runs) - min(runs)) / med * 100, 3)}

    summary = {"workload": f"{a.preset} synthetic fp16, fp16 KV, layers {a.layers}, positions 0..{a.max_seq - 1}, "
                           f"graph replay, {a.passes} alternating passes; tail = the last {a.tail} positions "
                           f"(history of `full` >= {head} ids)",
               "whole_run": {m: stats(whole[m]) for m in MODES},
               "tail": {m: stats(tail[m]) for m in MODES}}
    for part in ("whole_run", "tail"):
        off = summary[part]["off"]["us_median"]
        for m in MODES[1:]:
            summary[part][m]["over_off_us"] = round(summary[part][m]["us_median"] - off, 2)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
