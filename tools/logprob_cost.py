#!/usr/bin/env python3
"""What per-token log-probabilities cost: same-process A/B of the engine with logprobs off,
n_top 0 and n_top 8 on the bench workload (Llama-2-7B synthetic, fp16 weights and KV, 8 prompt
ids, greedy, graph-replayed forwards at positions 0..max_seq-1, so the mean context is
max_seq / 2), alternating the modes pass by pass so box drift hits all of them alike, and the
logprob kernel timed alone.

    python tools/logprob_cost.py [--passes 5] [--max-seq 2048] [--out profiles/logprob_cost.jsonl]

Prints one JSON line per (pass, mode) and a summary line (medians, the launch's µs per token =
on minus off) at the end; --out writes the same lines.
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
import torch  # noqa: E402  (before llmi: the library then binds the HIP runtime torch has loaded)

import llmi  # noqa: E402
from llmi import ops  # noqa: E402
from llmi.engine import Engine, preset, synth_prompt  # noqa: E402

MODES = {"off": -1, "n_top0": 0, "n_top8": 8}


def kernel_alone(vocab, iters):
    rng = np.random.default_rng(0)
    z = torch.from_numpy((rng.standard_normal((1, vocab)) * 3).astype(np.float32)).cuda()
    ids = torch.zeros(1, device="cuda", dtype=torch.int32)
    out = {}
    for n_top in (0, 8):
        ops.logprobs(z, ids, n_top)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                for _ in range(iters):
                    ops.logprobs(z, ids, n_top)
        g.replay()
        torch.cuda.synchronize()
        runs = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            g.replay()
            t1.record()
            torch.cuda.synchronize()
            runs.append(t0.elapsed_time(t1) * 1e3 / iters)
        out[f"n_top{n_top}"] = {"us_median": round(statistics.median(runs), 2), "us_runs": [round(r, 2) for r in runs]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-seq", type=int, default=2048)
    ap.add_argument("--preset", default="llama2-7b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = preset(a.preset, layers=a.layers, max_seq=a.max_seq)
    cfg.kv_dtype = llmi.F16
    prompt = synth_prompt(0, 8, cfg.vocab)
    us = {m: [] for m in MODES}
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    with Engine(cfg) as e:
        e.load_synthetic(0)
        for p in range(a.passes):
            for m, n_top in MODES.items():
                e.set_logprobs(n_top)  # drops the captured graphs
                e.set_prompt(prompt)
                e.decode(a.max_seq)  # every split count's graph captured outside the timed region
                e.set_prompt(prompt)
                e.sync()
                t0 = time.perf_counter()
                e.decode(a.max_seq)
                e.sync()
                dt = time.perf_counter() - t0
                us[m].append(dt / a.max_seq * 1e6)
                emit({"pass": p, "mode": m, "us_per_token": round(us[m][-1], 2)})
    med = {m: statistics.median(us[m]) for m in MODES}
    emit({"workload": f"{a.preset} synthetic fp16, fp16 KV, layers {a.layers}, greedy, positions 0..{a.max_seq - 1} "
                      f"(mean context {a.max_seq // 2}), graph replay, {a.passes} alternating passes",
          "token_us_median": {m: round(v, 2) for m, v in med.items()},
          "launch_us_per_token": {m: round(med[m] - med["off"], 2) for m in MODES if m != "off"},
          "over_off_pct": {m: round((med[m] / med["off"] - 1) * 100, 3) for m in MODES if m != "off"},
          "off_spread_pct": round((max(us["off"]) / min(us["off"]) - 1) * 100, 3),
          "kernel_alone_us": kernel_alone(cfg.vocab, 200)})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
