#!/usr/bin/env python3
"""What the logit-rules launch costs: llmi_process_logits timed alone under graph replay at
the Llama-2-7B vocabulary (one row of 32000 fp32 logits), in four cases -- rules empty, bias
plus mask, penalties over a 64-id generated history, penalties over a 2000-id one -- beside
the project's own yardstick in the same process, the logprob launch (n_top 0).

    python tools/logit_rules_cost.py [--iters 200] [--runs 7] [--out profiles/logit_rules_cost.jsonl]

Prints one JSON line per case (median and spread of the per-launch time over the runs) and a
summary line; --out writes the same lines.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before llmi: the library then binds the HIP runtime torch has loaded)

import llmi  # noqa: E402,F401
from llmi import ops  # noqa: E402

VOCAB = 32000


def replay_us(launch, iters, runs):
    """Median / runs of one launch's time inside a graph of `iters` back-to-back launches."""
    launch()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for _ in range(iters):
                launch()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        g.replay()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / iters)
    return {"us_median": round(statistics.median(out), 2), "us_min": round(min(out), 2), "us_max": round(max(out), 2),
            "spread_pct": round((max(out) / min(out) - 1) * 100, 2)}


def cases(rng):
    z = torch.from_numpy((rng.standard_normal((1, VOCAB)) * 3).astype(np.float32)).cuda()
    out = torch.empty_like(z)
    ids = torch.empty(1, device="cuda", dtype=torch.int32)
    zero = torch.zeros(1, device="cuda", dtype=torch.int32)
    bias = np.zeros(VOCAB, np.float32)
    idx = rng.choice(VOCAB, 300, replace=False)
    bias[idx] = rng.standard_normal(300).astype(np.float32)
    bias[idx[:50]] = -np.inf
    bias = torch.from_numpy(bias).cuda()
    mask = torch.from_numpy(rng.integers(0, 2 ** 32, (VOCAB + 31) // 32, dtype=np.uint32).view(np.int32)).cuda()

    def hist(n):
        return torch.from_numpy(rng.integers(0, VOCAB, (1, n)).astype(np.int32)).cuda()

    h64, h2000 = hist(64), hist(2000)
    kw = dict(out=out, out_ids=ids)
    return {
        "empty": lambda: ops.process_logits(z, **kw),
        "bias_mask": lambda: ops.process_logits(z, bias=bias, allowed=mask, **kw),
        "penalties_h64": lambda: ops.process_logits(z, history=h64, presence_penalty=0.5, frequency_penalty=0.1, **kw),
        "penalties_h2000": lambda: ops.process_logits(z, history=h2000, presence_penalty=0.5, frequency_penalty=0.1,
                                                      **kw),
        "all_h2000": lambda: ops.process_logits(z, bias=bias, allowed=mask, history=h2000, presence_penalty=0.5,
                                                frequency_penalty=0.1, **kw),
        "yardstick_logprob_n_top0": lambda: ops.logprobs(z, zero, 0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    summary = {"workload": f"one row of {VOCAB} fp32 logits, graph of {a.iters} launches, {a.runs} replays"}
    for name, launch in cases(np.random.default_rng(0)).items():
        r = replay_us(launch, a.iters, a.runs)
        emit(dict(case=name, **r))
        summary[name] = r["us_median"]
    emit(summary)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
