#!/usr/bin/env python3
"""What the samplers cost per token: same-process A/B of the engine's three token choosers on
the bench workload (Llama-2-7B synthetic, fp16 weights and KV, 8 prompt ids, graph-replayed
forwards at positions 0..max_seq-1, so the mean context is max_seq / 2), alternating the modes
pass by pass so box drift hits all of them alike, and the sampling kernels timed alone.

    python tools/sampler_cost.py [--passes 5 | --passes 0: the kernels alone] [--max-seq 2048] [--out profiles/sampler_cost.json]

modes: greedy (fused argmax), topk16 (set_sampling(16): the reference's sampler),
nucleus (set_sampling_params(0, .9, .6, 1.1)). Prints one JSON line per (pass, mode) and a
summary (medians) at the end; --out writes the summary.
"""
import argparse
import contextlib
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

MODES = ("greedy", "topk16", "nucleus")


def set_mode(e, mode):
    if mode == "greedy":
        e.set_sampling(0)
    elif mode == "topk16":
        e.set_sampling(16, 1)
    else:
        e.set_sampling_params(top_k=0, top_p=0.9, temperature=0.6, repetition_penalty=1.1, seed=1)


def kernels_alone(vocab, n_hist, iters):
    rng = np.random.default_rng(0)
    z = torch.from_numpy((rng.standard_normal((1, vocab)) * 3).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.integers(0, vocab, (1, n_hist)).astype(np.int32)).cuda()
    hl = torch.full((1,), n_hist, device="cuda", dtype=torch.int32)
    oid = torch.zeros(1, device="cuda", dtype=torch.int32)
    okept = torch.zeros(1, device="cuda", dtype=torch.int32)
    seqlen = torch.zeros(1, device="cuda", dtype=torch.int32)
    fin = torch.zeros(1, device="cuda", dtype=torch.uint8)

    def nucleus(k, p, t, r):
        def f():
            ops.sample_nucleus(z, 5, top_k=k, top_p=p, temperature=t, repetition_penalty=r, history=h,
                               history_len=hl, out_id=oid, out_kept=okept)
        return f

    def topk16():
        ids, vals = ops.launchTopKforBeamSearch(z, 16)
        ops.launchSampling(ids, vals, seqlen, fin, oid, 5, -1, vocab)

    out = {}
    for name, f in (("nucleus_k0_p0.9_t0.6_r1.1", nucleus(0, 0.9, 0.6, 1.1)),
                    ("nucleus_k50_p0.95_t0.8_r1.2", nucleus(50, 0.95, 0.8, 1.2)),
                    ("nucleus_k0_p1_t1_r1", nucleus(0, 1.0, 1.0, 1.0)),
                    ("topk16_plus_sampling", topk16)):
        # captured into a graph: the launch cost the engine's token graph pays, no host gaps.
        # (the operator's history check reads ids back only outside a capture)
        f()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                for _ in range(iters):
                    f()
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
        out[name] = {"us_median": round(statistics.median(runs), 2), "us_runs": [round(r, 2) for r in runs]}
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
    with Engine(cfg) if a.passes else contextlib.nullcontext() as e:
        if a.passes:
            e.load_synthetic(0)
        for p in range(a.passes):
            for m in MODES:
                set_mode(e, m)  # drops the captured graphs
                e.set_prompt(prompt)
                e.decode(a.max_seq)  # every split count's graph captured outside the timed region
                e.set_prompt(prompt)
                e.sync()
                t0 = time.perf_counter()
                e.decode(a.max_seq)
                e.sync()
                dt = time.perf_counter() - t0
                us[m].append(dt / a.max_seq * 1e6)
                print(json.dumps({"pass": p, "mode": m, "us_per_token": round(us[m][-1], 2)}), flush=True)
    summary = {"workload": f"{a.preset} synthetic fp16, fp16 KV, layers {a.layers}, positions 0..{a.max_seq - 1} "
                           f"(mean context {a.max_seq // 2}), graph replay, {a.passes} alternating passes",
               "token_us_median": {m: round(statistics.median(us[m]), 2) for m in MODES if us[m]},
               "token_us_runs": {m: [round(x, 2) for x in us[m]] for m in MODES}}
    if a.passes == 0:  # the kernels alone
        print(json.dumps(kernels_alone(cfg.vocab, a.max_seq // 2, 200)), flush=True)
        return
    med = summary["token_us_median"]
    summary["nucleus_over_topk16_pct"] = round((med["nucleus"] / med["topk16"] - 1) * 100, 3)
    summary["nucleus_over_greedy_pct"] = round((med["nucleus"] / med["greedy"] - 1) * 100, 3)
    summary["topk16_over_greedy_pct"] = round((med["topk16"] / med["greedy"] - 1) * 100, 3)
    summary["kernels_alone_us"] = kernels_alone(cfg.vocab, a.max_seq // 2, 200)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
