#!/usr/bin/env python3
"""Engine option "gqa_attn" (csrc/attn_gqa.hip) against the default decode attention, same process,
alternating (Llama-2-7B shape with kv_heads 8 -- group 4 -- and 4 -- group 8; fp16 synthetic
weights; fp16 and int8 KV cache; ctx 2048, 8192, 16384).

    python tools/gqa_attn_probe.py [--layers 8] [--passes 5] [--ctx 2048,8192,16384]
                                   [--out profiles/gqa_attn_probe.jsonl]

One engine per (kv_heads, cache) decodes a forced prompt up to each ctx with the option off (the
parent's path) and measures there, option 0 and 1 in turn in every pass:
  attn  the attention launch alone: Engine.time_kernel("attn", 64), launches cycling the layers.
        us, the kv_heads-based byte model of attn.hip (K and V rows read once, scales included) and
        bytes / us. `cycled_bytes` is what the cycled layers' rows add up to: below the 256 MiB
        Infinity Cache the launches are served from it, not from HBM -- read the rate accordingly.
  step  graph-replayed token steps: each 64-position block before ctx gives one window per
        option (8 untimed steps after the switch, which capture the block's graph, then 24 timed
        steps ending in a synchronise), the order swapping from block to block.
Then one summary line per (kv_heads, cache, ctx, part): medians, option 0's spread
((max - min) / median) and the ratio of the medians (option 1 time over option 0 time)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

WARM, TIMED = 8, 24  # steps of a window; two windows fill a 64-position block


def probe(a, kvh, kv, emit):
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    stops = sorted(int(v) for v in a.ctx.split(","))
    cfg = preset("llama2-7b", kv_heads=kvh, layers=a.layers, max_seq=stops[-1], kv_dtype=getattr(llmi, kv))
    lines = []

    def rec(**r):
        r = dict(kv_heads=kvh, group=cfg.heads // kvh, cache=kv, layers=a.layers, **r)
        lines.append(r)
        emit(r)

    with Engine(cfg) as e:
        e.load_synthetic(0)
        e.set_prompt(synth_prompt(1, stops[-1], cfg.vocab))
        at = 0
        for ctx in stops:
            first = ctx - 64 * a.passes  # the step windows' first block
            e.set_option("gqa_attn", 0)
            e.decode(first - at)
            at = first
            for p in range(a.passes):  # one 64-position block per pass
                for opt in ((0, 1), (1, 0))[p % 2]:
                    e.set_option("gqa_attn", opt)
                    e.decode(WARM)
                    e.sync()
                    t0 = time.perf_counter()
                    e.decode(TIMED)
                    e.sync()
                    rec(part="step", ctx=ctx, pass_=p, opt=opt, pos=at + WARM,
                        us=round((time.perf_counter() - t0) / TIMED * 1e6, 2))
                    at += WARM + TIMED
            for p in range(a.passes):
                for opt in (0, 1):
                    e.set_option("gqa_attn", opt)
                    us, b = e.time_kernel("attn", 64)
                    rec(part="attn", ctx=ctx, pass_=p, opt=opt, us=round(us, 3), bytes=b, tb_s=round(b / us / 1e6, 3),
                        cycled_bytes=b * a.layers)
    for ctx in stops:
        for part in ("attn", "step"):
            us = [[r["us"] for r in lines if r["part"] == part and r["ctx"] == ctx and r["opt"] == o] for o in (0, 1)]
            m0, m1 = statistics.median(us[0]), statistics.median(us[1])
            emit(dict(summary=True, kv_heads=kvh, cache=kv, layers=a.layers, part=part, ctx=ctx, us_opt0=m0, us_opt1=m1,
                      spread_opt0=round((max(us[0]) - min(us[0])) / m0, 4), opt1_over_opt0=round(m1 / m0, 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--ctx", default="2048,8192,16384")
    ap.add_argument("--kv-heads", default="8,4")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gqa_attn_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(r):
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
            f.flush()
        for kvh in (int(v) for v in a.kv_heads.split(",")):
            for kv in ("F16", "I8"):
                probe(a, kvh, kv, emit)


if __name__ == "__main__":
    main()
