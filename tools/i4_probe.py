#!/usr/bin/env python3
"""W4A16 against W8A16 and fp16, same process, alternating (Llama-2-7B and 13B shapes, synthetic
weights, fp16 KV, 8 prompt ids, graph-replayed forwards at positions 0 .. ctx-1, ctx 256).

    python tools/i4_probe.py [--passes 3] [--ctx 256] [--models llama2-7b,llama2-13b] [--out profiles/i4_probe.jsonl]

For each model the three engines (weight_dtype fp16, int8, int4) are created once and every pass
times them in turn, so drift of the box hits all of them alike; the int8 engine of the same run is
the yardstick. Each timed window is ctx forwards ending in a stream synchronise, after an untimed
run of the same window that captured every graph it replays. One JSON line per (model, pass,
dtype):

  us_per_token   host clock over the window / ctx
  tok_s          ctx / window
  stream_bytes   llmi_engine_bytes: the weight bytes one forward reads
  kv_bytes       kv_bytes_per_pos * mean cached positions of the window
  tb_s           (stream_bytes + kv_bytes) / step time, in TB/s

then per (model, dtype) the qkv, gate_up and down kernels alone (llmi_engine_time_kernel: layers
cycled so every launch streams from HBM), and a summary line per model: medians, the spread
between passes of each dtype, and int4's speed-up over int8 per pass.
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
from llmi.engine import Engine, preset, synth_prompt  # noqa: E402

DTYPES = (("f16", llmi.F16), ("i8", llmi.I8), ("i4", llmi.I4))


def window(e, prompt, ctx):
    def run():
        e.set_prompt(prompt)
        e.sync()
        t0 = time.perf_counter()
        e.decode(ctx)
        e.sync()
        return time.perf_counter() - t0
    run()  # untimed: captures every graph the window replays, warms the code objects
    return run()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--models", default="llama2-7b,llama2-13b")
    ap.add_argument("--layers", type=int, default=0, help="0: the preset's")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "i4_probe.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for model in a.models.split(","):
        over = {"max_seq": a.ctx, "kv_dtype": llmi.F16}
        if a.layers:
            over["layers"] = a.layers
        engines = {}
        try:
            for name, dt in DTYPES:
                engines[name] = Engine(preset(model, weight_dtype=dt, **over))
                engines[name].load_synthetic(0)
            prompt = synth_prompt(0, 8, engines["f16"].cfg.vocab)
            mean_pos = (a.ctx + 1) / 2.0  # positions 1 .. ctx are cached over the window
            for p in range(a.passes):
                for name, _ in DTYPES:
                    e = engines[name]
                    dt = window(e, prompt, a.ctx)
                    w, kv_pos = e.bytes_per_token()
                    kv = kv_pos * mean_pos
                    emit({"model": model, "pass": p, "dtype": name, "us_per_token": round(dt / a.ctx * 1e6, 2),
                          "tok_s": round(a.ctx / dt, 2), "stream_bytes": w, "kv_bytes": int(kv),
                          "tb_s": round((w + kv) / (dt / a.ctx) / 1e12, 3)})
            for name, _ in DTYPES:
                rec = {"model": model, "dtype": name, "kernels": True}
                for k in ("qkv", "o", "gate_up", "down"):
                    us, b = engines[name].time_kernel(k, 64)
                    rec[k] = {"us": round(us, 2), "bytes": b, "tb_s": round(b / us / 1e6, 3)}
                emit(rec)
        finally:
            for e in engines.values():
                e.close()
        summary = {"model": model, "summary": True}
        per = {name: [r["tok_s"] for r in lines if r.get("model") == model and r.get("dtype") == name and "pass" in r]
               for name, _ in DTYPES}
        for name, t in per.items():
            us = [r["us_per_token"] for r in lines if r.get("model") == model and r.get("dtype") == name and "pass" in r]
            summary[name] = {"tok_s_median": statistics.median(t), "us_per_token_median": statistics.median(us),
                             "spread": round((max(t) - min(t)) / statistics.median(t), 4)}
        ratios = [x / y for x, y in zip(per["i4"], per["i8"])]
        summary["i4_over_i8"] = {"min": round(min(ratios), 4), "median": round(statistics.median(ratios), 4)}
        summary["i4_over_f16_median"] = round(statistics.median(x / y for x, y in zip(per["i4"], per["f16"])), 4)
        emit(summary)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
