#!/usr/bin/env python3
"""Time the batched prefill (config 3: Llama-2-7B, 512 prompt rows) on one GPU,
both GEMM precisions, and print JSON (ms, TFLOP/s on the algorithmic FLOPs).
    python tools/prefill_probe.py [rows] [iters] [exact|exact8|fast]
int8 weights (W8A16), the option "w8_gemm" 0 (gemm.hip) against 1 (gemm_w8.hip) in one process,
interleaved round by round, then the fp16-weight engine of the same shape as the ceiling:
    python tools/prefill_probe.py [rows] [iters] w8 [llama2-7b|llama2-13b] [f16|i8]
Per option and precision: the minimum, the median and the spread (max - min) over the rounds."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import llmi  # noqa: E402
from llmi.engine import Engine, preset, synth_prompt  # noqa: E402


def prefill_flops(cfg, m):
    lin = cfg.hidden * ((cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim) + cfg.hidden * cfg.hidden \
        + 3 * cfg.hidden * cfg.inter
    attn = 2 * 2 * cfg.heads * cfg.head_dim * (m * (m + 1) // 2)
    return cfg.layers * (2 * m * lin + attn) + 2 * cfg.hidden * cfg.vocab


def timed_prefill(e, prompt, m, exact):
    e.set_prompt(prompt)
    e.sync()
    t0 = time.perf_counter()
    e.prefill(m, exact)
    e.sync()
    return 1e3 * (time.perf_counter() - t0)


def stats(ts):
    return {"ms": min(ts), "median_ms": statistics.median(ts), "spread_ms": max(ts) - min(ts)}


def w8_main(m, iters, model, kv):
    kv_dtype = {"f16": llmi.F16, "i8": llmi.I8}[kv]
    cfg = preset(model, max_seq=m + 64, weight_dtype=llmi.I8, kv_dtype=kv_dtype)
    prompt = synth_prompt(1, m, cfg.vocab)
    out = {"model": model, "kv": kv, "m": m, "flops": prefill_flops(cfg, m)}
    ts, tok = {}, {}
    with Engine(cfg) as e:
        e.load_synthetic(0)
        for i in range(iters + 1):  # round 0 warms every shape up
            for exact in (1, 0):
                for opt in (0, 1):
                    e.set_option("w8_gemm", opt)
                    t = timed_prefill(e, prompt, m, exact)
                    if i:
                        ts.setdefault((exact, opt), []).append(t)
                    tok[exact, opt] = int(e.tokens()[m])
    cfg16 = preset(model, max_seq=m + 64, kv_dtype=kv_dtype)
    with Engine(cfg16) as e:
        e.load_synthetic(0)
        for i in range(iters + 1):
            for exact in (1, 0):
                t = timed_prefill(e, prompt, m, exact)
                if i:
                    ts.setdefault((exact, "f16"), []).append(t)
    for (exact, opt), v in ts.items():
        key = f"{'exact' if exact else 'fast'}_{'w8_gemm' + str(opt) if opt != 'f16' else 'f16_weights'}"
        out[key] = dict(stats(v), token=tok.get((exact, opt)))
    print(json.dumps(out))


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if len(sys.argv) > 3 and sys.argv[3] == "w8":
        return w8_main(m, iters, sys.argv[4] if len(sys.argv) > 4 else "llama2-7b",
                       sys.argv[5] if len(sys.argv) > 5 else "f16")
    modes = {"exact": (1,), "exact8": (2,), "fast": (0,)}.get(sys.argv[3] if len(sys.argv) > 3 else "", (1, 2, 0))
    cfg = preset("llama2-7b", max_seq=m + 64)
    prompt = synth_prompt(1, m, cfg.vocab)
    out = {"m": m, "flops": prefill_flops(cfg, m)}
    with Engine(cfg) as e:
        e.load_synthetic(0)
        for exact in modes:
            ts = []
            for i in range(iters + 1):
                e.set_prompt(prompt)
                e.sync()
                t0 = time.perf_counter()
                e.prefill(m, exact)
                e.sync()
                ts.append(time.perf_counter() - t0)
            ms = 1e3 * min(ts[1:])
            key = {1: "exact", 2: "exact8", 0: "fast"}[exact]
            out[key] = {"ms": ms, "tflops": out["flops"] / (ms * 1e-3) / 1e12, "token": int(e.tokens()[m])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
