#!/usr/bin/env python3
"""Time the batched prefill (config 3: Llama-2-7B, 512 prompt rows) on one GPU,
both GEMM precisions, and print JSON (ms, TFLOP/s on the algorithmic FLOPs).
    python tools/prefill_probe.py [rows] [iters] [exact|exact8|fast]
int8 weights (W8A16), the option "w8_gemm" 0 (gemm.hip) against 1 (gemm_w8.hip) in one process,
interleaved round by round, then the fp16-weight engine of the same shape as the ceiling:
    python tools/prefill_probe.py [rows] [iters] w8 [llama2-7b|llama2-13b] [f16|i8]
Per option and precision: the minimum, the median and the spread (max - min) over the rounds.
int4 weights (W4A16), option "w4_gemm" 1 (gemm_w4.hip), against the same engine's prompt as decode
steps (graph replay) and the int8 engine on gemm_w8.hip, the three alternated round by round in
one process; one JSON line per shape, also appended to [out] (profiles/w4_prefill_probe.json):
    python tools/prefill_probe.py [rows] [iters] w4 [llama2-7b|llama2-13b] [out]"""
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


def w4_main(m, iters, model, path):
    prompt = None
    out = {"model": model, "kv": "f16", "m": m}
    ts, tok = {}, {}
    with Engine(preset(model, max_seq=m + 64, weight_dtype=llmi.I4)) as e4, \
            Engine(preset(model, max_seq=m + 64, weight_dtype=llmi.I8)) as e8:
        prompt = synth_prompt(1, m, e4.cfg.vocab)
        out["flops"] = prefill_flops(e4.cfg, m)
        e4.load_synthetic(0)
        e8.load_synthetic(0)
        e4.set_option("w4_gemm", 1)
        for i in range(iters + 1):  # round 0 warms every shape up (and captures the token graph)
            for key, e, exact in (("exact_w4_gemm", e4, 1), ("fast_w4_gemm", e4, 0), ("decode_steps_int4", e4, None),
                                  ("exact_w8_gemm", e8, 1), ("fast_w8_gemm", e8, 0)):
                if exact is None:
                    e.set_prompt(prompt)
                    e.sync()
                    t0 = time.perf_counter()
                    e.decode(m)
                    e.sync()
                    t = 1e3 * (time.perf_counter() - t0)
                else:
                    t = timed_prefill(e, prompt, m, exact)
                if i:
                    ts.setdefault(key, []).append(t)
                tok[key] = int(e.tokens()[m])
    for key, v in ts.items():
        out[key] = dict(stats(v), token=tok[key])
    for mode in ("exact", "fast"):
        out[f"{mode}_speedup_over_decode_steps"] = out["decode_steps_int4"]["ms"] / out[f"{mode}_w4_gemm"]["ms"]
        out[f"{mode}_w4_over_w8"] = out[f"{mode}_w4_gemm"]["ms"] / out[f"{mode}_w8_gemm"]["ms"]
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if len(sys.argv) > 3 and sys.argv[3] == "w8":
        return w8_main(m, iters, sys.argv[4] if len(sys.argv) > 4 else "llama2-7b",
                       sys.argv[5] if len(sys.argv) > 5 else "f16")
    if len(sys.argv) > 3 and sys.argv[3] == "w4":
        return w4_main(m, iters, sys.argv[4] if len(sys.argv) > 4 else "llama2-7b",
                       sys.argv[5] if len(sys.argv) > 5 else None)
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
