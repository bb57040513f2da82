#!/usr/bin/env python3
"""The int8 KV cache (kv_dtype LLMI_I8, "KV8") against the fp16 cache, same process, alternating
(Llama-2-7B shape, fp16 synthetic weights).

    python tools/kv8_probe.py [--kv f16,i8] [--parts attn,loop,batch,prefill,depth] [--passes 2]
                              [--tag new] [--out profiles/kv8_probe.json]

The engines of one part are created once and every pass times them in turn, so drift of the box
hits them alike. `--kv f16 --tag parent` in a checkout of the parent commit gives the yardstick the
same script measures there (the parts that need no int8 cache). One JSON object per measurement,
appended to --out as a list:

  attn     the attention launch alone (Engine.time_kernel("attn"): layers cycled, so every launch
           streams its K/V rows from HBM) at ctx 512 and 2048 (32 layers) and 16384 (8 layers,
           max_seq 16384): us, algorithmic bytes (rows and, for int8, their scales), TB/s
  loop     tokens/s of graph-replayed decode from position 0 to ctx 2048 (host clock over the
           window, after an untimed run of the same window that captured every graph): the fp16
           engine with the fused q/k/v + attention launch and with qkv_attn 0, the int8 engine
           (which always takes the two launches)
  batch    Batch of 8 slots, aggregate tokens/s over positions 1792 .. 2047
  prefill  one 512-row prefill in ms: int8 KV against fp32 KV (both run the scalar attention)
  depth    32 layers: the fp32-KV engine's 8 prompt ids + 16 greedy tokens are fed to every engine
           (one sequence for all); final logits rel-L2 of the int8-KV and the fp16-KV engine
           against the fp32-KV engine, and how many tokens of each engine's own greedy run agree
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
from llmi.engine import Batch, Engine, preset, synth_prompt  # noqa: E402

KV = {"f16": llmi.F16, "f32": llmi.F32, "i8": llmi.I8}
OUT = []


def emit(**kw):
    OUT.append(kw)
    print(json.dumps(kw), flush=True)


def engine(kv, **over):
    e = Engine(preset("llama2-7b", kv_dtype=KV[kv], **over))
    e.load_synthetic(0)
    return e


def attn_at(engs, ctx, passes, tag, layers):
    """time_kernel("attn") with the device at position ctx - 1, the engines in turn."""
    for p in range(passes):
        for kv, e in engs.items():
            us, b = e.time_kernel("attn", 64)
            emit(part="attn", tag=tag, kv=kv, layers=layers, ctx=ctx, pass_=p, us=round(us, 3), bytes=b,
                 tb_s=round(b / us / 1e6, 3))


def part_attn(kvs, passes, tag):
    for layers, max_seq, stops in ((32, 2048, (512, 2048)), (8, 16384, (16384,))):
        engs = {kv: engine(kv, layers=layers, max_seq=max_seq) for kv in kvs}
        prompt = synth_prompt(1, max_seq, 32000)
        for e in engs.values():
            e.set_prompt(prompt)
        at = 0
        for ctx in stops:
            for e in engs.values():
                e.decode(ctx - at)
                e.sync()
            at = ctx
            attn_at(engs, ctx, passes, tag, layers)
        for e in engs.values():
            e.close()


def window(e, prompt, n):
    e.set_prompt(prompt)
    e.sync()
    t0 = time.perf_counter()
    e.decode(n)
    e.sync()
    return time.perf_counter() - t0


def part_loop(kvs, passes, tag, ctx=2048):
    prompt = synth_prompt(2, 8, 32000)
    runs = []
    for kv in kvs:
        e = engine(kv, max_seq=ctx)
        runs.append((kv, "default", e))
        if kv == "f16":
            e2 = engine(kv, max_seq=ctx)
            e2.set_option("qkv_attn", 0)
            runs.append((kv, "qkv_attn 0", e2))
    for _, _, e in runs:
        window(e, prompt, ctx)  # untimed: captures every graph the window replays
    for p in range(passes):
        for kv, form, e in runs:
            dt = window(e, prompt, ctx)
            emit(part="loop", tag=tag, kv=kv, form=form, ctx=ctx, pass_=p, tok_s=round(ctx / dt, 2),
                 us_per_token=round(dt / ctx * 1e6, 2), kv_bytes_per_pos=e.bytes_per_token()[1])
    for _, _, e in runs:
        e.close()


def part_batch(kvs, passes, tag, n_seq=8, ctx=2048, tail=256):
    prompts = [synth_prompt(10 + i, 8, 32000) for i in range(n_seq)]
    bs = {}
    for kv in kvs:
        b = Batch(preset("llama2-7b", kv_dtype=KV[kv], max_seq=ctx), n_seq)
        b.load_synthetic(0)
        bs[kv] = b

    def run(b):
        for i, p in enumerate(prompts):
            b.reset(i)
            b.set_prompt(i, p)
        b.decode(ctx - tail)
        b.sync()
        t0 = time.perf_counter()
        b.decode(tail)
        b.sync()
        return time.perf_counter() - t0
    for b in bs.values():
        run(b)  # untimed: the graphs
    for p in range(passes):
        for kv, b in bs.items():
            dt = run(b)
            emit(part="batch", tag=tag, kv=kv, n_seq=n_seq, ctx=ctx, pass_=p, agg_tok_s=round(n_seq * tail / dt, 1),
                 ms_per_step=round(dt / tail * 1e3, 3))
    for b in bs.values():
        b.close()


def part_prefill(kvs, passes, tag, rows=512):
    kvs = [kv for kv in ("f32", "i8", "f16") if kv in set(kvs) | {"f32"}]
    engs = {kv: engine(kv, max_seq=rows + 64) for kv in kvs}
    prompt = synth_prompt(3, rows + 1, 32000)

    def run(e):
        e.set_prompt(prompt)
        e.sync()
        t0 = time.perf_counter()
        e.prefill(rows)
        e.sync()
        return time.perf_counter() - t0
    for e in engs.values():
        run(e)
    for p in range(passes):
        for kv, e in engs.items():
            emit(part="prefill", tag=tag, kv=kv, rows=rows, pass_=p, ms=round(run(e) * 1e3, 3))
    for e in engs.values():
        e.close()


def part_depth(kvs, tag, n_prompt=8, n_new=16):
    prompt = synth_prompt(0, n_prompt, 32000)
    res = {}
    for kv in ["f32"] + [k for k in kvs if k != "f32"]:
        with engine(kv, max_seq=64) as e:
            free = e.generate(prompt, n_new)
            if kv == "f32":
                text = np.concatenate([prompt, free]).astype(np.int32)  # the 24 ids every engine is fed
            # teacher-forced: the fp32-KV engine's tokens as the prompt, so the logits compared are
            # those of ONE sequence (synthetic weights give near-flat logits: a free run drifts apart)
            e.set_prompt(text)
            e.decode(len(text))
            res[kv] = (free, e.logits().astype(np.float64))
    t32, l32 = res["f32"]
    for kv, (t, l) in res.items():
        if kv != "f32":
            same = int(np.argmax(t != t32)) if (t != t32).any() else n_new
            emit(part="depth", tag=tag, kv=kv, layers=32, tokens=len(text),
                 logits_rel_l2_vs_f32_kv=float(np.linalg.norm(l - l32) / np.linalg.norm(l32)),
                 argmax_equal=bool(np.argmax(l) == np.argmax(l32)), free_run_tokens_equal=same, free_run_tokens=n_new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv", default="f16,i8")
    ap.add_argument("--parts", default="attn,loop,batch,prefill,depth")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--tag", default="new")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kv8_probe.json"))
    a = ap.parse_args()
    kvs, parts = a.kv.split(","), a.parts.split(",")
    llmi.lib()
    if "attn" in parts:
        part_attn(kvs, a.passes, a.tag)
    if "loop" in parts:
        part_loop(kvs, a.passes, a.tag)
    if "batch" in parts:
        part_batch(kvs, a.passes, a.tag)
    if "prefill" in parts:
        part_prefill(kvs, a.passes, a.tag)
    if "depth" in parts:
        part_depth(kvs, a.tag)
    # medians per (part, kv, form / ctx)
    groups = {}
    for r in OUT:
        key = (r["part"], r["kv"], r.get("form"), r.get("ctx"), r.get("layers"))
        for f in ("us", "tok_s", "agg_tok_s", "ms"):
            if f in r:
                groups.setdefault(key + (f,), []).append(r[f])
    for key, v in groups.items():
        emit(part="summary", tag=a.tag, key=[k for k in key if k is not None], median=statistics.median(v),
             spread=max(v) - min(v), n=len(v))
    prev = []
    if os.path.exists(a.out):
        with open(a.out) as fh:
            prev = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(prev + OUT, fh, indent=0)


if __name__ == "__main__":
    main()
