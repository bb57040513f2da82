#!/usr/bin/env python3
"""Batch option "rows_mfma" against the default batch path and the plain engine, same process,
alternating (Llama-2-7B synthetic weights, fp16 then int8, fp16 KV, 8 prompt ids, graph-replayed
forwards at positions 0 .. ctx-1, ctx 256: the window and protocol of tools/batch_probe.py).

    python tools/rows_mfma_probe.py [--passes 3] [--ctx 256] [--layers 32] [--n-seq 1,2,4,8]
                                    [--out profiles/rows_mfma_probe.jsonl]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python tools/rows_mfma_probe.py --trace
    python tools/rows_mfma_probe.py --trace-csv DIR/.../kt_kernel_trace.csv     (appends to --out)

Every pass times the plain Engine, then at each n_seq the Batch with the option 0 and with the
option 1 (every slot active, its own prompt), so drift of the box hits all of them alike. Each
timed window is ctx forwards ending in a stream synchronise, after an untimed run of the same
window that captured every graph it replays. One JSON line per (weights, pass, variant, n_seq)
with the fields of batch_probe.py (us_per_step, tok_s, weight_bytes, kv_bytes, bytes_s,
model_bytes_per_token), then one summary line per weight type: medians, the spread of each point
((max - min) / median over the passes), bytes_s of the median, the ratio of option 1 to option 0
pass by pass, and both against the Engine of the same pass.

--trace runs a few eager steps (a kernel trace does not see graph replays) of 8 slots with the
option 0, then 1, for both weight types and times nothing; --trace-csv turns that run's kernel
trace into one line per (kernel, grid) whose name holds "rows" (the multi-row GEMVs of both
paths: calls and median / min / max microseconds) and appends them to --out.
"""
import argparse
import collections
import csv
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))


def window(run, reset, ctx):
    reset()
    run(ctx)          # untimed: captures every graph the window replays, warms the code objects
    reset()
    t0 = time.perf_counter()
    run(ctx)          # ends in a stream synchronise
    return time.perf_counter() - t0


def trace_records(path):
    acc = collections.defaultdict(list)
    for row in csv.DictReader(open(path)):
        m = re.search(r"(\w+_kernel)(<[^()]*>)?", row["Kernel_Name"])
        name = (m.group(1) + (m.group(2) or "")) if m else row["Kernel_Name"][:80]
        if "rows" in name:
            acc[(name, row.get("Grid_Size_X", row.get("Grid_Size", "?")))].append(
                int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for (name, grid), v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
        v.sort()
        yield {"trace": True, "kernel": name, "grid": grid, "calls": len(v), "median_us": round(v[len(v) // 2] / 1e3, 2),
               "min_us": round(v[0] / 1e3, 2), "max_us": round(v[-1] / 1e3, 2)}


def probe(a, int8, emit):
    import llmi
    from llmi.engine import Batch, Engine, preset, synth_prompt
    ns = [8] if a.trace else [int(v) for v in a.n_seq.split(",")]
    wname = "i8" if int8 else "f16"
    cfg = preset("llama2-7b", layers=a.layers, max_seq=a.ctx)
    cfg.kv_dtype = llmi.F16
    if int8:
        cfg.weight_dtype = llmi.I8
    prompts = [synth_prompt(i, 8, cfg.vocab) for i in range(max(ns))]
    mean_pos = (a.ctx + 1) / 2.0  # positions 1 .. ctx are cached over the window
    lines = []
    with Engine(cfg) as e, Batch(cfg, max(ns)) as b:
        e.load_synthetic(0)
        b.load_synthetic(0)
        w_engine, kv_pos = e.bytes_per_token()
        c = cfg
        w_o = c.layers * c.hidden * c.hidden * (1 if int8 else 2) + (c.layers * c.hidden * 2 if int8 else 0)

        def run_e(n):
            e.decode(n)
            e.sync()

        def run_b(n):
            b.decode(n, use_graph=not a.trace)
            b.sync()

        def reset_b(n_seq):
            for i in range(max(ns)):
                b.reset(i)
            for i in range(n_seq):
                b.set_prompt(i, prompts[i])

        if a.trace:
            for on in (0, 1):
                b.set_option("rows_mfma", on)
                reset_b(8)
                run_b(8)
            return

        def rec(p, variant, n, dt, w):
            kv = n * kv_pos * mean_pos
            r = {"weights": wname, "pass": p, "variant": variant, "n_seq": n, "us_per_step": round(dt / a.ctx * 1e6, 2),
                 "tok_s": round(n * a.ctx / dt, 2), "weight_bytes": w, "kv_bytes": int(kv),
                 "bytes_s": round((w + kv) / (dt / a.ctx), 0),
                 "model_bytes_per_token": int((w_engine - w_o) / n + w_o + kv_pos * mean_pos)}
            lines.append(r)
            emit(r)

        for p in range(a.passes):
            rec(p, "engine", 1, window(run_e, lambda: e.set_prompt(prompts[0]), a.ctx), w_engine)
            for n in ns:
                for on in (0, 1):
                    b.set_option("rows_mfma", on)
                    dt = window(run_b, lambda n=n: reset_b(n), a.ctx)
                    rec(p, f"batch_opt{on}", n, dt, b.bytes_per_step()[0])
        b.set_option("rows_mfma", 0)

    def col(variant, n, key):
        return [r[key] for r in lines if r["variant"] == variant and r["n_seq"] == n]

    def point(variant, n):
        us, bs = col(variant, n, "us_per_step"), col(variant, n, "bytes_s")
        return {"us_per_step_median": statistics.median(us), "tok_s_median": statistics.median(col(variant, n, "tok_s")),
                "bytes_s_median": statistics.median(bs), "spread": round((max(us) - min(us)) / statistics.median(us), 4)}

    eng = col("engine", 1, "tok_s")
    summary = {"summary": True, "weights": wname, "engine": point("engine", 1), "n_seq": {}}
    for n in ns:
        t0, t1 = col("batch_opt0", n, "tok_s"), col("batch_opt1", n, "tok_s")
        summary["n_seq"][str(n)] = {
            "opt0": point("batch_opt0", n), "opt1": point("batch_opt1", n),
            "opt1_over_opt0": [round(y / x, 4) for x, y in zip(t0, t1)],
            "opt0_over_engine_median": round(statistics.median(x / z for x, z in zip(t0, eng)), 4),
            "opt1_over_engine_median": round(statistics.median(y / z for y, z in zip(t1, eng)), 4)}
    emit(summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=256)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--n-seq", default="1,2,4,8")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-csv")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rows_mfma_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.trace_csv else "w") if not a.trace else open(os.devnull, "w") as f:
        def emit(r):
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")
            f.flush()
        if a.trace_csv:
            for r in trace_records(a.trace_csv):
                emit(r)
            return
        for int8 in (False, True):
            probe(a, int8, emit)


if __name__ == "__main__":
    main()
