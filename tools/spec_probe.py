#!/usr/bin/env python3
"""The verify step of speculative decoding against the plain token step and against a Batch of
the same row count, same process, alternating (Llama-2-7B shape, fp16 synthetic weights, fp16
KV, graph replay).

    python tools/spec_probe.py [--passes 3] [--rows 1,2,4,8] [--pos 256,1900] [--window 128]
                               [--layers 32] [--limit 120] [--out profiles/spec_probe.jsonl]

Around each start position P the sequence is a synthetic prompt of P ids run through the
prefill, then `window` positions of greedy decode. The plain Engine decodes them first; its
tokens are the true continuation, so a verify step of m rows (the pending token + m - 1 true
drafts) accepts everything and advances m positions. Before anything is reported the tokens of
every verify run are compared with the plain engine's (a mismatch aborts the probe). A Batch of
m slots, each holding the same prompt at the same position, is the way to run m rows without
this change: per-slot attention and o_proj, W_o and the KV streamed m times.

Every pass times, per position: the Engine window, then per row count the verify window and the
Batch window (window / m steps each), each after an untimed run of the same window that
captured its graphs. A timed window is a host clock around work that ends in a stream
synchronise (every verify step ends in one: its read-back is part of the step). Each window
runs under a time limit of its own (--limit seconds: the process exits when one overruns it).
One JSON line per (pass, position, variant, rows):

  us_per_step        window time / steps
  x_engine           us_per_step over the Engine step's of the same pass and position: the
                     break-even number of tokens a verify step must yield
  x_batch            verify us_per_step over the Batch step's of the same rows (verify lines)
  model_bytes        the byte model of one step: (W - W_o) + W_o + KV(p) for a verify step,
                     (W - W_o) + m W_o + m KV(p) for the Batch, p = the window's mean position
  bytes_s            model_bytes / step time: achieved algorithmic bytes per second

and a last line with the medians and spreads. End-to-end tokens/s with lookup drafting depends
on the text's acceptance rate and is not measured here.
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import llmi  # noqa: E402
from llmi.engine import Batch, Engine, preset, synth_prompt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rows", default="1,2,4,8")
    ap.add_argument("--pos", default="256,1900")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spec_probe.jsonl"))
    a = ap.parse_args()
    rows = [int(v) for v in a.rows.split(",")]
    starts = [int(v) for v in a.pos.split(",")]
    W = a.window
    assert all(1 <= m <= 8 and W % m == 0 for m in rows), "rows must be 1..8 and divide the window"
    cfg = preset("llama2-7b", layers=a.layers, max_seq=max(starts) + W + 8)
    cfg.kv_dtype = llmi.F16
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def limited(fn):
        """fn() under the window's time limit: an overrun dumps the stacks and ends the process."""
        faulthandler.dump_traceback_later(a.limit, exit=True)
        try:
            return fn()
        finally:
            faulthandler.cancel_dump_traceback_later()

    with Engine(cfg) as e, Batch(cfg, max(rows)) as b:
        e.load_synthetic(0)
        b.load_synthetic(0)
        e.set_speculation(max(max(rows) - 1, 0))
        w_all, kv_pos = e.bytes_per_token()
        w_o = cfg.layers * cfg.hidden * cfg.hidden * 2

        def engine_window(prompt):
            e.set_prompt(prompt)
            e.prefill(len(prompt))
            e.sync()
            t0 = time.perf_counter()
            e.decode(W)
            e.sync()
            return time.perf_counter() - t0

        def verify_window(prompt, true, m):
            P = len(prompt)
            e.set_prompt(prompt)
            e.prefill(P)
            e.sync()
            t0 = time.perf_counter()
            for p in range(P, P + W, m):
                acc = e.verify(true[p + 1:p + m])
                assert acc == m - 1, f"verify at {p}: {acc} of {m - 1} true drafts accepted"
            dt = time.perf_counter() - t0
            got = e.tokens(P + W + 1)
            assert got.tolist() == true[:P + W + 1].tolist(), "verify tokens differ from the plain engine's"
            return dt

        def batch_window(prompt, m):
            for i in range(max(rows)):
                b.reset(i)
            for i in range(m):
                b.set_prompt(i, prompt)
                b.prefill(i)
            b.sync()
            t0 = time.perf_counter()
            b.decode(W // m)
            b.sync()
            return time.perf_counter() - t0

        for P in starts:
            prompt = synth_prompt(P, P, cfg.vocab)
            limited(lambda: engine_window(prompt))  # untimed: graphs, code objects
            true = e.tokens(P + W + 1).copy()
            for m in rows:                          # untimed, and the token check of every row count
                limited(lambda: verify_window(prompt, true, m))
                limited(lambda: batch_window(prompt, m))
            mean_pos = P + (W + 1) / 2.0
            kv = kv_pos * mean_pos
            for ps in range(a.passes):
                dt_e = limited(lambda: engine_window(prompt))
                us_e = dt_e / W * 1e6
                emit({"pass": ps, "pos": P, "variant": "engine", "rows": 1, "us_per_step": round(us_e, 2),
                      "x_engine": 1.0, "model_bytes": int(w_all + kv), "bytes_s": round((w_all + kv) / (dt_e / W), 0),
                      "tokens_equal": True})
                for m in rows:
                    steps = W // m
                    dt_v = limited(lambda: verify_window(prompt, true, m))
                    dt_b = limited(lambda: batch_window(prompt, m))
                    us_v, us_b = dt_v / steps * 1e6, dt_b / steps * 1e6
                    mb_v = w_all + kv
                    mb_b = (w_all - w_o) + m * w_o + m * kv
                    emit({"pass": ps, "pos": P, "variant": "verify", "rows": m, "us_per_step": round(us_v, 2),
                          "x_engine": round(us_v / us_e, 4), "x_batch": round(us_v / us_b, 4),
                          "model_bytes": int(mb_v), "bytes_s": round(mb_v / (dt_v / steps), 0), "tokens_equal": True})
                    emit({"pass": ps, "pos": P, "variant": "batch", "rows": m, "us_per_step": round(us_b, 2),
                          "x_engine": round(us_b / us_e, 4), "model_bytes": int(mb_b),
                          "bytes_s": round(mb_b / (dt_b / steps), 0), "tokens_equal": True})

    def med(xs):
        return round(statistics.median(xs), 4)

    def spread(xs):
        return round((max(xs) - min(xs)) / statistics.median(xs), 4)

    summary = {"summary": True, "window": W, "passes": a.passes, "by_pos": {}}
    for P in starts:
        at = [r for r in lines if r["pos"] == P]
        eng = [r["us_per_step"] for r in at if r["variant"] == "engine"]
        s = {"engine_us": med(eng), "engine_spread": spread(eng), "rows": {}}
        for m in rows:
            v = [r for r in at if r["variant"] == "verify" and r["rows"] == m]
            bt = [r for r in at if r["variant"] == "batch" and r["rows"] == m]
            s["rows"][str(m)] = {
                "verify_us": med([r["us_per_step"] for r in v]), "verify_spread": spread([r["us_per_step"] for r in v]),
                "x_engine": med([r["x_engine"] for r in v]), "x_batch": med([r["x_batch"] for r in v]),
                "verify_bytes_s": med([r["bytes_s"] for r in v]),
                "batch_us": med([r["us_per_step"] for r in bt]), "batch_x_engine": med([r["x_engine"] for r in bt])}
        summary["by_pos"][str(P)] = s
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
