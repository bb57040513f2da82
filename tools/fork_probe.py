#!/usr/bin/env python3
"""What a fork of a batch slot costs against the ways to do without it (Llama-2-7B shape,
max_seq 2048, synthetic weights, a Batch of 8; fp16 KV cache, then the int8 one).

    python tools/fork_probe.py [--kv f16,i8] [--keep 2047] [--dst 1,7] [--reps 20] [--layers 32]
                               [--limit 300] [--out profiles/fork_probe.jsonl]

Slot 0 holds a synthetic prompt of keep + 1 ids with its first `keep` rows prefilled. One JSON
line per (kv, what, destinations), times the median of `reps` repeats after a warm-up:

  fork        Batch.fork(0, dst, keep, [last id]): both launches (the row copy and the sequence
              state), a host clock around `reps` forks between two stream synchronises (the
              batch's stream is its own; a fork enqueues in microseconds, the copy takes longer).
  copy_rows   ops.kv_copy_rows alone on caches of the same shape, one device event pair a launch.
  memcpy      the same bytes as one device-to-device memcpy per contiguous segment (layers *
              kv_heads * 2 segments a destination, the scales' as many again), device events
              around the whole sequence: the obvious alternative, its enqueue cost included.
  memcpy_all  one device-to-device memcpy of a whole K and a whole V cache: the chip's own copy
              rate at this size (it moves max_seq rows, not keep).
  prefill     what there is without a fork: Batch.prefill of the `keep` rows in every
              destination slot, a host clock around the calls and a synchronise.
  hbm_read    llmi_hbm_read_bench at 1 GiB, the read ceiling measured in the same run.

bytes = read + written (the fork reads each source byte once and writes it once per destination);
bytes_s = bytes / time. A window that overruns --limit seconds dumps the stacks and ends the
process."""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))

import llmi  # noqa: E402
from llmi.engine import Batch, preset, synth_prompt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv", default="f16,i8")
    ap.add_argument("--keep", type=int, default=2047)
    ap.add_argument("--dst", default="1,7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fork_probe.jsonl"))
    a = ap.parse_args()
    import torch
    from llmi import ops
    from llmi._lib import call

    fans = [int(v) for v in a.dst.split(",")]
    assert all(1 <= n <= 7 for n in fans), "1..7 destinations"
    keep = a.keep
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def limited(fn):
        faulthandler.dump_traceback_later(a.limit, exit=True)
        try:
            return fn()
        finally:
            faulthandler.cancel_dump_traceback_later()

    def events(fn, reps):
        """Median device time in us of fn(), one event pair a call."""
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(out), (max(out) - min(out)) / statistics.median(out)

    us, gbps, rd = ctypes.c_float(), ctypes.c_float(), ctypes.c_size_t()
    limited(lambda: call("llmi_hbm_read_bench", ctypes.c_size_t(1 << 30), 10, ctypes.byref(us), ctypes.byref(gbps),
                         ctypes.byref(rd)))
    emit({"what": "hbm_read", "us": round(us.value, 2), "bytes": rd.value, "bytes_s": round(gbps.value * 1e9, 0)})

    for kv in a.kv.split(","):
        q8 = kv == "i8"
        cfg = preset("llama2-7b", layers=a.layers, max_seq=2048)
        cfg.kv_dtype = llmi.I8 if q8 else llmi.F16
        assert 1 <= keep < cfg.max_seq
        segs = cfg.layers * cfg.kv_heads
        row = cfg.head_dim * (1 if q8 else 2)
        once = 2 * segs * keep * (row + (2 if q8 else 0))  # K and V rows (and scales) of one sequence

        def rec(what, n_dst, t_us, spread, nbytes, **more):
            emit(dict({"kv": kv, "what": what, "n_dst": n_dst, "keep": keep, "us": round(t_us, 2),
                       "spread": round(spread, 4), "bytes": int(nbytes), "bytes_s": round(nbytes / (t_us * 1e-6), 0)},
                      **more))

        # ---- the operator and the memcpys, on caches of the engine's shape
        td = torch.int8 if q8 else torch.float16
        shape = (cfg.layers, cfg.kv_heads, cfg.max_seq, cfg.head_dim)
        src = [torch.zeros(shape, dtype=td, device="cuda") for _ in range(2)]
        dst = [[torch.zeros(shape, dtype=td, device="cuda") for _ in range(max(fans))] for _ in range(2)]
        src_s = dst_s = None
        if q8:
            src_s = [torch.ones(shape[:3], dtype=torch.float16, device="cuda") for _ in range(2)]
            dst_s = [[torch.zeros(shape[:3], dtype=torch.float16, device="cuda") for _ in range(max(fans))]
                     for _ in range(2)]
        for n in fans:
            kw = {}
            if q8:
                kw = dict(src_k_scale=src_s[0], src_v_scale=src_s[1], dst_k_scale=dst_s[0][:n],
                          dst_v_scale=dst_s[1][:n])

            def op():
                ops.kv_copy_rows(src[0], src[1], dst[0][:n], dst[1][:n], keep, **kw)

            def memcpys():
                for w in range(2):
                    for d in range(n):
                        for l in range(cfg.layers):
                            for h in range(cfg.kv_heads):
                                dst[w][d][l, h, :keep].copy_(src[w][l, h, :keep])
                                if q8:
                                    dst_s[w][d][l, h, :keep].copy_(src_s[w][l, h, :keep])

            def memcpy_all():
                for w in range(2):
                    for d in range(n):
                        dst[w][d].copy_(src[w])

            limited(op)
            t, sp = limited(lambda: events(op, a.reps))
            rec("copy_rows", n, t, sp, once * (1 + n))
            limited(memcpys)
            t, sp = limited(lambda: events(memcpys, 3))
            rec("memcpy", n, t, sp, once * (1 + n) + once * (n - 1), calls=2 * n * segs * (2 if q8 else 1))
            limited(memcpy_all)
            t, sp = limited(lambda: events(memcpy_all, 5))
            rec("memcpy_all", n, t, sp, 2 * n * 2 * segs * cfg.max_seq * row)
        del src, dst, src_s, dst_s
        torch.cuda.empty_cache()

        # ---- the slots themselves
        prompt = synth_prompt(keep + 1, keep + 1, cfg.vocab)
        with Batch(cfg, 8) as b:
            limited(lambda: b.load_synthetic(0))
            b.set_prompt(0, prompt)
            limited(lambda: (b.prefill(0, keep), b.sync()))
            for n in fans:
                to = list(range(1, 1 + n))

                def forks():
                    b.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        b.fork(0, to, keep, prompt[-1:])
                    b.sync()
                    return (time.perf_counter() - t0) / a.reps * 1e6

                limited(forks)
                ts = [limited(forks) for _ in range(5)]
                rec("fork", n, statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts), once * (1 + n),
                    forks_per_window=a.reps)

                def prefills():
                    for i in to:
                        b.set_prompt(i, prompt)
                    b.sync()
                    t0 = time.perf_counter()
                    for i in to:
                        b.prefill(i, keep)
                    b.sync()
                    return (time.perf_counter() - t0) * 1e6

                limited(prefills)
                ts = [limited(prefills) for _ in range(3)]
                rec("prefill", n, statistics.median(ts), (max(ts) - min(ts)) / statistics.median(ts), 0)
                # the forked slots go on as the prefilled ones: one step of all, tokens compared
                for i in range(1, 8):
                    if i not in to:
                        b.reset(i)
                b.edit(0, keep, prompt[-1:])
                b.decode(1)
                want = b.tokens(0, keep + 2)
                b.edit(0, keep, prompt[-1:])
                b.fork(0, to, keep, prompt[-1:])
                b.decode(1)
                for i in [0] + to:
                    assert b.tokens(i, keep + 2).tolist() == want.tolist(), f"slot {i} differs after the fork"
                b.edit(0, keep, prompt[-1:])

    def pick(kv, what, n):
        return next(r for r in lines if r.get("kv") == kv and r["what"] == what and r["n_dst"] == n)

    summary = {"summary": True, "ratios": {}}
    for kv in a.kv.split(","):
        for n in fans:
            f, p, m = pick(kv, "fork", n), pick(kv, "prefill", n), pick(kv, "memcpy", n)
            summary["ratios"][f"{kv}-{n}"] = {"prefill_over_fork": round(p["us"] / f["us"], 1),
                                              "memcpy_over_fork": round(m["us"] / f["us"], 2),
                                              "fork_bytes_s_over_hbm_read":
                                                  round(f["bytes_s"] / lines[0]["bytes_s"], 3)}
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
