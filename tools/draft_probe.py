#!/usr/bin/env python3
"""What one cycle of draft-model speculative decoding costs (llmi_engine_generate_draft), same
process, against the plain token step.

    python tools/draft_probe.py [--passes 3] [--k 1,3,5,7] [--pos 256,1792] [--cycles 24]
                                [--limit 120] [--out profiles/draft_probe.jsonl]

Target: the llama2-7b preset, fp16 synthetic weights (seed 0). Draft: the same preset overridden
to hidden 2048, 16 heads, 16 KV heads, inter 5504, 24 layers (the Sheared-LLaMA-1.3B shape: head
dim 128, the same vocabulary), synthetic weights of ANOTHER seed -- so next to nothing is
accepted, every cycle advances one position, and a cycle's full cost is what gets timed.
Synthetic weights have no meaningful acceptance rate: none is reported. What is reported is the
number of accepted ids per cycle at which a cycle breaks even with plain decode.

Around each start position P: a synthetic prompt of P ids through both engines' prefill, then,
per k and pass, from the same state (both engines rewound with Engine.edit):

  plain    P .. P + cycles as plain decode steps of the target (graph replay): us per token
  cycle    `cycles` cycles driven from Python with the library's own calls, a host clock
           around each part: the draft's k steps + the read-back of its k ids (draft_us), the
           target's verify step of k + 1 rows, which ends in its own synchronise (verify_us);
           the medians over the cycles
  loop     llmi_engine_generate_draft over `cycles` positions: time / verify steps (loop_us;
           its last cycles draft fewer than k ids -- remaining - 1 -- so it reads a little low)

One JSON line per (pass, position, k) and a last line with the medians over the passes and

  break_even_accepted = cycle_us / plain_us - 1

the mean number of accepted proposals per cycle above which the cycle beats plain decode (a
cycle yields accepted + 1 tokens). Before anything is timed the loop's tokens are compared with
plain decode's (a mismatch aborts the probe). Each timed section runs under a time limit of its
own (--limit seconds: the process exits when one overruns it).
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

from llmi.engine import Engine, preset, synth_prompt  # noqa: E402

DRAFT_SHAPE = dict(hidden=2048, heads=16, kv_heads=16, inter=5504, layers=24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--k", default="1,3,5,7")
    ap.add_argument("--pos", default="256,1792")
    ap.add_argument("--cycles", type=int, default=24)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "draft_probe.jsonl"))
    a = ap.parse_args()
    ks = [int(v) for v in a.k.split(",")]
    starts = [int(v) for v in a.pos.split(",")]
    W = a.cycles
    assert all(1 <= k <= 7 for k in ks)
    max_seq = max(2048, max(starts) + W * 8 + 8)
    tcfg = preset("llama2-7b", max_seq=max_seq)
    dcfg = preset("llama2-7b", max_seq=max_seq, **DRAFT_SHAPE)
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

    with Engine(tcfg) as t, Engine(dcfg) as d:
        t.load_synthetic(0)
        d.load_synthetic(1)
        t.set_speculation(max(ks))

        def rewind(hist, P):
            """both engines back at position P: the target with its pending token hist[P], the
            draft with hist[P] forced"""
            t.edit(P - 1, hist[P - 1:P])
            t.decode(1)
            d.edit(P - 1, hist[P - 1:P + 1])
            d.decode(1)
            t.sync()
            d.sync()

        def plain_window():
            t0 = time.perf_counter()
            t.decode(W)
            t.sync()
            return (time.perf_counter() - t0) / W * 1e6

        def cycle_window(P, k):
            p, dr, ve, acc = P, [], [], 0
            for _ in range(W):
                t0 = time.perf_counter()
                d.decode(p + k - d.position()[0])
                props = d.tokens(p + k + 1)[p + 1:]
                t1 = time.perf_counter()
                n_acc = t.verify(props)
                t2 = time.perf_counter()
                dr.append((t1 - t0) * 1e6)
                ve.append((t2 - t1) * 1e6)
                acc += n_acc
                hist = t.tokens(p + n_acc + 2)  # (untimed: the library's loop gets g from the verify step)
                keep = min(p + n_acc + 1, d.position()[0])
                d.edit(keep, hist[keep:])
                p += n_acc + 1
            return statistics.median(dr), statistics.median(ve), acc

        def loop_window(k):
            t0 = time.perf_counter()
            s = t.generate_draft(d, W, k)
            dt = time.perf_counter() - t0
            return dt / s.verify_steps * 1e6, s

        for P in starts:
            prompt = synth_prompt(P, P, tcfg.vocab)
            t.set_prompt(prompt)
            t.prefill(P)
            hist = t.tokens(P + 1).copy()
            d.set_prompt(hist)
            d.prefill(P)
            limited(plain_window)  # untimed: graphs, code objects; and the true continuation
            true = t.tokens(P + W + 1).copy()
            for k in ks:           # untimed, and the token check of every k
                rewind(hist, P)
                limited(lambda: loop_window(k))
                assert t.tokens(P + W + 1).tolist() == true.tolist(), "generate_draft's tokens differ from plain decode's"
                rewind(hist, P)
                limited(lambda: cycle_window(P, k))
            for ps in range(a.passes):
                for k in ks:
                    rewind(hist, P)
                    us_plain = limited(plain_window)
                    rewind(hist, P)
                    us_d, us_v, acc = limited(lambda: cycle_window(P, k))
                    rewind(hist, P)
                    us_loop, s = limited(lambda: loop_window(k))
                    emit({"pass": ps, "pos": P, "k": k, "cycles": W, "plain_us": round(us_plain, 2),
                          "draft_us": round(us_d, 2), "verify_us": round(us_v, 2), "cycle_us": round(us_d + us_v, 2),
                          "loop_us": round(us_loop, 2), "accepted_py": acc, "loop_verify_steps": s.verify_steps,
                          "loop_drafted": s.drafted, "loop_accepted": s.accepted, "tokens_equal": True})

    def med(xs):
        return round(statistics.median(xs), 2)

    summary = {"summary": True, "cycles": W, "passes": a.passes, "by_pos": {}}
    for P in starts:
        s = {}
        for k in ks:
            at = [r for r in lines if r["pos"] == P and r["k"] == k]
            cyc, plain = med([r["cycle_us"] for r in at]), med([r["plain_us"] for r in at])
            s[str(k)] = {"plain_us": plain, "draft_us": med([r["draft_us"] for r in at]),
                         "verify_us": med([r["verify_us"] for r in at]), "cycle_us": cyc,
                         "loop_us": med([r["loop_us"] for r in at]),
                         "break_even_accepted": round(cyc / plain - 1, 2)}
        summary["by_pos"][str(P)] = s
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
