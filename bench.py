#!/usr/bin/env python3
"""Decode benchmark: Llama-2-7B fp16 single-stream greedy decode to 2048 tokens.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N)

A plain run does only what `value` needs: it builds the engine, runs W warmup
steps, times K steps, writes the last step's outputs if `--dump-outputs` is
given, and prints one JSON line (`value`, `ms_per_step`, the decode loop's
algorithmic HBM fraction). Everything else described below -- the per-kernel and
roofline timings, the measured HBM read peak, the TP exchange, graph timeline,
prefill and int8 side measurements and the CPU baseline -- runs only with `--full`.

`--dump-outputs DIR` writes what a caller of the timed path receives after the
last timed step as DIR/<name>.npy: `tokens` (prompt + generated ids, float64),
`logits` (the last forward's logits, float32; this rank's vocabulary shard at
N > 1) and `hidden` (the last forward's final hidden state, float32). Ranks other
than 0 write <name>_rank<r>.npy. Weights and prompt come from a fixed seed, so
the same arguments give the same inputs in every run and on every build.

One "step" = one full greedy generation on the BASELINE.json configs[1]
workload: synthetic random-init Llama-2-7B weights (llmi-prng-v1, fp16), an
8-token synthetic prompt, then single-token decode forwards at positions
0..2047 (ctx 1..2048; 2048 forwards, 2041 generated tokens), all inside the
native engine (one hipGraph replay per token). N > 1 runs tensor parallel over
N GPUs (config 4: head/FFN row/col shard; the per-layer residual exchange is the
one-shot peer exchange over xGMI once it has matched RCCL's tokens on a short
run, else RCCL all-reduce); each rank streams 1/N of the weights, total work is
fixed ("strong" scaling). Started without a launcher, `--gpus N` spawns the N
rank processes itself (before any GPU call).

value = generated tokens / s (whole job). Also reported with `--full`: HBM roofline of the
dominant kernel (gate_up GEMV, HIP events on the engine stream, launches cycling
through the 32 layers so the weights stream from HBM as in the loop), the whole
decode loop's algorithmic HBM fraction, and a CPU baseline (the numpy oracle,
rank 0 at N = 1 only, bounded sample, scaled to the same unit). At N = 1 two
side measurements of the other single-GPU configs ride along (never `value`):
"prefill" (config 3: 512-row prompt, MFMA GEMMs, TFLOP/s vs the 2.5 PF dense
fp16 peak) and "int8_13b" (config 5: Llama-2-13B-shape W8A16 decode).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "llm-inference_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md chip table (spec)
MAX_SEQ = 2048
PROMPT = 8
SEED = 0


def progress(msg: str):
    """Phase markers on stderr (a long silent run looks hung to a watchdog)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def algorithmic_bytes(weight_bytes: int, kv_per_pos: int, n_fwd: int) -> int:
    """Sum over forwards at ctx = 1..n_fwd of weights + KV read (ctx slots) + KV write (1 slot)."""
    ctx_sum = n_fwd * (n_fwd + 1) // 2
    return n_fwd * weight_bytes + kv_per_pos * (ctx_sum + n_fwd)


def cpu_info():
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"cpu_count": os.cpu_count(), "cpu_model": model}


def cpu_baseline(sample_layers: int = 2, n_short: int = 12, n_long: int = 6, long_ctx: int = 1024):
    """The numpy restatement of modeling_llama.py (oracle/llama_ref.py, fp32) on this
    host, like-for-like with the GPU numbers (a bounded sample, scaled):
      decode  (configs[1]): 7B width, `sample_layers` layers; forwards at ctx 1..n_short and,
              with the cache pre-filled to long_ctx positions, at ctx long_ctx+1..+n_long. A
              layer's time is linear in ctx (weights + attention over ctx), so the two samples
              give its mean over the GPU run's ctx 1..2048; + lm_head; x 32 layers.
      prefill (configs[2]): the same model, one 512-row batched prefill, x 32 layers.
      int8_13b (configs[4]): 13B width, one W8A16 layer (dequantised to fp32), x 40 layers."""
    from threadpoolctl import threadpool_info

    from oracle import llama_ref as R
    from oracle import prng
    threads = max([d.get("num_threads", 1) for d in threadpool_info()] or [1])
    cfg = R.LlamaConfig(layers=sample_layers, max_seq=MAX_SEQ)
    o = R.LlamaOracle(cfg, seed=SEED)
    ids = prng.prompt_ids(SEED, PROMPT, cfg.vocab)

    def fwd_time(n, pos0):
        o.pos = pos0
        logits, t = None, 0.0
        for i in range(n):
            tok = int(ids[i % PROMPT]) if logits is None or i < PROMPT else int(np.argmax(logits))
            t0 = time.perf_counter()
            logits = o.forward_token(tok)
            t += time.perf_counter() - t0
        return t / n

    o.forward_token(int(ids[0]))  # warm the BLAS pools
    progress("cpu baseline: decode samples")
    t_short = fwd_time(n_short, 0)                      # ctx 1..n_short
    rng = np.random.default_rng(SEED)
    o.k_cache[:, :, :long_ctx] = rng.standard_normal(o.k_cache[:, :, :long_ctx].shape, dtype=np.float32)
    o.v_cache[:, :, :long_ctx] = rng.standard_normal(o.v_cache[:, :, :long_ctx].shape, dtype=np.float32)
    t_long = fwd_time(n_long, long_ctx)                 # ctx long_ctx+1..long_ctx+n_long
    x = o.last_hidden
    t0 = time.perf_counter()
    for _ in range(n_short):
        R.linear(R.rmsnorm(x, o.final_norm, cfg.rms_eps), o.lm_head)
    t_head = (time.perf_counter() - t0) / n_short
    c_short, c_long = (n_short + 1) / 2, long_ctx + (n_long + 1) / 2
    l_short, l_long = (t_short - t_head) / sample_layers, (t_long - t_head) / sample_layers
    slope = (l_long - l_short) / (c_long - c_short)
    l_mean = l_short + slope * ((MAX_SEQ + 1) / 2 - c_short)   # mean layer time over ctx 1..2048
    per_tok = t_head + 32 * l_mean
    out = {"value": round(1.0 / per_tok, 4), "unit": "tokens/s", "cores": int(threads), "kind": "port",
           "threads_note": "BLAS threads = the box's per-GPU CPU share (OMP_NUM_THREADS is pinned to 16 there; "
                           "os.cpu_count() reports the whole host)",
           **cpu_info(), "ctx": f"1..{MAX_SEQ} (modelled from samples at ctx 1..{n_short} and "
                                 f"{long_ctx + 1}..{long_ctx + n_long})",
           "sample": f"numpy oracle (oracle/llama_ref.py, fp32 weights from the fp16 PRNG values), Llama-2-7B "
                     f"width, {sample_layers} layers + lm_head; per-layer {l_short * 1e3:.1f} ms at ctx ~{c_short:.0f}, "
                     f"{l_long * 1e3:.1f} ms at ctx ~{c_long:.0f}; lm_head {t_head * 1e3:.1f} ms; "
                     f"per token = lm_head + 32 x mean layer time over ctx 1..{MAX_SEQ}"}
    # configs[2]: one 512-row prefill on the same model
    progress("cpu baseline: prefill sample")
    m = 512
    o.pos = 0
    t0 = time.perf_counter()
    o.prefill(prng.prompt_ids(SEED + 1, m, cfg.vocab))
    t_pf = time.perf_counter() - t0
    pf_ms = (t_pf - t_head) / sample_layers * 32 * 1e3 + t_head * 1e3
    out["prefill"] = {"ms": round(pf_ms, 1), "rows": m,
                      "sample": f"oracle prefill of {m} rows, {sample_layers} layers ({t_pf * 1e3:.0f} ms), x 32 layers"}
    del o
    # configs[4]: one 13B-width int8 layer
    progress("cpu baseline: int8 13B sample")
    c13 = R.LlamaConfig(hidden=5120, heads=40, kv_heads=40, inter=13824, layers=1, max_seq=64)
    o13 = R.LlamaOracle(c13, seed=SEED, int8=True)
    o13.forward_token(int(ids[0]))
    t0 = time.perf_counter()
    for i in range(n_long):
        o13.forward_token(int(ids[i % PROMPT]))
    t13 = (time.perf_counter() - t0) / n_long
    x = o13.last_hidden
    t0 = time.perf_counter()
    for _ in range(n_long):
        R.linear(R.rmsnorm(x, o13.final_norm, c13.rms_eps), o13.lm_head)
    h13 = (time.perf_counter() - t0) / n_long
    out["int8_13b"] = {"tokens_per_s": round(1.0 / (h13 + 40 * (t13 - h13)), 4),
                       "sample": f"oracle, 13B width, 1 W8A16 layer (dequantised fp32) + lm_head, {n_long} forwards at "
                                 f"ctx <= {n_long + 1}; per token = lm_head + 40 x layer time"}
    return out


def hbm_read_peak(bytes_: int):
    """The roofline's second denominator (SURVEY.md §8d timing rules): the measured one-shot
    HBM read rate, llmi_hbm_read_bench -- launches that each read `bytes_` with 16-B
    non-temporal loads, cycling a 2 GiB buffer so every launch streams from HBM; best of four
    grids. Run twice: at the dominant kernel's byte count and at 1 GiB (sustained)."""
    import ctypes
    from llmi._lib import call
    out = {}
    for name, b in (("same_bytes", bytes_), ("sustained_1GiB", 1 << 30)):
        us, gbps, rd = ctypes.c_float(), ctypes.c_float(), ctypes.c_size_t()
        call("llmi_hbm_read_bench", ctypes.c_size_t(int(b)), 40 if b < (1 << 30) else 10, ctypes.byref(us),
             ctypes.byref(gbps), ctypes.byref(rd))
        out[name] = {"GBps": round(gbps.value, 1), "us": round(us.value, 2), "bytes": rd.value}
    return out


def pmc_traffic(kernel: str):
    """HBM bytes per launch from the committed rocprofv3 --pmc pass (profiles/), if present."""
    p = os.path.join(REPO, "profiles", "pmc_traffic.json")
    try:
        d = json.load(open(p))
        return d["kernels"][kernel]["hbm_bytes_per_launch"], d.get("source")
    except Exception:
        return None, None


MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16 MFMA (MI355X_MICROARCH.md; 2:1 sparse figures excluded)


def prefill_side(eng, prompt_len: int = 512, reps: int = 3):
    """Config 3 beside the headline: one 512-row prefill (firstTokenGen) in both
    GEMM precisions on the already-loaded 7B engine. Algorithmic FLOPs: the four
    projections 2*M*N*K per layer + causal attention 4*heads*d*M(M+1)/2 + lm_head row."""
    import llmi
    from llmi.engine import synth_prompt
    cfg = eng.cfg
    m = min(prompt_len, cfg.max_seq - 1)
    lin = cfg.hidden * (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim + cfg.hidden * cfg.hidden \
        + 3 * cfg.hidden * cfg.inter
    flops = cfg.layers * (2 * m * lin + 4 * cfg.heads * cfg.head_dim * (m * (m + 1) // 2)) \
        + 2 * cfg.hidden * cfg.vocab
    ids = synth_prompt(SEED + 1, m, cfg.vocab)
    out = {"config": f"Llama-2-7B fp16 prefill, {m} rows, batch 1 (BASELINE.json configs[2])",
           "flops": flops, "peak_tflops": MFMA_F16_PEAK_TFLOPS}
    eng.set_prompt(ids)
    eng.prefill(m, 2)  # the e4m3 weight copies are made on the first exact=2 call (not timed)
    eng.sync()
    for exact in (1, 2, 0):
        best = None
        for _ in range(reps):
            eng.set_prompt(ids)
            eng.sync()
            t0 = time.perf_counter()
            eng.prefill(m, exact)
            eng.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        tf = flops / best / 1e12
        # exact: hi + lo fp16 planes (2x the fp16 MFMA work); exact_fp8lo: fp16 hi + e4m3 lo
        # planes on the block-scaled fp8 MFMA (1.5x; F6 logits 1.16e-4 vs 1.14e-4 exact);
        # fp16_activations_approx: hi plane only -- NOT parity-qualified (its F6 logits error,
        # 3.8e-4 at 1 layer, grows to ~2e-3 at 32 layers in the oracle study, above the north
        # star's 1e-3): a throughput figure, labelled as such
        key = {1: "exact", 2: "exact_fp8lo", 0: "fp16_activations_approx"}[exact]
        out[key] = {
            "ms": round(best * 1e3, 3), "tflops": round(tf, 1), "frac_of_peak": round(tf / MFMA_F16_PEAK_TFLOPS, 4),
            "mfma_work_factor": {1: 2, 2: 1.5, 0: 1}[exact]}
        if exact == 0:
            out[key]["parity"] = ("approximate: fp16 activations; F6 logits rel-L2 3.8e-4 (1 layer), ~2.0e-3 at 32 "
                                  "layers (oracle study, profiles/r02_prefill_precision_study.json) vs the 1e-3 bar")
    return out


def int8_side(n_new: int = MAX_SEQ - PROMPT + 1):
    """Config 5 beside the headline: Llama-2-13B-shape int8 W8A16 single-stream decode,
    over the same ctx 1..2048 as the headline (2048 forwards)."""
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-13b", max_seq=PROMPT + n_new)
    cfg.weight_dtype, cfg.kv_dtype = llmi.I8, llmi.F16
    with Engine(cfg) as e:
        e.load_synthetic(SEED)
        prompt = synth_prompt(SEED, PROMPT, cfg.vocab)
        e.generate(prompt, 16)  # warm: graph capture
        e.set_prompt(prompt)
        e.sync()
        t0 = time.perf_counter()
        e.decode(PROMPT + n_new - 1)
        e.sync()
        dt = time.perf_counter() - t0
        wbytes, kvb = e.bytes_per_token()
        gu_us, gu_b = e.time_kernel("gate_up", iters=128)
    n_fwd = PROMPT + n_new - 1
    total = algorithmic_bytes(wbytes, kvb, n_fwd)
    return {"config": "Llama-2-13B shape, int8 weights + fp16 row scales (W8A16), fp16 KV, batch 1 "
                      "(BASELINE.json configs[4])",
            "tokens_per_s": round(n_new / dt, 2), "forwards": n_fwd, "ctx": f"1..{n_fwd}",
            "weight_bytes_per_token": wbytes,
            "loop_GBps": round(total / dt / 1e9, 1), "loop_frac_of_8TBps": round(total / dt / 1e9 / HBM_PEAK_GBS, 4),
            "gate_up_GBps": round(gu_b / (gu_us * 1e-6) / 1e9, 1)}


def graph_timeline_side(eng, prompt, ctx: int = 1024):
    """One token of the timed configuration (graph replay) stamped per workgroup
    (llmi.timeline, llmi_engine_debug_timeline): kernel spans and in-graph boundaries at
    context `ctx` -- the graph-mode counterpart of the eager HIP-event kernels_us."""
    from llmi.timeline import stamped_token
    eng.set_prompt(prompt)
    r = stamped_token(eng, ctx - 1)
    r["ctx"] = ctx
    r["per_kernel_span_us"] = {k: v["span_us_mean"] for k, v in r.pop("per_kernel").items()}
    return r


def open_oneshot_exchange(eng, dist, prompt, world, n_check: int = 64, rccl: bool = True):
    """Config 4's exchange: every rank maps every peer's inbox (IPC handles all-gathered
    over gloo), then a short greedy run over RCCL and over the one-shot peer exchange must
    give the same tokens on every rank before the one-shot path is used for the timed run;
    otherwise (or on any error, e.g. a peer that never arrives: error bit 8, no hang) the
    run stays on RCCL and the JSON line says why. Without RCCL (the one-device rehearsal,
    LLMI_BENCH_ONE_DEVICE) the one-shot tokens must agree across the ranks, or it raises."""
    info = {"mode": "rccl"}
    ok, why = False, ""
    tb = None
    try:
        hs = [None] * world
        dist.all_gather_object(hs, eng.xchg_handle())
        eng.xchg_open(hs)
        ta = eng.generate(prompt, n_check) if rccl else None
        eng.set_exchange(1)
        tb = eng.generate(prompt, n_check)
        ok = True if ta is None else bool((ta == tb).all())
        why = "" if ok else "one-shot tokens differ from RCCL"
    except Exception as e:  # reported, never fatal: RCCL carries the run
        why = repr(e)[:300]
    oks = [None] * world
    dist.all_gather_object(oks, (ok, why, None if tb is None else tb.tolist()))
    if ok and not rccl and any(o[2] != oks[0][2] for o in oks):
        ok = False
    if all(o[0] for o in oks) and (rccl or all(o[2] == oks[0][2] for o in oks)):
        info["mode"] = "oneshot"
        fused = pick_fused_exchange(eng, dist, prompt, world, tb)
        info.update(fused)
    elif not rccl:
        raise RuntimeError(f"one-device rehearsal: one-shot exchange failed: {[o[1] for o in oks]}")
    else:
        try:
            eng.set_exchange(0)
        except Exception:
            pass
        info["oneshot_rejected"] = [o[1] for o in oks if not o[0]][:2]
    return info


def pick_fused_exchange(eng, dist, prompt, world, ref_tokens, n_time: int = 128):
    """Exchange mode 2 (the push / wait / reduce fused into the o_proj, down and lm_head
    launches) against mode 1 (one exchange launch each): both must give the tokens the
    checked mode-1 run gave on every rank; then each is timed over n_time graph-replayed
    forwards on every rank (a collective) and the faster by the slowest rank carries the
    timed run. Any error keeps mode 1, with the reason."""
    import time as _t
    out = {}
    ok, why = False, ""
    try:
        eng.set_exchange(2)
        t2 = eng.generate(prompt, len(ref_tokens)) if ref_tokens is not None else None
        ok = t2 is not None and bool((t2 == ref_tokens).all())
        why = "" if ok else "fused-exchange tokens differ"
    except Exception as e:
        why = repr(e)[:300]
    oks = [None] * world
    dist.all_gather_object(oks, (ok, why))
    if not all(o[0] for o in oks):
        eng.set_exchange(1)
        out["fused_rejected"] = [o[1] for o in oks if not o[0]][:2]
        return out
    times, terr = {}, ""
    n = min(n_time, eng.cfg.max_seq - 1)
    try:  # local work only: no collective may sit inside a block that can raise on one rank
        for m in (1, 2, 1, 2):
            eng.set_exchange(m)
            eng.set_prompt(prompt)
            eng.decode(n)  # graph capture + warm
            eng.sync()
            eng.set_prompt(prompt)
            t0 = _t.perf_counter()
            eng.decode(n)
            eng.sync()
            dt = _t.perf_counter() - t0
            times[m] = min(dt, times.get(m, dt))
    except Exception as e:
        terr = repr(e)[:300]
    allt = [None] * world
    dist.all_gather_object(allt, (times, terr))
    if any(t[1] or len(t[0]) != 2 for t in allt):
        eng.set_exchange(1)
        out["fused_rejected"] = [t[1] for t in allt if t[1]][:2] or ["timing incomplete"]
        return out
    worst = {m: max(t[0][m] for t in allt) for m in (1, 2)}
    best = 2 if worst[2] < worst[1] else 1
    eng.set_exchange(best)
    out["mode"] = "fused" if best == 2 else "oneshot"
    out["us_per_forward_oneshot_vs_fused"] = [round(worst[1] / n * 1e6, 2), round(worst[2] / n * 1e6, 2)]
    return out


def tp_exchange_side(eng, layers, ms_per_token, wbytes, mode="rccl", rccl=True):
    """TP exchange budget: per token 2 * layers int64 all-reduces of the
    hidden-size fixed-point residual (32 KB) plus one uint64 max over the lm_head
    partials. Times the engine's own residual all-reduce on its RCCL communicator --
    eagerly and replayed from one captured graph, as the decode step replays them (a
    collective: every rank runs this) -- and sets calls x latency against the measured
    ms per token and the per-rank weight stream."""
    out = {"calls_per_token": 2 * layers + 1, "payload_bytes": 4096 * 8}
    out["mode"] = mode
    lat = None
    if rccl:
        out["allreduce_us_eager"] = round(eng.time_kernel("allreduce", iters=200)[0], 2)
        out["allreduce_us_graph"] = round(eng.time_kernel("allreduce_graph", iters=256)[0], 2)
        lat = out["allreduce_us_graph"]
    if mode in ("oneshot", "fused"):
        out["oneshot_us_eager"] = round(eng.time_kernel("xchg", iters=200)[0], 2)
        out["oneshot_us_graph"] = round(eng.time_kernel("xchg_graph", iters=256)[0], 2)
        lat = out["oneshot_us_graph"]
    out["exchange_us_per_token_est"] = round(lat * out["calls_per_token"], 1)
    out["ms_per_token"] = round(ms_per_token, 4)
    out["weight_stream_us_per_token_at_6.2TBps"] = round(wbytes / 6.2e12 * 1e6, 1)
    out["exchange_share_of_token"] = round(out["exchange_us_per_token_est"] / (ms_per_token * 1e3), 3)
    return out


def dump_outputs(dirname: str, eng, toks, rank: int):
    """--dump-outputs: the timed path's results after its last step, as a caller reads them
    back from the engine -- the whole token sequence, the last forward's logits (this rank's
    vocabulary shard) and its final hidden state. A few hundred KB in all."""
    os.makedirs(dirname, exist_ok=True)
    sfx = "" if rank == 0 else f"_rank{rank}"
    arrays = {"tokens": np.asarray(toks, np.float64), "logits": eng.logits().astype(np.float32),
              "hidden": eng.hidden().astype(np.float32)}
    for name, a in arrays.items():
        np.save(os.path.join(dirname, f"{name}{sfx}.npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def spawn_workers(n: int, argv) -> int:
    """`--gpus N` (N > 1) started without a launcher: start N workers of this script,
    one per GPU (RANK = LOCAL_RANK = r, WORLD_SIZE = N, rendezvous on 127.0.0.1), and
    relay rank 0's JSON line. The parent itself never imports the engine library or
    touches a GPU; if any worker fails, the others are stopped and its code returned."""
    import socket
    import subprocess
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out0 = tempfile.TemporaryFile(mode="w+")
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL))
    progress(f"spawned {n} workers (rendezvous 127.0.0.1:{port})")
    rc = 0
    while any(p.poll() is None for p in procs):
        bad = [p.returncode for p in procs if p.returncode not in (None, 0)]
        if bad:
            rc = bad[0]
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
        if rc == 0 and p.returncode != 0:
            rc = p.returncode
    out0.seek(0)
    for line in out0.read().splitlines():  # the JSON line to stdout, library chatter to stderr
        print(line, file=sys.stdout if line.startswith("{") else sys.stderr, flush=True)
    return rc


def dry_run(rank: int, world: int):
    """Launcher check: the rendezvous and the gloo group, no GPU, no engine."""
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        ranks = [None] * world
        dist.all_gather_object(ranks, {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")),
                                       "pid": os.getpid()})
        dist.barrier()
        dist.destroy_process_group()
    else:
        ranks = [{"rank": 0, "local_rank": 0, "pid": os.getpid()}]
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks": ranks}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-seq", type=int, default=MAX_SEQ)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the per-kernel / roofline timings, the measured HBM read "
                         "peak, the side measurements (TP exchange, graph timeline, prefill, int8 13B) and the CPU "
                         "baseline; a plain run stops at the headline figure")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's tokens, logits and hidden state as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-side", action="store_true",
                    help="with --full: skip the graph timeline / prefill / int8-13B side measurements")
    ap.add_argument("--kv", choices=["f16", "f32"], default="f16")
    ap.add_argument("--tp-exchange", action="store_true",
                    help="world 1: give the engine a single-rank RCCL communicator (its all-reduces run in the "
                         "decode graph) and, with --full, time the TP exchange -- a rehearsal of the world > 1 side "
                         "measurement")
    ap.add_argument("--eager", action="store_true",
                    help="launch kernels eagerly instead of replaying the hipGraph (profiling: rocprofv3 "
                         "kernel tracing of graph replays crashes on ROCm 7.2)")
    ap.add_argument("--dry-run", action="store_true",
                    help="check the launcher only: spawn / rendezvous / gloo group, then exit before any GPU call")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_workers(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry_run:
        dry_run(rank, world)
        return

    import llmi
    from llmi.engine import Engine, preset, synth_prompt, tp_unique_id

    dist = None
    tp_id = None
    # one-device rehearsal of the N > 1 path (a one-GPU box): every rank on device 0, no RCCL
    # (it refuses two ranks on one device), the one-shot exchange carries the TP reduction;
    # the throughput is then N ranks sharing one GPU -- a path check, not a scaling number
    one_dev = world > 1 and os.environ.get("LLMI_BENCH_ONE_DEVICE") == "1"
    if world > 1:
        import torch.distributed as dist  # plumbing only: id exchange, barrier, max
        dist.init_process_group("gloo", rank=rank, world_size=world)
        if not one_dev:
            obj = [tp_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(obj, src=0)
            tp_id = obj[0]
    elif args.tp_exchange:  # world-1 rehearsal: a single-rank RCCL communicator in the engine
        tp_id = tp_unique_id()

    cfg = preset("llama2-7b", max_seq=args.max_seq, tp_rank=rank, tp_world=world)
    cfg.kv_dtype = llmi.F16 if args.kv == "f16" else llmi.F32
    eng = Engine(cfg, device=0 if one_dev else local, tp_id=tp_id)
    eng.load_synthetic(SEED)
    prompt = synth_prompt(SEED, PROMPT, cfg.vocab)
    n_fwd = cfg.max_seq
    gen_per_step = n_fwd - PROMPT + 1

    def barrier():
        if dist is not None:
            dist.barrier()

    xchg = {"mode": "rccl" if tp_id is not None else "none"}
    if dist is not None and (one_dev or os.environ.get("LLMI_TP_EXCHANGE", "oneshot") == "oneshot"):
        progress("one-shot peer exchange: open + check against RCCL")
        xchg = open_oneshot_exchange(eng, dist, prompt, world, rccl=not one_dev)
        if one_dev:
            xchg["one_device_rehearsal"] = True
        progress(f"tp exchange: {xchg}")

    def one_generation():
        eng.set_prompt(prompt)
        eng.decode(n_fwd, use_graph=not args.eager)

    progress(f"warmup x{args.warmup}")
    for _ in range(args.warmup):
        one_generation()
    eng.sync()
    barrier()
    eng.sync()
    progress(f"timed x{args.steps}")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_generation()
    eng.sync()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    toks = eng.tokens(n_fwd + 1)
    consistent = True
    if dist is not None:
        objs = [None] * world
        dist.all_gather_object(objs, toks[:64].tolist())
        consistent = all(o == objs[0] for o in objs)

    wbytes, kvb = eng.bytes_per_token()
    dumped = dump_outputs(args.dump_outputs, eng, toks, rank) if args.dump_outputs else None
    gu_us = gu_bytes = None
    kern, peak_meas, side = {}, {}, {}
    if args.full:
        progress("kernel timings")
        # dominant kernel: gate_up GEMV, timed with HIP events on the engine stream
        gu_us, gu_bytes = eng.time_kernel("gate_up", iters=256)
        kern = {k: eng.time_kernel(k, iters=128) for k in ("qkv", "attn", "o", "down", "lm_head")}
        try:  # the decode graph's q/k/v + attention launch (the two kernels above, fused)
            kern["qkv_attn"] = eng.time_kernel("qkv_attn", iters=128)
        except Exception as e:  # reported, never fatal to the GPU number
            progress(f"qkv_attn timing skipped: {e!r}"[:200])
        try:
            peak_meas = hbm_read_peak(gu_bytes)
        except Exception as e:  # reported, never fatal to the GPU number
            peak_meas = {"error": repr(e)[:300]}
        if tp_id is not None or one_dev:
            progress("tp exchange side measurement")
            try:
                side["tp_exchange"] = tp_exchange_side(eng, cfg.layers, elapsed * 1e3 / args.steps / n_fwd, wbytes,
                                                       mode=xchg["mode"], rccl=tp_id is not None)
                if one_dev:
                    side["tp_exchange"]["one_device_rehearsal"] = True
                for k in ("oneshot_rejected", "fused_rejected", "us_per_forward_oneshot_vs_fused"):
                    if k in xchg:
                        side["tp_exchange"][k] = xchg[k]
            except Exception as e:  # reported, never fatal to the GPU number
                side["tp_exchange"] = {"error": repr(e)[:300]}
        if world == 1 and not args.no_side and not args.eager:
            progress("graph timeline side measurement")
            try:
                side["graph_timeline"] = graph_timeline_side(eng, prompt)
            except Exception as e:  # reported, never fatal to the GPU number
                side["graph_timeline"] = {"error": repr(e)[:300]}
        if world == 1 and not args.no_side:
            progress("prefill side measurement")
            side["prefill"] = prefill_side(eng, prompt_len=512)
    eng.close()
    if args.full and world == 1 and not args.no_side:
        progress("int8 13B side measurement")
        side["int8_13b"] = int8_side()
    if rank != 0:
        if dist is not None:
            dist.barrier()
        return
    value = gen_per_step * args.steps / elapsed
    ms_per_step = elapsed * 1e3 / args.steps
    per_rank_bytes = algorithmic_bytes(wbytes, kvb, n_fwd)
    full = {}
    if args.full:  # what the per-kernel timings and the measured read peak feed
        traffic, traffic_src = pmc_traffic("gate_up")
        achieved = gu_bytes / (gu_us * 1e-6) / 1e9
        full["roofline"] = {
            "bound": "hbm", "kernel": "gate_up GEMV (rmsnorm+gate_up+silu*mul), layers cycled",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
            "algorithmic_bytes": gu_bytes, "avg_us": round(gu_us, 2),
            "traffic_source": traffic_src,
            # the headline frac is against the 8 TB/s spec (peak); peak_measured is a
            # one-shot HBM read of the same bytes in this process (and a 1 GiB read)
            "denominator": "peak = 8 TB/s spec (headline); frac_of_measured uses peak_measured.same_bytes",
            "peak_measured": peak_meas,
            "frac_of_measured": (round(achieved / peak_meas["same_bytes"]["GBps"], 4)
                                 if "same_bytes" in peak_meas else None)}
        full["kernels_us"] = {"gate_up": round(gu_us, 2), **{k: round(v[0], 2) for k, v in kern.items()}}
        full["kernels_GBps"] = {"gate_up": round(achieved, 1),
                                **{k: round(v[1] / (v[0] * 1e-6) / 1e9, 1) for k, v in kern.items()}}
    out = {
        "metric": "decode tokens/sec Llama-2-7B fp16 @1 GPU; % HBM roofline; 1->8 TP curve",
        "value": round(value, 2),
        "unit": "tokens/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 2),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "fp16",
        "data": "synthetic (llmi-prng-v1 random-init Llama-2-7B weights, 8 PRNG prompt ids)",
        "config": {"workload": "Llama-2-7B fp16 single-stream greedy decode to 2048 tokens "
                               "(BASELINE.json configs[1]); TP over n_gpus when > 1",
                   "batch": 1, "prompt": PROMPT, "ctx": f"1..{n_fwd}", "forwards_per_step": n_fwd,
                   "generated_per_step": gen_per_step, "kv_cache": args.kv,
                   "weights": "fp16, fp32 activations/accumulate",
                   "parallelism": f"tp{world}" if world > 1 else "single"},
        "full": args.full,
        "decode_loop_hbm": {"bytes_per_step_per_rank": per_rank_bytes,
                            "achieved_GBps_per_rank": round(per_rank_bytes / (elapsed / args.steps) / 1e9, 1),
                            "frac_of_8TBps": round(per_rank_bytes / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                            "frac_of_measured_1GiB_read": (
                                round(per_rank_bytes / (elapsed / args.steps) / 1e9 /
                                      peak_meas["sustained_1GiB"]["GBps"], 4)
                                if "sustained_1GiB" in peak_meas else None),
                            "weight_bytes_per_token": wbytes, "kv_bytes_per_pos": kvb},
        **full,
        "tp_tokens_consistent": consistent,
        **side,
    }
    if dumped is not None:
        out["dumped_outputs"] = dumped
    if args.full and world == 1 and not args.no_cpu_baseline:
        try:
            progress("cpu baseline")
            out["cpu_baseline"] = cpu_baseline()
            if "prefill" in out and "exact" in out["prefill"]:
                out["cpu_baseline"]["prefill"]["gpu_speedup_exact"] = round(
                    out["cpu_baseline"]["prefill"]["ms"] / out["prefill"]["exact"]["ms"], 1)
        except Exception as e:  # reported, never fatal to the GPU number
            out["cpu_baseline"] = {"value": None, "error": repr(e)}
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()


if __name__ == "__main__":
    main()
