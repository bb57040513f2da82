"""The int8 KV cache (kv_dtype LLMI_I8, "KV8": include/llmi.h) through the engine, on the tiny
model of tests/golden/tiny.npz: 8-token prompt + 8 greedy tokens, fp16 weights unless said.

The reference is Kv8Oracle (tests/kv8_ref.py): the numpy oracle whose cache writes quantise and
dequantise the rows. d8 is that oracle's distance from the fp32-KV oracle (7.5e-4 here): an engine
that kept its rows unquantised would sit at d8 from Kv8Oracle, a quantising one at the fp32
kernels' own ~1e-5, so `r < d8 / 4` separates the two (besides LOGIT_TOL, the project's bar).

Prefill and decode write a row from values that differ by the GEMM-vs-GEMV rounding (~1e-6
relative, 1e-4 of a quantisation step), so the two may round a byte differently once in ten
thousand: the row comparisons cap differing bytes at 1 %, each by one step."""
import os

import numpy as np
import pytest

import kv8_ref

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3  # tests/test_gpu_engine.py
TP_TOL = 1e-5     # reassociation of the TP partial sums
N_NEW = 8


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(**over):
    import llmi
    from llmi.engine import preset
    over.setdefault("kv_dtype", llmi.I8)
    return preset("tiny", **over)


def _ocfg(kv_heads=4, max_seq=64):
    return R.LlamaConfig(hidden=512, heads=4, kv_heads=kv_heads, inter=1024, layers=2, max_seq=max_seq)


@pytest.fixture(scope="module")
def tiny():
    import llmi
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    seed, prompt = int(f["seed"]), np.asarray(f["prompt"], np.int32)
    out = dict(seed=seed, prompt=prompt)
    for kvh in (4, 2):
        o8 = kv8_ref.Kv8Oracle(_ocfg(kvh), seed=seed)
        t8, l8 = o8.greedy(prompt, N_NEW)
        t32, l32 = R.LlamaOracle(_ocfg(kvh), seed=seed).greedy(prompt, N_NEW)
        out[kvh] = dict(tokens=t8, logits=l8, d8=_rel(l8, l32), k=o8.k_cache.copy(), v=o8.v_cache.copy())
        assert (t8 == t32).all()
    llmi.lib()
    return out


def _engine(tiny, **over):
    from llmi.engine import Engine
    e = Engine(_cfg(**over))
    e.load_synthetic(tiny["seed"])
    return e


_ALONE = {}


def _decode_only(tiny, n_new=N_NEW, prompt=None, **over):
    """(tokens, logits, {(layer, pos, which_v): (q, scale bits)}) of the decode-only eager run."""
    prompt = tiny["prompt"] if prompt is None else prompt
    key = (tuple(int(t) for t in prompt), n_new, tuple(sorted(over.items())))
    if key not in _ALONE:
        with _engine(tiny, **over) as e:
            toks = e.generate(prompt, n_new, use_graph=False)
            rows = {(l, p, v): e.kv_slot_q8(l, p, bool(v)) for l in (0, 1) for p in range(len(prompt)) for v in (0, 1)}
            _ALONE[key] = (toks.copy(), e.logits().copy(), rows)
    return _ALONE[key]


def _rows_close(got, want, what):
    (q, s), (wq, ws) = got, want
    assert (np.abs(s.astype(np.int32) - ws.astype(np.int32)) <= 1).all(), (what, s, ws)
    diff = np.abs(q.astype(np.int32) - wq.astype(np.int32))
    assert diff.max(initial=0) <= 1, (what, int(diff.max()))
    assert (diff != 0).mean() <= 0.01, (what, float((diff != 0).mean()))


@pytest.mark.parametrize("kvh", [4, 2])
def test_engine_matches_the_quantising_oracle(tiny, kvh):
    ref = tiny[kvh]
    with _engine(tiny, kv_heads=kvh) as e:
        toks = e.generate(tiny["prompt"], N_NEW)
        logits = e.logits()
        slots = {(p, v): (e.kv_slot_q8(0, p, bool(v)), e.kv_slot(0, p, bool(v))) for p in (0, 7) for v in (0, 1)}
    r, d8 = _rel(logits, ref["logits"]), ref["d8"]
    print(f"kv_heads {kvh}: engine vs Kv8Oracle logits rel-L2 {r:.3e}; Kv8Oracle vs fp32-KV oracle d8 {d8:.3e}")
    np.testing.assert_array_equal(toks, ref["tokens"])
    assert r < LOGIT_TOL and r < d8 / 4
    for (p, v), ((q, s), deq) in slots.items():
        # the oracle's cache holds qdq(row): quantising it again is the identity on (q, s)
        want = kv8_ref.quant_rows((ref["v"] if v else ref["k"])[0, :, p])
        _rows_close((q, s), want, f"layer 0 pos {p} {'v' if v else 'k'}")
        np.testing.assert_array_equal(_bits(deq), _bits(kv8_ref.dequant(q, s)))


@pytest.mark.parametrize("qkv_attn", [None, 0])
def test_graph_replay_is_bitwise_the_eager_run(tiny, qkv_attn):
    te, le, _ = _decode_only(tiny)
    with _engine(tiny) as e:
        if qkv_attn is not None:
            e.set_option("qkv_attn", qkv_attn)
        ta = e.generate(tiny["prompt"], N_NEW, use_graph=False)
        la = e.logits()
        tg = e.generate(tiny["prompt"], N_NEW, use_graph=True)
        lg = e.logits()
    for t, l in ((ta, la), (tg, lg)):
        np.testing.assert_array_equal(t, te)
        np.testing.assert_array_equal(_bits(l), _bits(le))
    np.testing.assert_array_equal(tg, tiny[4]["tokens"])


def test_bytes_per_token_counts_the_scales(tiny):
    from llmi.engine import Engine
    for kvh in (4, 2):
        c = _cfg(kv_heads=kvh)
        with Engine(c) as e:
            assert e.bytes_per_token()[1] == c.layers * kvh * 130 * 2


def test_logprobs_and_nucleus_sampling_run(tiny):
    n = len(tiny["prompt"]) + N_NEW
    with _engine(tiny) as e:
        e.set_logprobs(3)
        e.set_sampling_params(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1, seed=5)
        runs = []
        for use_graph in (False, True):
            toks = e.generate(tiny["prompt"], N_NEW, use_graph=use_graph)
            runs.append((toks, *e.logprobs(n)))
    (t0, lp0, ids0, tlp0), (t1, lp1, ids1, tlp1) = runs
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(_bits(lp0), _bits(lp1))
    np.testing.assert_array_equal(ids0, ids1)
    np.testing.assert_array_equal(_bits(tlp0), _bits(tlp1))
    assert len(t0) == N_NEW and np.isfinite(lp0[1:]).all() and (lp0[1:] <= 0).all() and (ids0[1:] >= 0).all()


def _prompts():
    from llmi.engine import synth_prompt
    return [synth_prompt(3000 + i, n, 32000) for i, n in enumerate((3, 8, 5))]


def test_batch_slots_are_bitwise_the_engine_alone(tiny):
    from llmi.engine import Batch
    prompts = _prompts()
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(tiny["seed"])
        out = b.generate(prompts, N_NEW)
        logits = [b.logits(i).copy() for i in range(3)]
    for i, p in enumerate(prompts):
        wt, wl, _ = _decode_only(tiny, prompt=p)
        np.testing.assert_array_equal(out[i], wt)
        np.testing.assert_array_equal(_bits(logits[i]), _bits(wl))


def test_batch_prefill_matches_the_slots_decode_only_tokens(tiny):
    from llmi.engine import Batch
    prompts = _prompts()
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(tiny["seed"])
        out = b.generate(prompts, N_NEW, prefill=True)
    for i, p in enumerate(prompts):
        np.testing.assert_array_equal(out[i], _decode_only(tiny, prompt=p)[0])


def test_tp_group_of_two(tiny):
    from llmi.engine import TPGroup
    te, le, _ = _decode_only(tiny)
    with TPGroup(_cfg(), 2) as g:
        g.load_synthetic(tiny["seed"])
        tg = g.generate(tiny["prompt"], N_NEW)
        lg = g.logits()
    r = _rel(lg, le)
    print(f"TP 2 vs single engine logits rel-L2 {r:.3e}")
    np.testing.assert_array_equal(tg, te)
    assert r < TP_TOL


def test_ring_layer_decodes_the_same_tokens():
    """The ring layer needs hidden 4096: the 7B width, 2 layers (tests/test_gpu_ring.py's shape)."""
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-7b", layers=2, max_seq=64, kv_dtype=llmi.I8)
    prompt = synth_prompt(0, 8, cfg.vocab)
    out = {}
    with Engine(cfg) as e:
        e.load_synthetic(1)
        for mode in (0, 1):
            e.set_decode_mode(mode)
            out[mode] = (e.generate(prompt, N_NEW), e.logits().copy())
    r = _rel(out[1][1], out[0][1])
    print(f"ring vs launches (int8 KV) logits rel-L2 {r:.3e}")
    np.testing.assert_array_equal(out[1][0], out[0][0])
    assert r < LOGIT_TOL


@pytest.mark.parametrize("wname", ["i8", "f32"])
def test_other_weight_dtypes_generate_their_oracles_tokens(tiny, wname):
    import llmi
    wdt = dict(i8=llmi.I8, f32=llmi.F32)[wname]
    o = kv8_ref.Kv8Oracle(_ocfg(), seed=tiny["seed"], int8=(wname == "i8"))
    want_t, want_l = o.greedy(tiny["prompt"], N_NEW)
    with _engine(tiny, weight_dtype=wdt) as e:
        toks = e.generate(tiny["prompt"], N_NEW)
        r = _rel(e.logits(), want_l)
    print(f"{wname} weights + int8 KV: logits rel-L2 vs its Kv8Oracle {r:.3e}")
    np.testing.assert_array_equal(toks, want_t)
    assert r < LOGIT_TOL


# ------------------------------------------------------------------ prefill (exact mode)
def test_prefill_then_decode_against_decode_only(tiny):
    te, le, rows = _decode_only(tiny)
    n = len(tiny["prompt"])
    with _engine(tiny) as e:
        toks = e.generate(tiny["prompt"], N_NEW, prefill=True)
        logits = e.logits()
        got = {k: e.kv_slot_q8(k[0], k[1], bool(k[2])) for k in rows}
    r = _rel(logits, le)
    print(f"prefill({n}) + {N_NEW - 1} steps vs decode-only logits rel-L2 {r:.3e}")
    np.testing.assert_array_equal(toks, te)
    assert r < LOGIT_TOL
    # prefill-written rows against decode-written rows, all of them in one count
    _rows_close((np.stack([got[k][0] for k in rows]), np.stack([got[k][1] for k in rows])),
                (np.stack([rows[k][0] for k in rows]), np.stack([rows[k][1] for k in rows])), "prefill rows")


def test_prefill_after_decode_steps_unaligned_history(tiny):
    te, le, rows = _decode_only(tiny)
    with _engine(tiny) as e:
        e.set_prompt(tiny["prompt"])
        e.decode(3, use_graph=False)
        e.prefill(5)
        e.decode(N_NEW - 1)
        toks = e.tokens(len(tiny["prompt"]) + N_NEW)[len(tiny["prompt"]):]
        logits = e.logits()
        got = {k: e.kv_slot_q8(k[0], k[1], bool(k[2])) for k in rows}
    np.testing.assert_array_equal(toks, te)
    assert _rel(logits, le) < LOGIT_TOL
    _rows_close((np.stack([got[k][0] for k in rows]), np.stack([got[k][1] for k in rows])),
                (np.stack([rows[k][0] for k in rows]), np.stack([rows[k][1] for k in rows])), "3 steps + prefill(5)")


def test_scored_prefill_against_scoring_by_steps(tiny):
    """tests/test_gpu_prefill_scored.py's tolerance: lp = z_t - logsumexp(z) moves by at most
    2 max |dz| between the two runs' logits rows, plus both kernels' own error."""
    import logprob_ref as L
    ids = np.concatenate([tiny["prompt"], tiny[4]["tokens"]])
    n = len(ids)
    with _engine(tiny) as e:
        e.set_logprobs(0)
        by_steps, rows_steps = [], []
        e.set_prompt(ids)
        for p in range(n - 1):
            e.decode(1, use_graph=False)
            rows_steps.append(e.logits().copy())
        by_steps = e.logprobs(n)[0][1:]
        got = e.score(ids, prefill=True)
        rows_pf = [e.scored_logits(p) for p in range(n - 1)]
        again = e.score(ids, prefill=False)
    np.testing.assert_array_equal(_bits(again), _bits(by_steps))
    assert got.shape == (n - 1,) and np.isfinite(got).all()
    for p in range(n - 1):
        zs, zd = rows_pf[p].astype(np.float64), rows_steps[p].astype(np.float64)
        assert _rel(zs, zd) < LOGIT_TOL, (p, _rel(zs, zd))
        bound = 2.0 * np.abs(zs - zd).max() + L.tolerance(len(zs), got[p]) + L.tolerance(len(zs), by_steps[p])
        assert abs(float(got[p]) - float(by_steps[p])) <= bound, (p, got[p], by_steps[p], bound)


def test_fp8_lo_mode_falls_back_as_for_an_fp32_cache():
    """exact=2 (fp16 hi + e4m3 lo planes) needs the fp16 cache's MFMA attention: at the 7B width,
    where an fp16-KV engine takes it, the int8-KV engine runs the exact planes instead, bitwise."""
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-7b", layers=1, max_seq=64, kv_dtype=llmi.I8)
    prompt = synth_prompt(5, 24, cfg.vocab)
    outs = []
    with Engine(cfg) as e:
        e.load_synthetic(2)
        for exact in (1, 2):
            outs.append((e.generate(prompt, 4, prefill=True, exact=exact), e.logits().copy(),
                         e.kv_slot_q8(0, 23), e.kv_slot_q8(0, 11, True)))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
    for a, b in zip(outs[0][2] + outs[0][3], outs[1][2] + outs[1][3]):
        np.testing.assert_array_equal(a, b)
