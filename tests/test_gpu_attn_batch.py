"""csrc/attn_batch.hip through llmi_debug_attn_oproj_batch: up to eight unrelated sequences, each with
its own cache, position, split count, workspace and xacc, in one attention launch and one o_proj
launch. Per slot: float64 attention + W_o over the cache as the launch left it (rel-L2 < 4e-6, the bar
of tests/test_gpu_engine_kernels.py and tests/test_gpu_attn_gqa.py for this operator form), and xacc,
live partials, cache and scale bytes bitwise those of llmi_debug_attn_oproj on that slot alone.
max_seq 192 (three splits), W_o [256, heads * 128] (two taller ones reach the o_proj's wider row maps);
rows at and behind a slot's position are NaN (int8: NaN scales), workspaces 0xFF bytes, xacc a pattern
the per-row seed must replace."""
import numpy as np
import pytest

import kv8_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import llama_ref as R  # noqa: E402

D, MAX_SEQ, NS, BAR, FX = 128, 192, 3, 4e-6, 2.0 ** 32
PATTERN = 0x5A5A5A5A5A5A5A5A
# split counts that differ inside one launch, a workgroup past a slot's nact, every slot of eight
POSITIONS = [(0, 130), (63, 64, 65), (130, 0, 64, 1, 65, 63, 129, 64)]
# (..., W_o dtype, W_o rows): 256 rows are one row per 16-lane group; 8192 and 32768 reach 2 and 8
CASES = [(p, hk, c, "f16", 256) for p in POSITIONS for hk in ((4, 4), (4, 2)) for c in ("f16", "f32", "i8")] + \
    [(POSITIONS[1], (4, 2), "i8", "i8", 256), (POSITIONS[0], (4, 4), "f16", "f32", 256),
     (POSITIONS[1], (4, 2), "f16", "f16", 8192), (POSITIONS[0], (4, 2), "i8", "i8", 32768)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def reference(q, kc, vc, pos, w):
    """float64: RoPE of q, softmax(q K^T / sqrt(d)) V over rows 0 .. pos, W_o; caches [kv_heads, max_seq, d]."""
    heads = q.shape[0]
    cos, sin = R.rope_cos_sin([pos], D, 10000.0)
    q = q.astype(np.float64)
    q = q * cos[0].astype(np.float64) + R.rotate_half(q) * sin[0].astype(np.float64)
    k = np.repeat(kc[:, :pos + 1].astype(np.float64), heads // kc.shape[0], axis=0)
    v = np.repeat(vc[:, :pos + 1].astype(np.float64), heads // vc.shape[0], axis=0)
    s = np.einsum("hd,hjd->hj", q, k) / np.sqrt(np.float64(D))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    o = np.einsum("hj,hjd->hd", p / p.sum(axis=-1, keepdims=True), v)
    return w @ o.reshape(-1)


def weights(rng, heads, wdt, n_rows=256):
    """(keywords of the W_o side, W_o as float64)."""
    w = 0.05 * rng.standard_normal((n_rows, heads * D))
    if wdt == "i8":
        q, sc = rng.integers(-127, 128, w.shape, dtype=np.int8), (2.0 ** rng.uniform(-12, -10, n_rows)).astype(np.float16)
        return dict(w=T(q), scales=T(sc), w_dtype=_lib.I8), q.astype(np.float64) * sc.astype(np.float64)[:, None]
    w = w.astype(np.float16 if wdt == "f16" else np.float32)
    return dict(w=T(w), w_dtype=_lib.F16 if wdt == "f16" else _lib.F32), w.astype(np.float64)


def slot(rng, heads, kvh, cache, pos, n_rows=256):
    """A sequence's host buffers: q/k/v row, residual seed, [k, k scale, v, v scale] as stored."""
    qkv = rng.standard_normal((heads + 2 * kvh) * D).astype(np.float32)
    seed = rng.integers(-2 ** 40, 2 ** 40, n_rows)
    rows = [rng.standard_normal((kvh, MAX_SEQ, D)) * 2.0 ** rng.uniform(-2, 2, (kvh, MAX_SEQ, 1)) for _ in range(2)]
    bufs = []
    for x in rows:
        if cache == "i8":
            q8, sc = kv8_ref.quant_rows(x.astype(np.float32))
            q8[:, pos:] = rng.integers(-128, 128, q8[:, pos:].shape, dtype=np.int8)
            sc[:, pos:] = kv8_ref.NAN_BITS
            bufs += [q8.view(np.uint8), sc.view(np.int16)]
        else:
            x = x.astype(np.float16 if cache == "f16" else np.float32)
            x[:, pos:] = np.nan
            bufs += [x.view(np.int16 if cache == "f16" else np.int32), np.zeros((kvh, MAX_SEQ), np.int16)]
    return dict(qkv=qkv, seed=seed, pos=pos, cache=bufs)


def prepare(slots, heads, kvh, cache, w_kw):
    """Fresh device buffers of every slot: (the launch's keyword dicts, the tensors to read back)."""
    from llmi import ops
    kws, outs = [], []
    for s in slots:
        dev = [T(a) for a in s["cache"]]
        outs.append((torch.full((len(s["seed"]),), PATTERN, dtype=torch.int64, device="cuda"), T(np.zeros(1, np.int32)),
                     ops.attn_workspace(heads, MAX_SEQ).fill_(255), dev))
        kws.append(dict(
            qkv=T(s["qkv"]), k_cache=dev[0], v_cache=dev[2], cache_dtype={"f16": _lib.F16, "f32": _lib.F32, "i8": _lib.I8}[cache],
            max_seq=MAX_SEQ, pos_dev=T(np.array([s["pos"]], np.int32)), nact=s["pos"] // 64 + 1, heads=heads, kv_heads=kvh,
            rope=1, workspace=outs[-1][2], xacc=outs[-1][0], resid_fixed=T(s["seed"]), n_rows=len(s["seed"]), ldw=heads * D,
            err=outs[-1][1], k_scale=dev[1] if cache == "i8" else None, v_scale=dev[3] if cache == "i8" else None, **w_kw))
    return kws, outs


def collect(outs, heads):
    """Per slot: xacc, err, the partials (m, l) and o as [heads, splits, ...] bits, the cache buffers."""
    torch.cuda.synchronize()
    got = []
    for xacc, err, ws, dev in outs:
        f = ws.cpu().numpy().view(np.uint32)[heads * 64:]  # (behind the per-head counter lines)
        got.append((xacc.cpu().numpy(), int(err.cpu()[0]), f[:heads * NS * 2].reshape(heads, NS, 2),
                    f[heads * NS * 2:].reshape(heads, NS, D), [t.cpu().numpy() for t in dev]))
    return got


@pytest.mark.parametrize("positions,hk,cache,wdt,n_rows", CASES)
def test_every_slot_against_float64_and_its_own_launch(positions, hk, cache, wdt, n_rows):
    from llmi import ops
    heads, kvh = hk
    rng = np.random.default_rng(CASES.index((positions, hk, cache, wdt, n_rows)))
    w_kw, w64 = weights(rng, heads, wdt, n_rows)
    slots = [slot(rng, heads, kvh, cache, p, n_rows) for p in positions]
    kws, outs = prepare(slots, heads, kvh, cache, w_kw)
    ops.debug_attn_oproj_batch(kws)
    batch = collect(outs, heads)
    for i, (s, (xacc, err, ml, o, after)) in enumerate(zip(slots, batch)):
        pos, nact = s["pos"], s["pos"] // 64 + 1
        tag = f"slot {i} of {len(slots)} pos={pos} heads={heads}/{kvh} cache={cache} w={wdt}x{n_rows}"
        assert err == 0, tag
        kw1, out1 = prepare([s], heads, kvh, cache, w_kw)
        ops.debug_attn_oproj(**kw1[0])
        xacc1, err1, ml1, o1, after1 = collect(out1, heads)[0]
        assert err1 == 0 and np.array_equal(xacc, xacc1), (tag, "xacc differs from the slot's own launch")
        assert np.array_equal(ml[:, :nact], ml1[:, :nact]) and np.array_equal(o[:, :nact], o1[:, :nact]), (tag, "partials")
        for name, b, a, a1 in zip(("k", "k scale", "v", "v scale"), s["cache"], after, after1):
            assert np.array_equal(a, a1), (tag, name, "differs from the slot's own launch")
            keep = np.arange(MAX_SEQ) != pos
            assert np.array_equal(a[:, keep], b[:, keep]), (tag, name, "a row other than pos was written")
        if cache == "i8":
            kc = kv8_ref.dequant(after[0].view(np.int8), after[1].view(np.uint16))
            vc = kv8_ref.dequant(after[2].view(np.int8), after[3].view(np.uint16))
        else:
            kc, vc = (after[j].view(np.float16 if cache == "f16" else np.float32) for j in (0, 2))
        ref = reference(s["qkv"][:heads * D].reshape(heads, D), kc, vc, pos, w64)
        r = float(np.linalg.norm((xacc - s["seed"]).astype(np.float64) / FX - ref) / np.linalg.norm(ref))
        print(f"[rel-L2] batched attn+o_proj: {tag}: {r:.3e}")
        assert r < BAR, (tag, r)  # (NaN fails too)


def test_slots_that_disagree_on_heads_are_refused():
    """LLMI_EINVAL (-1) and nothing launched: xacc keeps its pattern, the caches their bytes."""
    from llmi import ops
    rng = np.random.default_rng(7)
    w_kw, _ = weights(rng, 4, "f16")
    slots = [slot(rng, 4, 2, "f16", p) for p in (5, 70)]
    kws, outs = prepare(slots, 4, 2, "f16", w_kw)
    kws[1]["heads"] = 2
    with pytest.raises(_lib.LlmiError, match=r"failed \(-1\).*share"):
        ops.debug_attn_oproj_batch(kws)
    for s, (xacc, err, _, _, after) in zip(slots, collect(outs, 4)):
        assert (xacc == PATTERN).all() and all(np.array_equal(a, b) for a, b in zip(after, s["cache"]))
