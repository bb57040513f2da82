"""csrc/attn_gqa.hip through llmi_debug_attn_oproj with gqa = 1 (one workgroup per kv head and split
on the matrix cores, then the unchanged o_proj) against float64 attention + o_proj over the cache as
the launch left it: rel-L2 < 4e-6, the bar of tests/test_gpu_engine_kernels.py for this operator form.
Rows at and behind the position are NaN (int8: NaN scales) and the workspace is 0xFF bytes; caches and
scales must equal, byte for byte, what gqa = 0 leaves. max_seq 192, fp16 W_o [256, heads * 128]."""
import numpy as np
import pytest

import kv8_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import llama_ref as R  # noqa: E402

D, MAX_SEQ, N_ROWS, BAR, FX = 128, 192, 256, 4e-6, 2.0 ** 32
F16_NAN = 0x7E00


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
    return w.astype(np.float64) @ o.reshape(-1)


def run(heads, kvh, cache, pos, nact, gqa):
    """One launch on fresh buffers from the case's seed."""
    from llmi import ops
    rng = np.random.default_rng([heads, kvh, pos, cache == "i8"])
    qkv = rng.standard_normal((heads + 2 * kvh) * D).astype(np.float32)
    w = (0.05 * rng.standard_normal((N_ROWS, heads * D))).astype(np.float16)
    seed = rng.integers(-2 ** 40, 2 ** 40, N_ROWS)
    rows = [rng.standard_normal((kvh, MAX_SEQ, D)) * 2.0 ** rng.uniform(-2, 2, (kvh, MAX_SEQ, 1)) for _ in range(2)]
    if cache == "i8":
        bufs = []
        for x in rows:
            q8, sc = kv8_ref.quant_rows(x.astype(np.float32))
            q8[:, pos:] = rng.integers(-128, 128, q8[:, pos:].shape, dtype=np.int8)
            sc[:, pos:] = kv8_ref.NAN_BITS
            bufs += [q8.view(np.uint8), sc.view(np.int16)]
        kq, ks, vq, vs = bufs
    else:
        kq, vq = (x.astype(np.float16).view(np.int16) for x in rows)
        kq[:, pos:], vq[:, pos:] = F16_NAN, F16_NAN
        ks = vs = np.zeros((kvh, MAX_SEQ), np.int16)
    before = [a.copy() for a in (kq, ks, vq, vs)]
    dev = [T(a) for a in before]
    ws = ops.attn_workspace(heads, MAX_SEQ).fill_(255)
    xacc = torch.full((N_ROWS,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    err = T(np.zeros(1, np.int32))
    dt = _lib.I8 if cache == "i8" else _lib.F16
    ops.debug_attn_oproj(
        qkv=T(qkv), k_cache=dev[0], v_cache=dev[2], cache_dtype=dt, max_seq=MAX_SEQ,
        pos_dev=T(np.array([pos], np.int32)), nact=nact, heads=heads, kv_heads=kvh, rope=1, workspace=ws, xacc=xacc,
        resid_fixed=T(seed), resid_scale=1.0, w=T(w), w_dtype=_lib.F16, n_rows=N_ROWS, ldw=heads * D, err=err,
        k_scale=dev[1] if cache == "i8" else None, v_scale=dev[3] if cache == "i8" else None, gqa=gqa)
    torch.cuda.synchronize()
    after = [t.cpu().numpy() for t in dev]
    return xacc.cpu().numpy(), seed, int(err.cpu()[0]), before, after, w, qkv[:heads * D].reshape(heads, D)


@pytest.mark.parametrize("pos", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("cache", ["f16", "i8"])
@pytest.mark.parametrize("heads,kvh", [(4, 2), (6, 2), (8, 2), (8, 1)])
def test_attention_oproj_against_float64(heads, kvh, cache, pos):
    """The host-sized grid everywhere, the max_seq-sized grid beside it at pos 64 and 130."""
    twin = run(heads, kvh, cache, pos, pos // 64 + 1, gqa=0)[4]
    for nact in (pos // 64 + 1, 0) if pos in (64, 130) else (pos // 64 + 1,):
        xacc, seed, err, before, after, w, q = run(heads, kvh, cache, pos, nact, gqa=1)
        tag = f"heads={heads}/{kvh} cache={cache} pos={pos} nact={nact}"
        assert err == 0, tag
        for name, b, a, t in zip(("k", "k scale", "v", "v scale"), before, after, twin):
            assert np.array_equal(a, t), (tag, name, "differs from what gqa = 0 leaves")
            keep = np.arange(MAX_SEQ) != pos
            assert np.array_equal(a[:, keep], b[:, keep]), (tag, name, "a row other than pos was written")
        if cache == "i8":
            kc = kv8_ref.dequant(after[0].view(np.int8), after[1].view(np.uint16))
            vc = kv8_ref.dequant(after[2].view(np.int8), after[3].view(np.uint16))
        else:
            kc, vc = after[0].view(np.float16), after[2].view(np.float16)
        ref = reference(q, kc, vc, pos, w)
        got = (xacc - seed).astype(np.float64) / FX
        r = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        print(f"[rel-L2] gqa attn+o_proj: {tag}: {r:.3e}")
        assert r < BAR, (tag, r)  # (NaN fails too)


@pytest.mark.parametrize("heads,kvh,dt", [(4, 4, _lib.F16), (16, 1, _lib.F16), (4, 2, _lib.F32)],
                         ids=["mha", "group16", "f32cache"])
def test_unsupported_shapes_are_refused(heads, kvh, dt):
    """LLMI_EUNSUPPORTED (-2) and nothing launched: xacc keeps its pattern, the cache its bytes."""
    from llmi import ops
    xacc = torch.full((N_ROWS,), 7, dtype=torch.int64, device="cuda")
    cache_bytes = kvh * MAX_SEQ * D * (4 if dt == _lib.F32 else 2)
    kc, vc = (torch.full((cache_bytes,), 3, dtype=torch.uint8, device="cuda") for _ in range(2))
    with pytest.raises(_lib.LlmiError, match=r"failed \(-2\).*gqa"):
        ops.debug_attn_oproj(
            qkv=torch.zeros((heads + 2 * kvh) * D, device="cuda"), k_cache=kc, v_cache=vc,
            cache_dtype=dt, max_seq=MAX_SEQ, pos_dev=T(np.array([65], np.int32)),
            nact=2, heads=heads, kv_heads=kvh, rope=1, workspace=ops.attn_workspace(heads, MAX_SEQ), xacc=xacc,
            resid_fixed=torch.zeros(N_ROWS, dtype=torch.int64, device="cuda"), resid_scale=1.0,
            w=torch.zeros(N_ROWS * heads * D, dtype=torch.float16, device="cuda"), w_dtype=_lib.F16, n_rows=N_ROWS,
            ldw=heads * D, err=T(np.zeros(1, np.int32)), gqa=1)
    torch.cuda.synchronize()
    assert bool((xacc == 7).all()) and bool((kc == 3).all()) and bool((vc == 3).all())
