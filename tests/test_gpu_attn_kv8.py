"""Decode attention over the int8 KV cache (KV8, include/llmi.h) through ops.attn_decode_q8, on
the MI355X: the output against the float64 attention over the dequantised cache, the row and the
scale the launch writes at `pos` against the numpy rule (tests/kv8_ref.py), and every other byte of
both layers unchanged.

Every row the context does not cover -- the rows past it, the slot at `pos` itself before the
launch, the whole other layer -- holds random bytes under a NaN scale (bits 0x7E00): a kernel that
multiplied an excluded row by a zero weight instead of selecting it out would return NaN.

OUT_TOL is tests/test_gpu_ops.py::_attn_case's 2e-6. The kernel applies a row's scale after its
integer sum (score = s_k * sum q_i k8_i; p * s_v folded before the P V FMAs); the measured
distance is printed by every case."""
import numpy as np
import pytest

import kv8_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

DEV = "cuda"
D, L, MAX_SEQ, LAYER = 128, 2, 256, 1
OUT_TOL = 2e-6
CTXS = [1, 2, 63, 64, 65, 129, 200, 256]
NAN_BITS = kv8_ref.NAN_BITS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def attention_f64(q, k_cache, v_cache, ctx):
    """R.attention_decode's arithmetic (modeling_llama.py:417-437) in float64."""
    heads, d = q.shape
    group = heads // k_cache.shape[0]
    k = np.repeat(k_cache[:, :ctx].astype(np.float64), group, axis=0)
    v = np.repeat(v_cache[:, :ctx].astype(np.float64), group, axis=0)
    s = np.einsum("hd,hjd->hj", q.astype(np.float64), k) / np.sqrt(np.float64(d))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return np.einsum("hj,hjd->hd", p / p.sum(axis=-1, keepdims=True), v)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _case(kv_heads, heads, ctx, seed=0):
    """Cache images (q int8, scale bits) with rows [0, ctx - 1) of LAYER real, the rest poison."""
    rng = np.random.default_rng(seed + 1000 * heads + ctx)
    pos = ctx - 1
    kq = rng.integers(-128, 128, (L, kv_heads, MAX_SEQ, D), dtype=np.int8)
    vq = rng.integers(-128, 128, (L, kv_heads, MAX_SEQ, D), dtype=np.int8)
    ks = np.full((L, kv_heads, MAX_SEQ), NAN_BITS, np.uint16)
    vs = np.full((L, kv_heads, MAX_SEQ), NAN_BITS, np.uint16)
    k = (rng.standard_normal((kv_heads, pos, D)) * 0.5).astype(np.float32)
    v = rng.standard_normal((kv_heads, pos, D)).astype(np.float32)
    kq[LAYER, :, :pos], ks[LAYER, :, :pos] = kv8_ref.quant_rows(k)
    vq[LAYER, :, :pos], vs[LAYER, :, :pos] = kv8_ref.quant_rows(v)
    qkv = rng.standard_normal((heads + 2 * kv_heads) * D).astype(np.float32)
    return dict(pos=pos, kq=kq, vq=vq, ks=ks, vs=vs, qkv=qkv)


def _launch(ops, c, heads, kv_heads, rope, repeat=1):
    dev = [T(c["kq"]), T(c["vq"]), T(c["ks"].view(np.float16)), T(c["vs"].view(np.float16))]
    ws = ops.attn_workspace(heads, MAX_SEQ)
    outs = [N(ops.attn_decode_q8(T(c["qkv"]), dev[0], dev[1], dev[2], dev[3], LAYER, c["pos"], heads, kv_heads, ws,
                                 rope=rope)) for _ in range(repeat)]
    kq, vq = N(dev[0]), N(dev[1])
    ks, vs = N(dev[2]).view(np.uint16), N(dev[3]).view(np.uint16)
    return outs, kq, vq, ks, vs


def _current_rows(c, heads, kv_heads, rope):
    qkv, pos = c["qkv"], c["pos"]
    q = qkv[:heads * D].reshape(heads, D)
    k = qkv[heads * D:(heads + kv_heads) * D].reshape(kv_heads, D)
    v = qkv[(heads + kv_heads) * D:].reshape(kv_heads, D)
    if rope:
        cos, sin = R.rope_cos_sin([pos], D, 10000.0)
        q, k = R.apply_rope(q, cos[0], sin[0]), R.apply_rope(k, cos[0], sin[0])
    return q, k.astype(np.float32), v.astype(np.float32)


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("heads,kv_heads", [(4, 4), (8, 2)])
def test_attn_decode_q8(ops, heads, kv_heads, ctx, rope):
    c = _case(kv_heads, heads, ctx)
    pos = c["pos"]
    (out,), kq, vq, ks, vs = _launch(ops, c, heads, kv_heads, rope)
    q, k, v = _current_rows(c, heads, kv_heads, rope)

    # ---- output: float64 attention over the dequantised cache, the current row as qdq
    kref = np.zeros((kv_heads, MAX_SEQ, D), np.float32)
    vref = np.zeros((kv_heads, MAX_SEQ, D), np.float32)
    kref[:, :pos] = kv8_ref.dequant(c["kq"][LAYER, :, :pos], c["ks"][LAYER, :, :pos])
    vref[:, :pos] = kv8_ref.dequant(c["vq"][LAYER, :, :pos], c["vs"][LAYER, :, :pos])
    kref[:, pos], vref[:, pos] = kv8_ref.qdq(k), kv8_ref.qdq(v)
    ref = attention_f64(q, kref, vref, ctx).reshape(-1)
    r = rel(out, ref)
    print(f"heads {heads} kv {kv_heads} ctx {ctx} rope {rope}: out rel-L2 {r:.3e}")
    assert np.isfinite(out).all()
    assert r < OUT_TOL, (heads, kv_heads, ctx, rope, r)

    # ---- the written row and scale
    wk, wks = kv8_ref.quant_rows(k)
    wv, wvs = kv8_ref.quant_rows(v)
    np.testing.assert_array_equal(vq[LAYER, :, pos], wv)
    np.testing.assert_array_equal(vs[LAYER, :, pos], wvs)
    if not rope:
        np.testing.assert_array_equal(kq[LAYER, :, pos], wk)
        np.testing.assert_array_equal(ks[LAYER, :, pos], wks)
    else:  # the fp32 rotation may contract differently: scale equal or adjacent, values within a step
        assert (np.abs(ks[LAYER, :, pos].astype(np.int32) - wks.astype(np.int32)) <= 1).all()
        got = kv8_ref.dequant(kq[LAYER, :, pos], ks[LAYER, :, pos])
        step = np.maximum(wks, ks[LAYER, :, pos]).view(np.float16).astype(np.float32)
        assert (np.abs(got - kv8_ref.dequant(wk, wks)) <= step[:, None]).all()

    # ---- nothing else changed, in either layer
    mask = np.ones((L, kv_heads, MAX_SEQ), bool)
    mask[LAYER, :, pos] = False
    np.testing.assert_array_equal(kq[mask], c["kq"][mask])
    np.testing.assert_array_equal(vq[mask], c["vq"][mask])
    np.testing.assert_array_equal(ks[mask], c["ks"][mask])
    np.testing.assert_array_equal(vs[mask], c["vs"][mask])


def test_infinity_in_v_writes_the_nan_scale(ops):
    heads, kv_heads, ctx = 4, 4, 65
    c = _case(kv_heads, heads, ctx, seed=7)
    c["qkv"][(heads + kv_heads) * D + D + 17] = np.inf  # kv head 1's v row
    (out,), kq, vq, ks, vs = _launch(ops, c, heads, kv_heads, False)
    pos = c["pos"]
    assert vs[LAYER, 1, pos] == NAN_BITS and (vq[LAYER, 1, pos] == 0).all()
    assert (vs[LAYER, [0, 2, 3], pos] != NAN_BITS).all() and (ks[LAYER, :, pos] != NAN_BITS).all()
    out = out.reshape(heads, D)
    assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2, 3]]).all()  # as with an fp16 cache


@pytest.mark.parametrize("ctx", [64, 200])
def test_repeated_launches_are_identical(ops, ctx):
    heads, kv_heads = 8, 2
    c = _case(kv_heads, heads, ctx, seed=3)
    outs, *_ = _launch(ops, c, heads, kv_heads, True, repeat=3)
    for o in outs[1:]:
        np.testing.assert_array_equal(o.view(np.uint32), outs[0].view(np.uint32))


def test_refusals(ops):
    from llmi._lib import LlmiError
    heads = kv_heads = 4
    c = _case(kv_heads, heads, 8)
    kq, vq = T(c["kq"]), T(c["vq"])
    ks, vs = T(c["ks"].view(np.float16)), T(c["vs"].view(np.float16))
    ws = ops.attn_workspace(heads, MAX_SEQ)
    with pytest.raises(TypeError):
        ops.attn_decode_q8(T(c["qkv"]), kq.to(torch.float16), vq, ks, vs, LAYER, 7, heads, kv_heads, ws)
    with pytest.raises(ValueError):
        ops.attn_decode_q8(T(c["qkv"]), kq, vq, ks[:, :, :8], vs, LAYER, 7, heads, kv_heads, ws)
    with pytest.raises(LlmiError):
        ops.attn_decode_q8(T(c["qkv"]), kq, vq, ks, vs, LAYER, MAX_SEQ, heads, kv_heads, ws)
    # the plain entry point takes no int8 cache (it has no scales to pass)
    with pytest.raises((LlmiError, KeyError)):
        ops.launchDecoderMaskedMHA(T(c["qkv"]), kq, vq, LAYER, 7, heads, kv_heads, ws)
    np.testing.assert_array_equal(N(kq), c["kq"])
