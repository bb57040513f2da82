"""numpy restatement of the KV8 cache format (include/llmi.h, llmi_attn_decode_q8) and an oracle
that keeps its K/V rows in it.

A row x[128] in fp32 is stored as 128 int8 and one fp16 scale by the W8A16 rule of
tests/test_gpu_quantize.py's quant_ref on the row: s = fp16_rne(amax / 127) (zero -> bits 0x0001,
infinity -> 0x7BFF), q = clip(rint(x / s), -127, 127); a row holding a NaN or an infinity stores
scale bits 0x7E00 (NaN) and q = 0. A cached value is float(q) * float(s), exact in fp32."""
import numpy as np

from oracle import llama_ref as R

NAN_BITS = 0x7E00


def quant_rows(x):
    """x [..., d] fp32 -> (q int8 [..., d], scale bits uint16 [...])."""
    x = np.asarray(x, np.float32)
    bad = ~np.isfinite(x).all(axis=-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        amax = np.abs(np.where(bad[..., None], np.float32(0), x)).max(axis=-1).astype(np.float32)
        bits = (amax / np.float32(127.0)).astype(np.float32).astype(np.float16).view(np.uint16).copy()
        bits[bits == 0] = 1
        bits[bits == 0x7C00] = 0x7BFF
        sf = bits.view(np.float16).astype(np.float32)
        q = np.clip(np.rint((x / sf[..., None]).astype(np.float32)), -127, 127)
    q = np.where(bad[..., None], 0, q).astype(np.int8)
    bits[bad] = NAN_BITS
    return q, bits


def dequant(q, bits):
    """The cached values: float(q) * float(s), fp32."""
    s = np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(q).astype(np.float32) * s[..., None]).astype(np.float32)


def qdq(x):
    return dequant(*quant_rows(x))


class Kv8Oracle(R.LlamaOracle):
    """LlamaOracle whose two cache writes store qdq(k), qdq(v) into fp32 caches; every other line
    of the two methods is the oracle's own."""

    def __init__(self, cfg, **kw):
        super().__init__(cfg, kv_dtype=np.float32, **kw)

    def layer_forward(self, l, x, pos):
        c, W = self.cfg, self.layers[l]
        h = R.rmsnorm(x, W["attn_norm"], c.rms_eps)
        qkv = R.linear(h, W["qkv"])
        q = qkv[:c.q_rows].reshape(c.heads, c.head_dim)
        k = qkv[c.q_rows:c.q_rows + c.kv_rows].reshape(c.kv_heads, c.head_dim)
        v = qkv[c.q_rows + c.kv_rows:].reshape(c.kv_heads, c.head_dim)
        cos, sin = R.rope_cos_sin([pos], c.head_dim, c.rope_base)
        q = R.apply_rope(q, cos[0], sin[0])
        k = R.apply_rope(k, cos[0], sin[0])
        self.k_cache[l, :, pos] = qdq(k)
        self.v_cache[l, :, pos] = qdq(v)
        attn = R.attention_decode(q, self.k_cache[l], self.v_cache[l], pos + 1).reshape(-1)
        x = x + R.linear(attn, W["o"])
        h = R.rmsnorm(x, W["ffn_norm"], c.rms_eps)
        gu = R.linear(h, W["gate_up"])
        act = R.silu(gu[:c.inter]) * gu[c.inter:]
        return (x + R.linear(act, W["down"])).astype(np.float32)

    def prefill(self, ids, round_a=None):
        c = self.cfg
        ra = (lambda t: t) if round_a is None else round_a
        ids = np.asarray(ids)
        m, p0 = len(ids), self.pos
        X = self.embed[ids].astype(np.float32)
        cos, sin = R.rope_cos_sin(np.arange(p0, p0 + m), c.head_dim, c.rope_base)
        cos, sin = cos[:, None, :], sin[:, None, :]
        for l in range(c.layers):
            W = self.layers[l]
            qkv = R.linear(ra(R.rmsnorm(X, W["attn_norm"], c.rms_eps)), W["qkv"])
            q = qkv[:, :c.q_rows].reshape(m, c.heads, c.head_dim)
            k = qkv[:, c.q_rows:c.q_rows + c.kv_rows].reshape(m, c.kv_heads, c.head_dim)
            v = qkv[:, c.q_rows + c.kv_rows:].reshape(m, c.kv_heads, c.head_dim)
            q, k = R.apply_rope(q, cos, sin), R.apply_rope(k, cos, sin)
            self.k_cache[l, :, p0:p0 + m] = qdq(k.transpose(1, 0, 2))
            self.v_cache[l, :, p0:p0 + m] = qdq(v.transpose(1, 0, 2))
            attn = R.attention_prefill(q, self.k_cache[l], self.v_cache[l], p0).reshape(m, -1)
            X = X + R.linear(ra(attn), W["o"])
            gu = R.linear(ra(R.rmsnorm(X, W["ffn_norm"], c.rms_eps)), W["gate_up"])
            X = (X + R.linear(ra(R.silu(gu[:, :c.inter]) * gu[:, c.inter:]), W["down"])).astype(np.float32)
        self.pos = p0 + m
        self.last_hidden_rows = X
        self.last_hidden = X[-1]
        return R.linear(R.rmsnorm(X[-1], self.final_norm, c.rms_eps), self.lm_head)
