"""Operator-level parity for the prefill path's own kernels, launched directly through the test
hooks llmi_debug_prefill_attn / llmi_debug_rows_split / llmi_debug_w8_prepare and compared with
float64 numpy on the same inputs: the rope + cache write, the scalar and the MFMA causal
attention (split-key partials and every merge instance, the lazy softmax rescale, the three
output formats, P = 1 and P = 2), the fp16 plane split of the GEMM activations and the fp8
weight copy. head_dim 128, max_seq <= 1024, (heads, kv_heads) in {(4,4), (12,4), (8,2)}: 12 and 4
heads leave workgroups of the XCD-interleaved grid without work.

Bars, and where each comes from:
  rotated q and the fp32 K against the float64 rotation: rel-L2 < 2e-6, the project's RoPE bar
    (test_gpu_ops.py). fp16 K: every element within one fp16 ulp of fp16(float64 value) and at
    most 0.5 % unequal (the double rounding fp32 -> fp16 flips a last bit on a fraction
    ~2^-13 x 2 of elements; the plain fp32 expression restated in numpy is held to the same cap
    on the test's inputs, so the cap is not taken from the kernel). V, the untouched cache slots,
    the untouched k / v columns of qkv: bitwise.
  attention against float64 causal softmax attention of the GPU's own read-back rotated q and
    cache (stage A's rounding stays out): the maximum over (row, head) of the rel-L2 over the
    128 outputs < 2e-6, the project's attention bar -- one bad row is not diluted. Scalar kernel
    and MFMA P = 2 alike (two fp16 planes carry 22 bits of q and of p; K, V are exact fp16).
  split against unsplit keys: <= 1e-5, the project's reassociation bar (BAR_KPAR); two
    identical launches: bitwise.
  MFMA P = 1: overall rel-L2 <= 2 x the error of a numpy model of the same float64 attention
    that rounds q log2(e)/sqrt(128) and p = 2^(s - m) to fp16 with m raised by the kTau = 8 rule
    per 32-key half (the model is computed here; 1.6e-4 .. 3.0e-4 on these inputs, and the
    kernel measured within 1 % of it). The factor 2 covers the fp32 accumulation and exp2 the
    model does not round.
  output planes: hi = fp16(v), lo = fp16(v - hi) bitwise; the e4m3 lo bytes as decoded values
    against torch.float8_e4m3fn (CPU) of clamp((v - hi) 2^12, +-448); v is the fp32 output of
    the same plan on the same inputs.
  range sweep (q 2^-j, K 2^j): max(2e-6, 2 x the error of a numpy hi/lo-plane model) -- the lo
    plane of q falls into fp16 subnormals from j ~ 3 on. Measured model / kernel: j = 0 1.5e-7 /
    2.4e-7, 3: 9.3e-7 / 9.7e-7, 6: 7.8e-6 / 7.8e-6, 10: 1.2e-4 / 1.2e-4 (no flush in hardware; the
    table is in DESIGN.md).
  crafted score shapes: the same 2e-6; the scores that carry a row are kept near 0 because fp32
    holds a score s to |s| 2^-24, a RELATIVE error of the weight after exp2 (see shaped_case).
  rows_split: the combined x bitwise against sequential fp32 adds in slice order; planes without
    gamma bitwise; with gamma hi + lo against float64 RMSNorm < 2e-6 (hi + the e4m3 lo:
    2e-6 + 2^-11 x 2^-4, the e4m3 half-ulp of a remainder below half an fp16 ulp).
  w8_prepare: the exponent exactly; the bytes as decoded values.
Every output buffer carries 64 sentinel elements behind its logical end, checked on every
read-back; logical parts start as NaN or a garbage pattern."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402

DEV = "cuda"
D = 128
BAR = 2e-6          # against float64 (the project's RoPE and attention bar)
BAR_KPAR = 1e-5     # split keys against the unsplit launch (the project's reassociation bar)
PAD = 64
KTAU = 8.0
PART = 64 * D + 2 * 64   # fp32 elements of one chunk's partial
LOG2E = 1.4426950408889634
HEADSETS = [(4, 4), (12, 4), (8, 2)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rowhead_err(out, ref, heads):
    """max over (row, head) of the rel-L2 over the head's 128 outputs."""
    o = np.asarray(out, np.float64).reshape(-1, heads, D)
    r = np.asarray(ref, np.float64).reshape(-1, heads, D)
    return float((np.linalg.norm(o - r, axis=2) / np.maximum(np.linalg.norm(r, axis=2), 1e-30)).max())


def report(group, what, r):
    print(f"[rel-L2] {group}: {what}: {r:.3e}")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_SENT = {torch.float32: (torch.int32, 0x7FC0BEEF),   # NaNs
         torch.float16: (torch.int16, 0x7EEF),
         torch.uint8: (torch.uint8, 0xA5)}


class Buf:
    """n elements + PAD sentinels. The logical part starts as `init` or as the sentinel pattern
    (a NaN for the float types); get() checks the sentinels."""

    def __init__(self, n, dtype=torch.float32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dtype)
        self.n = n
        if init is not None:
            self.t[:n] = T(np.asarray(init).reshape(-1))

    def get(self):
        torch.cuda.synchronize()
        assert (self.raw[self.n:].cpu().numpy() == self.pat).all(), "a store past the buffer's logical end"
        return self.t[:self.n].cpu().numpy().copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def f8_decode(b):
    return torch.from_numpy(np.ascontiguousarray(b, np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def f8_round(x):
    """decoded torch.float8_e4m3fn (CPU) of clamp(x, +-448); a NaN stays a NaN."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return torch.clamp(x, -448.0, 448.0).to(torch.float8_e4m3fn).float().numpy()


def lo8_ref(v, hi):
    return f8_round((v - hi.astype(np.float32)) * np.float32(4096.0))


# ------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def rope_tab(max_seq):
    """[max_seq][64] (cos, sin) pairs: the angle in float64, rounded to fp32."""
    ang = np.arange(max_seq, dtype=np.float64)[:, None] * (10000.0 ** (-np.arange(64, dtype=np.float64) / 64.0))[None]
    tab = np.stack([np.cos(ang), np.sin(ang)], axis=2).astype(np.float32)
    return tab


def rotate64(x, pos, tab, inverse=False):
    """float64 rotation of x [..., rows, n_heads, 128] (row i at position pos[i]) with the fp32 table."""
    c = tab[pos, :, 0].astype(np.float64)[:, None, :]
    s = tab[pos, :, 1].astype(np.float64)[:, None, :]
    if inverse:
        s = -s
    a0, a1 = x[..., :64], x[..., 64:]
    return np.concatenate([a0 * c - a1 * s, a1 * c + a0 * s], axis=-1)


class Case:
    """Host inputs of one launch: qkv (, qkv2) rows and the cache's starting contents."""

    def __init__(self, p0, m, heads, kvh, cache="f16", qkv2=False, seed=0, max_seq=None):
        rng = np.random.default_rng([seed, p0, m, heads])
        self.p0, self.m, self.heads, self.kvh, self.cache = p0, m, heads, kvh, cache
        self.max_seq = max_seq or (1024 if p0 + m > 256 else 256)
        self.ld = (heads + 2 * kvh) * D
        self.qkv = rng.standard_normal((m, self.ld)).astype(np.float32)
        self.qkv2 = (0.5 * rng.standard_normal((m, self.ld))).astype(np.float32) if qkv2 else None
        self.cdt = np.float16 if cache == "f16" else np.float32
        self.k0 = rng.standard_normal((kvh, self.max_seq, D)).astype(self.cdt)
        self.v0 = rng.standard_normal((kvh, self.max_seq, D)).astype(self.cdt)
        self.tab = rope_tab(self.max_seq)

    def summed(self):
        return self.qkv.astype(np.float64) + (0.0 if self.qkv2 is None else self.qkv2.astype(np.float64))


class Run:
    pass


def launch(ops, c, planes=0, split=None, fmt="f32", ws_floats=None):
    """One llmi_debug_prefill_attn launch on fresh device copies of c's inputs. split: None (no
    workspace), 0 (workspace, automatic chunks) or the key blocks per chunk. fmt: "f32", "planes"
    (out_hi + fp16 out_lo), "hi" (out_hi alone) or "lo8". Returns the read-back q rows, caches
    and outputs, sentinels checked, with the plan the library reported."""
    tdt = torch.float16 if c.cache == "f16" else torch.float32
    r = Run()
    qkv = Buf(c.m * c.ld, init=c.qkv)
    qkv2 = T(c.qkv2) if c.qkv2 is not None else None
    kc = Buf(c.k0.size, tdt, init=c.k0)
    vc = Buf(c.v0.size, tdt, init=c.v0)
    tab = T(c.tab)
    ldo = c.heads * D
    a = dict(qkv=qkv.t, qkv2=qkv2, k_cache=kc.t, v_cache=vc.t, cache_dtype=_lib.F16 if c.cache == "f16" else _lib.F32,
             max_seq=c.max_seq, m=c.m, p0=c.p0, heads=c.heads, kv_heads=c.kvh, rope_tab=tab, mfma_planes=planes)
    out = hi = lo = None
    if fmt == "f32":
        out = Buf(c.m * ldo)
        a["out"] = out.t
    else:
        hi = Buf(c.m * ldo, torch.float16)
        a["out_hi"] = hi.t
        if fmt == "planes":
            lo = Buf(c.m * ldo, torch.float16)
            a["out_lo"] = lo.t
        elif fmt == "lo8":
            lo = Buf(c.m * ldo * 2, torch.uint8)
            a.update(out_lo=lo.t, out_lo8=1)
    ws = None
    if split is not None:
        nqb = -(-c.m // 64)
        n = ws_floats if ws_floats is not None else c.heads * nqb * 8 * PART
        ws = Buf(n)                       # NaN: a partial that is read before it is written poisons the row
        a.update(split_ws=ws.t, split_ws_floats=n, chunk_blocks=split)
    r.plan = ops.debug_prefill_attn_plan(**a)
    ops.debug_prefill_attn(**a)
    full = qkv.get().reshape(c.m, c.ld)
    r.qkv = full
    r.q = full[:, :c.heads * D].reshape(c.m, c.heads, D)
    r.k = kc.get().reshape(c.k0.shape)
    r.v = vc.get().reshape(c.v0.shape)
    r.out = out.get().reshape(c.m, ldo) if out is not None else None
    r.hi = hi.get().reshape(c.m, ldo) if hi is not None else None
    r.lo = lo.get().reshape(c.m, -1) if lo is not None else None
    if ws is not None:
        ws.get()
    if qkv2 is not None:
        assert np.array_equal(bits(qkv2.cpu().numpy()), bits(c.qkv2)), "qkv2 was written"
    return r


def attn_ref(c, r):
    """float64 causal softmax attention from the read-back rotated q and cache -> [m, heads * 128]."""
    n = c.p0 + c.m
    g = c.heads // c.kvh
    out = np.empty((c.m, c.heads, D))
    pos = c.p0 + np.arange(c.m)
    mask = np.arange(n)[None, :] > pos[:, None]
    for h in range(c.heads):
        k = r.k[h // g, :n].astype(np.float64)
        v = r.v[h // g, :n].astype(np.float64)
        s = r.q[:, h].astype(np.float64) @ k.T / math.sqrt(D)
        s[mask] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out.reshape(c.m, c.heads * D)


def f16r(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def lazy_model(c, r, mode):
    """The MFMA kernel's softmax schedule in float64: per query row and 32-key half kp of every
    64-key block, p = 2^(s - m) with m raised only when the half's maximum exceeds it by more
    than kTau; the two halves' (O, m, l) combined at the end. mode "exact": nothing rounded (the
    schedule alone: returns the excesses too); "p1": q log2(e)/sqrt(d) and p rounded to fp16;
    "p2": both as hi + lo fp16 planes of their fp32 values.
    Returns (out [m, heads * 128], excess): excess lists, for every (row, half) step after the
    row's first visible one, (max score of the half - running reference, fired)."""
    n = c.p0 + c.m
    g = c.heads // c.kvh
    pos = c.p0 + np.arange(c.m)
    out = np.empty((c.m, c.heads, D))
    excess = []
    qs = np.float32(LOG2E) / np.sqrt(np.float32(D))

    def planes(x32):
        hi = x32.astype(np.float16)
        lo = (x32 - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64) + lo.astype(np.float64)

    for h in range(c.heads):
        k = r.k[h // g, :n].astype(np.float64)
        v = r.v[h // g, :n].astype(np.float64)
        q32 = r.q[:, h] * qs                                   # the kernel's fp32 product
        q = {"exact": lambda: r.q[:, h].astype(np.float64) * (LOG2E / math.sqrt(D)),
             "p1": lambda: f16r(q32), "p2": lambda: planes(q32)}[mode]()
        s_all = q @ k.T
        s_all[np.arange(n)[None, :] > pos[:, None]] = -np.inf
        O = np.zeros((2, c.m, D))
        mr = np.full((2, c.m), -np.inf)
        lr = np.zeros((2, c.m))
        for k0 in range(0, n, 32):
            kp = (k0 // 32) & 1
            s = s_all[:, k0:k0 + 32]
            mx = s.max(axis=1)
            seen = mr[kp] > -np.inf
            fire = mx > mr[kp] + KTAU
            if mode == "exact" and h == 0:
                vis = seen & (mx > -np.inf)
                excess += list(zip(mx[vis] - mr[kp][vis], fire[vis]))
            m_new = np.where(fire, mx, mr[kp])
            with np.errstate(invalid="ignore"):
                alpha = np.where(m_new == mr[kp], 1.0, np.exp2(mr[kp] - m_new))
            mr[kp] = m_new
            lr[kp] *= alpha
            O[kp] *= alpha[:, None]
            m_use = np.where(np.isneginf(mr[kp]), 0.0, mr[kp])
            p = np.exp2(s - m_use[:, None])
            lr[kp] += p.sum(axis=1)
            if mode == "p1":
                p = f16r(p)
            elif mode == "p2":
                p = planes(p.astype(np.float32))
            O[kp] += p @ v[k0:k0 + 32]
        M = np.maximum(mr[0], mr[1])
        w = np.exp2(mr - M[None])
        out[:, h] = (O * w[:, :, None]).sum(axis=0) / (lr * w).sum(axis=0)[:, None]
    return out.reshape(c.m, c.heads * D), excess


# ------------------------------------------------------------------ stage A: rope + cache write
def ulp_dist16(a, b):
    def key(x):
        u = bits(np.asarray(x, np.float16)).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)
    return np.abs(key(a) - key(b))


ROPE_CASES = [(0, 1), (0, 65), (20, 64), (500, 40)]
# 40 + 40 heads (Llama-2-13B): 1,280 k/q and 1,280 v work items over the write kernel's 1,024
# threads, so both of its loops take a second, partly filled pass
WIDE = (20, 3, 40, 40, 64)   # (p0, m, heads, kv_heads, max_seq)


def indexed_case(cases, i, hs):
    """(p0, m, heads, kv_heads, max_seq): cases[i] on head set hs, or WIDE for the index past the list."""
    if i == len(cases):
        return WIDE
    return cases[i] + HEADSETS[hs % 3] + (None,)


@pytest.mark.parametrize("cache", ["f16", "f32"])
@pytest.mark.parametrize("two", [False, True], ids=["qkv", "qkv+qkv2"])
@pytest.mark.parametrize("i", range(len(ROPE_CASES) + 1), ids=[f"p{p}m{m}" for p, m in ROPE_CASES] + ["p20m3h40"])
def test_rope_and_cache_write(ops, i, two, cache):
    """rope_kv_prefill_kernel<__half / float>, with and without the second summand."""
    p0, m, heads, kvh, max_seq = indexed_case(ROPE_CASES, i, i + two)
    c = Case(p0, m, heads, kvh, cache, qkv2=two, seed=1, max_seq=max_seq)
    r = launch(ops, c)
    pos = p0 + np.arange(m)
    x = c.summed()
    tag = f"p0={p0} m={m} heads={heads}/{kvh} {cache} qkv2={two}"
    q64 = rotate64(x[:, :heads * D].reshape(m, heads, D), pos, c.tab)
    k64 = rotate64(x[:, heads * D:(heads + kvh) * D].reshape(m, kvh, D), pos, c.tab)
    rq = rel(r.q, q64)
    report("rope", f"q {tag}", rq)
    assert rq < BAR, (tag, rq)
    kw = r.k[:, p0:p0 + m].transpose(1, 0, 2)           # [m, kvh, D]
    if cache == "f32":
        rk = rel(kw, k64)
        report("rope", f"K {tag}", rk)
        assert rk < BAR, (tag, rk)
    else:
        want = k64.astype(np.float16)
        # the plain fp32 expression, restated: it must itself meet the caps on these inputs
        x32 = c.qkv if c.qkv2 is None else c.qkv + c.qkv2
        a = x32[:, heads * D:(heads + kvh) * D].reshape(m, kvh, D)
        cs, sn = c.tab[pos, :, 0][:, None, :], c.tab[pos, :, 1][:, None, :]
        plain = np.concatenate([a[..., :64] * cs - a[..., 64:] * sn, a[..., 64:] * cs + a[..., :64] * sn], axis=-1)
        for name, got in (("restated fp32", plain.astype(np.float16)), ("kernel", kw)):
            d = ulp_dist16(got, want)
            frac = float((d != 0).mean())
            print(f"[ulp] rope: fp16 K {name} {tag}: max {int(d.max())} ulp, {100 * frac:.3f} % unequal of {d.size}")
            assert d.max() <= 1 and frac <= 0.005, (name, tag, int(d.max()), frac)
    # V: plain adds, bitwise
    x32 = c.qkv if c.qkv2 is None else c.qkv + c.qkv2
    v_want = x32[:, (heads + kvh) * D:].reshape(m, kvh, D).astype(c.cdt)
    assert np.array_equal(bits(r.v[:, p0:p0 + m].transpose(1, 0, 2)), bits(v_want)), tag
    # every other cache slot, and the k / v columns of qkv, bitwise untouched
    keep = np.ones(c.max_seq, bool)
    keep[p0:p0 + m] = False
    assert np.array_equal(bits(r.k[:, keep]), bits(c.k0[:, keep])), tag
    assert np.array_equal(bits(r.v[:, keep]), bits(c.v0[:, keep])), tag
    assert np.array_equal(bits(r.qkv[:, heads * D:]), bits(c.qkv[:, heads * D:])), tag


# ------------------------------------------------------------------ stage B: scalar kernel
SCALAR_CASES = [(0, 1), (0, 31), (0, 33), (20, 64), (500, 40)]


@pytest.mark.parametrize("cache", ["f16", "f32"])
@pytest.mark.parametrize("i", range(len(SCALAR_CASES) + 1), ids=[f"p{p}m{m}" for p, m in SCALAR_CASES] + ["p20m3h40"])
def test_scalar_attention(ops, i, cache):
    """attn_prefill_kernel<__half / float>: 32-row query blocks, 32-key chunks."""
    p0, m, heads, kvh, max_seq = indexed_case(SCALAR_CASES, i, i + (cache == "f32"))
    c = Case(p0, m, heads, kvh, cache, qkv2=bool(i & 1), seed=2, max_seq=max_seq)
    r = launch(ops, c)
    assert r.plan == (0, 1, -(-m // 32) * heads, 0), r.plan
    e = rowhead_err(r.out, attn_ref(c, r), heads)
    report("scalar attention", f"p0={p0} m={m} heads={heads}/{kvh} {cache}: max (row, head)", e)
    assert e < BAR, (p0, m, cache, e)


# ------------------------------------------------------------------ stage B: MFMA, P = 2
MFMA_CASES = [(0, 1, 0), (0, 63, 1), (0, 64, 2), (0, 65, 1), (0, 200, 1), (20, 64, 0), (31, 33, 2), (33, 64, 1),
              (500, 40, 2)]   # (p0, m, head set)


def need_floats(c, maxc):
    return c.heads * (-(-c.m // 64)) * maxc * PART


@pytest.mark.parametrize("p0,m,hs", MFMA_CASES, ids=[f"p{p}m{m}" for p, m, _ in MFMA_CASES])
def test_mfma_attention_p2(ops, p0, m, hs):
    """attn_prefill_tr_kernel<2> without a workspace, with the automatic chunking and with one
    key block per chunk (the merge kernel wherever a query block sees more than one key block)."""
    heads, kvh = HEADSETS[hs]
    c = Case(p0, m, heads, kvh, seed=3)
    base = launch(ops, c, planes=2)
    ref = attn_ref(c, base)
    nkb = [-(-(p0 + min(64 * q + 64, m)) // 64) for q in range(-(-m // 64))]
    assert base.plan == (max(nkb), 1, 8 * (-(-heads // 8)) * len(nkb), 0), base.plan
    for name, split in (("no workspace", None), ("automatic", 0), ("chunk_blocks 1", 1)):
        r = base if split is None else launch(ops, c, planes=2, split=split)
        assert np.array_equal(bits(r.q), bits(base.q)) and np.array_equal(bits(r.k), bits(base.k))
        e = rowhead_err(r.out, ref, heads)
        report("mfma P=2", f"p0={p0} m={m} heads={heads}/{kvh} {name} plan={r.plan}: max (row, head)", e)
        assert e < BAR, (p0, m, name, e)
        if split is not None:
            d = rowhead_err(r.out, base.out, heads)
            report("mfma P=2", f"p0={p0} m={m} {name} against unsplit", d)
            assert d <= BAR_KPAR, (p0, m, name, d)
        if split == 1:
            want_maxc = max(nkb) if max(nkb) <= 8 else 1
            assert r.plan[1] == want_maxc and r.plan[3] == {1: 0, 2: 2, 3: 4, 4: 4}.get(want_maxc, 8), r.plan
        again = launch(ops, c, planes=2, split=split)
        assert np.array_equal(bits(again.out), bits(r.out)), (p0, m, name, "two identical launches differ")


CHUNK_FORMS = [  # (name, p0, m, chunk_blocks, workspace floats: None = 8 slots / "need" / "short", expected (cb, maxc, slots))
    ("merge<2>", 64, 64, 1, None, (1, 2, 2)),
    ("merge<4>, 3 chunks", 128, 64, 1, None, (1, 3, 4)),
    ("merge<4>, 4 chunks", 192, 64, 1, None, (1, 4, 4)),
    ("merge<8>", 448, 64, 1, None, (1, 8, 8)),
    ("9 chunks: falls back to one", 512, 64, 1, None, (9, 1, 0)),
    ("3 chunks, the last short", 256, 64, 2, None, (2, 3, 4)),
    ("block 0 direct, block 1 merged", 0, 128, 1, None, (1, 2, 2)),
    ("chunk 1 masked for rows < 64", 20, 64, 1, None, (1, 2, 2)),
    ("workspace one float short: one chunk", 64, 64, 1, "short", (2, 1, 0)),
    ("workspace of exactly the need", 64, 64, 1, "need", (1, 2, 2)),
]


@pytest.mark.parametrize("name,p0,m,cbk,wsz,want", CHUNK_FORMS, ids=[f[0].split(":")[0].replace(" ", "_") for f in CHUNK_FORMS])
def test_mfma_chunk_forms(ops, name, p0, m, cbk, wsz, want):
    """Every merge instance and both fallbacks, each asserted through the plan hook to be the
    form it names (chunk_blocks fixes the plan whatever the CU count). The workspace starts as
    NaN and carries sentinels behind its end."""
    c = Case(p0, m, 4, 4, seed=4, max_seq=1024)
    ws = None
    if wsz is not None:
        ws = need_floats(c, 2) - (1 if wsz == "short" else 0)
    r = launch(ops, c, planes=2, split=cbk, ws_floats=ws)
    assert (r.plan[0], r.plan[1], r.plan[3]) == want, (name, r.plan)
    e = rowhead_err(r.out, attn_ref(c, r), 4)
    report("mfma chunks", f"{name} p0={p0} m={m} plan={r.plan}: max (row, head)", e)
    assert e < BAR, (name, e)
    d = rowhead_err(r.out, launch(ops, c, planes=2).out, 4)
    report("mfma chunks", f"{name} against unsplit", d)
    assert d <= BAR_KPAR, (name, d)


# ------------------------------------------------------------------ crafted score shapes
def shaped_case(p0, m, shape, seed=5, top=None):
    """heads 4: every rotated q row is g u + noise and rotated key j is a_j u + noise (u the
    unit vector along the rows' common component), so key j's score is t_j = a_j g / sqrt(128)
    log2(e) + a small jitter, in log2 units. The un-rotated rows go into qkv; history keys into
    the cache as they are. The largest t_j is `top` = 0: fp32 holds a score s to about
    |s| 2^-24, which exp2 turns into a RELATIVE error of the key's weight, so any fp32
    attention loses the 2e-6 bar once the scores that carry the row reach |s| ~ 25 (measured on
    both kernels); the shapes are about score DIFFERENCES, so the keys that carry a row sit
    near 0 and the ones far below weigh nothing. "one hot" keeps its 40 above keys at 0: the
    rows that see the hot key are carried by it alone, where a score error cancels in p / l."""
    c = Case(p0, m, 4, 4, seed=seed, max_seq=256 if p0 + m <= 256 else 1024)
    rng = np.random.default_rng([seed, 77, p0])
    n = p0 + m
    j = np.arange(n)
    # the kernel keeps one running maximum per (16 rows, key half kp of the 64-key blocks): a
    # wave's consecutive halves are 64 keys apart, so a slope of x per 32 keys is 2 x per step
    t = {"creep": 3.5 * (j // 32),               # + 7 a step: no rescale at 7, one at 14, ...
         "jump": 4.5 * (j // 32),                # + 9 a step: every block rescales
         "descending": -0.5 * j,                 # the maximum at key 0 (ten times the jitter a key apart)
         "one hot": np.where(j == n - 6, 40.0, 0.0)}[shape]
    t = t - t.max() + ((40.0 if shape == "one hot" else 0.0) if top is None else top)
    g = 4.0
    u = np.ones(D) / math.sqrt(D)
    a = t / (g * LOG2E / math.sqrt(D))
    pos = p0 + np.arange(m)
    q_rot = g * u[None, None, :] + 0.02 * rng.standard_normal((m, 4, D))
    k_rot = a[:, None, None] * u[None, None, :] + 0.1 * rng.standard_normal((n, 4, D))
    c.qkv[:, :4 * D] = rotate64(q_rot, pos, c.tab, inverse=True).reshape(m, -1).astype(np.float32)
    c.qkv[:, 4 * D:8 * D] = rotate64(k_rot[p0:], pos, c.tab, inverse=True).reshape(m, -1).astype(np.float32)
    c.k0[:, :p0] = k_rot[:p0].transpose(1, 0, 2).astype(np.float16)
    return c


def check_shape(shape, c, r):
    """The float64 scores of the read-back data are what the case claims (log2 units)."""
    _, ex = lazy_model(c, r, "exact")
    exc = np.array([e for e, _ in ex])
    fired = np.array([f for _, f in ex], bool)
    s = r.q[:, 0].astype(np.float64) @ r.k[0, :c.p0 + c.m].astype(np.float64).T * (LOG2E / math.sqrt(D))
    s[np.arange(c.p0 + c.m)[None, :] > (c.p0 + np.arange(c.m))[:, None]] = -np.inf
    if shape == "creep":
        quiet = exc[~fired]
        print(f"[shape] creep p0={c.p0}: largest excess without a rescale {quiet.max():.2f}, rescales {int(fired.sum())}")
        assert 6.0 < quiet.max() <= KTAU, quiet.max()
    elif shape == "jump":
        print(f"[shape] jump p0={c.p0}: smallest excess {exc.min():.2f} over {exc.size} steps")
        assert fired.all() and exc.size > 0 and exc.min() > KTAU, exc.min()
    elif shape == "descending":
        assert (s.argmax(axis=1) == 0).all() and not fired.any()
    else:
        hot = c.p0 + c.m - 6
        rows = c.p0 + np.arange(c.m) >= hot
        rest = np.delete(s[rows], hot, axis=1).max(axis=1)
        print(f"[shape] one hot p0={c.p0}: key {hot} leads by {float((s[rows, hot] - rest).min()):.2f} on {int(rows.sum())} rows")
        assert rows.sum() == 6 and (s[rows, hot] - rest >= 35.0).all() and hot >= c.p0


@pytest.mark.parametrize("p0,m", [(248, 8), (20, 64)])
@pytest.mark.parametrize("shape", ["creep", "jump", "descending", "one hot"])
def test_mfma_score_shapes_p2(ops, shape, p0, m):
    """The lazy running maximum: p near 256 with no rescale, a rescale in every block, none
    after the first, and one key that carries the whole row."""
    c = shaped_case(p0, m, shape)
    r = launch(ops, c, planes=2)
    check_shape(shape, c, r)
    e = rowhead_err(r.out, attn_ref(c, r), 4)
    report("mfma shapes P=2", f"{shape} p0={p0} m={m}: max (row, head)", e)
    assert e < BAR, (shape, p0, m, e)
    r1 = launch(ops, c, planes=2, split=1)
    d = rowhead_err(r1.out, attn_ref(c, r1), 4)
    report("mfma shapes P=2", f"{shape} p0={p0} m={m} chunk_blocks 1 plan={r1.plan}: max (row, head)", d)
    assert d < BAR, (shape, p0, m, d)


# ------------------------------------------------------------------ MFMA, P = 1
@pytest.mark.parametrize("p0,m,hs,shape", [(0, 65, 1, None), (20, 64, 0, None), (500, 40, 2, None), (248, 8, 0, "creep")],
                         ids=["p0m65", "p20m64", "p500m40", "creep"])
def test_mfma_attention_p1(ops, p0, m, hs, shape):
    """attn_prefill_tr_kernel<1>: the fp16 throughput mode against the fp16-rounding model."""
    heads, kvh = HEADSETS[hs]
    c = shaped_case(p0, m, shape) if shape else Case(p0, m, heads, kvh, seed=6)
    r = launch(ops, c, planes=1)
    ref = attn_ref(c, r)
    model = rel(lazy_model(c, r, "p1")[0], ref)
    e = rel(r.out, ref)
    report("mfma P=1", f"p0={p0} m={m} heads={heads}/{kvh} {shape or 'random'}: model {model:.3e}, kernel", e)
    assert model > 1e-5, model             # the model rounds to fp16: far above a float64 error, or it is broken
    assert e <= 2 * model, (p0, m, e, model)
    r1 = launch(ops, c, planes=1, split=1)
    e1 = rel(r1.out, ref)
    report("mfma P=1", f"p0={p0} m={m} chunk_blocks 1 plan={r1.plan}", e1)
    assert e1 <= 2 * model, (p0, m, e1, model)


# ------------------------------------------------------------------ output formats
@pytest.mark.parametrize("split", [None, 1], ids=["direct store", "merge kernel"])
def test_mfma_output_formats(ops, split):
    """fp16 planes and the e4m3 lo bytes from the same v as the fp32 output of the same plan:
    (0, 128) with one key block per chunk puts query block 0 through the attention kernel's
    store and block 1 through the merge kernel's."""
    c = Case(0 if split else 33, 128 if split else 64, 12, 4, seed=7)
    f = launch(ops, c, planes=2, split=split)
    assert f.plan[3] == (2 if split else 0), f.plan
    v = f.out
    hi_want = v.astype(np.float16)
    lo_want = (v - hi_want.astype(np.float32)).astype(np.float16)
    for fmt in ("hi", "planes", "lo8"):
        r = launch(ops, c, planes=2, split=split, fmt=fmt)
        assert r.plan == f.plan
        assert np.array_equal(bits(r.hi), bits(hi_want)), (fmt, "hi")
        if fmt == "planes":
            assert np.array_equal(bits(r.lo), bits(lo_want)), "lo"
        elif fmt == "lo8":
            ldo = c.heads * D
            assert np.array_equal(f8_decode(r.lo[:, :ldo]), lo8_ref(v, hi_want)), "e4m3 lo"
            assert (r.lo[:, ldo:] == 0xA5).all(), "the second half of a lo8 row was written"


# ------------------------------------------------------------------ range sweep
@pytest.mark.parametrize("j", [0, 3, 6, 10])
def test_mfma_p2_range_sweep(ops, j):
    """q 2^-j and K 2^j leave every score unchanged, but the lo plane of q log2(e)/sqrt(d) sinks
    into fp16 subnormals: the fp32-faithful claim has a range. Bar: max(2e-6, 2 x the numpy
    plane model's error)."""
    c = Case(20, 64, 4, 4, seed=8)
    sc = np.float32(2.0 ** j)
    c.qkv[:, :4 * D] /= sc
    c.qkv[:, 4 * D:8 * D] *= sc
    c.k0 = (c.k0.astype(np.float32) * sc).astype(np.float16)
    r = launch(ops, c, planes=2)
    ref = attn_ref(c, r)
    model = rel(lazy_model(c, r, "p2")[0], ref)
    e = rel(r.out, ref)
    qmax = float(np.abs(r.q).max())
    report("mfma P=2 range", f"j={j} max|q|={qmax:.3g}: plane model {model:.3e}, kernel", e)
    assert e <= max(BAR, 2 * model), (j, e, model)


# ------------------------------------------------------------------ rows_split
# (k, m, ksplit (None: no slab), gamma, lo, hi) -> the rows_split_kernel<NPT, KS, BS> instance
ROWS_SPLIT = [
    (4, 1, None, None, "f16", True),        # <1, 0, 1024>, no slab
    (1000, 3, None, "f16", "f16", True),    # <1, 0, 1024>
    (4096, 3, None, "f32", "lo8", True),    # <1, 0, 1024>
    (4096, 1, None, None, None, True),      # <1, 0, 1024>, hi alone
    (4100, 3, None, None, "f16", True),     # <5, 0>
    (5120, 1, None, "f16", "lo8", True),    # <5, 0>
    (5124, 3, None, "f32", "f16", True),    # <8, 0>
    (8192, 1, None, None, "lo8", True),     # <8, 0>
    (8192, 3, None, "f16", None, True),     # <8, 0>
    (4096, 3, 1, None, "f16", True),        # <1, 0, 1024>, runtime loop of 1
    (4096, 3, 2, "f16", "lo8", True),       # <1, 2, 1024>
    (4096, 1, 3, None, "f16", True),        # <1, 0, 1024>, runtime loop of 3
    (4096, 3, 8, None, "lo8", True),        # <1, 8, 1024>
    (1000, 1, 2, "f32", "f16", True),       # <1, 2, 1024>, a row tail
    (4, 3, 8, None, "f16", True),           # <1, 8, 1024>, one float4 a row
    (5120, 3, 2, None, "f16", True),        # <5, 2>
    (5120, 1, 8, "f16", "f16", True),       # <5, 8>
    (4100, 3, 3, None, "lo8", True),        # <5, 0>, runtime loop of 3
    (4100, 1, 1, "f32", "f16", True),       # <5, 0>, runtime loop of 1
    (5124, 3, 2, None, "f16", True),        # <8, 2>
    (8192, 3, 8, None, "f16", True),        # <8, 0>: ksplit 8 past 5 float4s a thread is the runtime loop
    (8192, 1, 3, "f16", "lo8", True),       # <8, 0>, runtime loop of 3
    (8192, 3, 2, "f32", "f16", True),       # <8, 2>
    (4096, 3, 2, None, None, False),        # <1, 2, 1024>, the combine alone
    (5120, 1, 8, None, None, False),        # <5, 8>, the combine alone
    (8192, 3, 8, None, None, False),        # <8, 0>, the combine alone
    (1000, 3, 3, None, None, False),        # <1, 0, 1024>, the combine alone
]
ROWS_SPLIT_PADDED = [(1000, 3, "f16"), (5124, 3, "lo8"), (8192, 1, "f16")]   # ldx = k + 8, ldh = k + 4, no slab


def rows_split_run(ops, k, m, ksplit, gdt, lo, hi, ldx=0, ldh=0, seed=0):
    rng = np.random.default_rng([11, k, m, ksplit or 0, seed])
    ldx, ldh = ldx or k, ldh or k
    x = rng.standard_normal((m, ldx)).astype(np.float32)
    slab = rng.standard_normal((ksplit, m, k)).astype(np.float32) if ksplit else None
    gamma = None if gdt is None else (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16 if gdt == "f16" else np.float32)
    xb = Buf(m * ldx, init=x)
    hb = Buf(m * ldh, torch.float16) if hi else None
    lb = None if lo is None else Buf(m * ldh * 2, torch.uint8) if lo == "lo8" else Buf(m * ldh, torch.float16)
    sl = T(slab) if ksplit else None
    ops.debug_rows_split(xb.t, m, k, hi=hb.t if hb else None, lo=lb.t if lb else None, ldx=ldx, ldh=ldh,
                         gamma=T(gamma) if gamma is not None else None, eps=1e-5, slab=sl, ksplit=ksplit or 0,
                         lo8=lo == "lo8")
    xo = xb.get().reshape(m, ldx)
    want = x[:, :k].copy()
    for s in range(ksplit or 0):
        want = want + slab[s]                                   # sequential fp32 adds, slice order
    assert np.array_equal(bits(xo[:, :k]), bits(want)), "x: not the slices added in order"
    assert np.array_equal(bits(xo[:, k:]), bits(x[:, k:])), "x padding written"
    if ksplit:
        assert np.array_equal(bits(sl.cpu().numpy()), bits(slab)), "the slab was written"
    if not hi:
        return None
    h = hb.get().reshape(m, ldh)
    assert (bits(h[:, k:]) == 0x7EEF).all(), "hi padding written"
    v64 = want.astype(np.float64)
    if gamma is not None:
        v64 = v64 / np.sqrt((v64 * v64).mean(axis=1, keepdims=True) + 1e-5) * gamma.astype(np.float64)
    got = h[:, :k].astype(np.float64)
    if gamma is None:
        hw = want.astype(np.float16)
        assert np.array_equal(bits(h[:, :k]), bits(hw)), "hi"
    if lo == "f16":
        l = lb.get().reshape(m, ldh)
        assert (bits(l[:, k:]) == 0x7EEF).all(), "lo padding written"
        got = got + l[:, :k].astype(np.float64)
        if gamma is None:
            assert np.array_equal(bits(l[:, :k]), bits((want - hw.astype(np.float32)).astype(np.float16))), "lo"
    elif lo == "lo8":
        l = lb.get().reshape(m, 2 * ldh)
        assert (l[:, k:] == 0xA5).all(), "lo8: bytes past the row's k written"
        dec = f8_decode(l[:, :k])
        got = got + dec.astype(np.float64) / 4096.0
        if gamma is None:
            assert np.array_equal(dec, lo8_ref(want, hw)), "e4m3 lo"
    return rel(got, v64)


@pytest.mark.parametrize("k,m,ksplit,gdt,lo,hi", ROWS_SPLIT,
                         ids=[f"k{k}m{m}ks{ks}g{g}lo{lo}{'' if hi else 'combine'}" for k, m, ks, g, lo, hi in ROWS_SPLIT])
def test_rows_split(ops, k, m, ksplit, gdt, lo, hi):
    """rows_split_kernel: each case's instance is listed beside it in ROWS_SPLIT (NPT from
    ceil(k / 4 / 256) -> 4 | 5 | 8, or the 1024-thread form up to k = 4096; KS = 2 always, KS = 8 up
    to NPT 5, else the runtime slice loop)."""
    r = rows_split_run(ops, k, m, ksplit, gdt, lo, hi)
    if r is None:
        return
    # hi alone is an fp16 rounding (2^-11 relative at most); hi + lo carries 22 bits
    bar = 2.0 ** -11 if lo is None else BAR + (2.0 ** -15 if lo == "lo8" else 0.0)
    report("rows_split", f"k={k} m={m} ksplit={ksplit} gamma={gdt} lo={lo}: hi + lo against float64", r)
    assert r < bar, (k, m, ksplit, gdt, lo, r)


@pytest.mark.parametrize("k,m,lo", ROWS_SPLIT_PADDED)
def test_rows_split_padded_rows(ops, k, m, lo):
    """ldx > k and ldh > k without a slab: the padding of x, hi and lo comes back untouched."""
    r = rows_split_run(ops, k, m, None, None, lo, True, ldx=k + 8, ldh=k + 4)
    assert r < BAR + (2.0 ** -15 if lo == "lo8" else 0.0), r


# ------------------------------------------------------------------ w8_prepare
def w8_exp_ref(w):
    amax = float(np.abs(w.astype(np.float64)).max())   # a NaN anywhere makes it a NaN
    if not (amax > 0 and math.isfinite(amax)):
        return 0
    e = math.floor(math.log2(448.0 / amax))
    while amax * 2.0 ** (e + 1) <= 448.0:
        e += 1
    while amax * 2.0 ** e > 448.0:
        e -= 1
    return e


@pytest.mark.parametrize("rows,cols", [(3, 8), (5, 136), (64, 4096)])
@pytest.mark.parametrize("content", ["random", "zeros", "65504", "exact", "nan"])
def test_w8_prepare(ops, rows, cols, content):
    """The exponent is the largest e with max |W| 2^e <= 448 (0 for a zero or non-finite
    maximum); the first cols bytes of each 2 cols-byte row are e4m3(clamp(W 2^e, +-448)) and
    the second half is untouched."""
    rng = np.random.default_rng([12, rows, cols])
    w = (0.05 * rng.standard_normal((rows, cols))).astype(np.float16)
    spot = (rows - 1, cols - 3)
    if content == "zeros":
        w[:] = 0
    elif content == "65504":
        w[spot] = -65504.0
    elif content == "exact":
        w = np.clip(w, -0.5, 0.5)
        w[spot] = 448.0 * 2.0 ** -9          # 0.875: e = 9 exactly, and the element lands on 448
    elif content == "nan":
        w[spot] = np.nan
    out = Buf(rows * cols * 2, torch.uint8)
    e = ops.debug_w8_prepare(T(w), out.t, rows, cols)
    want_e = w8_exp_ref(w)
    b = out.get().reshape(rows, 2 * cols)
    print(f"[w8] {rows}x{cols} {content}: exp {e} (expected {want_e})")
    assert e == want_e, (e, want_e)
    if content == "exact":
        assert e == 9
    if content == "65504":
        assert e == -8
    assert (b[:, cols:] == 0xA5).all(), "the second half of a row was written"
    want = f8_round(w.astype(np.float32) * np.float32(2.0 ** e))
    got = f8_decode(b[:, :cols])
    assert np.array_equal(got, want, equal_nan=True), int((got != want).sum())
    if content == "exact":
        assert got[spot] == 448.0


# ------------------------------------------------------------------ argument checks
def test_launchers_refuse_bad_arguments(ops):
    """The LLMI_REQUIRE branches of the three launchers through the hooks: each call must fail
    and launch nothing (every output still holds its starting pattern)."""
    c = Case(0, 8, 4, 4, "f32", seed=13)
    qkv, out = Buf(c.m * c.ld, init=c.qkv), Buf(c.m * 4 * D)
    kc, vc = Buf(c.k0.size, init=c.k0), Buf(c.v0.size, init=c.v0)
    hi = Buf(c.m * 4 * D, torch.float16)
    ok = dict(qkv=qkv.t, k_cache=kc.t, v_cache=vc.t, cache_dtype=_lib.F32, max_seq=c.max_seq, m=c.m, p0=0, heads=4,
              kv_heads=4, rope_tab=T(c.tab), out=out.t)
    for bad in (dict(heads=6), dict(heads=0), dict(kv_heads=0), dict(p0=c.max_seq - 4), dict(m=0), dict(p0=-1),
                dict(head_dim=64), dict(qkv=None), dict(rope_tab=None), dict(k_cache=None), dict(out=None),
                dict(mfma_planes=2), dict(mfma_planes=1, out=None, out_hi=hi.t),          # planes need the fp16 cache
                dict(cache_dtype=_lib.F16, mfma_planes=3), dict(cache_dtype=_lib.F16, mfma_planes=2, out=None),
                dict(cache_dtype=_lib.I8), dict(cache_dtype=7), dict(chunk_blocks=-1)):
        a = dict(ok, **bad)
        with pytest.raises(_lib.LlmiError):
            ops.debug_prefill_attn(**a)
        with pytest.raises(_lib.LlmiError):
            ops.debug_prefill_attn_plan(**a)
    assert np.array_equal(bits(qkv.get()), bits(c.qkv.reshape(-1)))
    assert np.array_equal(bits(kc.get()), bits(c.k0.reshape(-1))) and np.array_equal(bits(vc.get()), bits(c.v0.reshape(-1)))
    assert np.isnan(out.get()).all() and (bits(hi.get()) == 0x7EEF).all()

    x0 = np.arange(3 * 8200, dtype=np.float32)
    x, h, l = Buf(3 * 8200, init=x0), Buf(3 * 8200, torch.float16), Buf(3 * 8200, torch.float16)
    slab = torch.zeros(2 * 3 * 8200, device=DEV)
    for kw in (dict(k=8196), dict(k=1002), dict(k=1000, ldx=1002), dict(k=1000, ldh=1002), dict(k=1000, m=0),
               dict(k=1000, hi=None), dict(k=1000, ldx=1004, slab=slab, ksplit=2), dict(k=1000, slab=slab, ksplit=0)):
        a = dict(dict(m=3, hi=h.t, lo=l.t), **kw)
        with pytest.raises(_lib.LlmiError):
            ops.debug_rows_split(x.t, **a)
    assert np.array_equal(x.get(), x0) and (bits(h.get()) == 0x7EEF).all() and (bits(l.get()) == 0x7EEF).all()

    w = T(np.ones((4, 16), np.float16))
    b = Buf(4 * 32 + 16, torch.uint8)
    for kw in (dict(rows=4, cols=12), dict(rows=0, cols=16), dict(rows=4, cols=0)):
        with pytest.raises(_lib.LlmiError):
            ops.debug_w8_prepare(w, b.t, **kw)
    with pytest.raises(_lib.LlmiError):
        ops.debug_w8_prepare(w, b.t[8:], 4, 16)          # w8 not 16-B aligned
    assert (b.get() == 0xA5).all()
