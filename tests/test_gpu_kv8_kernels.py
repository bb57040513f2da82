"""Operator-level parity for the int8 KV cache (KV8) in the three kernel forms an
int8-KV engine runs, launched directly through the test hooks llmi_debug_attn_oproj /
llmi_debug_prefill_attn with cache_dtype I8 and the two scale tensors, and compared with numpy:
  1. attn_decode_kernel<int8_t, HOST_SIZED> + o_proj: the engine's decode form (device position,
     a grid of nact splits, rows and scales loaded before the position arrives, partials only, xacc
     seeded, the o_proj launch merges), and the max_seq-sized grid beside it in every case;
  2. rope_kv_prefill_kernel<int8_t>: rotation, row maximum by a 16- (k) or 32-lane (v) butterfly,
     4 bytes a lane, the scale;
  3. attn_prefill_kernel<int8_t>: float(q) * s staged into LDS, 32-row query blocks, 32-key chunks.
head_dim 128; decode max_seq 256 (4 splits), (heads, kv_heads, o_proj rows) (4, 4, 512), (8, 2, 1024)
and once (32, 32, 4096); prefill max_seq <= 1024, m <= 65, (heads, kv_heads) in {(4,4), (12,4), (8,2)}
and once (40, 40) -- 1,280 k/q and 1,280 v work items over the write kernel's 1,024 threads, so both
of its loops take a second, partly filled pass.

Cache images (cache_image): the rows a launch may read -- rows < pos for decode, rows < p0 for
prefill -- are kv8_ref.quant_rows of random fp32 rows, K row j scaled by 0.5 x 2^u (u uniform in
[-2, 2]) and V row j by 2^u (u in [-3, 3]) per (kv head, row), so a scale taken from the wrong row,
the wrong kv head or the other cache is a gross error. Every other row -- the slot(s) the launch
writes, every row behind them up to max_seq -- holds random bytes under scale bits 0x7E00 (a NaN):
the engine's decode form preloads exactly those rows, and a kernel that weighted an excluded row by
zero instead of selecting it out would return NaN.

Bars, and where each comes from:
  attention + o_proj: (xacc - seed) 2^-32 against W_o in float64 applied to the float64 attention of
    the float64-rotated q over the GPU's own read-back, dequantised cache (the write's rounding
    stays out): rel-L2 < 4e-6 after an absolute allowance of heads x 2^-33 a row -- bar and
    allowance are test_gpu_engine_kernels.py's (the two stages' 2e-6 bars added; each head's
    product rounds to 2^-32 units once). q x s is exact in fp32, so from the unpacked value on the
    kernel runs the fp32 cache's arithmetic. Two launches over a workspace of 0xFF bytes: xacc bit
    for bit equal, err 0. With W_o = 0 xacc is exactly its seed.
  the row and scale written at pos (test_gpu_attn_kv8.py's rules): without RoPE the K bytes and
    scale bits are exactly kv8_ref.quant_rows of the fp32 row; with RoPE the scale bits are equal or
    adjacent and the dequantised values within one step of the reference's (the fp32 rotation may
    be contracted to an FMA); V always exact. Every other byte and scale of both caches, poison
    included, and the 64 sentinels behind all four buffers: unchanged.
  prefill write, identity (cos 1, sin 0) and quarter-turn (cos 0, sin 1) tables: the rotated row is
    exactly x, respectively (-x[64:], x[:64]), with or without FMA contraction, so the K bytes, K
    scale bits and the q columns left in qkv are bitwise; x = fp32(qkv + qkv2), the kernel's own add.
  prefill write, real table, against quant_rows(fp32(float64 rotation of x)): scale bits equal, or
    adjacent on at most 1 % of a case's rows; in rows with equal scale bits at most 0.1 % of the
    bytes differ, each by one; in rows with adjacent scale bits the dequantised values within one
    step; rotated q rel-L2 < 2e-6 (the project's RoPE bar). The caps are conditions, not
    measurements: tests/test_kv8_ref.py holds the plain and the FMA-contracted fp32 expression,
    restated in numpy, to them on these same inputs (write_caps is shared). V: bitwise
    quant_rows(x). Rows, scales, qkv's k / v columns and qkv2 outside the written range: bitwise.
  prefill attention: float64 causal softmax attention of the read-back rotated q and dequantised
    cache; the maximum over (row, head) of the rel-L2 over the head's 128 outputs < 2e-6, the
    project's attention bar, the measure of the fp16 / fp32 scalar test. Two launches: bitwise.
  refusals return LLMI_EINVAL (-1) and write nothing.

Measured maxima of the printed [rel-L2] lines on an MI355X (the bars are not taken from them):
  kv8 attn+o_proj ........... 4.2e-7 (the same before the allowance), at ctx 256, 4 heads
  kv8 rope (q, real table) .. 3.0e-8
  kv8 scalar attention ...... 1.8e-6 at (p0, m) = (500, 40), 12 / 4 heads (1.7e-6 on 8 / 2); every
                              other shape <= 1.5e-6. The fp32 cache measures 1.3e-6 at that shape with
                              unit-variance keys; here the K rows reach twice that amplitude and the
                              scores with them, and fp32 holds a score s to |s| 2^-24.
  real-table write .......... 0 rows with adjacent scale bits and 0 differing bytes in 42 launches
Every buffer a launch may write carries 64 sentinel elements behind its logical end, checked on
every read-back; outputs start as NaN / a garbage pattern."""
import functools
import math

import numpy as np
import pytest

import kv8_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import llama_ref as R  # noqa: E402
from oracle import prng  # noqa: E402

DEV = "cuda"
D = 128
BAR = 2e-6          # against float64 (the project's RoPE and attention bar)
BAR_AO = 4e-6       # attention + o_proj against float64 (test_gpu_engine_kernels.py)
PAD = 64
FX = 2.0 ** 32
NAN_BITS = kv8_ref.NAN_BITS
WDT = {"f16": _lib.F16, "f32": _lib.F32, "i8": _lib.I8}
TID = prng.layer_tid(0, prng.KIND_DOWN)
EINVAL = r"failed \(-1\)"

# the shapes of test_gpu_prefill_kernels.py, restated like the helpers: the modules stay independent
HEADSETS = [(4, 4), (12, 4), (8, 2)]
ROPE_CASES = [(0, 1), (0, 65), (20, 64), (500, 40)]
SCALAR_CASES = [(0, 1), (0, 31), (0, 33), (20, 64), (500, 40)]
WIDE = (20, 3, 40, 40, 64)   # (p0, m, heads, kv_heads, max_seq): a second pass of both write loops
TABLES = ["identity", "quarter", "real"]


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


def N(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


# kind -> (raw torch dtype, sentinel, torch dtype, numpy dtype read back, numpy dtype of the raw view)
_KIND = {"f32": (torch.int32, 0x7FC0BEEF, torch.float32, np.float32, np.int32),      # a NaN
         "i8": (torch.uint8, 0xA5, torch.int8, np.int8, np.uint8),
         "scale": (torch.int16, 0x7EEF, torch.float16, np.uint16, np.int16),          # fp16 as bits; a NaN
         "i64": (torch.int64, 0x5A5A5A5A5A5A5A5A, torch.int64, np.int64, np.int64)}


class Buf:
    """n elements + PAD sentinels. The logical part starts as `init` (copied as bits) or as the
    sentinel pattern; get() checks the sentinels and returns the logical part (scales as bits)."""

    def __init__(self, n, kind="f32", init=None):
        it, self.pat, dt, self.np_out, self.np_raw = _KIND[kind]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dt)
        self.n = n
        if init is not None:
            self.set(init)

    def set(self, init):
        self.raw[:self.n] = T(np.ascontiguousarray(init).reshape(-1).view(self.np_raw))

    def fill(self):
        self.raw[:self.n] = self.pat

    def get(self):
        torch.cuda.synchronize()
        assert (self.raw[self.n:].cpu().numpy() == self.pat).all(), "a store past the buffer's logical end"
        return self.raw[:self.n].cpu().numpy().view(self.np_out).copy()

    def untouched(self):
        return bool((self.raw.cpu().numpy() == self.pat).all())


# ------------------------------------------------------------------ cache images (no GPU needed)
class Image:
    """kq, vq int8 [kv_heads, max_seq, 128]; ks, vs scale bits uint16 [kv_heads, max_seq]; n_real."""


def cache_image(rng, kvh, max_seq, n_real):
    """Rows [0, n_real) of every kv head: quant_rows of random rows of per-row amplitude; every
    other row: random bytes under a NaN scale."""
    im = Image()
    im.n_real = n_real
    im.kq = rng.integers(-128, 128, (kvh, max_seq, D), dtype=np.int8)
    im.vq = rng.integers(-128, 128, (kvh, max_seq, D), dtype=np.int8)
    im.ks = np.full((kvh, max_seq), NAN_BITS, np.uint16)
    im.vs = np.full((kvh, max_seq), NAN_BITS, np.uint16)
    k = rng.standard_normal((kvh, n_real, D)) * (0.5 * 2.0 ** rng.uniform(-2, 2, (kvh, n_real, 1)))
    v = rng.standard_normal((kvh, n_real, D)) * 2.0 ** rng.uniform(-3, 3, (kvh, n_real, 1))
    im.kq[:, :n_real], im.ks[:, :n_real] = kv8_ref.quant_rows(k.astype(np.float32))
    im.vq[:, :n_real], im.vs[:, :n_real] = kv8_ref.quant_rows(v.astype(np.float32))
    return im


def decode_image(heads, kvh, ctx, rope, seed=0, max_seq=256):
    """(image with rows < ctx - 1 real, the qkv row of the token at ctx - 1, the case's generator)."""
    rng = np.random.default_rng([seed, heads, kvh, ctx, int(rope)])
    im = cache_image(rng, kvh, max_seq, ctx - 1)
    qkv = rng.standard_normal((heads + 2 * kvh) * D).astype(np.float32)
    return im, qkv, rng


@functools.lru_cache(maxsize=None)
def rope_tab(max_seq, kind="real"):
    """[max_seq][64] (cos, sin) pairs. real: the angle in float64, rounded to fp32 (the prefill
    module's table); identity: (1, 0) and quarter: (0, 1) at every position."""
    if kind == "real":
        ang = np.arange(max_seq, dtype=np.float64)[:, None] * (10000.0 ** (-np.arange(64, dtype=np.float64) / 64.0))[None]
        return np.stack([np.cos(ang), np.sin(ang)], axis=2).astype(np.float32)
    tab = np.zeros((max_seq, 64, 2), np.float32)
    tab[:, :, 0 if kind == "identity" else 1] = 1.0
    return tab


def rotate64(x, pos, tab):
    """float64 rotation of x [rows, n_heads, 128] (row i at position pos[i]) with the fp32 table."""
    c = tab[pos, :, 0].astype(np.float64)[:, None, :]
    s = tab[pos, :, 1].astype(np.float64)[:, None, :]
    a0, a1 = np.asarray(x[..., :64], np.float64), np.asarray(x[..., 64:], np.float64)
    return np.concatenate([a0 * c - a1 * s, a1 * c + a0 * s], axis=-1)


class Case8:
    """Host inputs of one prefill launch over an int8 cache: qkv (, qkv2) rows from the prefill
    module's distribution, the rope table and the cache image with rows < p0 real."""

    def __init__(self, p0, m, heads, kvh, qkv2=False, table="real", seed=0, max_seq=None):
        rng = np.random.default_rng([seed, p0, m, heads, kvh, int(qkv2)])
        self.p0, self.m, self.heads, self.kvh, self.table = p0, m, heads, kvh, table
        self.max_seq = max_seq or (1024 if p0 + m > 256 else 256)
        self.ld = (heads + 2 * kvh) * D
        self.qkv = rng.standard_normal((m, self.ld)).astype(np.float32)
        self.qkv2 = (0.5 * rng.standard_normal((m, self.ld))).astype(np.float32) if qkv2 else None
        self.img = cache_image(rng, kvh, self.max_seq, p0)
        self.tab = rope_tab(self.max_seq, table)
        self.pos = p0 + np.arange(m)
        self.tag = f"p0={p0} m={m} heads={heads}/{kvh} qkv2={qkv2} table={table}"

    def x32(self):
        """fp32(qkv + qkv2): the kernel's own add, the row every reference starts from."""
        return self.qkv if self.qkv2 is None else self.qkv + self.qkv2

    def parts(self):
        """(q [m, heads, 128], k [m, kvh, 128], v [m, kvh, 128]) of x32."""
        x, h, g = self.x32(), self.heads, self.kvh
        return (x[:, :h * D].reshape(self.m, h, D), x[:, h * D:(h + g) * D].reshape(self.m, g, D),
                x[:, (h + g) * D:].reshape(self.m, g, D))

    def exact_rotation(self, x):
        """The rotated rows where the table makes them exact in fp32 (None for the real table)."""
        if self.table == "identity":
            return x.copy()
        if self.table == "quarter":
            return np.concatenate([-x[..., 64:], x[..., :64]], axis=-1)
        return None


def write_cases():
    """(p0, m, heads, kv_heads, qkv2, max_seq) of every prefill-write case, whatever the table."""
    out = [(p0, m, h, g, two, None) for p0, m in ROPE_CASES for h, g in HEADSETS for two in (False, True)]
    return out + [WIDE[:4] + (False, WIDE[4])]


ATTN_CASES = [(p0, m, h, g, None) for p0, m in SCALAR_CASES for h, g in HEADSETS] + [WIDE]


def attn_case(n):
    """The n-th prefill-attention case: the real table, qkv2 on every second one."""
    p0, m, heads, kvh, max_seq = ATTN_CASES[n]
    return Case8(p0, m, heads, kvh, qkv2=bool(n & 1), seed=2, max_seq=max_seq)


def non_finite_case():
    """(20, 64) on 12 / 4 heads with +inf in kv head 1's v row of prompt row 5."""
    c = Case8(20, 64, 12, 4, seed=4)
    c.qkv[5, (12 + 4 + 1) * D + 17] = np.inf
    return c


def real_table_cases():
    """Every real-table case a test of this module launches (the write caps apply to each)."""
    for p0, m, heads, kvh, two, max_seq in write_cases():
        yield Case8(p0, m, heads, kvh, qkv2=two, table="real", max_seq=max_seq)
    for n in range(len(ATTN_CASES)):
        yield attn_case(n)
    yield non_finite_case()


def write_caps(got_q, got_s, want_q, want_s, tag=""):
    """The real-table conditions on a case's written K rows (module docstring); returns the
    figures (rows with adjacent scale bits, differing bytes in the other rows)."""
    got_s, want_s = np.asarray(got_s, np.uint16), np.asarray(want_s, np.uint16)
    ds = np.abs(got_s.astype(np.int32) - want_s.astype(np.int32))
    assert ds.max() <= 1, (tag, "scale bits further than adjacent", int(ds.max()))
    adj = ds == 1
    assert adj.sum() <= 0.01 * adj.size, (tag, "rows with adjacent scale bits", int(adj.sum()), adj.size)
    dq = np.abs(got_q.astype(np.int32) - want_q.astype(np.int32))[~adj]
    assert dq.max(initial=0) <= 1, (tag, "a byte differs by more than one", int(dq.max()))
    assert (dq != 0).sum() <= 0.001 * dq.size, (tag, "differing bytes", int((dq != 0).sum()), dq.size)
    if adj.any():
        step = np.maximum(got_s, want_s)[adj].view(np.float16).astype(np.float32)
        d = np.abs(kv8_ref.dequant(got_q[adj], got_s[adj]) - kv8_ref.dequant(want_q[adj], want_s[adj]))
        assert (d <= step[:, None]).all(), (tag, "adjacent scale: values further than one step")
    return int(adj.sum()), int((dq != 0).sum())


# ------------------------------------------------------------------ 1. decode + o_proj
def attention_f64(q, k_cache, v_cache, ctx):
    """softmax(q K^T / sqrt(d)) V in float64; q [heads, d], caches [kv_heads, >= ctx, d]."""
    heads, d = q.shape
    group = heads // k_cache.shape[0]
    k = np.repeat(k_cache[:, :ctx].astype(np.float64), group, axis=0)
    v = np.repeat(v_cache[:, :ctx].astype(np.float64), group, axis=0)
    s = np.einsum("hd,hjd->hj", q.astype(np.float64), k) / np.sqrt(np.float64(d))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return np.einsum("hj,hjd->hd", p / p.sum(axis=-1, keepdims=True), v)


@functools.lru_cache(maxsize=4)
def host_wo(wdt, n_rows, cols):
    """(W_o [n_rows, cols] as stored, per-row fp16 scales or None) from the project's generator."""
    if wdt == "i8":
        return prng.int8_weight(11, TID, n_rows, cols), prng.int8_row_scale(11, TID, n_rows)
    return prng.linear_fp16(11, TID, n_rows, cols), None


def to_fixed(v):
    """kernels.h to_fixed: fp32 v * 2^32 (exact), rounded to nearest-even."""
    return np.rint(np.asarray(v, np.float32) * np.float32(FX)).astype(np.int64)


class Decode:
    """Device buffers and the argument block of one debug_attn_oproj case."""

    def __init__(self, ops, heads, kvh, n_rows, ctx, rope, wdt="f16", resid="fixed", zero_w=False, seed=0):
        self.heads, self.kvh, self.n_rows, self.ctx, self.pos, self.rope = heads, kvh, n_rows, ctx, ctx - 1, rope
        self.max_seq = 256
        self.img, self.qkv, rng = decode_image(heads, kvh, ctx, rope, seed, self.max_seq)
        cols = heads * D
        self.w, self.s = host_wo(wdt, n_rows, cols)
        if zero_w:
            self.w = np.zeros_like(self.w)
        res = rng.standard_normal(n_rows).astype(np.float32)
        resfx = rng.integers(-2 ** 40, 2 ** 40, n_rows)
        self.seedv = {"f32": to_fixed(res), "fixed": resfx, "zero": np.zeros(n_rows, np.int64)}[resid]
        im = self.img
        self.kc, self.vc = Buf(im.kq.size, "i8", im.kq), Buf(im.vq.size, "i8", im.vq)
        self.ks, self.vs = Buf(im.ks.size, "scale", im.ks), Buf(im.vs.size, "scale", im.vs)
        self.ws = ops.attn_workspace(heads, self.max_seq)
        self.xacc = Buf(n_rows, "i64")
        self.err = T(np.zeros(1, np.int32))
        self.args = dict(
            qkv=T(self.qkv), k_cache=self.kc.t, v_cache=self.vc.t, cache_dtype=_lib.I8, max_seq=self.max_seq,
            pos_dev=T(np.array([self.pos], np.int32)), heads=heads, kv_heads=kvh, rope=int(rope), workspace=self.ws,
            xacc=self.xacc.t, resid=T(res) if resid != "fixed" else None,
            resid_fixed=T(resfx) if resid == "fixed" else None, resid_scale=0.0 if resid == "zero" else 1.0,
            w=T(self.w), scales=None if self.s is None else T(self.s), w_dtype=WDT[wdt], n_rows=n_rows, ldw=cols,
            err=self.err, k_scale=self.ks.t, v_scale=self.vs.t)

    def reset(self):
        self.ws.fill_(255)   # NaN bit patterns: a stale split behind nact must not leak
        self.kc.set(self.img.kq), self.vc.set(self.img.vq)
        self.ks.set(self.img.ks), self.vs.set(self.img.vs)
        self.xacc.fill()

    def read(self):
        """(xacc, kq, ks, vq, vs) after a launch, every sentinel checked."""
        shp = self.img.kq.shape
        return (self.xacc.get(), self.kc.get().reshape(shp), self.ks.get().reshape(shp[:2]),
                self.vc.get().reshape(shp), self.vs.get().reshape(shp[:2]))

    def caches_untouched(self):
        _, kq, ks, vq, vs = self.read()
        im = self.img
        return all(np.array_equal(a, b) for a, b in ((kq, im.kq), (ks, im.ks), (vq, im.vq), (vs, im.vs)))


def decode_case(ops, heads, kvh, n_rows, ctx, rope, **kw):
    """Both grid forms, two launches each; returns the largest rel-L2 after the allowance."""
    c = Decode(ops, heads, kvh, n_rows, ctx, rope, **kw)
    im, pos = c.img, c.pos
    cols = heads * D
    q = c.qkv[:cols].reshape(heads, D)
    k = c.qkv[cols:cols + kvh * D].reshape(kvh, D)
    v = c.qkv[cols + kvh * D:].reshape(kvh, D)
    q64 = q.astype(np.float64)
    if rope:
        cos, sin = R.rope_cos_sin([pos], D, 10000.0)
        k = R.apply_rope(k, cos[0], sin[0])
        q64 = q64 * cos[0].astype(np.float64) + R.rotate_half(q64) * sin[0].astype(np.float64)
    wk, wks = kv8_ref.quant_rows(k)
    wv, wvs = kv8_ref.quant_rows(v)
    worst = 0.0
    for host_sized in (True, False):
        nact = pos // 64 + 1 if host_sized else 0
        tag = (f"heads={heads}/{kvh} rows={n_rows} ctx={ctx} rope={rope} nact={nact} "
               f"w={kw.get('wdt', 'f16')} resid={kw.get('resid', 'fixed')}")
        runs = []
        for _ in range(2):
            c.reset()
            ops.debug_attn_oproj(**dict(c.args, nact=nact))
            runs.append(c.read())
        for a, b in zip(*runs):
            assert np.array_equal(a, b), (tag, "two identical launches differ")
        assert int(N(c.err)[0]) == 0, tag
        xacc, kq, ks, vq, vs = runs[0]
        # ---- the written row and scale at pos: one per kv head
        assert (ks[:, pos] != NAN_BITS).all() and (vs[:, pos] != NAN_BITS).all(), tag
        np.testing.assert_array_equal(vq[:, pos], wv, tag)
        np.testing.assert_array_equal(vs[:, pos], wvs, tag)
        if not rope:
            np.testing.assert_array_equal(kq[:, pos], wk, tag)
            np.testing.assert_array_equal(ks[:, pos], wks, tag)
        else:  # the fp32 rotation may contract differently: scale equal or adjacent, values within a step
            assert (np.abs(ks[:, pos].astype(np.int32) - wks.astype(np.int32)) <= 1).all(), tag
            step = np.maximum(wks, ks[:, pos]).view(np.float16).astype(np.float32)
            got = kv8_ref.dequant(kq[:, pos], ks[:, pos])
            assert (np.abs(got - kv8_ref.dequant(wk, wks)) <= step[:, None]).all(), tag
        # ---- every other byte and scale of both caches, poison included
        keep = np.ones(c.max_seq, bool)
        keep[pos] = False
        for got, was in ((kq, im.kq), (ks, im.ks), (vq, im.vq), (vs, im.vs)):
            assert np.array_equal(got[:, keep], was[:, keep]), (tag, "a row other than pos was written")
        # ---- the output
        if kw.get("zero_w"):
            np.testing.assert_array_equal(xacc, c.seedv, tag)
            continue
        o = attention_f64(q64, kv8_ref.dequant(kq[:, :ctx], ks[:, :ctx]), kv8_ref.dequant(vq[:, :ctx], vs[:, :ctx]), ctx)
        ref = c.w.astype(np.float64) @ o.reshape(-1)
        if c.s is not None:
            ref = ref * c.s.astype(np.float64)
        got = (xacc - c.seedv).astype(np.float64) / FX
        e = np.maximum(np.abs(got - ref) - heads * 2.0 ** -33, 0.0)  # each head's product rounds to 2^-32 once
        r, raw = float(np.linalg.norm(e) / np.linalg.norm(ref)), rel(got, ref)
        report("kv8 attn+o_proj", f"{tag} (raw {raw:.3e})", r)
        assert r < BAR_AO, (tag, r, raw)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("rope", [False, True], ids=["norope", "rope"])
@pytest.mark.parametrize("ctx", [1, 2, 63, 64, 65, 129, 130, 200, 256])
@pytest.mark.parametrize("heads,kvh,n_rows", [(4, 4, 512), (8, 2, 1024)])
def test_decode_contexts_and_grid_forms(ops, heads, kvh, n_rows, ctx, rope):
    """attn_decode_kernel<int8_t, HOST_SIZED and not> + o_proj at the split edges of max_seq 256."""
    decode_case(ops, heads, kvh, n_rows, ctx, rope)


def test_decode_int8_w_o(ops):
    decode_case(ops, 8, 2, 1024, 130, True, wdt="i8")


def test_decode_32_heads(ops):
    """32 heads over 32, 4,096 rows: the two-heads-per-workgroup o_proj, 8 rows a group."""
    decode_case(ops, 32, 32, 4096, 130, True)


@pytest.mark.parametrize("resid", ["f32", "fixed", "zero"])
def test_decode_seeds_xacc_exactly(ops, resid):
    """W_o = 0: xacc is fixed(resid), resid_fixed itself, or zeros (resid_scale 0), exactly."""
    decode_case(ops, 4, 4, 512, 130, True, resid=resid, zero_w=True)
    decode_case(ops, 8, 2, 1024, 130, False, resid=resid, zero_w=True)


def test_decode_refusals(ops):
    """Null scales and a cache 4 bytes off an 8-byte boundary: LLMI_EINVAL, nothing written."""
    c = Decode(ops, 4, 4, 512, 130, True)
    n = c.img.kq.size
    off = [Buf(n + 8, "i8", np.concatenate([np.zeros(4, np.int8), im.reshape(-1), np.zeros(4, np.int8)]))
           for im in (c.img.kq, c.img.vq)]
    assert off[0].t.data_ptr() % 8 == 0 and off[1].t.data_ptr() % 8 == 0
    for nact in (3, 0):
        for bad in (dict(k_scale=None), dict(v_scale=None), dict(k_cache=off[0].t[4:4 + n]),
                    dict(v_cache=off[1].t[4:4 + n])):
            with pytest.raises(_lib.LlmiError, match=EINVAL):
                ops.debug_attn_oproj(**dict(c.args, nact=nact, **bad))
    assert c.xacc.untouched(), "a refused launch wrote xacc"
    assert c.caches_untouched(), "a refused launch wrote a cache or a scale"
    for b, im in zip(off, (c.img.kq, c.img.vq)):
        assert np.array_equal(b.get()[4:4 + n], im.reshape(-1))
    assert int(N(c.err)[0]) == 0


# ------------------------------------------------------------------ 2, 3. prefill launches
class Run:
    pass


def launch(ops, c, plan_only=False, **override):
    """One llmi_debug_prefill_attn launch on fresh device copies of c's inputs; the read-back q
    rows, caches (bytes and scale bits), output and plan, every sentinel checked."""
    im = c.img
    r = Run()
    qkv = Buf(c.m * c.ld, init=c.qkv)
    qkv2 = Buf(c.m * c.ld, init=c.qkv2) if c.qkv2 is not None else None
    kc, vc = Buf(im.kq.size, "i8", im.kq), Buf(im.vq.size, "i8", im.vq)
    ks, vs = Buf(im.ks.size, "scale", im.ks), Buf(im.vs.size, "scale", im.vs)
    out = Buf(c.m * c.heads * D)
    a = dict(qkv=qkv.t, qkv2=None if qkv2 is None else qkv2.t, k_cache=kc.t, v_cache=vc.t, cache_dtype=_lib.I8,
             max_seq=c.max_seq, m=c.m, p0=c.p0, heads=c.heads, kv_heads=c.kvh, rope_tab=T(c.tab), mfma_planes=0,
             out=out.t, k_scale=ks.t, v_scale=vs.t)
    a.update(override)
    r.plan = ops.debug_prefill_attn_plan(**a)
    if not plan_only:
        ops.debug_prefill_attn(**a)
    r.qkv = qkv.get().reshape(c.m, c.ld)
    r.q = r.qkv[:, :c.heads * D].reshape(c.m, c.heads, D)
    r.kq, r.vq = kc.get().reshape(im.kq.shape), vc.get().reshape(im.vq.shape)
    r.ks, r.vs = ks.get().reshape(im.ks.shape), vs.get().reshape(im.vs.shape)
    r.out = out.get().reshape(c.m, c.heads * D)
    r.qkv2 = None if qkv2 is None else qkv2.get().reshape(c.m, c.ld)
    return r


def written(c, a):
    """The rows a launch writes, [m, kv_heads, ...] from a cache array [kv_heads, max_seq, ...]."""
    return np.swapaxes(a[:, c.p0:c.p0 + c.m], 0, 1)


def check_untouched(c, r):
    """Every cache row and scale outside [p0, p0 + m), the k / v columns of qkv and all of qkv2."""
    im = c.img
    keep = np.ones(c.max_seq, bool)
    keep[c.p0:c.p0 + c.m] = False
    for got, was in ((r.kq, im.kq), (r.ks, im.ks), (r.vq, im.vq), (r.vs, im.vs)):
        assert np.array_equal(got[:, keep], was[:, keep]), (c.tag, "a row outside [p0, p0 + m) was written")
    assert np.array_equal(bits(r.qkv[:, c.heads * D:]), bits(c.qkv[:, c.heads * D:])), (c.tag, "qkv k / v columns")
    if c.qkv2 is not None:
        assert np.array_equal(bits(r.qkv2), bits(c.qkv2)), (c.tag, "qkv2 was written")


def check_write(c, r):
    """Section 2's assertions on one launch; returns (q rel-L2, adjacent-scale rows, differing bytes)."""
    q, k, v = c.parts()
    wv, wvs = kv8_ref.quant_rows(v)
    assert np.array_equal(written(c, r.vq), wv) and np.array_equal(written(c, r.vs), wvs), (c.tag, "V")
    exact = c.exact_rotation(k)
    fig = (0.0, 0, 0)
    if exact is not None:
        wk, wks = kv8_ref.quant_rows(exact)
        assert np.array_equal(written(c, r.ks), wks), (c.tag, "K scale bits")
        assert np.array_equal(written(c, r.kq), wk), (c.tag, "K bytes")
        assert np.array_equal(bits(r.q), bits(c.exact_rotation(q))), (c.tag, "rotated q")
    else:
        wk, wks = kv8_ref.quant_rows(rotate64(k, c.pos, c.tab).astype(np.float32))
        nadj, nbytes = write_caps(written(c, r.kq), written(c, r.ks), wk, wks, c.tag)
        rq = rel(r.q, rotate64(q, c.pos, c.tab))
        report("kv8 rope", f"q {c.tag}", rq)
        print(f"[bytes] kv8 write: K {c.tag}: {nadj} of {wks.size} rows with adjacent scale bits, "
              f"{nbytes} of {wk.size} bytes differ")
        assert rq < BAR, (c.tag, rq)
        fig = (rq, nadj, nbytes)
    check_untouched(c, r)
    return fig


def attn_ref(c, r, heads=None):
    """float64 causal softmax attention of the read-back rotated q and dequantised cache
    -> [m, heads * 128] (NaN in the heads not asked for)."""
    n = c.p0 + c.m
    g = c.heads // c.kvh
    kd = kv8_ref.dequant(r.kq[:, :n], r.ks[:, :n]).astype(np.float64)
    vd = kv8_ref.dequant(r.vq[:, :n], r.vs[:, :n]).astype(np.float64)
    out = np.full((c.m, c.heads, D), np.nan)
    mask = np.arange(n)[None, :] > c.pos[:, None]
    for h in (range(c.heads) if heads is None else heads):
        s = r.q[:, h].astype(np.float64) @ kd[h // g].T / math.sqrt(D)
        s[mask] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (p / p.sum(axis=1, keepdims=True)) @ vd[h // g]
    return out.reshape(c.m, c.heads * D)


# ------------------------------------------------------------------ 2. prefill write
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("i", range(len(ROPE_CASES)), ids=[f"p{p}m{m}" for p, m in ROPE_CASES])
def test_prefill_write(ops, i, table):
    """rope_kv_prefill_kernel<int8_t> over the three head sets, with and without qkv2."""
    p0, m = ROPE_CASES[i]
    for heads, kvh in HEADSETS:
        for two in (False, True):
            c = Case8(p0, m, heads, kvh, qkv2=two, table=table)
            check_write(c, launch(ops, c))


@pytest.mark.parametrize("table", TABLES)
def test_prefill_write_second_pass(ops, table):
    """40 + 40 heads: 1,280 k/q items and 1,280 v items over 1,024 threads."""
    p0, m, heads, kvh, max_seq = WIDE
    c = Case8(p0, m, heads, kvh, table=table, max_seq=max_seq)
    check_write(c, launch(ops, c))


EDGE_ROWS = {3: "zero", 17: "inf", 31: "nan", 40: "1e7", 63: "1e-9"}   # row of the m rows -> content


def plant_edge_rows(c, rng):
    """Overwrite kv head 1's k row and kv head 2's v row of the rows in EDGE_ROWS."""
    for row, what in EDGE_ROWS.items():
        for col0 in ((c.heads + 1) * D, (c.heads + c.kvh + 2) * D):
            x = rng.standard_normal(D).astype(np.float32)
            if what == "zero":
                x[:] = 0
            elif what == "inf":
                x[rng.integers(D)] = np.inf
            elif what == "nan":
                x[rng.integers(D)] = np.nan
            elif what == "1e7":
                x[5], x[77] = 1e7, -1e7
                x[6], x[78] = 9e6, -9e6
            else:
                x = (x / np.abs(x).max() * np.float32(1e-9)).astype(np.float32)
                x[11] = 1e-9
            c.qkv[row, col0:col0 + D] = x


def test_prefill_write_edge_rows(ops):
    """An all-zero row, +inf, NaN, amax 1e7 and amax 1e-9 among the 64 rows of an identity-table
    launch, in K and in V: each against quant_rows, the other rows of the launch unaffected (the
    whole written range is compared). Nothing is asserted about this launch's attention output."""
    c = Case8(20, 64, 12, 4, table="identity", seed=3)
    plant_edge_rows(c, np.random.default_rng(5))
    r = launch(ops, c)
    check_write(c, r)     # bitwise quant_rows of every written row, planted ones included
    want = {"zero": 0x0001, "inf": NAN_BITS, "nan": NAN_BITS, "1e7": 0x7BFF, "1e-9": 0x0001}
    for row, what in EDGE_ROWS.items():
        pos = c.p0 + row
        for q, s, kvh in ((r.kq, r.ks, 1), (r.vq, r.vs, 2)):
            assert s[kvh, pos] == want[what], (what, hex(s[kvh, pos]))
            if what == "1e7":
                assert q[kvh, pos, 5] == 127 and q[kvh, pos, 77] == -127 and q[kvh, pos, 6] == 127 and \
                    q[kvh, pos, 78] == -127 and np.abs(q[kvh, pos].astype(np.int32)).max() == 127
            else:
                assert (q[kvh, pos] == 0).all(), what
    # the neighbours of the planted rows are ordinary rows
    assert (r.ks[1, c.p0:c.p0 + c.m] == NAN_BITS).sum() == 2 and (r.vs[2, c.p0:c.p0 + c.m] == NAN_BITS).sum() == 2
    assert (r.ks[[0, 2, 3], c.p0:c.p0 + c.m] != NAN_BITS).all() and (r.vs[[0, 1, 3], c.p0:c.p0 + c.m] != NAN_BITS).all()


# ------------------------------------------------------------------ 3. prefill attention
@pytest.mark.parametrize("n", range(len(ATTN_CASES)),
                         ids=[f"p{p}m{m}h{h}kv{g}" for p, m, h, g, _ in ATTN_CASES])
def test_prefill_attention(ops, n):
    """attn_prefill_kernel<int8_t>: a history, up to three query blocks and 17 key chunks."""
    c = attn_case(n)
    m, heads = c.m, c.heads
    r = launch(ops, c)
    assert r.plan == (0, 1, -(-m // 32) * heads, 0), r.plan
    check_write(c, r)
    assert np.isfinite(r.out).all(), c.tag
    e = rowhead_err(r.out, attn_ref(c, r), heads)
    report("kv8 scalar attention", f"{c.tag}: max (row, head)", e)
    assert e < BAR, (c.tag, e)
    again = launch(ops, c)
    assert np.array_equal(bits(again.out), bits(r.out)), (c.tag, "two identical launches differ")
    assert np.array_equal(again.kq, r.kq) and np.array_equal(again.ks, r.ks)


def test_prefill_attention_non_finite_v_row(ops):
    """+inf in kv head 1's v row of prompt row 5: that row's scale is the NaN scale over zero
    bytes; the heads of the other kv heads stay finite and within the bar."""
    c = non_finite_case()
    heads, kvh = c.heads, c.kvh
    r = launch(ops, c)
    check_write(c, r)
    pos = c.p0 + 5
    assert r.vs[1, pos] == NAN_BITS and (r.vq[1, pos] == 0).all()
    assert (r.vs[:, c.p0:c.p0 + c.m] == NAN_BITS).sum() == 1 and (r.ks[:, c.p0:c.p0 + c.m] != NAN_BITS).all()
    g = heads // kvh
    others = [h for h in range(heads) if h // g != 1]
    out = r.out.reshape(c.m, heads, D)[:, others]
    assert np.isfinite(out).all()
    ref = attn_ref(c, r, heads=others).reshape(c.m, heads, D)[:, others]
    e = rowhead_err(out, ref, len(others))
    report("kv8 scalar attention", f"{c.tag} +inf in kv head 1's v: heads of the other kv heads", e)
    assert e < BAR, e


def test_prefill_refusals(ops):
    """The MFMA forms over an int8 cache, null scales, a cache 2 bytes off a 4-byte boundary:
    LLMI_EINVAL from the launcher and from the plan, nothing written."""
    c = Case8(0, 8, 4, 4, seed=6)
    im = c.img
    n = im.kq.size
    off = Buf(n + 4, "i8", np.concatenate([np.zeros(2, np.int8), im.kq.reshape(-1), np.zeros(2, np.int8)]))
    hi = Buf(c.m * c.heads * D, "scale")
    assert off.t.data_ptr() % 4 == 0
    for bad in (dict(mfma_planes=1), dict(mfma_planes=2), dict(mfma_planes=1, out=None, out_hi=hi.t),
                dict(k_scale=None), dict(v_scale=None), dict(k_cache=off.t[2:2 + n]), dict(v_cache=off.t[2:2 + n])):
        with pytest.raises(_lib.LlmiError, match=EINVAL):
            launch(ops, c, plan_only=True, **bad)
        qkv, out = Buf(c.m * c.ld, init=c.qkv), Buf(c.m * c.heads * D)
        kc, vc = Buf(n, "i8", im.kq), Buf(n, "i8", im.vq)
        ks, vs = Buf(im.ks.size, "scale", im.ks), Buf(im.vs.size, "scale", im.vs)
        a = dict(qkv=qkv.t, k_cache=kc.t, v_cache=vc.t, cache_dtype=_lib.I8, max_seq=c.max_seq, m=c.m, p0=c.p0,
                 heads=c.heads, kv_heads=c.kvh, rope_tab=T(c.tab), mfma_planes=0, out=out.t, k_scale=ks.t, v_scale=vs.t)
        with pytest.raises(_lib.LlmiError, match=EINVAL):
            ops.debug_prefill_attn(**dict(a, **bad))
        assert np.array_equal(bits(qkv.get()), bits(c.qkv.reshape(-1))), bad.keys()
        assert np.array_equal(kc.get(), im.kq.reshape(-1)) and np.array_equal(vc.get(), im.vq.reshape(-1))
        assert np.array_equal(ks.get(), im.ks.reshape(-1)) and np.array_equal(vs.get(), im.vs.reshape(-1))
        assert out.untouched() and hi.untouched()
        assert np.array_equal(off.get()[2:2 + n], im.kq.reshape(-1))
