"""Operator-level parity for the kernel forms a decoded token runs: the decode GEMV's engine
variants (fixed-point x, split-K atomics, single-producer rows, seed hand-over, argmax keys,
K parts, row strides, every staging width and unroll) and the split-KV attention whose partials
the o_proj launch consumes, each launched directly through the test hooks llmi_debug_gemv /
llmi_debug_attn_oproj and compared with float64 numpy on the same inputs.

Bars: GEMV rel-L2 < 2e-6 (the project's bar for these kernels, test_gpu_ops.py); fixed-point
outputs are compared as int64 * 2^-32. Attention + o_proj: rel-L2 < 4e-6 (the two stages' 2e-6
bars added: first-order errors add) after an absolute allowance of heads * 2^-33 a row (each
head's product is rounded to 2^-32 units once). Bit-exact where the contract says "the same
integer" or a copy. Every output buffer carries 64 sentinel elements past its logical end that
must come back untouched; its logical part starts as NaN / a garbage pattern, so a row that
is never written fails the comparison too."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import llama_ref as R  # noqa: E402
from oracle import prng  # noqa: E402

DEV = "cuda"
BAR = 2e-6          # GEMV against float64
BAR_KPAR = 1e-5     # K-parted against the unsplit launch (the project's reassociation bar)
BAR_AO = 4e-6       # attention + o_proj against float64
PAD = 64            # sentinel elements behind every output buffer
FX = 2.0 ** 32
WDT = {"f16": _lib.F16, "f32": _lib.F32, "i8": _lib.I8}
STORE, ADD, SILU, ARGMAX, ATOMIC = range(5)
TID = prng.layer_tid(0, prng.KIND_DOWN)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmi import ops as O
    return O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def report(group, what, r):
    print(f"[rel-L2] {group}: {what}: {r:.3e}")


_SENT = {torch.float32: (torch.int32, 0x7FC0BEEF),            # a NaN
         torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A)}


class Buf:
    """An output buffer of n elements + PAD sentinels; get() checks the sentinels."""

    def __init__(self, n, dtype=torch.float32, init=None):
        it, self.pat = _SENT[dtype]
        self.raw = torch.full((n + PAD,), self.pat, dtype=it, device=DEV)
        self.t = self.raw.view(dtype)
        self.n = n
        if init is not None:
            self.t[:n] = T(np.asarray(init))

    def get(self):
        torch.cuda.synchronize()
        assert (self.raw[self.n:].cpu().numpy() == self.pat).all(), "a store past the buffer's logical end"
        return self.t[:self.n].cpu().numpy().copy()


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=6)
def host_w(wdt, n, k, seed=9):
    """(weights [n, k] as stored, per-row fp16 scales or None) from the project's generator."""
    if wdt == "i8":
        return prng.int8_weight(seed, TID, n, k), prng.int8_row_scale(seed, TID, n)
    w = prng.linear_fp16(seed, TID, n, k)
    return (w if wdt == "f16" else w.astype(np.float32)), None


def dev_w(w, ldw=0):
    """W on the device; ldw > k: rows padded with large finite values that must never be read."""
    if ldw:
        full = np.full((w.shape[0], ldw), 127 if w.dtype == np.int8 else 1e4, w.dtype)
        full[:, :w.shape[1]] = w
        w = full
    return T(w)


def make_gamma(rng, k, gdt):
    if gdt is None:
        return None
    return (1.0 + 0.1 * rng.standard_normal(k)).astype(np.float16 if gdt == "f16" else np.float32)


def to_fixed(v):
    """kernels.h to_fixed: fp32 v * 2^32 (exact), rounded to nearest-even."""
    return np.rint(np.asarray(v, np.float32) * np.float32(FX)).astype(np.int64)


def x_eff(x, gamma, eps=1e-5):
    x = np.asarray(x, np.float64)
    if gamma is None:
        return x
    return x * gamma.astype(np.float64) / np.sqrt(np.mean(x * x) + eps)


def acc_ref(w, s, xe):
    acc = w.astype(np.float64) @ xe
    return acc if s is None else acc * s.astype(np.float64)


def silu_ref(acc, po):
    g, u = acc[:po], acc[po:]
    return g / (1.0 + np.exp(-g)) * u


def wargs(wdt, w, s, ldw=0):
    d = dict(w=dev_w(w, ldw), w_dtype=WDT[wdt], n_rows=w.shape[0], k=w.shape[1], ldw=ldw)
    if s is not None:
        d["scales"] = T(s)
    return d


def gargs(gamma):
    if gamma is None:
        return {}
    return dict(gamma=T(gamma), g_dtype=_lib.F16 if gamma.dtype == np.float16 else _lib.F32, eps=1e-5)


def decode_key(key):
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


def run_store(ops, wdt, w, s, x, gamma, **extra):
    """One EPI_STORE launch -> (y, plan)."""
    y = Buf(w.shape[0])
    a = dict(wargs(wdt, w, s, extra.pop("ldw", 0)), x=T(x), y=y.t, epi=STORE, **gargs(gamma), **extra)
    plan = ops.debug_gemv_plan(**a)
    ops.debug_gemv(**a)
    return y.get(), plan


# ------------------------------------------------- staging width and unroll
def test_gemv_staging_widths_and_unrolls(ops):
    """fp16, 37 rows, store, with and without RMSNorm, at a K for every x-staging width
    {4, 5, 11, 14, strided} and every unroll {4, 5, 8}; K = 11008 (1376 chunks, unroll 8) and
    13824 (1728 chunks, unroll 4) leave masked slots in the last batch. The plans the library
    reports must cover both sets."""
    rng = np.random.default_rng(1)
    seen_x, seen_u = set(), set()
    worst = 0.0
    for k in (2048, 2560, 4096, 5120, 11008, 13824, 16384):
        w, s = host_w("f16", 37, k)
        x = rng.standard_normal(k).astype(np.float32)
        for gdt in (None, "f16"):
            gamma = make_gamma(rng, k, gdt)
            y, (grid, u, xpt) = run_store(ops, "f16", w, s, x, gamma)
            r = rel(y, acc_ref(w, s, x_eff(x, gamma)))
            report("staging/unroll", f"f16 k={k} norm={gdt} grid={grid} unroll={u} xpt={xpt}", r)
            worst = max(worst, r)
            seen_x.add(xpt)
            seen_u.add(u)
            assert grid == 5 and r < BAR, (k, gdt, r)
    assert seen_x == {4, 5, 11, 14, 0} and seen_u == {4, 5, 8}, (seen_x, seen_u)
    report("staging/unroll", "max", worst)


@pytest.mark.parametrize("wdt,ks", [("i8", (2048, 5120, 11008, 16384)), ("f32", (2048, 5120, 16384))])
def test_gemv_staging_other_weight_dtypes(ops, wdt, ks):
    rng = np.random.default_rng(2)
    plans = {}
    for k in ks:
        w, s = host_w(wdt, 37, k)
        x = rng.standard_normal(k).astype(np.float32)
        for gdt in (None, "f32"):
            gamma = make_gamma(rng, k, gdt)
            y, plan = run_store(ops, wdt, w, s, x, gamma)
            r = rel(y, acc_ref(w, s, x_eff(x, gamma)))
            report("staging/unroll", f"{wdt} k={k} norm={gdt} plan={plan}", r)
            assert r < BAR, (wdt, k, gdt, r)
            plans[k] = plan
    assert {p[2] for p in plans.values()} >= ({4, 5, 11, 0} if wdt == "i8" else {4, 5, 0})
    if wdt == "i8":
        assert plans[5120][1] == 5 and plans[2048][1] == 4 and plans[16384][1] == 8, plans  # 320 chunks: unroll 5
    else:
        assert plans[2048][1] == 8 and plans[5120][1] == 4, plans


# ------------------------------------------- epilogues x weight x gamma dtype
def _epilogues(ops, wdt, gdt, grid=0, n=37, po=21, k=4096, group="epilogues"):
    """store / add / silu-mul / argmax of one weight and gamma dtype against float64."""
    rng = np.random.default_rng(n * 7 + po + grid)
    gamma = make_gamma(rng, k, gdt)
    x = rng.standard_normal(k).astype(np.float32)
    xe = x_eff(x, gamma)
    w, s = host_w(wdt, n, k)
    ref = acc_ref(w, s, xe)
    common = dict(wargs(wdt, w, s), x=T(x), grid=grid, **gargs(gamma))
    tag = f"{wdt} gamma={gdt} grid={grid} rows={n}"
    # store
    y = Buf(n)
    ops.debug_gemv(**common, epi=STORE, y=y.t)
    r = rel(y.get(), ref)
    report(group, f"store {tag}", r)
    assert r < BAR
    # add, resid_scale != 1; without gamma the residual aliases y (kernels.h: "resid may alias y")
    res = rng.standard_normal(n).astype(np.float32)
    y = Buf(n, init=res) if gdt is None else Buf(n)
    ops.debug_gemv(**common, epi=ADD, y=y.t, resid=y.t if gdt is None else T(res), resid_scale=0.75)
    r = rel(y.get(), ref + 0.75 * res.astype(np.float64))
    report(group, f"add {tag}", r)
    assert r < BAR
    # argmax: y and the best key over the grid's partials
    g, _, _ = ops.debug_gemv_plan(**common, epi=ARGMAX, y=y.t, partials=y.t)
    y, part = Buf(n), Buf(g, torch.int64)
    ops.debug_gemv(**common, epi=ARGMAX, y=y.t, partials=part.t, idx_base=32000)
    yv = y.get()
    r = rel(yv, ref)
    report(group, f"argmax {tag}", r)
    assert r < BAR
    assert decode_key(part.get().view(np.uint64).max()) == 32000 + int(np.argmax(yv))
    # silu(gate) * up over the pairs (g, g + po)
    w2, s2 = host_w(wdt, 2 * po, k)
    y = Buf(po)
    ops.debug_gemv(**dict(common, **wargs(wdt, w2, s2)), epi=SILU, y=y.t, pair_off=po)
    r2 = rel(y.get(), silu_ref(acc_ref(w2, s2, xe), po))
    report(group, f"silu {tag}", r2)
    assert r2 < BAR


@pytest.mark.parametrize("gdt", [None, "f16", "f32"])
@pytest.mark.parametrize("wdt", ["f16", "f32", "i8"])
def test_gemv_epilogues_by_weight_and_gamma_dtype(ops, wdt, gdt):
    _epilogues(ops, wdt, gdt)


# ------------------------------------------------------------ looping waves
@pytest.mark.parametrize("n,po", [(37, 19), (1, 1)])
@pytest.mark.parametrize("grid", [2, 3])
def test_gemv_explicit_grid_waves_loop_over_row_groups(ops, grid, n, po):
    """An explicit grid of 2 / 3 workgroups: 19 row groups (the last one a single row, or
    19 gate/up pairs) over 8 / 12 waves, so waves take a second and third group and the last
    pass is ragged; one row alone leaves 7 / 11 waves without work. Every epilogue that takes
    an explicit grid (kpar does not)."""
    _epilogues(ops, "f16", "f16", grid=grid, n=n, po=po, group="looping waves")
    rng = np.random.default_rng(grid + n)
    k = 4096
    w, s = host_w("f16", n, k)
    x = rng.standard_normal(k).astype(np.float32)
    ref = acc_ref(w, s, x)
    seed = rng.integers(-2 ** 40, 2 ** 40, n)
    yacc = Buf(n, torch.int64, init=seed)
    ops.debug_gemv(**wargs("f16", w, s), x=T(x), epi=ATOMIC, yacc=yacc.t, grid=grid)
    va = yacc.get()
    r = rel((va - seed) / FX, ref)
    report("looping waves", f"atomic grid={grid} rows={n}", r)
    assert r < BAR
    # single producer, the copy aliasing the base (the engine's use): later groups re-read the base
    base = Buf(n, torch.int64, init=seed)
    ys = Buf(n, torch.int64)
    ops.debug_gemv(**wargs("f16", w, s), x=T(x), epi=ATOMIC, yacc=ys.t, yacc_single=1, yacc_base=base.t,
                   yacc_copy=base.t, grid=grid)
    np.testing.assert_array_equal(ys.get(), va)
    np.testing.assert_array_equal(base.get(), va)


# ------------------------------------------------------------------ x_fixed
@pytest.mark.parametrize("wdt,k", [("f16", 4096), ("i8", 5120), ("f32", 11008), ("f16", 16384)])
def test_gemv_fixed_point_x_and_write_back(ops, wdt, k):
    """x as int64 fixed point with RMSNorm, store / silu / argmax: x_out is fp32(x_fixed) * 2^-32
    bit for bit (one rounding), y within the bar of float64 on that x. K covers the register
    staging (4, 5, 11 float4s a thread) and the strided form."""
    rng = np.random.default_rng(k)
    n, po = 37, 21
    gamma = make_gamma(rng, k, "f16")
    xf = np.rint(rng.standard_normal(k) * FX).astype(np.int64)
    x32 = xf.astype(np.float32) * np.float32(1.0 / FX)
    xe = x_eff(x32, gamma)
    w, s = host_w(wdt, n, k)
    w2, s2 = host_w(wdt, 2 * po, k)
    for epi in (STORE, SILU, ARGMAX):
        ww, ss = (w2, s2) if epi == SILU else (w, s)
        ref = acc_ref(ww, ss, xe)
        ref = silu_ref(ref, po) if epi == SILU else ref
        y, xo, part = Buf(len(ref)), Buf(k), Buf(16, torch.int64)
        a = dict(wargs(wdt, ww, ss), x_fixed=T(xf), x_out=xo.t, y=y.t, epi=epi, **gargs(gamma))
        if epi == SILU:
            a["pair_off"] = po
        if epi == ARGMAX:
            a["partials"] = part.t
        ops.debug_gemv(**a)
        np.testing.assert_array_equal(xo.get().view(np.uint32), x32.view(np.uint32))
        r = rel(y.get(), ref)
        report("x_fixed", f"{wdt} k={k} epi={epi}", r)
        assert r < BAR
        part.get()
    # a fixed-point x without RMSNorm is outside the contract: rejected, nothing written
    y = Buf(n)
    with pytest.raises(_lib.LlmiError):
        ops.debug_gemv(**wargs(wdt, w, s), x_fixed=T(xf), y=y.t, epi=STORE)
    assert np.isnan(y.get()).all()


# ---------------------------------------------------------------------- ldw
@pytest.mark.parametrize("wdt", ["f16", "f32", "i8"])
def test_gemv_row_stride_never_reads_the_padding(ops, wdt):
    rng = np.random.default_rng(3)
    n, k = 37, 4096
    w, s = host_w(wdt, n, k)
    x = rng.standard_normal(k).astype(np.float32)
    gamma = make_gamma(rng, k, "f16")
    y0, _ = run_store(ops, wdt, w, s, x, gamma)
    y1, _ = run_store(ops, wdt, w, s, x, gamma, ldw=k + 64)
    np.testing.assert_array_equal(y0.view(np.uint32), y1.view(np.uint32))
    r = rel(y1, acc_ref(w, s, x_eff(x, gamma)))
    report("ldw", f"{wdt} ldw=k+64", r)
    assert r < BAR
    # rows that would not start on a 16-B boundary are outside the contract: rejected, nothing written
    y = Buf(n)
    with pytest.raises(_lib.LlmiError):
        ops.debug_gemv(**wargs(wdt, w, s, ldw=k + 2), x=T(x), y=y.t, epi=STORE)
    assert np.isnan(y.get()).all()


# --------------------------------------------------------------- EPI_ATOMIC
@pytest.mark.parametrize("wdt,n,k", [("f16", 37, 4096), ("f16", 37, 11008), ("i8", 37, 4096), ("i8", 37, 11008),
                                     ("f32", 37, 4096), ("f16", 4096, 4096), ("i8", 4096, 4096),
                                     ("f16", 4096, 11008)])
def test_gemv_split_k_atomics(ops, wdt, n, k):
    """yacc += fixed(W x) with K over 1, 2, 4, 8 workgroups: within the bar of float64 from a
    known int64 seed, and bit-identical between two runs (integer sums are order-free). 4096
    rows at ksplit 8 exceed the grid cap, so waves loop too."""
    rng = np.random.default_rng(n + k)
    w, s = host_w(wdt, n, k)
    x = rng.standard_normal(k).astype(np.float32)
    ref = acc_ref(w, s, x)
    seed = rng.integers(-2 ** 40, 2 ** 40, n)
    wa, xt = wargs(wdt, w, s), T(x)
    for ksplit in (1, 2, 4, 8):
        runs = []
        for _ in range(2):
            yacc = Buf(n, torch.int64, init=seed)
            ops.debug_gemv(**wa, x=xt, epi=ATOMIC, yacc=yacc.t, ksplit=ksplit)
            runs.append(yacc.get())
        np.testing.assert_array_equal(runs[0], runs[1])
        r = rel((runs[0] - seed) / FX, ref)
        report("atomic", f"{wdt} rows={n} k={k} ksplit={ksplit}", r)
        assert r < BAR, (ksplit, r)


# -------------------------------------------------------------- yacc_single
@pytest.mark.parametrize("wdt,n", [("f16", 37), ("i8", 37), ("f16", 4096)])
def test_gemv_single_producer_rows(ops, wdt, n):
    """yacc_single: yacc[r] = yacc_base[r] + fixed(acc) stored -- "the same integer" as the atomic
    add into a yacc seeded with the base (kernels.h), and the same value in yacc_copy."""
    rng = np.random.default_rng(n)
    k = 4096
    w, s = host_w(wdt, n, k)
    x = rng.standard_normal(k).astype(np.float32)
    seed = rng.integers(-2 ** 40, 2 ** 40, n)
    wa, xt = wargs(wdt, w, s), T(x)

    def atomic(init):
        yacc = Buf(n, torch.int64, init=init)
        ops.debug_gemv(**wa, x=xt, epi=ATOMIC, yacc=yacc.t)
        return yacc.get()

    want, want0 = atomic(seed), atomic(np.zeros(n, np.int64))
    r = rel((want - seed) / FX, acc_ref(w, s, x))
    report("yacc_single", f"{wdt} rows={n}", r)
    assert r < BAR
    yacc, copy = Buf(n, torch.int64), Buf(n, torch.int64)
    ops.debug_gemv(**wa, x=xt, epi=ATOMIC, yacc=yacc.t, yacc_single=1, yacc_base=T(seed), yacc_copy=copy.t)
    np.testing.assert_array_equal(yacc.get(), want)
    np.testing.assert_array_equal(copy.get(), want)
    yacc = Buf(n, torch.int64)
    ops.debug_gemv(**wa, x=xt, epi=ATOMIC, yacc=yacc.t, yacc_single=1)  # no base: fixed(acc) alone
    np.testing.assert_array_equal(yacc.get(), want0)
    yacc, base = Buf(n, torch.int64), Buf(n, torch.int64, init=seed)  # the copy aliases the base (engine)
    ops.debug_gemv(**wa, x=xt, epi=ATOMIC, yacc=yacc.t, yacc_single=1, yacc_base=base.t, yacc_copy=base.t)
    np.testing.assert_array_equal(yacc.get(), want)
    np.testing.assert_array_equal(base.get(), want)


def test_gemv_single_producer_rejects_split_k(ops):
    """One producer per row and K slices exclude each other: the second slice would overwrite
    the first. The launcher refuses, and nothing is written."""
    rng = np.random.default_rng(4)
    n, k = 37, 4096
    w, s = host_w("f16", n, k)
    seed = rng.integers(-2 ** 40, 2 ** 40, n)
    yacc, copy = Buf(n, torch.int64, init=seed), Buf(n, torch.int64)
    a = dict(wargs("f16", w, s), x=T(rng.standard_normal(k).astype(np.float32)), epi=ATOMIC, yacc=yacc.t,
             yacc_single=1, ksplit=2, yacc_copy=copy.t)
    with pytest.raises(_lib.LlmiError):
        ops.debug_gemv(**a)
    with pytest.raises(_lib.LlmiError):
        ops.debug_gemv_plan(**a)
    with pytest.raises(_lib.LlmiError):  # ... nor with another epilogue
        ops.debug_gemv(**dict(a, ksplit=1, epi=STORE, y=T(np.zeros(n, np.float32))))
    np.testing.assert_array_equal(yacc.get(), seed)
    assert (copy.get() == _SENT[torch.int64][1]).all()


# ----------------------------------------------------------- seed hand-over
@pytest.mark.parametrize("seed_n", [1, 100, 4096, 4099])
def test_gemv_seed_hand_over(ops, seed_n):
    """seed_dst[0, seed_n) = seed_src (or zeros) copied on the side, one slice a workgroup:
    bit-exact for counts below, equal to and not a multiple of the grid, automatic grids (5
    and 256 workgroups) and an explicit one; the GEMV's own result is unchanged. The
    gate_up shape reads its source from the x_fixed buffer, as the engine does."""
    rng = np.random.default_rng(seed_n)
    k = 2048
    gamma = make_gamma(rng, k, "f16")
    src = rng.integers(-2 ** 40, 2 ** 40, max(seed_n, k))
    x32 = src[:k].astype(np.float32) * np.float32(1.0 / FX)
    w, s = host_w("f16", 37, k)
    w2, s2 = host_w("f16", 2048, k)
    ref = acc_ref(w, s, x_eff(x32, gamma))
    ref2 = silu_ref(acc_ref(w2, s2, x_eff(x32, gamma)), 1024)
    srct = T(src)
    for keep in (1, 0):
        want = src[:seed_n] if keep else np.zeros(seed_n, np.int64)
        for grid in (0, 3):
            y, dst = Buf(37), Buf(seed_n, torch.int64)
            ops.debug_gemv(**wargs("f16", w, s), x_fixed=srct, y=y.t, epi=STORE, grid=grid, **gargs(gamma),
                           seed_src=srct, seed_dst=dst.t, seed_n=seed_n, seed_keep=keep)
            np.testing.assert_array_equal(dst.get(), want)
            assert rel(y.get(), ref) < BAR
        y, dst = Buf(1024), Buf(seed_n, torch.int64)
        ops.debug_gemv(**wargs("f16", w2, s2), x_fixed=srct, y=y.t, epi=SILU, pair_off=1024, **gargs(gamma),
                       seed_src=srct, seed_dst=dst.t, seed_n=seed_n, seed_keep=keep)
        np.testing.assert_array_equal(dst.get(), want)
        assert rel(y.get(), ref2) < BAR


# --------------------------------------------------------------- EPI_ARGMAX
@pytest.mark.parametrize("idx_base", [0, 32000])
@pytest.mark.parametrize("n", [37, 1000])
@pytest.mark.parametrize("wdt", ["f16", "i8"])
def test_gemv_argmax_keys(ops, wdt, n, idx_base):
    """Logits within the bar; the largest of the grid's keys names idx_base + argmax of the
    device's own y. Then the winning row's weights are copied to row 3 and row n - 3 (other
    workgroups): equal logits, and the lowest index must win."""
    rng = np.random.default_rng(n + idx_base)
    k = 4096
    w, s = host_w(wdt, n, k)
    x = rng.standard_normal(k).astype(np.float32)
    gamma = make_gamma(rng, k, "f32")
    xe = x_eff(x, gamma)

    def run(w, s):
        a = dict(wargs(wdt, w, s), x=T(x), epi=ARGMAX, idx_base=idx_base, **gargs(gamma))
        y0 = Buf(n)
        grid, _, _ = ops.debug_gemv_plan(**a, y=y0.t, partials=y0.t)
        y, part = Buf(n), Buf(grid, torch.int64)
        ops.debug_gemv(**a, y=y.t, partials=part.t)
        return y.get(), decode_key(part.get().view(np.uint64).max()), grid

    y, idx, grid = run(w, s)
    assert grid == (n + 7) // 8
    r = rel(y, acc_ref(w, s, xe))
    report("argmax", f"{wdt} rows={n} idx_base={idx_base}", r)
    assert r < BAR
    assert idx == idx_base + int(np.argmax(y))
    m = int(np.argmax(y))
    w, s = w.copy(), None if s is None else s.copy()
    for d in (3, n - 3):
        w[d] = w[m]
        if s is not None:
            s[d] = s[m]
    y, idx, _ = run(w, s)
    assert y[3] == y[m] == y[n - 3] == y.max()
    assert idx == idx_base + min(3, m)


# --------------------------------------------------------------------- kpar
@pytest.mark.parametrize("k", [512, 4096, 5120])
@pytest.mark.parametrize("wdt", ["f16", "i8"])
def test_gemv_k_parts_inside_a_workgroup(ops, wdt, k):
    """kpar 2 / 4 (the K-parted q/k/v and gate_up of a small TP shard): RMSNorm + fixed-point
    x, store and silu, against float64 and against the unsplit launch (reassociation only).
    37 rows / 21 pairs leave waves of the last workgroup without a group; 1536 rows is the
    TP-8 q/k/v shard."""
    rng = np.random.default_rng(k)
    gamma = make_gamma(rng, k, "f16")
    xf = np.rint(rng.standard_normal(k) * FX).astype(np.int64)
    xe = x_eff(xf.astype(np.float32) * np.float32(1.0 / FX), gamma)
    xt = T(xf)
    for n, epi, po in ((37, STORE, 0), (42, SILU, 21), (1536, STORE, 0), (1536, SILU, 768)):
        w, s = host_w(wdt, n, k)
        ref = acc_ref(w, s, xe)
        ref = silu_ref(ref, po) if epi == SILU else ref
        out = {}
        for kpar in (0, 2, 4):
            y = Buf(len(ref))
            a = dict(wargs(wdt, w, s), x_fixed=xt, y=y.t, epi=epi, pair_off=po, kpar=kpar, **gargs(gamma))
            grid, u, _ = ops.debug_gemv_plan(**a)
            ops.debug_gemv(**a)
            out[kpar] = y.get()
            r = rel(out[kpar], ref)
            report("kpar", f"{wdt} k={k} rows={n} epi={epi} kpar={kpar}", r)
            assert r < BAR, (n, epi, kpar, r)
            if kpar:
                groups = po if epi == SILU else (n + 1) // 2
                assert u == 4 and grid == -(-groups // (4 // kpar))
                r0 = rel(out[kpar], out[0])
                report("kpar", f"{wdt} k={k} rows={n} epi={epi} kpar={kpar} vs unsplit", r0)
                assert r0 < BAR_KPAR


# ------------------------------------------------------ attention + o_proj
@functools.lru_cache(maxsize=4)
def host_wo(wdt, n_rows, cols):
    return host_w(wdt, n_rows, cols, seed=11)


def _ao_case(ops, heads, kv_heads, n_rows, ctx, cache_dt=np.float16, wdt="f16", head_major=False, ld_mul=1,
             host_sized=True, rope=True, resid="f32", zero_w=False, max_seq=256, seed=0):
    """The engine's attention launch (partials only) + o_proj launch through llmi_debug_attn_oproj
    against oracle.llama_ref.attention_decode (the reference test_gpu_ops.py holds the attention
    kernel to) followed by W_o in float64; returns the rel-L2 of (xacc - seed) * 2^-32."""
    d = 128
    cols = heads * d
    rng = np.random.default_rng(seed + ctx + heads)
    kc = (rng.standard_normal((kv_heads, max_seq, d)) * 0.5).astype(np.float32).astype(cache_dt)
    vc = rng.standard_normal((kv_heads, max_seq, d)).astype(np.float32).astype(cache_dt)
    qkv = rng.standard_normal((heads + 2 * kv_heads) * d).astype(np.float32)
    pos = ctx - 1
    w, s = host_wo(wdt, n_rows, cols)
    if zero_w:
        w = np.zeros_like(w)
    ldw = cols * ld_mul
    if head_major:
        wd = T(np.ascontiguousarray(w.reshape(n_rows, heads, d).transpose(1, 0, 2)))
    else:
        wd = dev_w(w, ldw if ld_mul > 1 else 0)
    res = rng.standard_normal(n_rows).astype(np.float32)
    resfx = rng.integers(-2 ** 40, 2 ** 40, n_rows)
    seedv = {"f32": to_fixed(res), "fixed": resfx, "zero": np.zeros(n_rows, np.int64)}[resid]
    ktd, vtd = T(kc), T(vc)
    ws = ops.attn_workspace(heads, max_seq)
    xacc, err = Buf(n_rows, torch.int64), T(np.zeros(1, np.int32))
    a = dict(qkv=T(qkv), k_cache=ktd, v_cache=vtd, cache_dtype=_lib.F16 if cache_dt == np.float16 else _lib.F32,
             max_seq=max_seq, pos_dev=T(np.array([pos], np.int32)), nact=pos // 64 + 1 if host_sized else 0,
             heads=heads, kv_heads=kv_heads, rope=int(rope), workspace=ws, xacc=xacc.t,
             resid=T(res) if resid != "fixed" else None, resid_fixed=T(resfx) if resid == "fixed" else None,
             resid_scale=0.0 if resid == "zero" else 1.0, w=wd, scales=None if s is None else T(s),
             w_dtype=WDT[wdt], head_major=int(head_major), n_rows=n_rows, ldw=ldw, err=err)
    runs = []
    for _ in range(2):
        ws.fill_(255)  # NaN bit patterns: a stale split past nact must not leak
        ktd.copy_(T(kc))
        vtd.copy_(T(vc))
        xacc.t[:n_rows] = _SENT[torch.int64][1]
        ops.debug_attn_oproj(**a)
        runs.append(xacc.get())
    np.testing.assert_array_equal(runs[0], runs[1])
    assert int(N(err)[0]) == 0
    _ao_case.last = runs[0]
    # the cache write (the slot checks of test_gpu_ops._attn_case)
    q = qkv[:cols].reshape(heads, d)
    kk = qkv[cols:cols + kv_heads * d].reshape(kv_heads, d)
    v = qkv[cols + kv_heads * d:].reshape(kv_heads, d)
    if rope:
        cos, sin = R.rope_cos_sin([pos], d, 10000.0)
        q, kk = R.apply_rope(q, cos[0], sin[0]), R.apply_rope(kk, cos[0], sin[0])
    kref, vref = kc.copy(), vc.copy()
    kref[:, pos] = kk.astype(cache_dt)
    vref[:, pos] = v.astype(cache_dt)
    kn, vn = N(ktd), N(vtd)
    if rope:
        np.testing.assert_allclose(kn[:, pos].astype(np.float32), kref[:, pos].astype(np.float32),
                                   rtol=2e-3 if cache_dt == np.float16 else 1e-6, atol=1e-6)
    else:
        np.testing.assert_array_equal(kn[:, pos], kref[:, pos])
    np.testing.assert_array_equal(vn[:, pos], vref[:, pos])
    mask = np.ones(kn.shape[:2], bool)
    mask[:, pos] = False
    np.testing.assert_array_equal(kn[mask], kc[mask])
    np.testing.assert_array_equal(vn[mask], vc[mask])
    if zero_w:
        np.testing.assert_array_equal(runs[0], seedv)
        return 0.0
    o = R.attention_decode(q, kref.astype(np.float32), vref.astype(np.float32), ctx).reshape(-1)
    ref = acc_ref(w, s, o.astype(np.float64))
    got = (runs[0] - seedv).astype(np.float64) / FX
    e = np.maximum(np.abs(got - ref) - heads * 2.0 ** -33, 0.0)  # each head's product rounds to 2^-32 once
    r, raw = float(np.linalg.norm(e) / np.linalg.norm(ref)), rel(got, ref)
    report("attn+o_proj", f"heads={heads}/{kv_heads} rows={n_rows} ctx={ctx} cache={np.dtype(cache_dt).name} "
           f"w={wdt} head_major={head_major} ldw={ldw} host_sized={host_sized} rope={rope} (raw {raw:.3e})", r)
    assert r < BAR_AO, (r, raw)
    return r


@pytest.mark.parametrize("heads,n_rows,wdt,head_major", [
    (4, 4096, "f16", False), (5, 5120, "f16", False), (4, 4096, "i8", False), (4, 4096, "f32", False),  # 1 row a group
    (8, 4096, "f16", False), (8, 4096, "i8", True),                                                      # 2
    (16, 4096, "f16", False), (16, 4096, "i8", False),                                                   # 4
    (32, 4096, "f16", False), (32, 4096, "f16", True), (32, 4096, "i8", False), (32, 4096, "f32", False),  # 8
])
def test_attn_oproj_kernel_variants(ops, heads, n_rows, wdt, head_major):
    """Every rows-per-group instantiation of the o_proj (1, 2, 4, 8), the odd head count, the
    two-heads-per-workgroup fp16 kernel (32 heads, row-major), head-major W_o, int8 and fp32
    W_o; three splits, RoPE, host-sized grid."""
    _ao_case(ops, heads, heads, n_rows, 130, wdt=wdt, head_major=head_major, resid="fixed")


@pytest.mark.parametrize("heads,n_rows,wdt", [(32, 4100, "f16"), (8, 4100, "f16"), (32, 4100, "i8"), (4, 520, "f32")])
def test_attn_oproj_row_tail(ops, heads, n_rows, wdt):
    """n_rows not a multiple of the workgroup's row chunk (64, 32, 128, 16 rows): the last chunk's
    loads are clamped and its rows masked; the seed slices (ceil(n_rows / heads) a head) are ragged."""
    _ao_case(ops, heads, heads, n_rows, 65, wdt=wdt, host_sized=False)


def test_attn_oproj_column_shard_stride(ops):
    """ldw = 2 * heads * 128 (a TP rank's column shard of W_o); the other rank's columns hold
    large values that must never be read."""
    _ao_case(ops, 8, 8, 4096, 130, ld_mul=2)
    shard = _ao_case.last
    _ao_case(ops, 8, 8, 4096, 130)
    np.testing.assert_array_equal(shard, _ao_case.last)
    w, s = host_wo("f16", 512, 512)
    xacc = Buf(512, torch.int64)
    z = T(np.zeros(4096, np.float32))
    with pytest.raises(_lib.LlmiError):  # row slices off the 16-B grid: outside the contract
        ops.debug_attn_oproj(qkv=z, k_cache=z, v_cache=z, cache_dtype=_lib.F32, max_seq=64,
                             pos_dev=T(np.zeros(1, np.int32)), heads=4, kv_heads=4, workspace=ops.attn_workspace(4, 64),
                             xacc=xacc.t, resid=z, w=T(w), w_dtype=_lib.F16, n_rows=512, ldw=520,
                             err=T(np.zeros(1, np.int32)))
    assert (xacc.get() == _SENT[torch.int64][1]).all()


@pytest.mark.parametrize("cache_dt", [np.float16, np.float32])
@pytest.mark.parametrize("ctx", [1, 64, 65, 130, 256])
def test_attn_oproj_contexts_and_grid_forms(ops, ctx, cache_dt):
    """max_seq 256 (4 splits), contexts at the split edges, MHA and GQA (8 heads over 2), the
    host-sized grid (nact = pos / 64 + 1) and the max_seq-sized one; the workspace is full of
    NaN patterns before every launch."""
    for host_sized in (True, False):
        _ao_case(ops, 4, 4, 512, ctx, cache_dt, host_sized=host_sized, rope=False)
        _ao_case(ops, 8, 2, 1024, ctx, cache_dt, host_sized=host_sized, seed=1)


@pytest.mark.parametrize("resid", ["f32", "fixed", "zero"])
def test_attn_oproj_seeds_xacc_exactly(ops, resid):
    """With W_o = 0 xacc is exactly its seed: fixed(resid), resid_fixed itself, or zeros when
    resid_scale = 0 (a TP rank that does not carry the residual)."""
    for host_sized in (True, False):
        _ao_case(ops, 4, 4, 520, 130, resid=resid, zero_w=True, host_sized=host_sized)
        _ao_case(ops, 32, 32, 4096, 65, resid=resid, zero_w=True, host_sized=host_sized)
