"""CPU-side checks of the C ABI (no GPU needed): the library loads, exports
every symbol include/llmi.h declares, the host twin of the synthetic-weight
generator is bit-identical to the numpy oracle PRNG, and argument errors come
back as codes + messages (LLM_CHECK convention)."""
import ctypes as C

import numpy as np
import pytest

from llmi import _lib
from llmi._lib import call, lib
from llmi.engine import preset, synth_prompt
from oracle import prng


def test_library_exports_every_header_symbol():
    L = lib()
    names = _lib.header_functions()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert set(names) == set(_lib._SIGS), set(names) ^ set(_lib._SIGS)


def _host_fill(kind, dtype, seed, tid, rows, cols, row0=0, col0=0, ld=0):
    out = np.zeros((rows, cols), dtype)
    dt = {np.float16: _lib.F16, np.float32: _lib.F32, np.int8: _lib.I8}[dtype]
    call("llmi_synth_fill_host", out.ctypes.data, dt, kind, seed, tid, rows, cols, row0, col0, ld)
    return out


@pytest.mark.parametrize("seed", [0, 7, 2**40 + 3])
def test_host_generator_matches_numpy_prng(seed):
    tid = prng.layer_tid(3, prng.KIND_GATE)
    a = _host_fill(_lib.SYN_LINEAR, np.float16, seed, tid, 64, 96, 5, 17, 4096)
    b = prng.linear_fp16(seed, tid, 64, 96, 5, 17, 4096)
    np.testing.assert_array_equal(a.view(np.uint16), b.view(np.uint16))
    a32 = _host_fill(_lib.SYN_LINEAR, np.float32, seed, tid, 64, 96, 5, 17, 4096)
    np.testing.assert_array_equal(a32, b.astype(np.float32))
    e = _host_fill(_lib.SYN_EMBED, np.float16, seed, prng.GLOBAL_EMBED, 8, 512)
    np.testing.assert_array_equal(e.view(np.uint16), prng.embed_fp16(seed, prng.GLOBAL_EMBED, 8, 512).view(np.uint16))
    g = _host_fill(_lib.SYN_GAMMA, np.float16, seed, tid, 1, 4096, 0, 0, 4096)
    np.testing.assert_array_equal(g[0].view(np.uint16), prng.gamma_fp16(seed, tid, 4096).view(np.uint16))
    q = _host_fill(_lib.SYN_INT8, np.int8, seed, tid, 16, 64, 3, 32, 5120)
    np.testing.assert_array_equal(q, prng.int8_weight(seed, tid, 16, 64, 3, 32, 5120))
    s = _host_fill(_lib.SYN_INT8_SCALE, np.float16, seed, tid, 40, 1, 9, 0, 1)
    np.testing.assert_array_equal(s[:, 0].view(np.uint16), prng.int8_row_scale(seed, tid, 40, 9).view(np.uint16))


def test_prompt_ids_match():
    np.testing.assert_array_equal(synth_prompt(13, 8, 32000), prng.prompt_ids(13, 8, 32000))


def test_presets():
    c = preset("llama2-7b")
    assert (c.hidden, c.heads, c.kv_heads, c.head_dim, c.inter, c.layers, c.vocab) == \
        (4096, 32, 32, 128, 11008, 32, 32000)
    assert abs(c.rms_eps - 1e-5) < 1e-12 and c.rope_base == 10000.0
    c13 = preset("llama2-13b")
    assert (c13.hidden, c13.heads, c13.inter, c13.layers) == (5120, 40, 13824, 40)
    with pytest.raises(_lib.LlmiError, match="unknown name"):
        preset("gpt-2")


def test_errors_are_codes_with_messages():
    L = lib()
    rc = L.llmi_linear(None, None, _lib.F16, None, None, 0, 1, 1, None)
    assert rc == -1
    assert "[llmi][ERROR]" in L.llmi_last_error().decode()
    rc = L.llmi_synth_fill_host(None, _lib.F32, _lib.SYN_INT8, 0, 0, 1, 1, 0, 0, 0)
    assert rc == -1 and b"int8" in L.llmi_last_error()
    x = C.c_void_p(16)  # never dereferenced: the checks come first
    rc = L.llmi_linear_fused(x, x, _lib.F16, None, x, 8, 64, None, _lib.F16, 1e-5, 3, None, None)
    assert rc == -1 and b"epilogue" in L.llmi_last_error()
    rc = L.llmi_linear_fused(x, x, _lib.F16, None, x, 8, 64, None, _lib.F16, 1e-5, 1, x, None)
    assert rc == -1 and b"resid != y" in L.llmi_last_error()
    cfg = preset("tiny", tp_world=3)
    h = C.c_void_p()
    rc = L.llmi_engine_create(C.byref(cfg), 0, None, C.byref(h))
    assert rc == -1 and b"divide by tp_world" in L.llmi_last_error()


PF_ROWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 200), (20, 64), (31, 33), (33, 64), (500, 40)]
PF_PART = 64 * 128 + 2 * 64  # fp32 elements of one chunk's partial: O rows, then m, then l


def _pf_plan(**kw):
    F = 0x1000  # never dereferenced
    a = _lib.DebugPrefillAttnArgs()
    base = dict(qkv=F, k_cache=F, v_cache=F, rope_tab=F, out=F, cache_dtype=_lib.F16, max_seq=1024, mfma_planes=2)
    for key, v in dict(base, **kw).items():
        setattr(a, key, v)
    o = [C.c_int() for _ in range(4)]
    call("llmi_debug_prefill_attn_plan", C.byref(a), *[C.byref(x) for x in o])
    return tuple(x.value for x in o)


def _pf_model(p0, m, heads, ws_floats, chunk_blocks, n_cu=256):
    """The documented ladder (kernels.h PrefillAttnPlan, prefill.hip's split-key comment), restated:
    query blocks of 64 rows, block qb sees ceil((p0 + min(64 qb + 64, m)) / 64) key blocks."""
    nqb = -(-m // 64)
    nkb = [-(-(p0 + min(64 * q + 64, m)) // 64) for q in range(nqb)]
    cb = max(nkb)
    if ws_floats is not None:
        if nqb * heads < n_cu:
            cb = max(1, -(-sum(nkb) * heads // n_cu))
        if chunk_blocks:
            cb = chunk_blocks
    maxc = -(-max(nkb) // cb)
    if ws_floats is None or maxc > 8 or heads * nqb * maxc * PF_PART > ws_floats:
        cb, maxc = max(nkb), 1
    items = sum(-(-n // cb) for n in nkb)
    return cb, maxc, 8 * (-(-heads // 8)) * items, {1: 0, 2: 2, 3: 4, 4: 4}.get(maxc, 8)


def test_debug_prefill_attn_plan_walks_the_ladder():
    """llmi_debug_prefill_attn_plan launches nothing; without a GPU the CU count falls back to
    256. Every (p0, m) of the GPU file's MFMA list at heads 4, 12 and 8: no workspace, the
    automatic chunking and chunk_blocks 1, against the ladder restated above; then the forms
    by hand, the workspace-size fallback and the argument checks."""
    big = 1 << 30
    for heads, kvh in ((4, 4), (12, 4), (8, 2)):
        for p0, m in PF_ROWS:
            kw = dict(p0=p0, m=m, heads=heads, kv_heads=kvh)
            assert _pf_plan(**kw) == _pf_model(p0, m, heads, None, 0), kw
            assert _pf_plan(split_ws=0x1000, split_ws_floats=big, **kw) == _pf_model(p0, m, heads, big, 0), kw
            assert _pf_plan(split_ws=0x1000, split_ws_floats=big, chunk_blocks=1, **kw) == \
                _pf_model(p0, m, heads, big, 1), kw
            assert _pf_plan(chunk_blocks=1, **kw) == _pf_model(p0, m, heads, None, 0), kw  # no workspace: ignored
    ws = dict(split_ws=0x1000, split_ws_floats=big)
    assert _pf_plan(p0=0, m=1, heads=4, kv_heads=4, **ws) == (1, 1, 8, 0)
    assert _pf_plan(p0=0, m=200, heads=12, kv_heads=4, chunk_blocks=1, **ws) == (1, 4, 160, 4)   # 1+2+3+4 items
    assert _pf_plan(p0=33, m=64, heads=4, kv_heads=4, chunk_blocks=1, **ws) == (1, 2, 16, 2)
    assert _pf_plan(p0=128, m=64, heads=4, kv_heads=4, chunk_blocks=1, **ws) == (1, 3, 24, 4)
    assert _pf_plan(p0=448, m=64, heads=4, kv_heads=4, chunk_blocks=1, **ws) == (1, 8, 64, 8)
    assert _pf_plan(p0=500, m=40, heads=8, kv_heads=2, chunk_blocks=1, **ws) == (9, 1, 8, 0)     # 9 chunks: one
    assert _pf_plan(p0=500, m=40, heads=8, kv_heads=2, chunk_blocks=2, **ws) == (2, 5, 40, 8)
    assert _pf_plan(p0=500, m=40, heads=12, kv_heads=4, **ws) == (9, 1, 16, 0)   # automatic cb 1 -> 9 chunks: one
    need = 4 * 1 * 2 * PF_PART
    kw = dict(p0=64, m=64, heads=4, kv_heads=4, split_ws=0x1000, chunk_blocks=1)
    assert _pf_plan(split_ws_floats=need, **kw) == (1, 2, 16, 2)
    assert _pf_plan(split_ws_floats=need - 1, **kw) == (2, 1, 8, 0)
    assert _pf_plan(p0=20, m=64, heads=12, kv_heads=4, mfma_planes=0) == (0, 1, 24, 0)           # scalar: 32-row blocks
    ok = dict(p0=0, m=8, heads=4, kv_heads=4)
    for bad in (dict(heads=5), dict(heads=0), dict(kv_heads=0), dict(p0=1020), dict(m=0), dict(p0=-1),
                dict(head_dim=64), dict(qkv=0), dict(rope_tab=0), dict(cache_dtype=_lib.F32),
                dict(cache_dtype=_lib.I8, mfma_planes=0), dict(mfma_planes=3), dict(out=0), dict(out=0, mfma_planes=0),
                dict(chunk_blocks=-1)):
        with pytest.raises(_lib.LlmiError):
            _pf_plan(**dict(ok, **bad))
    assert _pf_plan(out=0, out_hi=0x1000, **ok) == (1, 1, 8, 0)


EPI_STORE, EPI_ADD, EPI_SILU, EPI_SLAB = 0, 1, 2, 5
# (kernel, m, n, k, epi, ksplit) of tests/test_gpu_prefill_gemm.py's sections A and C
GEMM_SHAPES = \
    [(2, m, n, k, EPI_STORE, 0) for m, n, k in ((1, 128, 64), (63, 128, 128), (64, 256, 192), (65, 128, 256),
                                                (129, 384, 320), (300, 128, 576), (257, 11008, 192),
                                                (300, 11008, 64), (130, 10240, 64))] + \
    [(2, 77, 256, 192, EPI_ADD, 0), (2, 130, 128, 64, EPI_ADD, 0)] + \
    [(2, m, n, k, EPI_SLAB, s) for m, n, k, s in ((16, 128, 64, 1), (100, 256, 512, 2), (130, 128, 192, 3),
                                                  (64, 128, 512, 8))] + \
    [(2, m, 2 * i, k, EPI_SILU, 0) for m, i, k in ((65, 64, 128), (130, 192, 64), (257, 5504, 64))] + \
    [(3, m, n, k, EPI_STORE, 0) for m, n, k in ((1, 256, 128), (255, 256, 192), (256, 512, 256), (257, 256, 320),
                                                (257, 256, 384), (300, 512, 448), (513, 256, 128),
                                                (513, 256, 192), (300, 12288, 512))] + \
    [(3, 300, 256, 128, EPI_ADD, 0), (3, 257, 512, 192, EPI_ADD, 0)] + \
    [(3, 300, n, k, EPI_SLAB, s) for n, k, s in ((256, 320, 2), (512, 832, 4), (256, 384, 2), (512, 1152, 8))] + \
    [(3, m, 2 * i, k, EPI_SILU, 0) for m, i, k in ((1, 128, 128), (257, 256, 192), (300, 384, 256))]
# section D: (epi, lo8, m, n, k, sk_pmax) for 256 workgroups
GEMM_SK = [(EPI_SILU, 0, 300, 2 * 4096, 512, 3), (EPI_SILU, 0, 300, 2 * 8192, 256, 1),
           (EPI_SILU, 1, 512, 2 * 6144, 512, 2), (EPI_STORE, 0, 300, 8192, 512, 3), (EPI_STORE, 1, 300, 12288, 512, 2)]


def _gemm_plan(**kw):
    F = 0x1000  # never dereferenced
    a = _lib.DebugGemmArgs()
    base = dict(kernel=2, a_hi=F, a_lo=F, planes=2, w=F, y=F, m=64, n=256, k=128)
    kw = dict(base, **kw)
    kw.setdefault("lda", kw["k"])
    kw.setdefault("ldy", kw["n"] // 2 if kw.get("epi") == EPI_SILU else kw["n"])
    for key, v in kw.items():
        setattr(a, key, v)
    o = [C.c_int() for _ in range(3)]
    call("llmi_debug_gemm_plan", C.byref(a), *[C.byref(x) for x in o])
    return tuple(x.value for x in o)


def _gemm_model(kernel, m, n, k, epi, ks):
    """The launchers' rule restated: gemm2 tiles 128 columns (gate_up: 64 gate columns), rows by
    128 iff split-K or ceil(m / 128) x column tiles >= 256, else by 64; gemm3 tiles 256 x 256
    (gate_up: 128 gate columns); one workgroup per tile and K slice."""
    s = ks if epi == EPI_SLAB else 1
    if kernel == 2:
        nt = (n // 2) // 64 if epi == EPI_SILU else n // 128
        bm = 128 if epi == EPI_SLAB or -(-m // 128) * nt >= 256 else 64
    else:
        nt = (n // 2) // 128 if epi == EPI_SILU else n // 256
        bm = 256
    return bm, -(-m // bm) * nt * s, 0


def test_debug_gemm_plan_reports_the_launchers_choices():
    """llmi_debug_gemm_plan launches and allocates nothing; without a GPU the CU count falls back
    to 256. bm and grid for the shapes of the GPU file against the rule restated above, one and
    two planes; the stream-K slots of the GPU file's section D (and the forms stream-K declines);
    then every argument check of the two launchers and of the hook."""
    F = 0x1000
    for kernel, m, n, k, epi, ks in GEMM_SHAPES:
        for planes in (1, 2):
            kw = dict(kernel=kernel, m=m, n=n, k=k, epi=epi, ksplit=ks, planes=planes, slab=F if epi == EPI_SLAB else 0)
            assert _gemm_plan(**kw) == _gemm_model(kernel, m, n, k, epi, ks), kw
    assert _gemm_plan(kernel=2, m=257, n=11008, k=192)[0] == 128 and _gemm_plan(kernel=2, m=300, n=11008, k=64)[0] == 128
    assert _gemm_plan(kernel=2, m=257, n=2 * 5504, k=64, epi=EPI_SILU)[0] == 128
    assert _gemm_plan(kernel=2, m=256, n=11008, k=192)[0] == 64            # 2 x 86 tiles < 256
    assert _gemm_plan(kernel=2, m=130, n=10240, k=64) == (64, 3 * 80, 0)    # 2 x 80 tiles >= 160: llmi_linear's ks = 1
    lo8 = dict(lo8=1, w8=F, w8_exp=-12)
    for epi, l8, m, n, k, pmax in GEMM_SK:
        kw = dict(kernel=3, m=m, n=n, k=k, epi=epi, y_hi=F, y_lo=F, **(lo8 if l8 else {}))
        assert _gemm_plan(stream_k=1, **kw) == (256, 256, pmax), kw          # every CU one workgroup
        assert _gemm_plan(stream_k=0, **kw) == _gemm_model(3, m, n, k, epi, 0), kw
        if not l8:                                                           # one plane: the plain kernel
            assert _gemm_plan(stream_k=1, **dict(kw, planes=1)) == _gemm_model(3, m, n, k, epi, 0), kw
    # declined: the tiles fill the CUs; fewer than two K-tile pairs a workgroup; split-K and add have no stream-K form
    assert _gemm_plan(kernel=3, stream_k=1, m=2048, n=8192, k=512) == (256, 256, 0)
    assert _gemm_plan(kernel=3, stream_k=1, m=300, n=512, k=4096) == (256, 4, 0)
    assert _gemm_plan(kernel=3, stream_k=1, m=300, n=8192, k=512, epi=EPI_ADD) == (256, 64, 0)
    assert _gemm_plan(kernel=3, stream_k=1, m=300, n=8192, k=512, epi=EPI_SLAB, ksplit=2, slab=F) == (256, 128, 0)
    g3 = dict(kernel=3, m=300, n=256, k=256)
    for bad in (dict(a_hi=0), dict(w=0), dict(m=0), dict(planes=0), dict(planes=3), dict(a_lo=0), dict(n=192),
                dict(k=96), dict(lda=132), dict(a_hi=F + 8), dict(a_lo=F + 8), dict(w=F + 8), dict(y=0),
                dict(epi=EPI_SILU, y=0), dict(epi=3), dict(epi=EPI_SLAB, ksplit=2), dict(epi=EPI_SLAB, ksplit=0, slab=F)):
        for base in (dict(), g3):
            with pytest.raises(_lib.LlmiError):
                _gemm_plan(**dict(base, **bad))
    for bad in (dict(epi=EPI_SLAB, slab=F, ksplit=3), dict(kernel=4), dict(kernel=0), dict(stream_k=1), dict(stream_k=2, kernel=3),
                dict(kernel=2, **lo8), dict(epi=EPI_SILU, n=192)):
        with pytest.raises(_lib.LlmiError):
            _gemm_plan(**bad)                                                # gemm2: k 128 in 3 slices; the hook's own checks
    for bad in (dict(k=64), dict(epi=EPI_SLAB, slab=F, ksplit=3), dict(planes=1, **lo8), dict(lo8=1, w8=0),
                dict(lo8=1, w8=F + 8), dict(k=192, **lo8), dict(epi=EPI_SLAB, slab=F, ksplit=3, k=256, **lo8),
                dict(epi=EPI_SILU, y_hi=F, y_lo=0, **lo8), dict(epi=EPI_SILU, y=F, **lo8),
                dict(epi=EPI_SILU, y=0, y_hi=F, ldy=132), dict(epi=EPI_SILU, y=0, y_hi=F + 8), dict(n=384)):
        with pytest.raises(_lib.LlmiError):
            _gemm_plan(**dict(g3, **bad))
    assert _gemm_plan(epi=EPI_SILU, y=0, y_hi=F) == (64, 2, 0)
    assert _gemm_plan(**dict(g3, epi=EPI_SLAB, slab=F, ksplit=2, y=0)) == (256, 4, 0)   # gemm3's slab form needs no y
    assert _gemm_plan(**dict(g3, epi=EPI_SLAB, slab=F, ksplit=2, **lo8)) == (256, 4, 0)  # one fp8 tile a slice


# (m, n, k, epi) of tests/test_gpu_gemm1.py: sections A (the m x k walk, the four forms, add), B, C, D, E, F
_G1_M, _G1_N, _G1_K = (1, 63, 64, 65, 130), (128, 256, 384), (64, 128, 192, 320)
GEMM1_FORMS = [(129, 16384, 64, 128, 256), (257, 11008, 64, 128, 258), (64, 1024, 128, 64, 8), (65, 384, 128, 64, 6)]
GEMM1_SHAPES = \
    [(m, _G1_N[(i + j) % 3], k, EPI_STORE) for i, m in enumerate(_G1_M) for j, k in enumerate(_G1_K)] + \
    [(m, n, k, EPI_STORE) for m, n, k, _, _ in GEMM1_FORMS] + \
    [(m, n, k, EPI_ADD) for m, n, k in ((65, 256, 192), (130, 128, 64), (129, 16384, 64))] + \
    [(m, n, k, e) for m, n, k in ((130, 256, 320), (129, 16384, 128)) for e in (EPI_STORE, EPI_ADD)] + \
    [(130, 256, 320, EPI_STORE), (257, 11008, 192, EPI_STORE), (130, 2 * 128, 320, EPI_SILU),
     (129, 2 * 8192, 192, EPI_SILU)] + \
    [(m, 2 * i, k, EPI_SILU) for m, i, k in ((65, 64, 128), (130, 128, 64), (1, 192, 192), (129, 8192, 64))] + \
    [(64, 128, 1024, EPI_STORE), (130, 256, 192, EPI_STORE), (9, 128, 64, EPI_STORE)]


def _gemm1_plan(**kw):
    F = 0x1000  # never dereferenced
    a = _lib.DebugGemm1Args()
    base = dict(a=F, w=F, y=F, w_dtype=_lib.F16, m=64, n=256, k=128, split=2, eps=1e-5)
    kw = dict(base, **kw)
    if kw.get("epi") == EPI_SILU:
        kw.setdefault("gamma", F)
        kw.setdefault("g_dtype", _lib.F16)
    kw.setdefault("lda", kw["k"])
    kw.setdefault("ldy", kw["n"] // 2 if kw.get("epi") == EPI_SILU else kw["n"])
    for key, v in kw.items():
        setattr(a, key, v)
    o = [C.c_int() for _ in range(2)]
    call("llmi_debug_gemm1_plan", C.byref(a), *[C.byref(x) for x in o])
    return tuple(x.value for x in o)


def _gemm1_model(m, n, k, epi):
    """gemm.hip's rule restated: 128 columns a tile (gate_up: 64 gate columns), rows by 128 iff
    ceil(m / 128) x column tiles >= 256, else by 64; one workgroup per tile."""
    nt = (n // 2) // 64 if epi == EPI_SILU else n // 128
    bm = 128 if -(-m // 128) * nt >= 256 else 64
    return bm, -(-m // bm) * nt


def test_debug_gemm1_plan_reports_the_launchers_choices():
    """llmi_debug_gemm1_plan launches and allocates nothing. bm and grid of every shape of
    tests/test_gpu_gemm1.py against the rule restated above (both weight types, both splits: the
    plan does not depend on them), the four forms by hand, then every argument check of
    gemm_plan."""
    F = 0x1000
    for m, n, k, epi in GEMM1_SHAPES:
        for wt, split in ((_lib.F16, 2), (_lib.I8, 1)):
            kw = dict(m=m, n=n, k=k, epi=epi, w_dtype=wt, scales=F, split=split)
            assert _gemm1_plan(**kw) == _gemm1_model(m, n, k, epi), kw
    for m, n, k, bm, grid in GEMM1_FORMS:
        assert _gemm1_plan(m=m, n=n, k=k) == (bm, grid)
    assert _gemm1_plan(m=129, n=2 * 8192, k=64, epi=EPI_SILU) == (128, 256)
    assert _gemm1_plan(m=128, n=16384, k=64) == (64, 256)                      # 1 x 128 tiles < 256
    assert _gemm1_plan(m=256, n=11008, k=64) == (64, 4 * 86)                    # 2 x 86 tiles < 256
    assert _gemm1_plan(m=257, n=4096, k=4096, w_dtype=_lib.I8, scales=F) == (64, 5 * 32)
    assert _gemm1_plan(m=512, n=3 * 5120, k=5120, w_dtype=_lib.I8, scales=F) == (128, 4 * 120)   # 13B qkv, 512 rows
    gam = dict(gamma=F, g_dtype=_lib.F16)
    silu = dict(epi=EPI_SILU, **gam)
    for bad in (dict(a=0), dict(w=0), dict(y=0), dict(m=0), dict(n=192), dict(k=96), dict(lda=124), dict(lda=130),
                dict(a=F + 8), dict(w=F + 8), dict(gamma=F + 4, g_dtype=_lib.F16), dict(gamma=F + 8, g_dtype=_lib.F32),
                dict(gamma=F, g_dtype=_lib.I8), dict(w_dtype=_lib.I8), dict(w_dtype=_lib.F32), dict(split=0),
                dict(split=3), dict(epi=3), dict(epi=EPI_SLAB), dict(epi=EPI_ADD, **gam), dict(epi=EPI_SILU, gamma=0),
                dict(silu, n=2 * 96), dict(ldy=255), dict(silu, ldy=127), dict(n=0), dict(k=0)):
        with pytest.raises(_lib.LlmiError):
            _gemm1_plan(**bad)
    # the forms the refusals start from are accepted
    for ok in (dict(), dict(lda=132), gam, dict(gamma=F + 8, g_dtype=_lib.F16), dict(gamma=F, g_dtype=_lib.F32),
               dict(w_dtype=_lib.I8, scales=F), dict(split=1), dict(epi=EPI_ADD), dict(ldy=264)):
        assert _gemm1_plan(**ok) == (64, 2)
    assert _gemm1_plan(**silu) == (64, 2) and _gemm1_plan(**dict(silu, ldy=128)) == (64, 2)
    with pytest.raises(_lib.LlmiError):
        call("llmi_debug_gemm1_plan", None, C.byref(C.c_int()), C.byref(C.c_int()))


def test_debug_gemv_plan_reports_the_launchers_choices():
    """llmi_debug_gemv_plan launches nothing, so its ladder is checked without a GPU: the
    x-staging width at each threshold (k / 4 float4s against 4, 5, 11, 14 x 256), the unroll
    that pads the row's chunk count least, the grid of each form, and the launcher's argument
    checks (the plan runs the same ones)."""
    F = 0x1000  # never dereferenced

    def plan(**kw):
        a = _lib.DebugGemvArgs()
        for key, v in dict(dict(w=F, scales=F, x=F, y=F, w_dtype=_lib.F16, n_rows=37, k=4096), **kw).items():
            setattr(a, key, v)
        g, u, x = C.c_int(), C.c_int(), C.c_int()
        call("llmi_debug_gemv_plan", C.byref(a), C.byref(g), C.byref(u), C.byref(x))
        return g.value, u.value, x.value

    assert [plan(k=k)[2] for k in (4096, 4104, 5120, 5128, 11264, 11272, 14336, 14344)] == [4, 5, 5, 11, 11, 14, 14, 0]
    assert [plan(k=k)[1] for k in (2048, 2560, 4096, 13824)] == [4, 5, 8, 4]         # 256, 320, 512, 1728 chunks
    assert plan(k=5120, w_dtype=_lib.I8)[1:] == (5, 5) and plan(k=5120, w_dtype=_lib.F32)[1:] == (4, 5)
    assert plan()[0] == 5 and plan(grid=3)[0] == 3
    assert plan(n_rows=1536, x=0, x_fixed=F, gamma=F, kpar=2)[:2] == (384, 4)       # one group a wave pair
    assert plan(n_rows=4096, epi=4, yacc=F, ksplit=8) == (1024, 4, 4)                # 128 blocks x 8 slices of 64 chunks
    assert plan(n_rows=16384, epi=3, partials=F)[0] == 1024                          # the grid cap
    assert plan(n_rows=2 * 11008, epi=2, pair_off=11008)[:2] == (1024, 4)            # many groups: unroll 4
    for bad in (dict(epi=4, yacc=F, yacc_single=1, ksplit=2), dict(yacc_single=1), dict(ldw=4098), dict(ldw=4088),
                dict(epi=5), dict(kpar=2, grid=2), dict(k=4100)):
        with pytest.raises(_lib.LlmiError):
            plan(**bad)
