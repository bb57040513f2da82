"""attn_prefill_q8_kernel (csrc/prefill.hip): the MFMA prefill attention over the int8 KV cache,
through llmi_debug_prefill_attn (q8_planes = 1 / 2) and through the engine.

Reference: float64 causal softmax attention of the read-back rotated q over the read-back
dequantised cache rows [0, p0 + m); error: the maximum over (row, head) of the rel-L2 over the
head's 128 outputs. Every case: max_seq 512, cache rows from p0 + m on poisoned (NaN scale bits,
bytes 0x80), the split workspace pre-filled with NaNs. Case8, Buf, launch (sentinels checked at
every read-back), attn_ref and rowhead_err are test_gpu_kv8_kernels'."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_kv8_kernels as K  # noqa: E402
from test_gpu_kv8_kernels import ops  # noqa: E402,F401  (the module fixture)
from llmi import _lib  # noqa: E402

D = 128
BAR = 2e-6  # P = 2: the project's attention bar
# P = 1: 2 x the largest error of the fp16-cache mfma_planes = 1 kernel (the parent commit's
# instructions) on P1_CASES against float64: 4.774e-4, 9.736e-4, 8.284e-4 -> 2 x 9.736e-4
BAR_P1 = 1.947e-3
LOGIT_TOL = 1e-3  # tests/test_gpu_engine.py
SHAPES = [(0, 1), (0, 64), (0, 65), (31, 33), (63, 2), (100, 130), (300, 70)]
HEADSETS = [(4, 4), (8, 2), (9, 3)]
P1_CASES = [(0, 65, 8, 2), (100, 130, 9, 3), (300, 70, 4, 4)]


def case(p0, m, heads, kvh, seed=7):
    c = K.Case8(p0, m, heads, kvh, seed=seed, max_seq=512)
    c.img.kq[:, p0 + m:] = -128  # the scales of rows >= p0 are NaN already (cache_image)
    c.img.vq[:, p0 + m:] = -128
    return c


def chunk_form(c, form):
    """Keywords of a chunk form: none (no workspace), auto, cb1 (one key block per chunk)."""
    if form == "none":
        return {}
    ws = K.Buf(c.heads * -(-c.m // 64) * 8 * (64 * D + 128))  # starts as NaNs
    return dict(split_ws=ws.t, split_ws_floats=ws.n, **({"chunk_blocks": 1} if form == "cb1" else {}))


def err_of(c, r, rows=slice(None), heads=None):
    hs = list(range(c.heads)) if heads is None else heads
    out = r.out.reshape(c.m, c.heads, D)[rows][:, hs]
    assert np.isfinite(out).all(), c.tag
    ref = K.attn_ref(c, r, heads=hs).reshape(c.m, c.heads, D)[rows][:, hs]
    return K.rowhead_err(out, ref, len(hs))


@pytest.mark.parametrize("form", ["none", "auto", "cb1"])
@pytest.mark.parametrize("heads,kvh", HEADSETS)
@pytest.mark.parametrize("p0,m", SHAPES)
def test_shapes_and_chunk_forms(ops, p0, m, heads, kvh, form):
    c = case(p0, m, heads, kvh)
    kw = chunk_form(c, form)
    r = K.launch(ops, c, q8_planes=2, **kw)
    assert r.plan == K.launch(ops, c, plan_only=True, cache_dtype=_lib.F16, mfma_planes=2, **kw).plan, r.plan
    if form == "cb1":
        assert r.plan[3] == {1: 0, 2: 2, 3: 4, 4: 4}.get(-(-(p0 + m) // 64), 8), r.plan
    e = err_of(c, r)
    K.report("kv8 MFMA attention P=2", f"{c.tag} {form} plan {r.plan}", e)
    assert e < BAR, (c.tag, form, e)
    scalar = K.launch(ops, c)  # q8_planes 0: the rope kernel is shared
    for a in ("kq", "ks", "vq", "vs", "qkv"):
        assert np.array_equal(K.bits(getattr(r, a)), K.bits(getattr(scalar, a))), (c.tag, a)
    K.check_untouched(c, r)
    again = K.launch(ops, c, q8_planes=2, **chunk_form(c, form))
    assert np.array_equal(K.bits(again.out), K.bits(r.out)), (c.tag, "two identical launches differ")


@pytest.mark.parametrize("p0,m,heads,kvh", P1_CASES)
def test_one_plane(ops, p0, m, heads, kvh):
    c = case(p0, m, heads, kvh)
    e = err_of(c, K.launch(ops, c, q8_planes=1, **chunk_form(c, "auto")))
    K.report("kv8 MFMA attention P=1", c.tag, e)
    assert e < BAR_P1, (c.tag, e)


def test_output_planes(ops, form="none"):
    """hi = fp16(v), lo = fp16(v - hi), bitwise, from the v the fp32-output launch stores: the
    kernel's own store (the merge kernel's is the fp16 form's: tests/test_gpu_prefill_kernels.py)."""
    c = case(100, 130, 8, 2)
    v = K.launch(ops, c, q8_planes=2, **chunk_form(c, form)).out
    hi_want = v.astype(np.float16)
    lo_want = (v - hi_want.astype(np.float32)).astype(np.float16)
    for planes in (1, 2):
        hi, lo = K.Buf(v.size, "scale"), K.Buf(v.size, "scale")
        K.launch(ops, c, q8_planes=2, out=None, out_hi=hi.t, out_lo=lo.t if planes == 2 else None, **chunk_form(c, form))
        assert np.array_equal(hi.get(), K.bits(hi_want).reshape(-1)), "hi"
        if planes == 2:
            assert np.array_equal(lo.get(), K.bits(lo_want).reshape(-1)), "lo"
        else:
            assert lo.untouched()


@pytest.mark.parametrize("what", ["spread", "2^17", "inf"])
def test_v_scale_handling(ops, what):
    """V amplitudes over 2^-6 .. 2^6; all at 2^17 (p s_v would overflow an fp16 plane); +inf in kv
    head 1's V row of prompt row 70 (the NaN scale over zero bytes)."""
    c = case(0, 130, 8, 2)
    v = c.qkv[:, (8 + 2) * D:].reshape(c.m, 2, D)
    if what == "inf":
        v[70, 1, 17] = np.inf
    else:
        v *= np.float32(2.0 ** 17) if what == "2^17" else (2.0 ** np.random.default_rng(3).uniform(-6, 6, (c.m, 2, 1))).astype(np.float32)
    r = K.launch(ops, c, q8_planes=2, **chunk_form(c, "cb1"))
    if what != "inf":
        e = err_of(c, r)
    else:
        assert r.vs[1, 70] == K.NAN_BITS and not np.isfinite(r.out.reshape(c.m, 8, D)[70:, 4:]).any()
        r.vs[1, 70] = 0x3C00  # for the reference: 0 x NaN is NaN in numpy, and the true weight is exactly 0
        e = max(err_of(c, r, rows=slice(0, 70)), err_of(c, r, heads=[0, 1, 2, 3]))
    K.report("kv8 MFMA attention P=2", f"{c.tag} V {what}", e)
    assert e < BAR, (what, e)


BAD = [dict(q8_planes=1, cache_dtype=_lib.F16), dict(q8_planes=2, cache_dtype=_lib.F16),
       dict(q8_planes=1, cache_dtype=_lib.F32), dict(q8_planes=2, cache_dtype=_lib.F32), dict(q8_planes=3),
       dict(q8_planes=1, mfma_planes=1), dict(q8_planes=2, k_scale=None), dict(q8_planes=2, v_scale=None),
       dict(q8_planes=2, out_lo8=1), dict(q8_planes=2, out=None)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_refusals(ops, bad):
    c = case(0, 8, 4, 4)
    im = c.img
    src = dict(qkv=(c.qkv, "f32"), k_cache=(im.kq, "i8"), v_cache=(im.vq, "i8"), k_scale=(im.ks, "scale"),
               v_scale=(im.vs, "scale"))
    bufs = {k: K.Buf(a.size, kind, a) for k, (a, kind) in src.items()}
    out, hi = K.Buf(c.m * c.heads * D), K.Buf(c.m * c.heads * D, "scale")
    a = dict({k: b.t for k, b in bufs.items()}, cache_dtype=_lib.I8, max_seq=c.max_seq, m=c.m, p0=c.p0, heads=c.heads,
             kv_heads=c.kvh, rope_tab=K.T(c.tab), out=out.t, out_hi=hi.t if "out_lo8" in bad else None)
    a.update(bad)
    for call in (ops.debug_prefill_attn_plan, ops.debug_prefill_attn):
        with pytest.raises(_lib.LlmiError, match=K.EINVAL):
            call(**a)
    for k, (arr, _) in src.items():
        assert np.array_equal(K.bits(bufs[k].get()), K.bits(arr.reshape(-1))), k
    assert out.untouched() and hi.untouched()


def _rows(e, n):
    got = [e.kv_slot_q8(l, p, bool(v)) for l in (0, 1) for p in range(n) for v in (0, 1)]
    return np.stack([g[0] for g in got]).astype(np.int32), np.stack([g[1] for g in got]).astype(np.int32)


def _rows_close(got, want):  # the caps of tests/test_gpu_engine_kv8.py
    assert np.abs(got[1] - want[1]).max() <= 1
    diff = np.abs(got[0] - want[0])
    assert diff.max() <= 1 and (diff != 0).mean() <= 0.01, (int(diff.max()), float((diff != 0).mean()))


@pytest.mark.parametrize("wname", ["f16", "i8"])
def test_engine_prefill_against_decode_only(wname):
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-7b", layers=2, max_seq=128, kv_dtype=llmi.I8, weight_dtype=dict(f16=llmi.F16, i8=llmi.I8)[wname])
    prompt = synth_prompt(5, 8, cfg.vocab)
    with Engine(cfg) as e:
        e.load_synthetic(2)
        want = (e.generate(prompt, 8, use_graph=False).copy(), e.logits().copy(), _rows(e, 8))
        runs = {}
        for exact in (1, 2):
            runs[exact] = (e.generate(prompt, 8, prefill=True, exact=exact).copy(), e.logits().copy(), _rows(e, 8))
        e.set_prompt(prompt)
        e.decode(3, use_graph=False)
        e.prefill(5)
        e.decode(7)
        runs["3 + 5"] = (e.tokens(16)[8:].copy(), e.logits().copy(), _rows(e, 8))
    for tag in (1, "3 + 5"):
        toks, logits, rows = runs[tag]
        r = K.rel(logits, want[1])
        print(f"{wname} weights, int8 KV, prefill {tag}: logits rel-L2 vs decode-only {r:.3e}")
        np.testing.assert_array_equal(toks, want[0])
        assert r < LOGIT_TOL
        _rows_close(rows, want[2])
    np.testing.assert_array_equal(runs[1][0], runs[2][0])  # the fp8-lo mode falls back to the exact planes
    assert np.array_equal(K.bits(runs[1][1]), K.bits(runs[2][1]))
    assert all(np.array_equal(a, b) for a, b in zip(runs[1][2], runs[2][2]))
