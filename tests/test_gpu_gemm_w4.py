"""gemm_w4_kernel (csrc/gemm_w4.hip), the int4-weight prefill GEMM, through the test hook
llmi_debug_gemm_w4 (planes, LLMI_I4 bytes and fp16 group scales fed directly) and through the
engine (option "w4_gemm" 1).

  a  integers: planes in [-4, 4] (hi and lo independent), q over [-8, 7] (nibble 0 included),
     power-of-two scales that differ between rows r, r + 1, r + 16, r + 64 and between groups: with
     K <= 768 every partial sum is an integer below 2^24 times a power of two, so y is BITWISE the
     int64 result whatever the order.
  b  gate_up on Gaussian planes against float64 silu(g) u of the dequantised weights: 2e-6.
  c  real data, two planes of x ~ N(0, 1), Gaussian weights through quant_i4_ref: 2e-6 against float64.
  d  the engine: prefill against the decode-only run; the scored prefill against stepped scores.
  e  the launcher's and the engine's refusals, outputs untouched.
Outputs follow tests/test_gpu_gemm_w8.py: sentinels behind the end, ldy = n + 8, two spare rows, a
NaN start; A has lda = k + 8 with NaN padding. The 16384-column shapes are the smallest that take
the 128-row tile under STORE and SILU_MUL (row tiles x column tiles >= 256)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import logprob_ref as L  # noqa: E402
from i4_ref import dequant, pack, quant_i4_ref  # noqa: E402
from llmi import _lib  # noqa: E402
from test_gpu_prefill_gemm import BAR, Out, T, bits, ops, padded, rel  # noqa: E402,F401

STORE, SILU, SLAB = 0, 2, 5
LOGIT_TOL = 1e-3  # tests/test_gpu_prefill.py, tests/test_gpu_gemm_w8.py


def launch(ops, m, n, k, hi, q, s, lo=None, epi=STORE, ks=0, planes_out=0, **over):
    """One llmi_debug_gemm_w4 launch on fresh device copies (q int [n, k] packed here); returns
    the read-back output(s): y [m, n], the slab [ks, m, n], or the (y_hi, y_lo) planes. `over`
    replaces hook fields."""
    lda, n_out = k + 8, n // 2 if epi == SILU else n
    ldy = n_out + 8
    pl = [T(padded(np.asarray(p, np.float16), lda, np.float16(np.nan))) for p in (hi, lo) if p is not None]
    keep = [T(pack(q)), T(np.asarray(s, np.float16))]
    a = dict(a_hi=pl[0], a_lo=pl[1] if lo is not None else None, planes=len(pl), lda=lda, w=keep[0], scales=keep[1],
             m=m, n=n, k=k, epi=epi, pair_off=n // 2 if epi == SILU else 0, ldy=ldy, ksplit=ks)
    if epi == SLAB:
        outs = [Out(ks * m + 2, ldy, ks * m, n)]
        a["slab"] = outs[0].t
    elif planes_out:
        outs = [Out(m + 2, ldy, m, n_out, dtype=torch.float16) for _ in range(planes_out)]
        a.update(zip(("y_hi", "y_lo"), (o.t for o in outs)))
    else:
        outs = [Out(m + 2, ldy, m, n_out)]
        a["y"] = outs[0].t
    a.update(over)
    try:
        ops.debug_gemm_w4(**a)
    except _lib.LlmiError:
        assert all((bits(o.read()) == o.b.pat).all() for o in outs), "a refused call wrote its output"
        raise
    got = [o.read() for o in outs]
    return got[0].reshape(ks, m, n) if epi == SLAB else got if planes_out else got[0]


def int_case(m, n, k, planes):
    rng = np.random.default_rng([41, m, n, k])
    hi, lo = rng.integers(-4, 5, (2, m, k))
    q = rng.integers(-8, 8, (n, k))
    r, g = np.arange(n)[:, None], np.arange(k // 128)[None, :]
    s = 2.0 ** ((r + r // 16 + 3 * g) % 5 - 2)
    a = hi + lo if planes == 2 else hi
    return hi, (lo if planes == 2 else None), q, s, a.astype(np.int64)


def int_ref(a, q, s, k0=0, k1=None):
    """sum over the groups of columns [k0, k1) of s[n, g] * (a q^T over the group), exactly."""
    k1 = q.shape[1] if k1 is None else k1
    y = np.zeros((a.shape[0], q.shape[0]))
    for g in range(k0 // 128, k1 // 128):
        c = slice(128 * g, 128 * g + 128)
        y += (a[:, c] @ q[:, c].astype(np.int64).T) * s[:, g]
    return y.astype(np.float32)


def planes_of(x):
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


# ------------------------------------------------------------------ a. integers, bitwise
@pytest.mark.parametrize("m,n,k,planes", [(77, 256, 384, 1), (77, 256, 384, 2), (16, 128, 128, 2), (130, 16384, 128, 2)])
def test_a_store_integers(ops, m, n, k, planes):
    hi, lo, q, s, a = int_case(m, n, k, planes)
    np.testing.assert_array_equal(launch(ops, m, n, k, hi, q, s, lo=lo), int_ref(a, q, s))


@pytest.mark.parametrize("k", [512, 768])  # 768 / 2: an odd group count per slice (the 7B down GEMM's)
def test_a_slab_integers(ops, k, m=130, n=128, ks=2):
    hi, lo, q, s, a = int_case(m, n, k, 2)
    slab = launch(ops, m, n, k, hi, q, s, lo=lo, epi=SLAB, ks=ks)
    kk = k // ks
    for i in range(ks):
        np.testing.assert_array_equal(slab[i], int_ref(a, q, s, i * kk, (i + 1) * kk))
    np.testing.assert_array_equal(slab[0] + slab[1], int_ref(a, q, s))


# ------------------------------------------------------------------ b. gate_up
@pytest.mark.parametrize("m,n,k", [(77, 256, 256), (130, 16384, 256)])
def test_b_silu_pairing(ops, m, n, k):
    rng = np.random.default_rng([42, m, n, k])
    hi, lo = planes_of(rng.standard_normal((m, k)).astype(np.float32))
    q = rng.integers(-7, 8, (n, k))
    # gate rows near 2^-6, up rows near 2^-2: a swapped scale is off by 16
    s = (np.where(np.arange(n) < n // 2, 2.0 ** -6, 2.0 ** -2)[:, None] * rng.uniform(1, 2, (n, k // 128))).astype(np.float16)
    z = (hi.astype(np.float64) + lo.astype(np.float64)) @ dequant(q, s, np.float64).T
    g, u = z[:, :n // 2], z[:, n // 2:]
    want = g / (1 + np.exp(-g)) * u
    y_hi, y_lo = launch(ops, m, n, k, hi, q, s, lo=lo, epi=SILU, planes_out=2)
    e = rel(y_hi.astype(np.float64) + y_lo.astype(np.float64), want)
    print(f"[rel-L2] gemm_w4 silu_mul {m}x{n}x{k}: {e:.3e}")
    assert e < BAR


# ------------------------------------------------------------------ c. real data
def test_c_real_against_float64(ops, m=130, n=384, k=1024):
    rng = np.random.default_rng(43)
    x = rng.standard_normal((m, k)).astype(np.float32)
    hi, lo = planes_of(x)
    q, s, bad = quant_i4_ref(rng.standard_normal((n, k)).astype(np.float32))
    assert bad == 0
    want = x.astype(np.float64) @ dequant(q, s, np.float64).T
    e = rel(launch(ops, m, n, k, hi, q, s.view(np.float16), lo=lo), want)
    print(f"[rel-L2] gemm_w4 store {m}x{n}x{k}: {e:.3e}")
    assert e <= BAR


# ------------------------------------------------------------------ d. the engine
@pytest.mark.parametrize("kv", ["F16", "I8", "F32"])
def test_d_engine_prefill_against_decode_only(kv):
    """The F16 case also holds score(ids, prefill=True) to the stepped scores by the bound of
    tests/test_gpu_prefill_scored.py (test_against_the_decode_path): 2 max |dz| over the two logit
    rows of a position plus both logprob kernels' own tolerance."""
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-7b", layers=2, max_seq=128, weight_dtype=llmi.I4, kv_dtype=getattr(llmi, kv))
    prompt = synth_prompt(7, 96, cfg.vocab)
    with Engine(cfg) as e:
        e.load_synthetic(2)
        want = e.generate(prompt, 8, use_graph=False).copy(), e.logits().copy()
        if kv == "F16":
            e.set_logprobs(0)
            e.set_prompt(prompt)
            dec_rows = []
            for _ in range(len(prompt) - 1):
                e.decode(1, use_graph=False)
                dec_rows.append(e.logits().astype(np.float64))
            dec_lp = e.score(prompt)
            e.set_logprobs(-1)
        e.set_option("w4_gemm", 1)
        toks, logits = e.generate(prompt, 8, prefill=True).copy(), e.logits().copy()
        r = rel(logits, want[1])
        print(f"int4 weights, {kv} cache, w4_gemm 1: logits rel-L2 vs decode-only {r:.3e}")
        assert np.isfinite(logits).all()
        np.testing.assert_array_equal(toks, want[0])
        assert r < LOGIT_TOL
        if kv == "F16":
            got = e.score(prompt, prefill=True)
            assert got.shape == dec_lp.shape and np.isfinite(got).all()
            worst = 0.0
            for p in range(len(prompt) - 1):
                zs = e.scored_logits(p).astype(np.float64)
                bound = 2.0 * np.abs(zs - dec_rows[p]).max() + L.tolerance(len(zs), got[p]) + L.tolerance(len(zs), dec_lp[p])
                d = abs(float(got[p]) - float(dec_lp[p]))
                worst = max(worst, d / bound)
                assert rel(zs, dec_rows[p]) < LOGIT_TOL and d <= bound, (p, d, bound)
            print(f"int4 scored prefill: worst |dlp| / bound {worst:.3f}")


# ------------------------------------------------------------------ e. refusals
@pytest.mark.parametrize("k,over,code", [(192, {}, -2), (128, dict(scales=None), -1)])
def test_e_refusals(ops, k, over, code):
    hi, lo, q, _, _ = int_case(16, 128, 256, 2)
    hi, lo, q, s = hi[:, :k], lo[:, :k], q[:, :k], np.ones((128, 2))
    with pytest.raises(_lib.LlmiError, match=rf"\({code}\)"):
        launch(ops, 16, 128, k, hi, q, s, lo=lo, **over)
    with pytest.raises(_lib.LlmiError, match=rf"\({code}\)"):
        launch(ops, 16, 128, k, hi, q, s, lo=lo, epi=SLAB, ks=1, **over)


def test_e_engine_refuses_an_unsupported_shape():
    """inter 24704 = 193 groups in one K slice (odd: no split), one more than the down GEMM's
    scale block holds in LDS."""
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("tiny", layers=1, inter=24704, weight_dtype=llmi.I4)
    prompt = synth_prompt(7, 24, cfg.vocab)
    with Engine(cfg) as e:
        e.load_synthetic(2)
        want = e.generate(prompt, 8, use_graph=False).copy()
        e.set_option("w4_gemm", 1)
        e.set_prompt(prompt)
        with pytest.raises(_lib.LlmiError, match=r"\(-2\).*int4.*multiple of 128"):
            e.prefill(len(prompt))
        np.testing.assert_array_equal(e.generate(prompt, 8), want)
