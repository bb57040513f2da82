"""gemm_w8_kernel (csrc/gemm_w8.hip), the int8-weight prefill GEMM, through the test hook
llmi_debug_gemm_w8 (planes, int8 weights and fp16 row scales fed directly) and through the engine.

  a  integers: planes in [-4, 4] (hi and lo independent), q over [-127, 127], power-of-two row
     scales: with K <= 512 every product, sum and scaling is an exact fp32 integer (|sum| <=
     512 x 8 x 127 < 2^24) whatever the order, so y is BITWISE the int64 product times the scale.
  b  gate_up on Gaussian planes against float64 silu(g) u of the dequantised weights: 2e-6.
  c  real data, two planes of x ~ N(0, 1), the synthetic int8 weights: 2e-6 against float64.
  d  the engine: prefill against the decode-only run, option "w8_gemm" 1 and 0.
  e  the launcher's refusals, outputs untouched.
Outputs follow tests/test_gpu_prefill_gemm.py: sentinels behind the end, ldy = n + 8, two spare
rows, a NaN start; A has lda = k + 8 with NaN padding. The 16384-column shapes are the smallest
that take the 128-row tile under STORE and SILU_MUL (row tiles x column tiles >= 256)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from oracle import prng  # noqa: E402
from test_gpu_prefill_gemm import BAR, Out, T, bits, ops, padded, rel  # noqa: E402,F401

STORE, SILU, SLAB = 0, 2, 5
LOGIT_TOL = 1e-3  # tests/test_gpu_prefill.py, tests/test_gpu_prefill_q8.py


def launch(ops, m, n, k, hi, w, s, lo=None, epi=STORE, ks=0, planes_out=0, **over):
    """One llmi_debug_gemm_w8 launch on fresh device copies; returns the read-back output(s):
    y [m, n], the slab [ks, m, n], or the (y_hi, y_lo) planes. `over` replaces hook fields."""
    lda, n_out = k + 8, n // 2 if epi == SILU else n
    ldy = n_out + 8
    pl = [T(padded(np.asarray(p, np.float16), lda, np.float16(np.nan))) for p in (hi, lo) if p is not None]
    keep = [T(w), T(np.asarray(s, np.float16))]
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
        ops.debug_gemm_w8(**a)
    except _lib.LlmiError:
        assert all((bits(o.read()) == o.b.pat).all() for o in outs), "a refused call wrote its output"
        raise
    got = [o.read() for o in outs]
    return got[0].reshape(ks, m, n) if epi == SLAB else got if planes_out else got[0]


def int_case(m, n, k, planes):
    rng = np.random.default_rng([31, m, n, k])
    hi, lo = rng.integers(-4, 5, (2, m, k))
    q = rng.integers(-127, 128, (n, k)).astype(np.int8)
    r = np.arange(n)
    s = 2.0 ** ((r + r // 16) % 5 - 2)  # rows r and r + 1, 16, 32, 64 differ
    a = hi + lo if planes == 2 else hi
    return hi, (lo if planes == 2 else None), q, s, a.astype(np.int64), q.astype(np.int64)


# ------------------------------------------------------------------ a. integers, bitwise
@pytest.mark.parametrize("m,n,k,planes", [(77, 256, 384, 1), (77, 256, 384, 2), (16, 128, 128, 2), (130, 16384, 128, 2)])
def test_a_store_integers(ops, m, n, k, planes):
    hi, lo, q, s, a, q64 = int_case(m, n, k, planes)
    y = launch(ops, m, n, k, hi, q, s, lo=lo)
    np.testing.assert_array_equal(y, ((a @ q64.T) * s).astype(np.float32))


def test_a_slab_integers(ops, m=130, n=128, k=512, ks=2):
    hi, lo, q, s, a, q64 = int_case(m, n, k, 2)
    slab = launch(ops, m, n, k, hi, q, s, lo=lo, epi=SLAB, ks=ks)
    kk = k // ks
    for i in range(ks):
        np.testing.assert_array_equal(slab[i], ((a[:, i * kk:(i + 1) * kk] @ q64[:, i * kk:(i + 1) * kk].T) * s).astype(np.float32))
    np.testing.assert_array_equal(slab[0] + slab[1], ((a @ q64.T) * s).astype(np.float32))


# ------------------------------------------------------------------ b. gate_up
@pytest.mark.parametrize("m,n,k", [(77, 256, 256), (130, 16384, 256)])
def test_b_silu_pairing(ops, m, n, k):
    rng = np.random.default_rng([32, m, n, k])
    x = rng.standard_normal((m, k)).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    q = rng.integers(-127, 128, (n, k)).astype(np.int8)
    # gate rows near 2^-9, up rows near 2^-5: a swapped scale is off by 16
    s = (np.where(np.arange(n) < n // 2, 2.0 ** -9, 2.0 ** -5) * rng.uniform(1, 2, n)).astype(np.float16)
    xp = hi.astype(np.float64) + lo.astype(np.float64)
    z = xp @ (q.astype(np.float64) * s.astype(np.float64)[:, None]).T
    g, u = z[:, :n // 2], z[:, n // 2:]
    want = g / (1 + np.exp(-g)) * u
    y_hi, y_lo = launch(ops, m, n, k, hi, q, s, lo=lo, epi=SILU, planes_out=2)
    e = rel(y_hi.astype(np.float64) + y_lo.astype(np.float64), want)
    print(f"[rel-L2] gemm_w8 silu_mul {m}x{n}x{k}: {e:.3e}")
    assert e < BAR


# ------------------------------------------------------------------ c. real data
def test_c_real_against_float64(ops, m=130, n=384, k=1024):
    x = np.random.default_rng(33).standard_normal((m, k)).astype(np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    q, s = prng.int8_weight(5, 1, n, k), prng.int8_row_scale(5, 1, n)
    want = x.astype(np.float64) @ (q.astype(np.float64) * s.astype(np.float64)[:, None]).T
    e = rel(launch(ops, m, n, k, hi, q, s, lo=lo), want)
    print(f"[rel-L2] gemm_w8 store {m}x{n}x{k}: {e:.3e}")
    assert e <= BAR


# ------------------------------------------------------------------ d. the engine
@pytest.mark.parametrize("kv", ["F16", "I8", "F32"])
def test_d_engine_prefill_against_decode_only(kv):
    import llmi
    from llmi.engine import Engine, preset, synth_prompt
    cfg = preset("llama2-7b", layers=2, max_seq=128, weight_dtype=llmi.I8, kv_dtype=getattr(llmi, kv))
    prompt = synth_prompt(7, 96, cfg.vocab)
    with Engine(cfg) as e:
        e.load_synthetic(2)
        want = e.generate(prompt, 8, use_graph=False).copy(), e.logits().copy()
        for opt in (1, 0):
            e.set_option("w8_gemm", opt)
            toks, logits = e.generate(prompt, 8, prefill=True).copy(), e.logits().copy()
            r = rel(logits, want[1])
            print(f"int8 weights, {kv} cache, w8_gemm {opt}: logits rel-L2 vs decode-only {r:.3e}")
            assert np.isfinite(logits).all()
            np.testing.assert_array_equal(toks, want[0])
            assert r < LOGIT_TOL


# ------------------------------------------------------------------ e. refusals
@pytest.mark.parametrize("k,over,code", [(192, {}, -2), (128, dict(scales=None), -1)])
def test_e_refusals(ops, k, over, code):
    hi, lo, q, s, _, _ = int_case(16, 128, k, 2)
    with pytest.raises(_lib.LlmiError, match=rf"\({code}\)"):
        launch(ops, 16, 128, k, hi, q, s, lo=lo, **over)
    with pytest.raises(_lib.LlmiError, match=rf"\({code}\)"):
        launch(ops, 16, 128, k, hi, q, s, lo=lo, epi=SLAB, ks=1, **over)
