"""The KV8 cache format on the CPU: the row rule's edge cases in its numpy restatement
(tests/kv8_ref.py), and what the format costs on the tiny model of tests/golden/tiny.npz -- the
int8-KV oracle is measurably further from the fp32-KV oracle than the fp16-KV oracle is (so an
engine test can tell a quantising engine from one that does not quantise) and still picks the same
greedy tokens."""
import os

import numpy as np

import kv8_ref
from oracle import llama_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = 8


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def test_zero_row():
    q, b = kv8_ref.quant_rows(np.zeros((2, 128), np.float32))
    assert (b == 0x0001).all() and (q == 0).all()
    # below half the smallest fp16 subnormal the scale is still 2^-24
    x = np.zeros((1, 128), np.float32)
    x[0, 5] = 1e-9
    q, b = kv8_ref.quant_rows(x)
    assert b[0] == 0x0001 and (q == 0).all()


def test_scale_saturates_at_65504():
    for amax in (127.0 * 65504.0, 127.0 * 65520.0, 1e10, 3e38):
        x = np.zeros((1, 128), np.float32)
        x[0, 3], x[0, 4] = amax, -amax
        q, b = kv8_ref.quant_rows(x)
        assert b[0] == 0x7BFF, (amax, hex(b[0]))
        assert q[0, 3] == 127 and q[0, 4] == -127 and np.abs(q.astype(np.int32)).max() == 127
    x = np.zeros((1, 128), np.float32)
    x[0, 0] = 127.0 * 65472.0  # rounds to 65472 in fp16 (even), below the cap
    assert kv8_ref.quant_rows(x)[1][0] < 0x7BFF


def test_non_finite_rows():
    x = np.ones((3, 128), np.float32)
    x[0, 7], x[1, 9] = np.nan, -np.inf
    q, b = kv8_ref.quant_rows(x)
    assert b[0] == 0x7E00 and b[1] == 0x7E00 and b[2] != 0x7E00
    assert (q[:2] == 0).all() and (q[2] == 127).all()
    assert np.isnan(kv8_ref.dequant(q, b)[:2]).all() and np.isfinite(kv8_ref.dequant(q, b)[2]).all()


def test_half_even_ties_and_range():
    # amax 127 -> s = 1 exactly: x is its own quotient
    x = np.zeros((1, 128), np.float32)
    x[0, :9] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -126.5]
    q, b = kv8_ref.quant_rows(x)
    assert b.view(np.float16)[0] == 1.0
    assert q[0, :9].tolist() == [127, 0, 2, 2, 0, -2, -2, 126, -126]
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((64, 128)) * np.exp(rng.uniform(-4, 10, (64, 1)))).astype(np.float32)
    q, b = kv8_ref.quant_rows(x)  # (scales in fp16's normal range: 2^-11 relative rounding)
    assert np.abs(q.astype(np.int32)).max() <= 127 and (np.abs(q.astype(np.int32)).max(axis=1) >= 126).all()
    # within half a step of the input (the scale rounds up or down by at most 2^-11 relative)
    s = b.view(np.float16).astype(np.float32)
    assert (np.abs(kv8_ref.qdq(x) - x) <= 0.5 * s[:, None] * (1 + 2.0 ** -10) + np.abs(x) * 2.0 ** -10).all()
    # the same bits as the project's W8A16 restatement on the row
    amax = np.abs(x).max(axis=1).astype(np.float32)
    want = (amax / np.float32(127.0)).astype(np.float32).astype(np.float16).view(np.uint16)
    np.testing.assert_array_equal(b, want)


def test_shapes_follow_the_leading_axes():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 3, 5, 128)).astype(np.float32)
    q, b = kv8_ref.quant_rows(x)
    assert q.shape == x.shape and b.shape == x.shape[:-1]
    q2, b2 = kv8_ref.quant_rows(x.reshape(-1, 128))
    np.testing.assert_array_equal(q.reshape(-1, 128), q2)
    np.testing.assert_array_equal(b.reshape(-1), b2)


def _rot32(x, pos, tab, order):
    """The prefill write kernel's fp32 rotation of x [rows, n_heads, 128], restated. plain:
    a*c - b*s, every operation rounded; fma: fma(a, c, -(b*s)), the product b*s rounded to fp32
    and the rest computed in float64 and rounded once."""
    c, s = tab[pos, :, 0][:, None, :], tab[pos, :, 1][:, None, :]
    a0, a1 = x[..., :64], x[..., 64:]
    if order == "plain":
        return np.concatenate([a0 * c - a1 * s, a1 * c + a0 * s], axis=-1)
    f = np.float64
    r0 = a0.astype(f) * c.astype(f) - (a1 * s).astype(f)
    r1 = a1.astype(f) * c.astype(f) + (a0 * s).astype(f)
    return np.concatenate([r0, r1], axis=-1).astype(np.float32)


def test_identity_and_quarter_turn_tables_rotate_exactly_in_both_orders():
    """What tests/test_gpu_kv8_kernels.py compares the kernel with bitwise, on its own cases."""
    import test_gpu_kv8_kernels as G
    for table in ("identity", "quarter"):
        for p0, m, heads, kvh, two, max_seq in G.write_cases():
            c = G.Case8(p0, m, heads, kvh, qkv2=two, table=table, max_seq=max_seq)
            for x in c.parts()[:2]:
                want = c.exact_rotation(x)
                for order in ("plain", "fma"):
                    got = _rot32(x, c.pos, c.tab, order)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c.tag, order)


def test_both_fp32_rotation_orders_meet_the_write_caps():
    """The real-table caps the GPU module holds the kernel to are met by the fp32 expression
    itself, plain and contracted, on every real-table case of that module (same generator)."""
    import test_gpu_kv8_kernels as G
    for c in G.real_table_cases():
        q, k, _ = c.parts()
        wk, wks = kv8_ref.quant_rows(G.rotate64(k, c.pos, c.tab).astype(np.float32))
        for order in ("plain", "fma"):
            gk, gks = kv8_ref.quant_rows(_rot32(k, c.pos, c.tab, order))
            nadj, nbytes = G.write_caps(gk, gks, wk, wks, (c.tag, order))
            rq = G.rel(_rot32(q, c.pos, c.tab, order), G.rotate64(q, c.pos, c.tab))
            print(f"{c.tag} {order}: {nadj} of {wks.size} rows adjacent, {nbytes} of {wk.size} bytes differ, q {rq:.2e}")
            assert rq < G.BAR


def test_requantising_a_dequantised_row_with_a_full_scale_byte_is_the_identity():
    """x = q * s with max |q| = 127: amax / 127 = s exactly, so quant_rows(x) = (q, s), over the
    full range of scale bits (subnormal scales and 65504 included)."""
    rng = np.random.default_rng(2)
    sb = rng.integers(1, 0x7BFF + 1, 1000).astype(np.uint16)
    sb[:4] = [0x0001, 0x03FF, 0x0400, 0x7BFF]
    q = rng.integers(-127, 128, (1000, 128)).astype(np.int8)
    q[np.arange(1000), rng.integers(0, 128, 1000)] = np.where(rng.random(1000) < 0.5, 127, -127)
    x = kv8_ref.dequant(q, sb)
    assert np.isfinite(x).all()
    q2, sb2 = kv8_ref.quant_rows(x)
    np.testing.assert_array_equal(sb2, sb)
    np.testing.assert_array_equal(q2, q)


def test_gpu_module_cache_images_poison_every_row_outside_the_real_range():
    import test_gpu_kv8_kernels as G
    images = [G.decode_image(8, 2, ctx, True)[0] for ctx in (1, 2, 65, 256)]
    images += [G.Case8(p0, m, 12, 4).img for p0, m in G.SCALAR_CASES] + [G.Case8(*G.WIDE[:4], max_seq=G.WIDE[4]).img]
    for im in images:
        n = im.n_real
        for q, s in ((im.kq, im.ks), (im.vq, im.vs)):
            assert (s[:, n:] == kv8_ref.NAN_BITS).all() and np.isnan(kv8_ref.dequant(q[:, n:], s[:, n:])).all()
            assert (s[:, :n] != kv8_ref.NAN_BITS).all() and np.isfinite(kv8_ref.dequant(q[:, :n], s[:, :n])).all()
            assert (q[:, n:] != 0).any() or n == q.shape[1]   # random bytes, not zeros, under the NaN scale
    # per-row amplitudes: the real rows' scales spread over more than a factor 8 (K) and 32 (V)
    im = G.decode_image(8, 2, 256, True)[0]
    for s, spread in ((im.ks, 8.0), (im.vs, 32.0)):
        f = s[:, :im.n_real].view(np.float16).astype(np.float64)
        assert f.max() / f.min() > spread


def test_tiny_model_int8_kv_is_visible_and_keeps_the_tokens():
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    seed, prompt = int(f["seed"]), np.asarray(f["prompt"], np.int32)
    cfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=4, inter=1024, layers=2, max_seq=64)
    w = R.make_model_weights(cfg, seed)
    t32, l32 = R.LlamaOracle(cfg, weights=w).greedy(prompt, N_NEW)
    t16, l16 = R.LlamaOracle(cfg, weights=w, kv_dtype=np.float16).greedy(prompt, N_NEW)
    t8, l8 = kv8_ref.Kv8Oracle(cfg, weights=w).greedy(prompt, N_NEW)
    d16, d8 = _rel(l16, l32), _rel(l8, l32)
    print(f"logits rel-L2 vs the fp32-KV oracle: fp16 KV {d16:.3e}, int8 KV {d8:.3e}")
    assert d8 > 10 * d16
    np.testing.assert_array_equal(t8, t32)
    np.testing.assert_array_equal(t16, t32)
    # prefill of the prompt writes the rows the token-by-token run writes (same rule, same rows)
    a, b = kv8_ref.Kv8Oracle(cfg, weights=w), kv8_ref.Kv8Oracle(cfg, weights=w)
    a.prefill(prompt)
    for t in prompt:
        b.forward_token(int(t))
    n = len(prompt)
    qa, sa = kv8_ref.quant_rows(a.k_cache[:, :, :n])
    qb, sb = kv8_ref.quant_rows(b.k_cache[:, :, :n])
    assert (np.abs(qa.astype(np.int32) - qb) <= 1).all() and (qa != qb).mean() <= 0.01
