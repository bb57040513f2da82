"""The o_proj merge sized by the live split count (csrc/attn_impl.h oproj_body / oproj_body2): a
host-sized launch (nact > 0) runs the kernel instantiated on its split bucket -- 8, 16, 24 or 32
register-held partials, the loop past 32 -- and loads only its nact partials, each split's (m, l)
as one 8-byte load.

Operator level (llmi_debug_attn_oproj, test_gpu_engine_kernels._ao_case): every context at a
split or bucket edge of max_seq 2176 (34 splits, so the last one runs the loop past 32) against
the float64 numpy restatement at that file's bar (rel-L2 < 4e-6 after heads * 2^-33 a row), the
workspace full of NaN patterns before each launch, and bitwise against the position-derived launch
(nact = 0) on the same inputs: that form loads every slot and lets selects decide, as every launch
did before the buckets, so equal integers mean the bucket changed no xacc bit. Shapes: the tiny
config's (4 heads, 512 rows: one row a group), 7B width (32 heads, 4096 rows: the two-heads fp16
kernel) and 13B width with int8 W_o (40 heads, 5120 rows), fp16 and fp32 caches.

Engine level: graph replay == eager launches, bit for bit, from context 1 past every bucket edge
and past 2048."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from llmi import _lib  # noqa: E402
from llmi.engine import Engine, preset, synth_prompt  # noqa: E402
from test_gpu_engine_kernels import _ao_case, ops  # noqa: E402,F401  (the module-scoped fixture)

MAX_SEQ = 2176  # 34 splits
# split edges (63 | 64 | 65), bucket edges (8 | 9 splits: 512 | 513; 24 | 25: 1536 | 1537), the last
# register slot (2047, 2048) and the loop past it (2113: 34 splits)
CTXS = [1, 63, 64, 65, 511, 512, 513, 1535, 1536, 1537, 2047, 2048, 2113]
# one context per bucket (5, 11, 18, 30 splits) and the loop (34)
CTXS_BUCKET = [300, 700, 1100, 1900, 2113]


def both_forms(ops, heads, n_rows, ctx, cache_dt, wdt="f16"):
    kw = dict(cache_dt=cache_dt, wdt=wdt, max_seq=MAX_SEQ, resid="fixed")
    _ao_case(ops, heads, heads, n_rows, ctx, host_sized=True, **kw)
    sized = _ao_case.last
    _ao_case(ops, heads, heads, n_rows, ctx, host_sized=False, **kw)
    np.testing.assert_array_equal(sized, _ao_case.last)


@pytest.mark.parametrize("cache_dt", [np.float16, np.float32])
@pytest.mark.parametrize("ctx", CTXS)
def test_oproj_buckets_tiny_width(ops, ctx, cache_dt):
    both_forms(ops, 4, 512, ctx, cache_dt)


@pytest.mark.parametrize("cache_dt", [np.float16, np.float32])
@pytest.mark.parametrize("ctx", CTXS)
def test_oproj_buckets_7b_width(ops, ctx, cache_dt):
    both_forms(ops, 32, 4096, ctx, cache_dt)


@pytest.mark.parametrize("ctx", CTXS_BUCKET)
def test_oproj_buckets_13b_int8(ops, ctx):
    both_forms(ops, 40, 5120, ctx, np.float16, wdt="i8")


@pytest.mark.parametrize("case", ["tiny_f16kv", "tiny_f32kv", "7b_one_layer_f16kv"])
def test_graph_equals_eager_across_buckets(case):
    """One captured step per split count against eager launches: tokens of every position, the last
    logits and hidden state, at context 520 (just past the 8 | 9 split bucket edge) and at 2120
    (every edge, and the loop past 32 splits)."""
    if case.startswith("tiny"):
        cfg = preset("tiny", max_seq=MAX_SEQ)
        cfg.weight_dtype = _lib.F16
    else:
        cfg = preset("llama2-7b", layers=1, max_seq=MAX_SEQ)
    cfg.kv_dtype = _lib.F32 if "f32kv" in case else _lib.F16
    prompt = synth_prompt(3, 8, cfg.vocab)
    out = {}
    with Engine(cfg) as e:
        e.load_synthetic(7)
        for n in (512, 2112):
            for g in (True, False):
                toks = e.generate(prompt, n, use_graph=g)
                out[(n, g)] = (toks.copy(), e.logits().copy(), e.hidden().copy())
    for n in (512, 2112):
        for i in range(3):
            np.testing.assert_array_equal(out[(n, True)][i], out[(n, False)][i])
        assert np.isfinite(out[(n, True)][1]).all()
