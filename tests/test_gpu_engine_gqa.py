"""Engine / batch option "gqa_attn" (csrc/attn_gqa.hip): the tiny model with 2 and 1 kv heads, fp16 and
int8 cache, 8 prompt ids + 70 greedy steps (max_seq 128: two splits) against the numpy oracle under
the bars of tests/test_gpu_engine.py and tests/test_gpu_engine_kv8.py for the default path."""
import os

import numpy as np
import pytest

import kv8_ref

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL, N_NEW, MAX_SEQ = 1e-3, 70, 128
CASES = pytest.mark.parametrize("kvh,kv", [(2, "F16"), (2, "I8"), (1, "F16"), (1, "I8")])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tiny():
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    return int(f["seed"]), np.asarray(f["prompt"], np.int32)


def _cfg(kvh, kv):
    import llmi
    from llmi.engine import preset
    return preset("tiny", kv_heads=kvh, max_seq=MAX_SEQ, kv_dtype=getattr(llmi, kv))


def _run(tiny, kvh, kv, option, use_graph=False):
    from llmi.engine import Engine
    with Engine(_cfg(kvh, kv)) as e:
        e.load_synthetic(tiny[0])
        e.set_option("gqa_attn", option)
        return e.generate(tiny[1], N_NEW, use_graph=use_graph).copy(), e.logits().copy()


@CASES
def test_tokens_and_logits_against_the_oracle_and_graph_replay(tiny, kvh, kv):
    ocfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=kvh, inter=1024, layers=2, max_seq=MAX_SEQ)
    want_t, want_l = R.LlamaOracle(ocfg, seed=tiny[0], kv_dtype=np.float32 if kv == "I8" else np.float16) \
        .greedy(tiny[1], N_NEW)
    bar = LOGIT_TOL
    if kv == "I8":  # an engine that kept its rows unquantised would sit at d8 from the quantising oracle
        t8, l8 = kv8_ref.Kv8Oracle(ocfg, seed=tiny[0]).greedy(tiny[1], N_NEW)
        bar, want_t, want_l = min(bar, _rel(l8, want_l) / 4), t8, l8
    toks, logits = _run(tiny, kvh, kv, 1)
    r = _rel(logits, want_l)
    print(f"kv_heads {kvh} {kv} cache, gqa_attn 1: logits rel-L2 to the oracle {r:.3e} (bar {bar:.3e})")
    np.testing.assert_array_equal(toks, want_t)
    assert r < bar
    gt, gl = _run(tiny, kvh, kv, 1, use_graph=True)
    np.testing.assert_array_equal(gt, toks)
    np.testing.assert_array_equal(_bits(gl), _bits(logits))


def test_mha_falls_back_to_the_default_path(tiny):
    on, off = _run(tiny, 4, "F16", 1), _run(tiny, 4, "F16", 0)
    np.testing.assert_array_equal(on[0], off[0])
    np.testing.assert_array_equal(_bits(on[1]), _bits(off[1]))


@pytest.mark.parametrize("kv", ["F16", "I8"])
def test_batch_slot_is_bitwise_the_engine(tiny, kv):
    from llmi.engine import Batch
    toks, logits = _run(tiny, 2, kv, 1)
    with Batch(_cfg(2, kv), 2) as b:
        b.load_synthetic(tiny[0])
        b.set_option("gqa_attn", 1)
        out = b.generate([tiny[1], tiny[1][:5]], N_NEW)
        np.testing.assert_array_equal(out[0], toks)
        np.testing.assert_array_equal(_bits(b.logits(0)), _bits(logits))


def test_bad_value_raises_and_leaves_the_engine_usable(tiny):
    from llmi import _lib
    from llmi.engine import Batch, Engine
    with Engine(_cfg(2, "F16")) as e:
        e.load_synthetic(tiny[0])
        with pytest.raises(_lib.LlmiError, match="gqa_attn"):
            e.set_option("gqa_attn", 2)
        assert len(e.generate(tiny[1], 4)) == 4
    with Batch(_cfg(2, "F16"), 1) as b:
        with pytest.raises(_lib.LlmiError, match="gqa_attn"):
            b.set_option("gqa_attn", -1)
