"""The W4A16 engine (weight_dtype LLMI_I4) end to end on the tiny model of tests/golden/tiny.npz:
q/k/v, gate_up and down in 4-bit groups of 128 columns (tests/i4_ref.py), W_o W8A16 (quant_ref,
as tests/test_gpu_quantize.py restates it), everything else fp16.

The oracle (oracle/llama_ref.py) runs on the weights dequantised in numpy -- fp32 matrices with
scales None -- and the engine, loading the fp32 .bin files with quantize=True or generating the
same model with load_synthetic, must give exactly its greedy tokens and its final logits within
LOGIT_TOL = 1e-3 rel-L2 (tests/test_gpu_engine.py's bar)."""
import dataclasses
import os

import numpy as np
import pytest

import i4_ref

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 1e-3  # tests/test_gpu_engine.py
N_NEW = 8


def quant_ref(w):
    """W8A16 (tests/test_gpu_quantize.py: quant_ref) of whole rows -> (q int8, scales fp16)."""
    w = np.asarray(w, np.float32)
    amax = np.abs(w).max(axis=1).astype(np.float32)
    bits = (amax / np.float32(127.0)).astype(np.float32).astype(np.float16).view(np.uint16).copy()
    bits[bits == 0] = 1
    bits[bits == 0x7C00] = 0x7BFF
    sf = bits.view(np.float16).astype(np.float32)
    q = np.clip(np.rint((w / sf[:, None]).astype(np.float32)), -127, 127).astype(np.int8)
    return q, bits.view(np.float16)


def dequantised(w):
    """ModelWeights as the int4 engine holds them, every linear matrix back in fp32."""
    layers = []
    for lw in w.layers:
        new = {}
        for name in ("qkv", "gate_up", "down"):
            q, bits, bad = i4_ref.quant_i4_ref(np.asarray(getattr(lw, name), np.float32))
            assert bad == 0
            new[name], new[name + "_s"] = i4_ref.dequant(q, bits), None
        new["o"], new["o_s"] = R.dequant(*quant_ref(lw.o)), None
        layers.append(dataclasses.replace(lw, **new))
    return R.ModelWeights(embed=w.embed, lm_head=w.lm_head, final_norm=w.final_norm, layers=layers)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    import llmi
    from llmi import convert as CV
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    seed = int(f["seed"])
    cfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=4, inter=1024, layers=2, max_seq=64)
    w32 = R.make_model_weights(cfg, seed)  # the fp16 engine's synthetic model (fp16 values)
    t = {"model.embed_tokens.weight": w32.embed, "lm_head.weight": w32.lm_head, "model.norm.weight": w32.final_norm}
    for l, L in enumerate(w32.layers):
        p = f"model.layers.{l}."
        t.update({p + "input_layernorm.weight": L.attn_norm, p + "post_attention_layernorm.weight": L.ffn_norm,
                  p + "self_attn.qkv.weight": L.qkv, p + "self_attn.o_proj.weight": L.o,
                  p + "mlp.gate_up_proj.weight": L.gate_up, p + "mlp.down_proj.weight": L.down})
    prefix = str(tmp_path_factory.mktemp("i4bin")) + "/"
    CV.write_bin(prefix, {k: np.asarray(v, np.float32) for k, v in t.items()})
    prompt = np.asarray(f["prompt"], np.int32)
    toks, logits = R.LlamaOracle(cfg, weights=dequantised(w32)).greedy(prompt, N_NEW)
    # the quantisation is visible at the bar's scale: the unquantised model is further away
    toks32, logits32 = R.LlamaOracle(cfg, weights=w32).greedy(prompt, N_NEW)
    d32 = _rel(logits32, logits)
    print(f"oracle: unquantised vs int4 logits rel-L2 {d32:.3e}, tokens equal: {bool((toks32 == toks).all())}")
    assert d32 > 2 * LOGIT_TOL
    llmi.lib()
    return dict(cfg=cfg, seed=seed, prefix=prefix, prompt=prompt, tokens=toks, logits=logits)


def _cfg(**over):
    import llmi
    from llmi.engine import preset
    return preset("tiny", weight_dtype=llmi.I4, kv_dtype=llmi.F32, **over)


def test_load_bin_quantized_matches_the_oracle(tiny):
    from llmi.engine import Engine
    with Engine(_cfg()) as e:
        e.load_bin(tiny["prefix"], quantize=True)
        toks = e.generate(tiny["prompt"], N_NEW)
        logits = e.logits()
    r = _rel(logits, tiny["logits"])
    print(f"int4 engine, quantised on load: logits rel-L2 vs oracle {r:.3e}")
    np.testing.assert_array_equal(toks, tiny["tokens"])
    assert r < LOGIT_TOL


def test_load_tensor_quantized_matches_load_bin(tiny):
    from llmi.engine import Engine
    with Engine(_cfg()) as a, Engine(_cfg()) as b:
        a.load_bin(tiny["prefix"], quantize=True)
        for fn in sorted(os.listdir(tiny["prefix"])):
            assert fn.endswith(".bin")
            b.load_tensor(fn[:-4], np.fromfile(os.path.join(tiny["prefix"], fn), np.float32), quantize=True)
        ta, tb = a.generate(tiny["prompt"], N_NEW), b.generate(tiny["prompt"], N_NEW)
        np.testing.assert_array_equal(ta, tb)
        np.testing.assert_array_equal(a.logits().view(np.uint32), b.logits().view(np.uint32))


def test_load_synthetic_is_the_quantised_fp16_model(tiny):
    from llmi.engine import Engine
    with Engine(_cfg()) as e:
        e.load_synthetic(tiny["seed"])
        toks = e.generate(tiny["prompt"], N_NEW)
        logits = e.logits()
    r = _rel(logits, tiny["logits"])
    print(f"int4 engine, synthetic: logits rel-L2 vs oracle {r:.3e}")
    np.testing.assert_array_equal(toks, tiny["tokens"])
    assert r < LOGIT_TOL


def test_graph_replay_is_bitwise_the_eager_run(tiny):
    from llmi.engine import Engine
    with Engine(_cfg()) as e:
        e.load_synthetic(tiny["seed"])
        te = e.generate(tiny["prompt"], N_NEW, use_graph=False)
        le = e.logits()
        tg = e.generate(tiny["prompt"], N_NEW, use_graph=True)
        lg = e.logits()
    np.testing.assert_array_equal(te, tg)
    np.testing.assert_array_equal(le.view(np.uint32), lg.view(np.uint32))
    np.testing.assert_array_equal(tg, tiny["tokens"])


def test_logprobs_and_nucleus_sampling_run(tiny):
    from llmi.engine import Engine
    n = len(tiny["prompt"]) + N_NEW
    with Engine(_cfg()) as e:
        e.load_synthetic(tiny["seed"])
        e.set_logprobs(3)
        e.set_sampling_params(top_k=20, top_p=0.9, temperature=0.8, repetition_penalty=1.1, seed=5)
        runs = []
        for use_graph in (False, True):
            toks = e.generate(tiny["prompt"], N_NEW, use_graph=use_graph)
            runs.append((toks, *e.logprobs(n)))
        # text scoring through decode steps (prefill=False) needs no int4 code of its own
        sc = e.score(np.concatenate([tiny["prompt"], runs[0][0]]), prefill=False)
    (t0, lp0, ids0, tlp0), (t1, lp1, ids1, tlp1) = runs
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(lp0.view(np.uint32), lp1.view(np.uint32))
    np.testing.assert_array_equal(ids0, ids1)
    np.testing.assert_array_equal(tlp0.view(np.uint32), tlp1.view(np.uint32))
    assert len(t0) == N_NEW and np.isfinite(lp0[1:]).all() and (lp0[1:] <= 0).all() and (ids0[1:] >= 0).all()
    assert sc.shape == (n - 1,) and np.isfinite(sc).all()


def test_bytes_per_token_counts_nibbles_scales_and_int8_wo():
    from llmi.engine import Engine
    c = _cfg()
    H, I, L, V = c.hidden, c.inter, c.layers, c.vocab
    qkv_rows = (c.heads + 2 * c.kv_heads) * c.head_dim
    lin = qkv_rows * H + 2 * I * H + H * I             # int4 weights of a layer
    per_layer = lin // 2 + lin // 128 * 2              # nibbles + fp16 group scales
    per_layer += H * (c.heads * c.head_dim) + H * 2    # W_o int8 + its row scales
    per_layer += 2 * H * 2                             # the two norms
    want = L * per_layer + V * H * 2 + H * 2 + H * 2   # + lm_head, final norm, one embedding row
    with Engine(c) as e:
        w, kv = e.bytes_per_token()
    assert w == want
    assert kv == L * c.kv_heads * c.head_dim * 2 * 4


def test_refusals_name_int4(tiny):
    import llmi
    from llmi._lib import LlmiError
    from llmi.engine import Batch, Engine, TPGroup, preset
    with Engine(_cfg()) as e:
        with pytest.raises(LlmiError, match=r"int8 and int4 engines.*quantised loaders"):
            e.load_bin(tiny["prefix"])
        with pytest.raises(LlmiError, match=r"int8 and int4 engines.*quantised loaders"):
            e.load_tensor("model.layers.0.mlp.down_proj.weight", np.zeros((512, 1024), np.float32))
        bad = np.ones((512, 1024), np.float32)
        bad[17, 900] = np.inf
        with pytest.raises(LlmiError, match=r"layers\.1\.mlp\.down_proj.*NaN or an infinity"):
            e.load_tensor("model.layers.1.mlp.down_proj.weight", bad, quantize=True)
        e.load_synthetic(tiny["seed"])
        e.set_prompt(tiny["prompt"])
        with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
            e.prefill(len(tiny["prompt"]))
        with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
            e.score(tiny["prompt"], prefill=True)
        with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
            e.set_decode_mode(1)
        # the refused calls left the engine usable
        np.testing.assert_array_equal(e.generate(tiny["prompt"], N_NEW), tiny["tokens"])
    with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
        Batch(_cfg(), 2)
    with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
        TPGroup(_cfg(), 2)
    with pytest.raises(LlmiError, match=r"\(-2\).*int4"):
        Engine(_cfg(tp_rank=0, tp_world=2))
    # the fp16 engine's message keeps its text
    with Engine(preset("tiny")) as e:
        with pytest.raises(LlmiError, match="quantize needs an int8 engine"):
            e.load_bin(tiny["prefix"], quantize=True)
        with pytest.raises(LlmiError, match="quantize needs an int8 engine"):
            e.load_tensor("model.norm.weight", np.ones(512, np.float32), quantize=True)
    assert llmi.I4 == 5
