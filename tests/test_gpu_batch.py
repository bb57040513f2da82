"""Batched decode (llmi_batch_*, struct Batch in engine_batch.hip): a sequence decoded in a batch
gives BITWISE the tokens and the final logits it gives alone in a plain Engine with the same
configuration, seed and default options. No tolerance anywhere: np.array_equal on ids and on
the logits' raw bits.

The `tiny` preset with max_seq 192, so the slots cross the 64-position attention split
boundary, each at a different step (prompts of different lengths; a restarted slot)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 192
N_NEW = 70


def _cfg(**over):
    from llmi.engine import preset
    over.setdefault("max_seq", MAX_SEQ)
    return preset("tiny", **over)


def _prompt(i, n, vocab=32000):
    from llmi.engine import synth_prompt
    return synth_prompt(1000 + i, n, vocab)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_REF = {}


def _alone(prompt, n_new, sampling=None, load=None, **cfg_over):
    """(tokens, final logits) of the sequence decoded alone in a plain Engine; computed once."""
    from llmi.engine import Engine
    key = (tuple(int(t) for t in prompt), n_new, tuple(sorted((sampling or {}).items())), load,
           tuple(sorted(cfg_over.items())))
    if key not in _REF:
        with Engine(_cfg(**cfg_over)) as e:
            if load:
                e.load_bin(load[0], quantize=load[1])
            else:
                e.load_synthetic(SEED)
            if sampling:
                e.set_sampling_params(**sampling)
            toks = e.generate(prompt, n_new)
            _REF[key] = (toks.copy(), e.logits().copy())
    return _REF[key]


def _check_slot(b, i, toks, prompt, n_new, **kw):
    want_t, want_l = _alone(prompt, n_new, **kw)
    assert np.array_equal(toks, want_t), (i, toks, want_t)
    assert np.array_equal(_bits(b.logits(i)), _bits(want_l)), f"slot {i}: final logits differ from the engine's"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_different_prompt_lengths(use_graph):
    from llmi.engine import Batch
    prompts = [_prompt(0, 1), _prompt(1, 5), _prompt(2, 8)]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        out = b.generate(prompts, N_NEW, use_graph=use_graph)
        for i, p in enumerate(prompts):
            assert len(out[i]) == N_NEW
            _check_slot(b, i, out[i], p, N_NEW)
        # three sequences of one model do not decode to the same ids
        assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])


def test_idle_slots_cost_nothing_and_change_nothing():
    from llmi.engine import Batch
    prompts = [None, _prompt(1, 5), None, _prompt(2, 8)]
    with Batch(_cfg(), 4) as b:
        b.load_synthetic(SEED)
        w1, _ = b.bytes_per_step()
        out = b.generate(prompts, N_NEW)
        assert out[0] is None and out[2] is None
        assert len(b.tokens(0)) == 0 and len(b.tokens(2)) == 0
        for i in (1, 3):
            _check_slot(b, i, out[i], prompts[i], N_NEW)
        # the byte model: weights once, W_o once more per further active slot
        b.set_prompt(1, prompts[1])
        wa, kv = b.bytes_per_step()
        b.set_prompt(3, prompts[3])
        wb, _ = b.bytes_per_step()
        c = b.cfg
        assert wa == w1 and wb - wa == c.layers * c.hidden * c.hidden * 2
        assert kv == c.layers * c.kv_heads * c.head_dim * 2 * 2


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_restart_of_one_slot(use_graph):
    """Slot 1 is restarted after 30 steps with another prompt: slots 0 and 2 run on as if nothing
    happened (77 steps: past position 64 while slot 1 is below it), slot 1 equals a fresh engine."""
    from llmi.engine import Batch
    p = [_prompt(0, 8), _prompt(1, 5), _prompt(2, 8)]
    again = _prompt(3, 6)
    first, total = 30, 8 + N_NEW - 1
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i in range(3):
            b.set_prompt(i, p[i])
        b.decode(first, use_graph)
        mid = b.tokens(1)
        b.set_prompt(1, again)
        b.decode(total - first, use_graph)
        for i in (0, 2):
            _check_slot(b, i, b.tokens(i)[8:], p[i], N_NEW)
        n1 = total - first - 6 + 1  # new tokens slot 1 has after its restart
        _check_slot(b, 1, b.tokens(1)[6:], again, n1)
    want_mid, _ = _alone(p[1], first - 5 + 1)
    assert np.array_equal(mid[5:], want_mid)


def test_per_slot_sampling():
    from llmi.engine import Batch
    params = [dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, seed=4242),
              dict(top_k=0, top_p=0.9, temperature=1.1, repetition_penalty=1.0, seed=7),
              None]
    prompts = [_prompt(0, 8), _prompt(0, 8), _prompt(0, 8)]  # one prompt: only the samplers differ
    n_new = 24
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i, s in enumerate(params):
            if s:
                b.set_sampling_params(i, **s)
        out = b.generate(prompts, n_new)
        for i, s in enumerate(params):
            _check_slot(b, i, out[i], prompts[i], n_new, sampling=s)
        assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[1], out[2])


def test_int8_synthetic_weights():
    import llmi
    from llmi.engine import Batch
    over = dict(weight_dtype=llmi.I8)
    prompts = [_prompt(4, 3), _prompt(5, 7)]
    with Batch(_cfg(**over), 2) as b:
        b.load_synthetic(SEED)
        out = b.generate(prompts, N_NEW)
        for i, p in enumerate(prompts):
            _check_slot(b, i, out[i], p, N_NEW, **over)


def test_fp32_weights_with_fp32_kv():
    import llmi
    from llmi.engine import Batch
    over = dict(weight_dtype=llmi.F32, kv_dtype=llmi.F32)
    prompts = [_prompt(6, 2), _prompt(7, 6), _prompt(8, 4)]
    with Batch(_cfg(**over), 3) as b:
        b.load_synthetic(SEED)
        out = b.generate(prompts, N_NEW)
        for i, p in enumerate(prompts):
            _check_slot(b, i, out[i], p, N_NEW, **over)


def test_checkpoint_loaders(tmp_path):
    """llmi_batch_load_bin / _load_bin_quantized from a checkpoint written here (vocab 256 keeps
    the files small): fp16 and int8 batches equal engines loaded from the same files."""
    import llmi
    from llmi import convert as CV
    from llmi.engine import Batch
    rng = np.random.default_rng(11)
    H, I, V, L = 512, 1024, 256, 2

    def lin(n, k):
        return (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)

    def gam():
        return (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)

    t = {"model.embed_tokens.weight": rng.standard_normal((V, H)).astype(np.float32),
         "lm_head.weight": lin(V, H), "model.norm.weight": gam()}
    for l in range(L):
        p = f"model.layers.{l}."
        t.update({p + "input_layernorm.weight": gam(), p + "post_attention_layernorm.weight": gam(),
                  p + "self_attn.qkv.weight": lin(3 * H, H), p + "self_attn.o_proj.weight": lin(H, H),
                  p + "mlp.gate_up_proj.weight": lin(2 * I, H), p + "mlp.down_proj.weight": lin(H, I)})
    prefix = str(tmp_path) + "/"
    CV.write_bin(prefix, t)
    prompts = [_prompt(9, 4, V), _prompt(10, 9, V)]
    for quant, over in ((False, dict(vocab=V)), (True, dict(vocab=V, weight_dtype=llmi.I8))):
        with Batch(_cfg(**over), 2) as b:
            b.load_bin(prefix, quantize=quant)
            out = b.generate(prompts, 20)
            for i, p in enumerate(prompts):
                _check_slot(b, i, out[i], p, 20, load=(prefix, quant), **over)


def test_7b_width_eight_slots():
    """hidden 4096, inter 11008, vocab 32000: the widths the multi-row GEMV is built for (8
    images of the hidden state fill the LDS; the down projection's 11008 runs 3 + 3 + 2)."""
    from llmi.engine import Batch, Engine, preset
    cfg = preset("llama2-7b", layers=2, max_seq=128)
    prompts = [_prompt(20 + i, 8) for i in range(8)]
    with Batch(cfg, 8) as b:
        b.load_synthetic(SEED)
        out = b.generate(prompts, 8)
        logits = [b.logits(i) for i in range(8)]
    with Engine(cfg) as e:
        e.load_synthetic(SEED)
        for i, p in enumerate(prompts):
            want = e.generate(p, 8)
            assert np.array_equal(out[i], want), (i, out[i], want)
            assert np.array_equal(_bits(logits[i]), _bits(e.logits())), i
    assert len({tuple(o) for o in out}) > 1


def test_errors():
    from llmi._lib import LlmiError
    from llmi.engine import Batch
    for n_seq in (0, 9):
        with pytest.raises(LlmiError, match="n_seq"):
            Batch(_cfg(), n_seq)
    with pytest.raises(LlmiError, match="tp_world"):
        Batch(_cfg(tp_world=2), 2)
    with Batch(_cfg(max_seq=64), 2) as b:
        b.load_synthetic(SEED)
        with pytest.raises(LlmiError, match="no active slot"):
            b.decode(1)
        for seq in (-1, 2):
            with pytest.raises(LlmiError, match="seq out of range"):
                b.set_prompt(seq, _prompt(0, 4))
            with pytest.raises(LlmiError, match="seq out of range"):
                b.tokens(seq)
            with pytest.raises(LlmiError, match="seq out of range"):
                b.reset(seq)
        b.set_prompt(0, _prompt(0, 4))
        b.decode(60)
        with pytest.raises(LlmiError, match="past max_seq"):
            b.decode(5)
        b.decode(4)  # exactly to max_seq is allowed
        assert len(b.tokens(0)) == 65
        b.reset(0)
        with pytest.raises(LlmiError, match="no active slot"):
            b.decode(1)
