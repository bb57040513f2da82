"""llmi_batch_prefill: a batch slot consumes its prompt in one batched pass through the batch's
one prefill scratch (slot 0's, lent like the weights). The pattern is tests/test_gpu_batch.py's:
a slot's tokens, final logits and log-probability records are BITWISE those of a plain Engine
that prefilled the same sequence alone -- np.array_equal on ids and raw bits, no tolerance.

The `tiny` preset with max_seq 192, so the slots cross the 64-position attention split at
different steps; one case at the Llama-2-7B width for the e4m3 weight copies of exact=2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 192
N_NEW = 70


def _cfg(name="tiny", **over):
    from llmi.engine import preset
    over.setdefault("max_seq", MAX_SEQ)
    return preset(name, **over)


def _prompt(i, n, vocab=32000):
    from llmi.engine import synth_prompt
    return synth_prompt(2000 + i, n, vocab)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


_REF = {}


def _alone(prompt, n_new, prefill=True):
    """(tokens, final logits) of Engine.generate alone; computed once."""
    from llmi.engine import Engine
    key = (tuple(int(t) for t in prompt), n_new, prefill)
    if key not in _REF:
        with Engine(_cfg()) as e:
            e.load_synthetic(SEED)
            toks = e.generate(prompt, n_new, prefill=prefill)
            _REF[key] = (toks.copy(), e.logits().copy())
    return _REF[key]


def _check_slot(b, i, prompt, n_new, prefill=True):
    want_t, want_l = _alone(prompt, n_new, prefill)
    toks = b.tokens(i, len(prompt) + n_new)[len(prompt):]
    assert np.array_equal(toks, want_t), (i, toks, want_t)
    assert np.array_equal(_bits(b.logits(i)), _bits(want_l)), f"slot {i}: final logits differ from the engine's"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_three_slots_prefilled_then_decoded_together(use_graph):
    from llmi.engine import Batch
    prompts = [_prompt(0, 5), _prompt(1, 40), _prompt(2, 70)]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i, p in enumerate(prompts):
            b.set_prompt(i, p)
        for i in (1, 0, 2):  # any order: one stream, one scratch
            b.prefill(i)
        b.decode(N_NEW - 1, use_graph)
        for i, p in enumerate(prompts):
            _check_slot(b, i, p, N_NEW)
        # the same through generate
        out = b.generate(prompts, N_NEW, use_graph=use_graph, prefill=True)
        for i, p in enumerate(prompts):
            assert np.array_equal(out[i], _alone(p, N_NEW)[0])


def test_prefill_into_a_running_batch():
    """Slots 0 and 2 are 30 steps into their sequences when slot 1 is restarted and prefilled;
    all three decode on. Slots 0 and 2 are as if alone (their prompts consumed by steps), slot
    1 is a fresh engine that prefilled."""
    from llmi.engine import Batch
    p = [_prompt(3, 8), _prompt(4, 5), _prompt(5, 8)]
    again = _prompt(6, 50)
    first, total = 30, 8 + N_NEW - 1
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i in range(3):
            b.set_prompt(i, p[i])
        b.decode(first)
        b.set_prompt(1, again)
        b.prefill(1)
        b.decode(total - first)
        for i in (0, 2):
            _check_slot(b, i, p[i], N_NEW, prefill=False)
        n1 = total - first + 1  # slot 1: the prefill's token and one per step since
        _check_slot(b, 1, again, n1)


def test_scored_slot_prefill_gives_the_engines_records():
    from llmi.engine import Batch, Engine
    texts = [_prompt(7, 33), _prompt(8, 90), _prompt(9, 6)]
    want, want_score = [], []
    with Engine(_cfg()) as e:
        e.load_synthetic(SEED)
        e.set_logprobs(2)
        for t in texts:
            e.set_prompt(t)
            e.prefill(len(t), score=True)
            want.append(e.logprobs())
            assert np.isfinite(want[-1][0][1:]).all()
        e.set_logprobs(-1)
        want_score = [e.score(t, prefill=True) for t in texts]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i, t in enumerate(texts):
            b.set_logprobs(i, 2)
            b.set_prompt(i, t)
        for i in (2, 0, 1):
            b.prefill(i, score=True)
        for i in range(3):
            assert _same(b.logprobs(i), want[i]), i
        for i in range(3):
            b.set_logprobs(i, -1)
        got = b.score(texts, prefill=True)
        for i in range(3):
            assert got[i].shape == (len(texts[i]) - 1,)
            assert np.array_equal(_bits(got[i]), _bits(want_score[i])), i


def test_exact2_on_another_slot_follows_a_weight_reload():
    """The e4m3 weight copies of exact=2 exist once per batch and are derived from slot 0's
    weights: after llmi_batch_load_synthetic with another seed, slot 1's next exact=2 prefill
    runs on the new weights (the batch counterpart of
    tests/test_gpu_prefill.py::test_prefill_fp8_lo_mode_follows_weight_reload)."""
    from llmi.engine import Batch, Engine
    cfg = dict(layers=1, max_seq=160)
    prompt = _prompt(10, 128)
    with Engine(_cfg("llama2-7b", **cfg)) as e:
        e.load_synthetic(6)
        e.set_prompt(prompt)
        e.prefill(len(prompt), exact=2)
        want_t, want_l = e.tokens(len(prompt) + 1), e.logits()
    with Batch(_cfg("llama2-7b", **cfg), 2) as b:
        b.load_synthetic(5)
        b.set_prompt(1, prompt)
        b.prefill(1, exact=2)  # builds the e4m3 copies of seed 5
        old = b.logits(1)
        b.load_synthetic(6)
        b.set_prompt(1, prompt)
        b.prefill(1, exact=2)
        np.testing.assert_array_equal(b.tokens(1, len(prompt) + 1), want_t)
        new = b.logits(1)
    assert np.array_equal(_bits(new), _bits(want_l))
    r_old = float(np.linalg.norm(new.astype(np.float64) - old) / np.linalg.norm(old.astype(np.float64)))
    print(f"slot prefill after the reload vs the old weights' logits: rel-L2 {r_old:.3e}")
    assert r_old > 0.1


def test_errors():
    from llmi._lib import LlmiError
    from llmi.engine import Batch
    prompt = _prompt(11, 12)
    with Batch(_cfg(), 2) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, prompt)
        for seq in (-1, 2):
            with pytest.raises(LlmiError, match=r"failed \(-1\).*seq out of range"):
                b.prefill(seq, 4)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*the slot is idle"):
            b.prefill(1, 4)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*the slot is idle"):
            b.prefill(1)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*rows must lie inside the prompt"):
            b.prefill(0, 13)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*set_logprobs first"):
            b.prefill(0, 12, score=True)
        with pytest.raises(ValueError):
            b.prefill(0, 12, exact=3)
        b.prefill(0, 4)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*rows must lie inside the prompt"):
            b.prefill(0, 9)
        b.prefill(0)  # the rest
        b.decode(3)  # and the slot goes on from where the two calls left it
        toks = b.tokens(0)
        assert len(toks) == 16
        np.testing.assert_array_equal(toks[:12], prompt)
