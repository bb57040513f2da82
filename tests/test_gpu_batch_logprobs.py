"""Per-slot log-probabilities of a batch (llmi_batch_set_logprobs / llmi_batch_logprobs): a
slot's records are BITWISE those of a plain Engine running that sequence alone, whatever the
other slots do (another prompt length, another n_top, logprobs off); restarting a slot clears
that slot's records only; Batch.score of texts of unequal length is Engine.score of each."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 96
N_NEW = 66  # the slots cross the 64-position attention split boundary at different steps
LENS = (1, 5, 8)
TOPS = (2, -1, 0)  # slot 1 has logprobs off
NUCLEUS = dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, seed=99)


def _cfg():
    from llmi.engine import preset
    return preset("tiny", max_seq=MAX_SEQ)


def _prompt(i, n, vocab=32000):
    from llmi.engine import synth_prompt
    return synth_prompt(1000 + i, n, vocab)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


_REF = {}


def _alone(prompt, n_new, n_top, sampling=None):
    """(tokens, records) of the sequence decoded alone in a plain Engine; computed once."""
    from llmi.engine import Engine
    key = (tuple(int(t) for t in prompt), n_new, n_top, tuple(sorted((sampling or {}).items())))
    if key not in _REF:
        with Engine(_cfg()) as e:
            e.load_synthetic(SEED)
            if sampling:
                e.set_sampling_params(**sampling)
            e.set_logprobs(n_top)
            toks = e.generate(prompt, n_new)
            _REF[key] = (toks.copy(), e.logprobs())
    return _REF[key]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_slot_records_are_the_single_engines(use_graph):
    from llmi._lib import LlmiError
    from llmi.engine import Batch
    prompts = [_prompt(i, n) for i, n in enumerate(LENS)]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        b.set_sampling_params(2, **NUCLEUS)  # one slot samples: its records follow its own tokens
        for i, t in enumerate(TOPS):
            b.set_logprobs(i, t)
        for i, p in enumerate(prompts):
            b.set_prompt(i, p)
        # every slot takes the same number of steps here: each ends len(prompt) + steps tokens in
        steps = N_NEW
        b.decode(steps, use_graph)
        for i, p in enumerate(prompts):
            n_new = steps + 1 - len(p)
            toks = b.tokens(i, len(p) + n_new)[len(p):]
            want_t, want_r = _alone(p, n_new, max(TOPS[i], 0), NUCLEUS if i == 2 else None)
            np.testing.assert_array_equal(toks, want_t)
            if TOPS[i] < 0:
                with pytest.raises(LlmiError, match="set_logprobs first"):
                    b.logprobs(i)
                continue
            got = b.logprobs(i)
            assert len(got[0]) == steps + 1 and got[1].shape == (steps + 1, TOPS[i])
            assert np.isnan(got[0][0]) and np.isfinite(got[0][1:]).all()
            assert _same(got, want_r), f"slot {i}: records differ from the engine's"


def test_restarting_a_slot_clears_only_its_records():
    from llmi.engine import Batch
    prompts = [_prompt(i, n) for i, n in enumerate(LENS)]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i, p in enumerate(prompts):
            b.set_logprobs(i, 1)
            b.set_prompt(i, p)
        b.decode(12)
        before = [b.logprobs(i) for i in range(3)]
        b.set_prompt(1, prompts[1])
        lp, tids, tlp = b.logprobs(1)
        assert len(lp) == 1 and np.isnan(lp).all() and (tids == -1).all() and np.isnan(tlp).all()
        for i in (0, 2):
            assert _same(b.logprobs(i), before[i])
        b.decode(12)
        assert _same(b.logprobs(1), before[1])  # the same sequence again, beside slots 12 steps ahead
        for i in (0, 2):
            after = b.logprobs(i)
            assert len(after[0]) == 25 and _same([x[:13] for x in after], before[i])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_batch_score_is_three_engine_scores(use_graph):
    from llmi._lib import LlmiError
    from llmi.engine import Batch, Engine
    texts = [_prompt(10 + i, n) for i, n in enumerate((7, 30, 70))]
    with Engine(_cfg()) as e:
        e.load_synthetic(SEED)
        want = [e.score(t) for t in texts]
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        b.set_logprobs(2, 4)  # one slot already on: its setting is kept
        got = b.score(texts, use_graph=use_graph)
        for g, w, t in zip(got, want, texts):
            assert g.shape == (len(t) - 1,) and np.isfinite(g).all()
            assert np.array_equal(_bits(g), _bits(w))
        b.set_prompt(0, texts[0])
        with pytest.raises(LlmiError, match="set_logprobs first"):  # score restored "off"
            b.logprobs(0)
        b.set_prompt(2, texts[2])
        assert b.logprobs(2)[1].shape == (1, 4)
        with pytest.raises(ValueError):
            b.score(texts + [texts[0]])
