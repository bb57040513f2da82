"""llmi_engine_set_sampling_params: the nucleus sampler inside the token step. The sampler
is isolated from the model's numerics by running the numpy restatement (tests/nucleus_ref.py)
on the engine's OWN logits of every step, with the history tokens[:pos + 1] and the step
seed + pos + 1 the kernel reads from the device state: on decided steps (both slacks >= 1e-6)
the engine's next token is the restatement's, with no tolerance. The graph and prefill paths
give the step-by-step tokens; the two setters replace each other."""
import os

import numpy as np
import pytest

import nucleus_ref as N

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, seed=4242)
# The tiny model's weights are random: no id of the history is ever among its 50 best
# candidates, so with top_k = 50 the penalty cannot change a token. Without the top-k cut the
# nucleus holds thousands of ids, penalised ones among them, and every penalised weight moves
# the id-order running sums of all higher ids: this set is where the penalty path shows.
WIDE = dict(PARAMS, top_k=0)
N_NEW = 24


def _fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)


def _engine():
    import llmi
    from llmi.engine import Engine, preset
    cfg = preset("tiny")
    cfg.kv_dtype = llmi.F32
    e = Engine(cfg)
    e.load_synthetic(int(_fixture()["seed"]))
    return e


_STEPWISE = {}


def _stepwise(params=None):
    """One eager step at a time -> (tokens [N_NEW], per step (want id, cut slack, draw slack))."""
    params = PARAMS if params is None else params
    key = tuple(sorted(params.items()))
    if key not in _STEPWISE:
        prompt = _fixture()["prompt"]
        n = len(prompt)
        got, want = [], []
        with _engine() as e:
            e.set_sampling_params(**params)
            e.set_prompt(prompt)
            e.decode(n, use_graph=False)
            for i in range(N_NEW):
                pos = n - 1 + i  # the forward that just ran; its logits choose the token of pos + 1
                logits = e.logits()
                toks = e.tokens(pos + 2)
                assert len(toks) == pos + 2
                tok, _, cs, ds = N.sample(logits, toks[:pos + 1], params["repetition_penalty"], params["temperature"],
                                          params["top_k"], params["top_p"], params["seed"] + pos + 1)
                got.append(int(toks[pos + 1]))
                want.append((tok, cs, ds))
                if i + 1 < N_NEW:
                    e.decode(1, use_graph=False)
        _STEPWISE[key] = (np.array(got, np.int32), want)
    return _STEPWISE[key]


def _generate(use_graph=True, prefill=False, **params):
    with _engine() as e:
        e.set_sampling_params(**params)
        return e.generate(_fixture()["prompt"], N_NEW, use_graph=use_graph, prefill=prefill)


@pytest.mark.parametrize("params", [PARAMS, WIDE], ids=["top_k50", "wide"])
def test_engine_tokens_are_the_restatement_on_the_engines_own_logits(params):
    got, want = _stepwise(params)
    undecided = 0
    for i, (g, (tok, cs, ds)) in enumerate(zip(got, want)):
        print(i, g, tok, cs, ds)
        if cs >= N.DECIDED and ds >= N.DECIDED:
            assert g == tok, (i, g, tok, cs, ds)
        else:
            undecided += 1
    if params is PARAMS:
        assert undecided <= 0.05 * N_NEW
    else:
        # the wide nucleus of a near-flat row keeps n ~ 2e4 ids of weight ~ S / n each: the
        # 1e-6 bands around the n prefix boundaries cover ~ 2e-6 n = 4 % of the draws, and the
        # band around the cut is ~ 2e-6 n of the boundary token's own weight, so a fifth or so
        # of the steps are undecided by construction; half of them decided is the floor here
        assert undecided <= N_NEW // 2


def test_graph_and_prefill_paths_give_the_stepwise_tokens():
    got, _ = _stepwise()
    np.testing.assert_array_equal(_generate(use_graph=True, **PARAMS), got)
    np.testing.assert_array_equal(_generate(use_graph=True, prefill=True, **PARAMS), got)
    np.testing.assert_array_equal(_generate(use_graph=False, **PARAMS), got)


def test_sequence_differs_from_greedy_and_from_no_penalty():
    got, _ = _stepwise()
    assert (got != _fixture()["tokens"][:N_NEW]).any()
    wide, _ = _stepwise(WIDE)
    assert (wide != got).any()
    np.testing.assert_array_equal(_generate(**WIDE), wide)
    no_pen = _generate(**dict(WIDE, repetition_penalty=1.0))
    assert (wide != no_pen).any()
    # top_k = 1 is greedy whatever the other controls' draw
    np.testing.assert_array_equal(_generate(top_k=1, top_p=0.9, seed=3), _fixture()["tokens"][:N_NEW])


def test_setters_replace_each_other():
    f = _fixture()
    with _engine() as e:
        e.set_sampling(5, 11)
        ref_topk = e.generate(f["prompt"], 10)
    with _engine() as e:
        e.set_sampling_params(**PARAMS)
        first = e.generate(f["prompt"], 10)
        e.set_sampling(5, 11)  # what tests/test_gpu_engine_sampling.py pins against the oracle
        np.testing.assert_array_equal(e.generate(f["prompt"], 10), ref_topk)
        e.set_sampling_params(**PARAMS)
        np.testing.assert_array_equal(e.generate(f["prompt"], 10), first)
        e.set_sampling(0)
        np.testing.assert_array_equal(e.generate(f["prompt"], 10), f["tokens"][:10])
    np.testing.assert_array_equal(first, _stepwise()[0][:10])


def test_set_sampling_5_11_after_params_matches_the_oracle():
    from oracle import llama_ref as R
    from oracle import sampling as S
    f = _fixture()
    o = R.LlamaOracle(R.LlamaConfig(hidden=512, heads=4, kv_heads=4, inter=1024, layers=2, max_seq=64),
                      seed=int(f["seed"]))
    prompt = [int(t) for t in f["prompt"]]
    seq, want = list(prompt), []
    for p in range(len(prompt) + 10 - 1):
        logits = o.forward_token(seq[p], p)
        if p + 1 < len(prompt):
            continue
        ids, vals = S.topk(np.asarray(logits, np.float32)[None], 5)
        tok, _, _, _ = S.sampling(ids, vals, [0], [0], 11 + p + 1, -1, logits.shape[-1])
        seq.append(int(tok[0]))
        want.append(int(tok[0]))
    with _engine() as e:
        e.set_sampling_params(**PARAMS)
        e.set_sampling(5, 11)
        np.testing.assert_array_equal(e.generate(f["prompt"], 10), np.array(want, np.int32))


def test_argument_checks_and_tp_refusal():
    from llmi._lib import LlmiError
    from llmi.engine import Engine, preset
    with _engine() as e:
        with pytest.raises(LlmiError, match=r"temperature must be > 0 \(greedy decoding is top_k = 1\)"):
            e.set_sampling_params(temperature=0.0)
        with pytest.raises(LlmiError, match=r"top_p must be in \(0, 1\]"):
            e.set_sampling_params(top_p=1.01)
        with pytest.raises(LlmiError, match="repetition_penalty must be > 0"):
            e.set_sampling_params(repetition_penalty=-1.0)
        with pytest.raises(LlmiError, match="top_k must be >= 0"):
            e.set_sampling_params(top_k=-2)
        # a refused call leaves the engine greedy
        np.testing.assert_array_equal(e.generate(_fixture()["prompt"], 6), _fixture()["tokens"][:6])
    with Engine(preset("tiny", tp_rank=0, tp_world=2)) as e:
        with pytest.raises(LlmiError, match=r"set_sampling_params: sampling needs the full logits \(tp_world 1\)"):
            e.set_sampling_params(top_p=0.9)
