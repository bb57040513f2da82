"""llmi_engine_set_logprobs: per-token log-probabilities inside the token step. The launch is
isolated from the model's numerics by running the float64 restatement (tests/logprob_ref.py)
on the engine's OWN logits of every eager step: record pos + 1 is the logprob of
tokens[pos + 1] under the RAW row of the forward at pos -- under greedy decoding, under the
top-k sampler and under the nucleus sampler alike -- within logprob_ref.tolerance, and the
top-n ids are the restatement's. Graph replay, score and the off / on invariants are bitwise."""
import os

import numpy as np
import pytest

import logprob_ref as L

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUCLEUS = dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, seed=4242)
SAMPLERS = {"greedy": None, "top5": ("set_sampling", (5, 11), {}), "nucleus": ("set_sampling_params", (), NUCLEUS)}
N_NEW = 8
N_TOP = 3


def _fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)


def _engine(sampler="greedy", n_top=N_TOP, **cfg_over):
    import llmi
    from llmi.engine import Engine, preset
    cfg = preset("tiny", **cfg_over)
    cfg.kv_dtype = llmi.F32
    e = Engine(cfg)
    e.load_synthetic(int(_fixture()["seed"]))
    if SAMPLERS[sampler]:
        name, args, kw = SAMPLERS[sampler]
        getattr(e, name)(*args, **kw)
    if n_top >= 0:
        e.set_logprobs(n_top)
    return e


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


_EAGER = {}


def _eager(sampler):
    """The prompt and N_NEW tokens, one eager step at a time -> (tokens, records, per-step logits)."""
    if sampler not in _EAGER:
        prompt = _fixture()["prompt"]
        total = len(prompt) + N_NEW - 1  # forwards at positions 0 .. total - 1
        rows = []
        with _engine(sampler) as e:
            e.set_prompt(prompt)
            for _ in range(total):
                e.decode(1, use_graph=False)
                rows.append(e.logits())
            _EAGER[sampler] = (e.tokens(total + 1), e.logprobs(), rows, e.logits())
    return _EAGER[sampler]


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_records_are_the_restatement_on_the_engines_own_logits(sampler):
    prompt = _fixture()["prompt"]
    toks, (lp, tids, tlp), rows, _ = _eager(sampler)
    vocab = len(rows[0])
    assert len(toks) == len(rows) + 1 == len(lp) and tids.shape == tlp.shape == (len(lp), N_TOP)
    np.testing.assert_array_equal(toks[:len(prompt)], prompt)
    assert np.isnan(lp[0]) and (tids[0] == -1).all() and np.isnan(tlp[0]).all()  # record 0: never computed
    for pos, z in enumerate(rows):
        want, _ = L.logprobs(z)
        tok = int(toks[pos + 1])  # the prompt's token inside the prompt, the sampler's after it
        L.assert_close(lp[pos + 1:pos + 2], want[tok:tok + 1], vocab, f"{sampler} pos {pos} token {tok}")
        wi, wl = L.top_n(z, N_TOP)
        np.testing.assert_array_equal(tids[pos + 1], wi)
        L.assert_close(tlp[pos + 1], wl, vocab, f"{sampler} pos {pos} top")
        if sampler == "greedy" and pos + 1 >= len(prompt):
            assert tids[pos + 1][0] == tok and np.array_equal(_bits(tlp[pos + 1][:1]), _bits(lp[pos + 1:pos + 2]))
    if sampler != "greedy":  # the sampled sequence is not the greedy one, the distribution is still the raw one
        assert (toks[len(prompt):] != _eager("greedy")[0][len(prompt):]).any()


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_graph_decode_gives_the_eager_records(sampler):
    prompt = _fixture()["prompt"]
    toks, rec, _, last = _eager(sampler)
    with _engine(sampler) as e:
        e.set_prompt(prompt)
        e.decode(len(toks) - 1, use_graph=True)
        np.testing.assert_array_equal(e.tokens(len(toks)), toks)
        assert _same(e.logprobs(), rec)
        assert np.array_equal(_bits(e.logits()), _bits(last))


def test_prefill_scores_its_last_row_only_then_every_decode_step():
    """generate(prefill=True): prompt records 1 .. len - 1 stay "not computed" (their rows ran
    through the batched pass, which forms no logits), the record of the first generated token
    comes from the prefill's last row and the later ones from the decode steps. The prefill's
    GEMMs are not the decode kernels' bits, so the records are held against the restatement on
    this run's own logits, and the tokens against the eager run's."""
    prompt = _fixture()["prompt"]
    n = len(prompt)
    toks = _eager("greedy")[0]
    with _engine() as e:
        np.testing.assert_array_equal(e.generate(prompt, N_NEW, use_graph=True, prefill=True), toks[n:])
        glp, gids, gtlp = e.logprobs()
        assert len(glp) == n + N_NEW
        assert np.isnan(glp[:n]).all() and (gids[:n] == -1).all() and np.isnan(gtlp[:n]).all()
        assert np.isfinite(glp[n:]).all() and (gids[n:, 0] == toks[n:]).all()
        e.set_prompt(prompt)
        e.prefill(n)
        for pos in range(n - 1, n + 2):
            z = e.logits()
            lp, tids, tlp = e.logprobs()
            assert len(lp) == pos + 2 and np.isnan(lp[:n]).all()
            want, _ = L.logprobs(z)
            tok = int(toks[pos + 1])
            L.assert_close(lp[pos + 1:], want[tok:tok + 1], len(z), f"prefill pos {pos}")
            np.testing.assert_array_equal(tids[pos + 1], L.top_n(z, N_TOP)[0])
            assert np.array_equal(_bits(lp[n:pos + 1]), _bits(glp[n:pos + 1]))  # the run above, replayed
            e.decode(1, use_graph=False)


def test_prefill_of_a_prefix_then_decode_steps():
    prompt = _fixture()["prompt"]
    n = len(prompt)
    with _engine() as e:
        e.set_prompt(prompt)
        e.prefill(n - 2)
        e.decode(2 + N_NEW - 1)
        glp, gids, _ = e.logprobs()
    # the prefix's last row scores prompt[n - 2]; the rows before it are not computed
    assert np.isnan(glp[:n - 2]).all() and np.isfinite(glp[n - 2:]).all() and (gids[n - 2:] >= 0).all()


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_tokens_and_logits_do_not_depend_on_logprobs(use_graph):
    prompt = _fixture()["prompt"]
    for sampler in SAMPLERS:
        with _engine(sampler, n_top=-1) as e:
            off = e.generate(prompt, N_NEW, use_graph=use_graph)
            off_logits = e.logits()
        with _engine(sampler, n_top=8) as e:
            on = e.generate(prompt, N_NEW, use_graph=use_graph)
            assert np.array_equal(_bits(e.logits()), _bits(off_logits))
        np.testing.assert_array_equal(on, off)
    np.testing.assert_array_equal(_eager("greedy")[0][len(prompt):], _fixture()["tokens"][:N_NEW])


def test_off_on_off_recaptures_the_graphs():
    from llmi._lib import LlmiError
    prompt = _fixture()["prompt"]
    toks, rec, _, _ = _eager("greedy")
    with _engine(n_top=-1) as e:
        with pytest.raises(LlmiError, match="set_logprobs first"):
            e.logprobs()
        want = e.generate(prompt, N_NEW)  # graphs captured without the launch
        e.set_logprobs(N_TOP)
        np.testing.assert_array_equal(e.generate(prompt, N_NEW), want)
        assert _same(e.logprobs(), rec)
        e.set_logprobs(-1)
        np.testing.assert_array_equal(e.generate(prompt, N_NEW), want)
        # off again: set_prompt cleared the records and nothing wrote them since (turning the
        # same n_top back on keeps the records as they are)
        e.set_logprobs(N_TOP)
        lp, tids, _ = e.logprobs()
        assert len(lp) == len(rec[0]) and np.isnan(lp).all() and (tids == -1).all()
        np.testing.assert_array_equal(e.generate(prompt, N_NEW), want)
        assert _same(e.logprobs(), rec)


def test_survives_a_change_of_sampler():
    prompt = _fixture()["prompt"]
    with _engine("greedy") as e:
        e.set_sampling_params(**NUCLEUS)
        e.set_prompt(prompt)
        e.decode(len(prompt) + N_NEW - 1)
        assert _same(e.logprobs(), _eager("nucleus")[1])


def test_score_is_a_plain_decode_over_the_ids():
    toks, (lp, _, _), _, _ = _eager("greedy")
    with _engine(n_top=-1) as e:
        for use_graph in (True, False):
            got = e.score(toks, use_graph=use_graph)
            assert got.shape == (len(toks) - 1,) and np.array_equal(_bits(got), _bits(lp[1:]))
        from llmi._lib import LlmiError
        with pytest.raises(LlmiError, match="set_logprobs first"):  # score restored "off"
            e.logprobs()
    with _engine(n_top=2) as e:  # on: the caller's setting is kept
        got = e.score(toks)
        assert np.array_equal(_bits(got), _bits(lp[1:])) and e.logprobs()[1].shape[1] == 2


def test_a_record_at_max_seq_is_written():
    f = _fixture()
    with _engine(n_top=1) as e:
        max_seq = e.cfg.max_seq
        e.set_prompt(f["prompt"])
        e.decode(max_seq)
        toks = e.tokens()
        lp, tids, tlp = e.logprobs()
        z = e.logits()
    assert len(toks) == max_seq + 1 == len(lp)
    assert np.isfinite(lp[1:]).all()
    want, _ = L.logprobs(z)
    L.assert_close(lp[max_seq:], want[toks[max_seq]:toks[max_seq] + 1], len(z), "record max_seq")
    assert tids[max_seq][0] == toks[max_seq] == int(np.argmax(z))


def test_argument_checks_and_tp_refusal():
    from llmi._lib import LlmiError
    from llmi.engine import Engine, preset
    with _engine(n_top=-1) as e:
        for bad in (-2, 9):
            with pytest.raises(LlmiError, match=r"failed \(-1\).*n_top must be -1 \(off\) or in \[0, 8\]"):
                e.set_logprobs(bad)
    with Engine(preset("tiny", tp_rank=0, tp_world=2)) as e:
        with pytest.raises(LlmiError, match=r"failed \(-2\).*logprobs need the full logits row"):
            e.set_logprobs(0)
        e.set_logprobs(-1)  # off is always accepted
