"""Logit rules in the token step of Engine (llmi_engine_set_logit_rules / _set_allowed): the
rules launch is isolated from the model's numerics by running the numpy restatement
(tests/logit_rules_ref.py) on the engine's OWN raw logits of every eager step, with the history
window the kernel reads from the device state: the processed row is the restatement's bit for
bit and the next token its argmax, with no tolerance. The graph and prefill paths give the
stepwise tokens; the samplers read the processed row; logprobs stay those of the raw row.

Run this file in its own pytest process: its exit status is part of the result."""
import os

import numpy as np
import pytest

import logit_rules_ref as L
import logprob_ref as LP
import nucleus_ref as N
from test_gpu_engine_nucleus import PARAMS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = 24
A = 1234          # the biased id
ONLY = 4321       # a one-id allowed set
PRESENCE, FREQUENCY = 0.5, 40.0


def _fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)


GOLDEN = [int(t) for t in _fixture()["tokens"]]
PROMPT = _fixture()["prompt"]
BANNED = GOLDEN[0]  # the fixture's first greedy token
V = 32000
assert A not in GOLDEN and ONLY not in GOLDEN and A not in PROMPT


def _dense(bias):
    d = np.zeros(V, np.float32)
    for k, v in bias.items():
        d[k] = v
    return d


BIAS = {A: 64.0, BANNED: -np.inf}
RULES = dict(bias=BIAS, presence_penalty=PRESENCE, frequency_penalty=FREQUENCY)


def _engine(**cfg_over):
    import llmi
    from llmi.engine import Engine, preset
    cfg = preset("tiny", **cfg_over)
    cfg.kv_dtype = llmi.F32
    assert cfg.vocab == V
    e = Engine(cfg)
    e.load_synthetic(int(_fixture()["seed"]))
    return e


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _walk(e, n_prompt, n_new, h0, bias=None, allowed=None, presence=0.0, frequency=0.0):
    """The engine has consumed its prompt (the forward at n_prompt - 1 just ran). n_new eager
    steps -> (tokens, raw rows); every step's processed row and next token are held against the
    restatement over history tokens[h0 .. pos]."""
    got, raws = [], []
    for i in range(n_new):
        pos = n_prompt - 1 + i  # the forward that just ran; its row chooses the token of pos + 1
        raw, proc = e.logits(), e.processed_logits()
        toks = e.tokens(pos + 2)
        assert len(toks) == pos + 2
        want_row, want_id = L.process(raw, bias, allowed, toks[h0:pos + 1], presence, frequency)
        assert np.array_equal(_bits(proc), _bits(want_row)), (i, np.flatnonzero(_bits(proc) != _bits(want_row))[:8])
        assert int(toks[pos + 1]) == want_id, (i, int(toks[pos + 1]), want_id)
        got.append(want_id)
        raws.append(raw)
        if i + 1 < n_new:
            e.decode(1, use_graph=False)
    return got, raws


_STEPWISE = {}


def _stepwise(count_prompt=False, prompt=None, n_new=N_NEW):
    prompt = PROMPT if prompt is None else np.asarray(prompt, np.int32)
    key = (count_prompt, tuple(int(t) for t in prompt), n_new)
    if key not in _STEPWISE:
        with _engine() as e:
            e.set_logit_rules(count_prompt=count_prompt, **RULES)
            e.set_prompt(prompt)
            e.decode(len(prompt), use_graph=False)
            _STEPWISE[key] = _walk(e, len(prompt), n_new, 0 if count_prompt else len(prompt), _dense(BIAS), None,
                                   PRESENCE, FREQUENCY)
    return _STEPWISE[key]


def _generate(setup, n_new=N_NEW, prompt=None, **kw):
    with _engine() as e:
        setup(e)
        return [int(t) for t in e.generate(PROMPT if prompt is None else prompt, n_new, **kw)]


def test_stepwise_rows_and_tokens_are_the_restatement_bit_for_bit():
    seq, raws = _stepwise()
    # not vacuous, on the engine's own raw rows: the +64 bias lifts A above every other id until
    # A has been picked twice (penalties 0.5 + 40 a pick: 64 - 40.5 > 20 > 64 - 80.5)
    for i, raw in enumerate(raws):
        gap = float(raw.max() - raw[A])
        print(i, seq[i], gap)
        assert gap < 20, (i, gap)
    assert seq[0] != BANNED and BANNED not in seq
    assert seq[:2] == [A, A] and A not in seq[2:]
    assert seq != GOLDEN[:N_NEW]
    bias_only = _generate(lambda e: e.set_logit_rules(bias=BIAS))
    pen_only = _generate(lambda e: e.set_logit_rules(presence_penalty=PRESENCE, frequency_penalty=FREQUENCY))
    assert bias_only == [A] * N_NEW
    assert seq != bias_only and seq != pen_only


@pytest.mark.parametrize("kw", [dict(use_graph=True), dict(use_graph=True, prefill=True), dict(use_graph=False)],
                         ids=["graph", "graph_prefill", "eager"])
def test_generate_paths_give_the_stepwise_tokens(kw):
    assert _generate(lambda e: e.set_logit_rules(**RULES), **kw) == _stepwise()[0]


def test_count_prompt_moves_the_history_window():
    prompt = PROMPT.copy()
    prompt[3] = A  # the prompt holds A once: with count_prompt one more pick of A ends its lead
    with_prompt, _ = _stepwise(True, prompt, 8)
    without, _ = _stepwise(False, prompt, 8)
    assert with_prompt != without
    assert with_prompt[0] == A and with_prompt[1] != A and without[:2] == [A, A]
    assert _generate(lambda e: e.set_logit_rules(count_prompt=True, **RULES), 8, prompt) == with_prompt


CHOOSERS = {
    "greedy": lambda e: None,
    "nucleus": lambda e: e.set_sampling_params(top_k=50, top_p=0.95, temperature=0.8, seed=4242),
    "top5": lambda e: e.set_sampling(5, 11),
}


@pytest.mark.parametrize("chooser", list(CHOOSERS))
def test_a_one_id_mask_holds_under_every_chooser(chooser):
    def setup(e):
        CHOOSERS[chooser](e)
        e.set_allowed([ONLY])
    assert _generate(setup) == [ONLY] * N_NEW


def test_a_three_id_mask_holds_under_the_top_k_sampler():
    ids = [ONLY, 7, V - 1]

    def setup(e):
        e.set_sampling(5, 11)
        e.set_allowed(ids)
    got = _generate(setup)
    assert set(got) <= set(ids), got


def test_the_nucleus_sampler_reads_the_processed_row():
    bans = {GOLDEN[0]: -np.inf, GOLDEN[1]: -np.inf, GOLDEN[2]: -np.inf, 1: -np.inf, 3: -np.inf}
    odd = np.arange(1, V, 2)
    words = L.words_of(V, odd)
    assert (words == np.uint32(0xAAAAAAAA)).all()
    n = len(PROMPT)
    undecided = 0
    with _engine() as e:
        e.set_sampling_params(**PARAMS)
        e.set_logit_rules(bias=bans)
        e.set_allowed(odd)
        e.set_prompt(PROMPT)
        e.decode(n, use_graph=False)
        got = []
        for i in range(N_NEW):
            pos = n - 1 + i
            raw, proc, toks = e.logits(), e.processed_logits(), e.tokens(pos + 2)
            want_row, _ = L.process(raw, _dense(bans), words)
            assert np.array_equal(_bits(proc), _bits(want_row)), i
            tok, _, cs, ds = N.sample(proc, toks[:pos + 1], PARAMS["repetition_penalty"], PARAMS["temperature"],
                                      PARAMS["top_k"], PARAMS["top_p"], PARAMS["seed"] + pos + 1)
            g = int(toks[pos + 1])
            print(i, g, tok, cs, ds)
            got.append(g)
            assert g & 1 and g not in bans
            if cs >= N.DECIDED and ds >= N.DECIDED:
                assert g == tok, (i, g, tok, cs, ds)
            else:
                undecided += 1
            if i + 1 < N_NEW:
                e.decode(1, use_graph=False)
    assert undecided <= 0.05 * N_NEW
    plain = _generate(lambda e: e.set_sampling_params(**PARAMS))
    assert got != plain  # the sampler alone picks other (even, unbanned) ids


def test_choose_changes_the_mask_between_replayed_steps():
    x, p = 17, 29
    choices = [[x], [GOLDEN[0], p], [GOLDEN[0], GOLDEN[1], 41], [GOLDEN[0], GOLDEN[1], GOLDEN[2]]]
    n = len(PROMPT)
    with _engine() as ref:
        ref.set_prompt(PROMPT)
        ref.decode(n - 1, use_graph=False)

        def pick(kids, step):
            ref.set_allowed(kids)
            ref.decode(1, use_graph=False)
            tok = L.process(ref.logits(), None, L.words_of(V, kids))[1]
            assert int(ref.tokens(n + step + 1)[n + step]) == tok
            return tok
        want = L.walk(choices, pick)
    assert want == (3, GOLDEN[:3])  # greedy decoding's own tokens are always allowed here: the deepest leaf
    with _engine() as e:
        e.set_allowed([ONLY])
        got = e.choose(PROMPT, choices, use_graph=True)
        assert (got[0], [int(t) for t in got[1]]) == want
        # the mask in force before the call is back
        assert [int(t) for t in e._allowed] == [ONLY]
        assert [int(t) for t in e.generate(PROMPT, 6)] == [ONLY] * 6
        e.set_allowed(None)
        assert [int(t) for t in e.generate(PROMPT, 6)] == GOLDEN[:6]
        assert e.choose(PROMPT, [[x], [p]])[1] in ([x], [p]) and e._allowed is None
        assert [int(t) for t in e.generate(PROMPT, 6)] == GOLDEN[:6]


def test_logprobs_stay_those_of_the_raw_row():
    n, n_new = len(PROMPT), 8
    total = n + n_new - 1
    rows = []
    with _engine() as e:
        e.set_logit_rules(**RULES)
        e.set_logprobs(0)
        e.set_prompt(PROMPT)
        for _ in range(total):
            e.decode(1, use_graph=False)
            rows.append(e.logits())
        toks, (lp, _, _) = e.tokens(total + 1), e.logprobs()
    assert [int(t) for t in toks[n:]] == _stepwise()[0][:n_new]
    assert len(lp) == total + 1 and np.isnan(lp[0])
    for pos, z in enumerate(rows):
        want, _ = LP.logprobs(z)
        tok = int(toks[pos + 1])
        LP.assert_close(lp[pos + 1:pos + 2], want[tok:tok + 1], V, f"pos {pos} token {tok}")


def test_off_means_off():
    with _engine() as e:
        e.set_logit_rules()  # all defaults, no mask: rules stay off
        with pytest.raises(Exception, match="logit rules are off"):
            e.processed_logits()
        assert [int(t) for t in e.generate(PROMPT, N_NEW)] == GOLDEN[:N_NEW]
        e.set_logit_rules(**RULES)
        e.set_allowed([A, ONLY, GOLDEN[3]])
        assert [int(t) for t in e.generate(PROMPT, 6)] != GOLDEN[:6]
        e.clear_logit_rules()
        with pytest.raises(Exception, match="logit rules are off"):
            e.processed_logits()
        assert [int(t) for t in e.generate(PROMPT, N_NEW)] == GOLDEN[:N_NEW]
        assert [int(t) for t in e.generate(PROMPT, N_NEW, use_graph=False)] == GOLDEN[:N_NEW]
        # each of the three alone turns the rules on, and taking it away turns them off
        e.set_allowed([ONLY])
        assert [int(t) for t in e.generate(PROMPT, 4)] == [ONLY] * 4
        e.set_allowed(None)
        assert [int(t) for t in e.generate(PROMPT, 6)] == GOLDEN[:6]
        e.set_logit_rules(bias={A: 64.0})
        assert [int(t) for t in e.generate(PROMPT, 4)] == [A] * 4
        e.set_logit_rules()
        assert [int(t) for t in e.generate(PROMPT, 6)] == GOLDEN[:6]


def test_edit_with_rules_equals_a_fresh_engine_with_the_longer_prompt():
    n, keep, forced, n_new = len(PROMPT), 10, [501, A, 503], 6
    dense = _dense(BIAS)
    with _engine() as a:
        a.set_logit_rules(**RULES)
        a.set_prompt(PROMPT)
        a.decode(n + 5, use_graph=False)
        head = [int(t) for t in a.tokens(keep)]
        assert head[n:n + 2] == [A, A]
        a.edit(keep, forced)
        a.decode(len(forced), use_graph=False)
        # the forced ids count as prompt: the window starts after them
        got, _ = _walk(a, keep + len(forced), n_new, keep + len(forced), dense, None, PRESENCE, FREQUENCY)
        rows_a = a.processed_logits()
    with _engine() as b:
        b.set_logit_rules(**RULES)
        b.set_prompt(head + forced)
        b.decode(keep + len(forced), use_graph=False)
        want, _ = _walk(b, keep + len(forced), n_new, keep + len(forced), dense, None, PRESENCE, FREQUENCY)
        rows_b = b.processed_logits()
    assert got == want and got[:2] == [A, A]  # A's earlier picks and the forced A are prompt now
    assert np.array_equal(_bits(rows_a), _bits(rows_b))
    with _engine() as c:
        c.set_logit_rules(**RULES)
        assert [int(t) for t in c.generate(head + forced, n_new)] == want


def test_refusals_and_argument_checks_leave_the_engine_as_it_was():
    from llmi import _lib
    from llmi._lib import LlmiError
    from llmi.engine import Engine, preset
    lib = _lib.lib()
    before = _stepwise()[0][:6]
    with _engine() as e:
        e.set_logit_rules(**RULES)

        def same():
            assert [int(t) for t in e.generate(PROMPT, 6)] == before

        same()
        for bad, msg in (({V: 1.0}, r"token ids must be in \[0, vocab\)"), ({V + 5: -1.0}, "token ids"),
                         ({-1: 1.0}, "token ids"), ({5: float("nan")}, "finite or -inf"),
                         ({5: float("inf")}, "finite or -inf")):
            with pytest.raises(LlmiError, match=msg):
                e.set_logit_rules(bias=bad)
            same()
        ids, vals = np.array([9, 4, 9], np.int32), np.array([1, 2, 3], np.float32)
        assert lib.llmi_engine_set_logit_rules(e._h, ids.ctypes.data, vals.ctypes.data, 3, 0.0, 0.0, 0) == -1
        assert b"given twice" in lib.llmi_last_error()
        assert lib.llmi_engine_set_logit_rules(e._h, None, None, 2, 0.0, 0.0, 0) == -1
        assert lib.llmi_engine_set_logit_rules(e._h, ids.ctypes.data, vals.ctypes.data, -1, 0.0, 0.0, 0) == -1
        assert lib.llmi_engine_set_logit_rules(e._h, None, None, 0, 0.0, 0.0, 2) == -1  # count_prompt
        same()
        for pen in (dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan")),
                    dict(presence_penalty=float("-inf"))):
            with pytest.raises(LlmiError, match="penalties must be finite"):
                e.set_logit_rules(**pen)
        same()
        with pytest.raises(LlmiError, match="token ids"):
            e.set_allowed([3, V])
        with pytest.raises(ValueError):
            e.set_allowed([])
        assert lib.llmi_engine_set_allowed(e._h, ids.ctypes.data, 0) == -1  # an empty set
        buf = np.zeros(V, np.float32)
        assert lib.llmi_engine_processed_logits(e._h, buf.ctypes.data, V - 1) == -1
        assert lib.llmi_engine_processed_logits(e._h, None, V) == -1
        same()
        # speculation and the ring mode, with the rules on first
        with pytest.raises(LlmiError, match="set_speculation: logit rules are on"):
            e.set_speculation(2)
        with pytest.raises(LlmiError, match="set_decode_mode: logit rules are on"):
            e.set_decode_mode(1)
        same()
    # ... and with speculation on first
    with _engine() as e:
        e.set_speculation(2)
        for call in (lambda: e.set_logit_rules(**RULES), lambda: e.set_allowed([ONLY]),
                     lambda: e.set_logit_rules(presence_penalty=1.0)):
            with pytest.raises(LlmiError, match="speculation is on"):
                call()
        assert lib.llmi_engine_set_allowed(e._h, None, 0) == 0  # nothing to remove: no refusal
        e.set_logit_rules()                                     # all defaults: nothing turns on
        assert [int(t) for t in e.generate(PROMPT, 6, speculate=2)] == GOLDEN[:6]
        e.set_speculation(0)
        e.set_logit_rules(**RULES)
        assert [int(t) for t in e.generate(PROMPT, 6)] == before
    # a tensor-parallel rank holds a vocab shard only
    with Engine(preset("tiny", tp_rank=0, tp_world=2)) as e:
        with pytest.raises(LlmiError, match=r"set_logit_rules: the rules need the full logits row"):
            e.set_logit_rules(bias={1: 1.0})
        with pytest.raises(LlmiError, match=r"set_allowed: the rules need the full logits row"):
            e.set_allowed([1])
        assert lib.llmi_engine_set_logit_rules(e._h, None, None, 0, 1.0, 0.0, 0) == -2  # LLMI_EUNSUPPORTED


def test_rules_are_refused_while_the_ring_mode_is_on():
    """The smallest engine the ring layer runs on (tests/test_gpu_ring.py's: 7B width, 2 layers)."""
    from llmi._lib import LlmiError
    from llmi.engine import Engine, preset
    cfg = preset("llama2-7b", layers=2, max_seq=64)
    with Engine(cfg) as e:
        e.load_synthetic(3)
        prompt = np.arange(1, 9, dtype=np.int32)
        e.set_decode_mode(1)
        before = e.generate(prompt, 4)
        with pytest.raises(LlmiError, match="set_logit_rules: the ring decode mode is on"):
            e.set_logit_rules(bias={5: 1.0})
        with pytest.raises(LlmiError, match="set_allowed: the ring decode mode is on"):
            e.set_allowed([5])
        np.testing.assert_array_equal(e.generate(prompt, 4), before)
        e.set_decode_mode(0)
        e.set_allowed([5])
        np.testing.assert_array_equal(e.generate(prompt, 4), [5] * 4)
        with pytest.raises(LlmiError, match="set_decode_mode: logit rules are on"):
            e.set_decode_mode(1)
