"""Forking a batch slot (llmi_batch_fork / Batch.fork / Batch.sample; engine_fork.hip, kv_fork.hip):
one slot's sequence -- cache rows, ids, decode state -- copied into other slots on the device.
The contract is BITWISE: a destination of the cut form goes on as a slot that was edited the same
way (Batch.edit), a destination of the continue form as the source itself, and every slot as an
Engine decoding the sequence alone. np.array_equal on ids and on uint32 views of logits and
logprob records; no tolerance anywhere.

The `tiny` preset with max_seq 192, so positions cross the 64-row attention split boundary twice.
References are computed once per key and kept as numpy arrays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 192
VOCAB = 32000
FIRST, MORE = 130, 40
NUCLEUS = dict(top_p=0.9, temperature=0.8)


def _cfg(**over):
    from llmi.engine import preset
    over.setdefault("max_seq", MAX_SEQ)
    return preset("tiny", **over)


def _ids(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(1000 + i, n, VOCAB)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _over(name):
    from llmi import _lib
    return {
        "w16-kv16": {},
        "w16-kv32": dict(kv_dtype=_lib.F32),
        "w16-kv8": dict(kv_dtype=_lib.I8),
        "w8-kv16": dict(weight_dtype=_lib.I8),
        "w8-kv8": dict(weight_dtype=_lib.I8, kv_dtype=_lib.I8),
        "gqa": dict(kv_heads=2),
    }[name]


P = _ids(0, 8)
_REF = {}


def _alone(script, sampling=None, lp=None, **over):
    """An Engine alone run through script = (("prompt", ids) | ("decode", n) | ("prefill", n) |
    ("edit", keep, ids) | ("seed", s)), ...): (tokens, final logits bits[, logprob records])."""
    from llmi.engine import Engine
    key = (tuple((s[0],) + tuple(tuple(int(t) for t in x) if hasattr(x, "__len__") else x for x in s[1:])
                 for s in script), tuple(sorted((sampling or {}).items())), lp, tuple(sorted(over.items())))
    if key not in _REF:
        with Engine(_cfg(**over)) as e:
            e.load_synthetic(SEED)
            if sampling:
                e.set_sampling_params(**sampling)
            if lp is not None:
                e.set_logprobs(lp)
            for s in script:
                if s[0] == "prompt":
                    e.set_prompt(s[1])
                elif s[0] == "decode":
                    e.decode(s[1])
                elif s[0] == "prefill":
                    e.prefill(s[1])
                elif s[0] == "edit":
                    e.edit(s[1], s[2])
                elif s[0] == "seed":
                    e.set_sampling_params(**dict(sampling, seed=s[1]))
            _REF[key] = (e.tokens().copy(), _bits(e.logits()).copy()) + ((e.logprobs(),) if lp is not None else ())
    return _REF[key]


def _slot(b, i):
    return b.tokens(i).copy(), _bits(b.logits(i)).copy()


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: tokens differ\n{got[0]}\n{want[0]}"
    assert np.array_equal(got[1], want[1]), f"{what}: final logits differ"


def _forced(n):
    return _ids(60 + n, n)


def _edited(keep, n, more=MORE, first=FIRST, **over):
    """The sequence P decoded `first` steps, edited at keep with n forced ids, decoded `more`."""
    return _alone((("prompt", P), ("decode", first), ("edit", keep, _forced(n)), ("decode", more)), **over)


CUTS = [(keep, n) for keep in (0, 1, 63, 64, 65, 130) for n in (1, 9)]  # 9 ids: the staged path


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("config", ["w16-kv16", "w16-kv32", "w16-kv8", "w8-kv16", "w8-kv8", "gqa"])
def test_cut_form_equals_edit(config, use_graph):
    """Slots 0, 2, 4 and 6 hold one sequence; three cuts a run: fork(0, 1 + 2j) against
    edit(2 + 2j). The forked slot equals the edited one, the source the sequence decoded alone."""
    from llmi.engine import Batch
    over = _over(config)
    for g in range(0, len(CUTS), 3):
        with Batch(_cfg(**over), 7) as b:
            b.load_synthetic(SEED)
            for s in (0, 2, 4, 6):
                b.set_prompt(s, P)
            b.decode(FIRST, use_graph)
            for j, (keep, n) in enumerate(CUTS[g:g + 3]):
                b.fork(0, 1 + 2 * j, keep, _forced(n))
                b.edit(2 + 2 * j, keep, _forced(n))
            b.decode(MORE, use_graph)
            for j, (keep, n) in enumerate(CUTS[g:g + 3]):
                got = _slot(b, 1 + 2 * j)
                assert len(got[0]) == keep + MORE + 1
                _same(got, _slot(b, 2 + 2 * j), f"keep {keep}, {n} ids: fork against edit")
            _same(_slot(b, 0), _alone((("prompt", P), ("decode", FIRST + MORE)), **over), "the source")
    # and the edited slot is the engine edited alone (once: the slots' own contract)
    keep, n = CUTS[-1]
    _same(got, _edited(keep, n, **over), "fork against the engine edited alone")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("config", ["w16-kv16", "w16-kv8"])
def test_continue_form_greedy(config, use_graph):
    from llmi.engine import Batch
    over = _over(config)
    with Batch(_cfg(**over), 3) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, P)
        b.decode(70, use_graph)
        b.fork(0, [1, 2])
        b.decode(30, use_graph)
        want = _alone((("prompt", P), ("decode", 100)), **over)
        for i in range(3):
            _same(_slot(b, i), want, f"slot {i}")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_continue_form_with_samplers(use_graph):
    """The token pending at the fork was drawn by the source; from the next one on every slot
    follows its own seed: an Engine alone whose seed was switched at that position."""
    from llmi.engine import Batch
    seeds = (77, 78, 79)
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i in range(3):
            b.set_sampling_params(i, seed=seeds[i], **NUCLEUS)
        b.set_prompt(0, P)
        b.decode(70, use_graph)
        b.fork(0, [1, 2], keep=None)
        b.decode(30, use_graph)
        got = [_slot(b, i) for i in range(3)]
    for i in range(3):
        want = _alone((("prompt", P), ("decode", 70), ("seed", seeds[i]), ("decode", 30)),
                      sampling=dict(NUCLEUS, seed=seeds[0]))
        _same(got[i], want, f"slot {i}")
        assert np.array_equal(got[i][0][:71], got[0][0][:71])  # the history and the pending token
    assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[1][0], got[2][0])
    assert not np.array_equal(got[0][0], got[2][0])


@pytest.mark.parametrize("config", ["w16-kv16", "w16-kv8"])
def test_fan_out_to_seven(config):
    from llmi.engine import Batch
    over = _over(config)
    with Batch(_cfg(**over), 8) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, P)
        b.decode(FIRST)
        b.fork(0, range(1, 8), 65, _forced(1))
        b.decode(MORE)
        want = _edited(65, 1, **over)
        for i in range(1, 8):
            _same(_slot(b, i), want, f"slot {i}")
        _same(_slot(b, 0), _alone((("prompt", P), ("decode", FIRST + MORE)), **over), "the source")


def test_destination_active_or_idle_ends_the_same():
    """Slot 1 is mid-sequence with a longer history than the source, slot 2 idle. tokens() raises
    on a non-zero device error word, so reading them asserts the copied word of a healthy source."""
    from llmi.engine import Batch
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        b.set_prompt(1, _ids(1, 5))
        b.decode(50)
        b.set_prompt(0, P)
        b.decode(100)   # slot 1 at 150, slot 0 at 100
        b.fork(0, [1, 2], 65, _forced(1))
        b.decode(30)
        want = _edited(65, 1, more=30, first=100)
        _same(_slot(b, 1), want, "the active destination")
        _same(_slot(b, 2), want, "the idle destination")
        # ... and the continue form over whatever they hold now
        b.fork(0, [1, 2])
        b.decode(10)
        want = _alone((("prompt", P), ("decode", 140)))
        for i in range(3):
            _same(_slot(b, i), want, f"slot {i} continued")


def _lp_bits(rec):
    return [np.ascontiguousarray(a).view(np.uint32) for a in rec]


def test_logprob_records():
    """n_top 2 on the source, on destination 1 and on the edited slot 4; n_top 3 on destination 2;
    off on destination 3."""
    from llmi.engine import Batch
    keep = 65
    with Batch(_cfg(), 5) as b:
        b.load_synthetic(SEED)
        for s, top in ((0, 2), (1, 2), (2, 3), (4, 2)):
            b.set_logprobs(s, top)
        b.set_prompt(0, P)
        b.set_prompt(4, P)
        b.set_prompt(1, _ids(1, 5))  # destination 1 holds records of its own
        b.decode(100)
        src = _lp_bits(b.logprobs(0))
        b.fork(0, [1, 2, 3], keep, _forced(1))
        b.edit(4, keep, _forced(1))
        got = _lp_bits(b.logprobs(1))
        assert len(got[0]) == keep + 1 and got[1].shape == (keep + 1, 2)
        for g, s in zip(got, src):
            assert np.array_equal(g[:keep], s[:keep]), "records below keep are the source's"
            assert np.all(g[keep:] == 0xFFFFFFFF), "record keep is not computed"
        other = _lp_bits(b.logprobs(2))
        assert other[1].shape == (keep + 1, 3)
        assert all(np.all(a == 0xFFFFFFFF) for a in other), "another n_top: nothing is computed"
        b.decode(30)
        got, want = _lp_bits(b.logprobs(1)), _lp_bits(b.logprobs(4))
        assert len(got[0]) == keep + 31
        for g, w in zip(got, want):
            assert np.array_equal(g, w), "records after the fork against the edited slot's"
        other = _lp_bits(b.logprobs(2))
        assert np.all(other[0][:keep + 1] == 0xFFFFFFFF) and not np.any(other[0][keep + 1:] == 0xFFFFFFFF)
        for i in (1, 2, 3):
            _same(_slot(b, i), _slot(b, 4), f"slot {i}")
        # the continue form copies the pending token's record too
        b.fork(4, 1)
        got = _lp_bits(b.logprobs(1))
        for g, w in zip(got, want):
            assert np.array_equal(g, w), "continue form: records [0, position]"
        assert np.all(_lp_bits(b.logprobs(2))[0][:keep + 1] == 0xFFFFFFFF)


def test_rules_of_the_destination():
    from llmi.engine import Batch
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, P)
        b.set_prompt(2, P)
        b.decode(100)
        for s in (1, 2):
            b.set_logit_rules(s, presence_penalty=0.5, frequency_penalty=0.25, count_prompt=True)
        b.fork(0, 1, 64, _forced(1))
        b.edit(2, 64, _forced(1))
        b.decode(30)
        _same(_slot(b, 1), _slot(b, 2), "fork against edit, penalties on")
        assert np.array_equal(_bits(b.processed_logits(1)), _bits(b.processed_logits(2)))
        assert not np.array_equal(_bits(b.processed_logits(1)), _bits(b.logits(1)))
        _same(_slot(b, 0), _alone((("prompt", P), ("decode", 130))), "the source")


def _script(b, use_graph, refusals=False):
    from llmi._lib import LlmiError
    b.set_prompt(0, P)
    b.set_prompt(1, _ids(1, 5))
    b.decode(70, use_graph)
    b.fork(0, 2, 64, _forced(9))
    b.decode(10, use_graph)
    if refusals:
        bad = [
            ("idle", lambda: b.fork(3, 1, 0, _forced(1))),
            ("out of range", lambda: b.fork(0, 4, 10, _forced(1))),
            ("out of range", lambda: b.fork(0, [1, -1], 10, _forced(1))),
            ("out of range", lambda: b.fork(4, 1, 10, _forced(1))),
            ("is the source", lambda: b.fork(0, [1, 0], 10, _forced(1))),
            ("listed twice", lambda: b.fork(0, [1, 3, 1], 10, _forced(1))),
            ("1..7 destinations", lambda: b.fork(0, [], 10, _forced(1))),
            ("id out of range", lambda: b.fork(0, 1, 10, [VOCAB])),
            ("id out of range", lambda: b.fork(0, 1, 10, [5, -1])),
            ("id out of range", lambda: b.fork(0, 1, 10, list(range(8)) + [VOCAB])),
            ("pending token", lambda: b.fork(0, 1, 10)),
            ("keep must be", lambda: b.fork(0, 1, 81, _forced(1))),
            ("keep must be", lambda: b.fork(0, 1, -2, _forced(1))),
            ("max_seq", lambda: b.fork(0, 1, 80, _ids(7, MAX_SEQ - 79))),
        ]
        for text, call in bad:
            with pytest.raises(LlmiError) as err:
                call()
            assert "(-1)" in str(err.value) and text in str(err.value), (text, str(err.value))
        assert b._pos[:4] == [80, 80, 74, 0] and b._plen[:4] == [8, 5, 73, 0]
    b.fork(1, 3)
    b.decode(20, use_graph)
    return [_slot(b, i) for i in range(4)]


def test_graphs_survive_a_fork_and_refusals_change_nothing():
    """One script three ways: eager, with graphs (decode, fork, decode: no captured step is
    invalidated, and none is stale), and with every refused call in the middle."""
    from llmi.engine import Batch
    runs = []
    for use_graph, refusals in ((False, False), (True, False), (True, True)):
        with Batch(_cfg(), 4) as b:
            b.load_synthetic(SEED)
            runs.append(_script(b, use_graph, refusals))
    for other, what in ((runs[1], "graphs"), (runs[2], "refused calls")):
        for i in range(4):
            _same(other[i], runs[0][i], f"{what}: slot {i}")
    _same(runs[0][0], _alone((("prompt", P), ("decode", 100))), "slot 0")
    _same(runs[0][3], _alone((("prompt", _ids(1, 5)), ("decode", 100))), "slot 3, slot 1 continued")
    _same(runs[0][2], _alone((("prompt", P), ("decode", 70), ("edit", 64, _forced(9)), ("decode", 30))), "slot 2")


SAMPLE = dict(temperature=0.8, top_p=0.9)


def test_sample_by_decode_steps():
    from llmi.engine import Batch
    prompt, n_new, seeds = _ids(3, 9), 70, [11, 12, 13, 14]
    with Batch(_cfg(), 4) as b:
        b.load_synthetic(SEED)
        out = b.sample(prompt, 4, n_new, seeds=seeds, prefill=False, **SAMPLE)
        assert len(out) == 4
        for i in range(4):
            want = _alone((("prompt", prompt), ("decode", 9 + n_new - 1)), sampling=dict(SAMPLE, seed=seeds[i]))
            assert np.array_equal(out[i], want[0][9:]) and len(out[i]) == n_new, (i, out[i], want[0][9:])
            assert np.array_equal(_bits(b.logits(i)), want[1])
        for i in range(4):
            for j in range(i):
                assert not np.array_equal(out[i], out[j])
        # default seeds: the seed keyword + 0 .. n - 1; n below n_seq leaves the other slots idle
        out = b.sample(prompt, 2, n_new, prefill=False, seed=12, **SAMPLE)
        for i in range(2):
            want = _alone((("prompt", prompt), ("decode", 9 + n_new - 1)), sampling=dict(SAMPLE, seed=12 + i))
            assert np.array_equal(out[i], want[0][9:])
        assert len(b.tokens(2)) == 0


def test_sample_by_prefill_one_row_prompt_and_logprob_sums():
    from llmi.engine import Batch
    prompt, n_new, seeds = _ids(3, 9), 70, [11, 12, 13, 14]
    with Batch(_cfg(), 4) as b:
        b.load_synthetic(SEED)
        out = b.sample(prompt, 4, n_new, seeds=seeds, **SAMPLE)
        for i in range(4):
            want = _alone((("prompt", prompt), ("prefill", 8), ("decode", n_new)), sampling=dict(SAMPLE, seed=seeds[i]))
            assert np.array_equal(out[i], want[0][9:]) and len(out[i]) == n_new, (i, out[i], want[0][9:])
            assert np.array_equal(_bits(b.logits(i)), want[1])
        # a prompt of one id: the keep == 0 case
        one = _ids(4, 1)
        out = b.sample(one, 3, 20, seeds=seeds[:3], **SAMPLE)
        for i in range(3):
            want = _alone((("prompt", one), ("decode", 20)), sampling=dict(SAMPLE, seed=seeds[i]))
            assert np.array_equal(out[i], want[0][1:]) and len(out[i]) == 20
        # logprobs on: the summed token logprob of every continuation
        for i in range(4):
            b.set_logprobs(i, 0)
        out, sums = b.sample(prompt, 4, n_new, seeds=seeds, prefill=False, **SAMPLE)
        assert len(sums) == 4
        for i in range(4):
            lp = b.logprobs(i, 9 + n_new)[0]
            assert len(lp) == 9 + n_new and not np.any(np.isnan(lp[9:]))
            assert sums[i] == np.sum(lp[9:], dtype=np.float64) and sums[i] < 0
            want = _alone((("prompt", prompt), ("decode", 9 + n_new - 1)), sampling=dict(SAMPLE, seed=seeds[i]), lp=0)
            assert np.array_equal(out[i], want[0][9:])
            assert np.array_equal(_bits(lp[9:]), _bits(want[2][0][9:9 + n_new]))
