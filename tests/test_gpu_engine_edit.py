"""Editing a sequence in place (llmi_engine_edit / llmi_engine_position / llmi_batch_edit,
engine_edit.hip): an engine whose sequence was rewound or extended goes on BITWISE as a fresh
engine that was given the kept ids + the forced ids as its prompt. Every comparison is on uint32
views (or the stored int8 bytes and scale bits of an int8 cache); no tolerance anywhere.

The `tiny` preset with max_seq 192, so positions 64 and 128 (the attention split boundaries) can
be crossed. References are computed once per key and kept as numpy arrays; every engine lives in
a `with` block."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 192
VOCAB = 32000
NUCLEUS = dict(top_p=0.9, temperature=0.8, seed=77)


def _cfg(**over):
    from llmi.engine import preset
    over.setdefault("max_seq", MAX_SEQ)
    return preset("tiny", **over)


def _ids(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(1000 + i, n, VOCAB)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _kv(e, positions):
    from llmi import _lib
    out = []
    for l in (0, 1):
        for v in (False, True):
            for p in positions:
                if e.cfg.kv_dtype == _lib.I8:
                    q, s = e.kv_slot_q8(l, p, v)
                    out += [q.view(np.uint8).copy(), s.copy()]
                else:
                    out.append(_bits(e.kv_slot(l, p, v)).copy())
    return out


def _state(e, n_tok, kv_at=()):
    return (e.tokens(n_tok).copy(), _bits(e.logits()).copy(), _bits(e.hidden()).copy(), _kv(e, kv_at))


def _same(got, want):
    assert np.array_equal(got[0], want[0]), "tokens differ"
    assert np.array_equal(got[1], want[1]), "final logits differ"
    assert np.array_equal(got[2], want[2]), "final hidden state differs"
    assert len(got[3]) == len(want[3])
    for g, w in zip(got[3], want[3]):
        assert np.array_equal(g, w), "a KV cache slot differs"


def _over(wdt="w16", kv="kv16"):
    from llmi import _lib
    return dict(weight_dtype=_lib.I8 if wdt == "w8" else _lib.F16, kv_dtype=_lib.I8 if kv == "kv8" else _lib.F16)


def _setup(e, nucleus=False, lp=None):
    e.load_synthetic(SEED)
    if nucleus:
        e.set_sampling_params(**NUCLEUS)
    if lp is not None:
        e.set_logprobs(lp)


_REF = {}


def _fresh(prompt, plan, kv_at=(), nucleus=False, lp=None, **over):
    """A fresh engine given `prompt`, run through plan = (("decode" | "prefill", n), ...): its end
    state (and the logprob records when lp is set). Computed once per key."""
    from llmi.engine import Engine
    key = (tuple(int(t) for t in prompt), tuple(plan), tuple(kv_at), nucleus, lp, tuple(sorted(over.items())))
    if key not in _REF:
        with Engine(_cfg(**over)) as e:
            _setup(e, nucleus, lp)
            e.set_prompt(prompt)
            for what, n in plan:
                getattr(e, what)(n)
            end = sum(n for _, n in plan)
            _REF[key] = _state(e, end + 1, kv_at) + ((e.logprobs(),) if lp is not None else ())
    return _REF[key]


Q = _ids(50, 8)   # an appended turn
R = _ids(51, 3)   # the ids forced after a rewind
KV1 = (0, 59, 60, 63, 64, 79)
KV2 = (0, 39, 40, 42, 43, 63, 64, 74)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kv", ["kv16", "kv8"])
@pytest.mark.parametrize("wdt", ["w16", "w8"])
def test_extend_equals_a_longer_prompt(wdt, kv, use_graph):
    from llmi.engine import Engine
    over = _over(wdt, kv)
    with Engine(_cfg(**over)) as a:
        _setup(a)
        a.set_prompt(_ids(0, 5))
        a.decode(60, use_graph)
        toks = a.tokens(61)
        assert len(toks) == 61
        a.edit(60, np.concatenate([toks[60:61], Q]))  # 9 ids: the copied form
        a.decode(20, use_graph)
        got = _state(a, 81, KV1)
    _same(got, _fresh(np.concatenate([toks, Q]), (("decode", 80),), KV1, **over))


def _rewind(use_graph, nucleus=False, **over):
    from llmi.engine import Engine
    with Engine(_cfg(**over)) as a:
        _setup(a, nucleus)
        a.set_prompt(_ids(0, 5))
        a.decode(70, use_graph)
        toks = a.tokens(71)
        a.edit(40, R)  # 3 ids: they travel in the launch arguments
        a.decode(35, use_graph)
        got = _state(a, 76, KV2)
    _same(got, _fresh(np.concatenate([toks[:40], R]), (("decode", 75),), KV2, nucleus=nucleus, **over))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("wdt,kv", [("w16", "kv16"), ("w8", "kv8")])
def test_rewind(wdt, kv, use_graph):
    _rewind(use_graph, **_over(wdt, kv))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_rewind_with_the_nucleus_sampler(use_graph):
    """The draw is a function of the seed and the position, so a rewound sampling engine draws
    what the fresh one draws."""
    _rewind(use_graph, nucleus=True)


def test_prefill_after_an_edit():
    from llmi.engine import Engine
    forced = _ids(52, 20)
    kv_at = (0, 29, 30, 49, 50, 59)
    with Engine(_cfg()) as a:
        _setup(a)
        a.set_prompt(_ids(0, 5))
        a.decode(30)
        toks = a.tokens(31)
        a.edit(30, forced)
        assert a.position() == (30, 50)
        a.prefill(20)
        a.decode(10)
        got = _state(a, 61, kv_at)
    want = _fresh(np.concatenate([toks[:30], forced]), (("decode", 30), ("prefill", 20), ("decode", 10)), kv_at)
    _same(got, want)


def test_logprob_records_after_an_edit():
    from llmi.engine import Engine
    keep = 40

    def not_computed(lp, ids, tlp, q):
        return np.isnan(lp[q]) and (ids[q] == -1).all() and np.isnan(tlp[q]).all()

    def same_records(x, y, lo, hi):
        return all(np.array_equal(_bits(u[lo:hi]) if u.dtype == np.float32 else u[lo:hi],
                                  _bits(w[lo:hi]) if w.dtype == np.float32 else w[lo:hi]) for u, w in zip(x, y))

    with Engine(_cfg()) as a:
        _setup(a, lp=2)
        a.set_prompt(_ids(0, 5))
        a.decode(70)
        toks = a.tokens(71)
        before = a.logprobs()
        assert len(before[0]) == 71 and not np.isnan(before[0][1:]).any()
        a.edit(keep, R)
        now = a.logprobs()
        assert len(now[0]) == keep + 1
        assert not_computed(*now, keep), "record `keep` must read not computed after the edit"
        assert same_records(now, before, 0, keep), "records below keep must keep their bits"
        a.decode(35)
        after = a.logprobs()
        toks_a = a.tokens(76)
        # a second, shorter rewind: record 50 is wiped, what lies below stays
        a.edit(50, R[:1])
        again = a.logprobs()
        assert len(again[0]) == 51 and not_computed(*again, 50) and same_records(again, after, 0, 50)
    want = _fresh(np.concatenate([toks[:keep], R]), (("decode", 75),), lp=2)
    assert np.array_equal(toks_a, want[0])
    ref = want[4]
    assert len(after[0]) == len(ref[0]) == 76
    assert not_computed(*after, keep), "the forward at keep - 1 is not run again: record keep stays not computed"
    assert same_records(after, before, 0, keep)
    assert same_records(after, ref, keep + 1, 76), "records above keep must be the fresh engine's"
    assert same_records(after, ref, 1, keep)
    assert not np.isnan(ref[0][keep])


def test_extend_and_position():
    from llmi import _lib
    from llmi.engine import Engine
    with Engine(_cfg()) as a:
        _setup(a)
        assert a.position() == (0, 0)
        a.set_prompt(_ids(0, 5))
        assert a.position() == (0, 5)
        a.decode(3)
        assert a.position() == (3, 5)
        with pytest.raises(_lib.LlmiError):
            a.extend(Q)  # the prompt is not consumed
        assert a.position() == (3, 5)
        a.decode(57)
        assert a.position() == (60, 5)
        toks = a.tokens(61)
        a.extend(Q)
        assert a.position() == (60, 69)
        a.decode(20)
        assert a.position() == (80, 69)
        got = _state(a, 81, KV1)
        a.edit(80, [])  # keep == P with no ids: nothing happens
        assert a.position() == (80, 69)
        a.edit(10, R)
        assert a.position() == (10, 13)
    _same(got, _fresh(np.concatenate([toks, Q]), (("decode", 80),), KV1, **_over()))


def test_errors_change_nothing():
    from llmi import _lib
    from llmi.engine import Engine, preset
    L = _lib.lib()
    one = np.array([7], np.int32)
    many = np.arange(MAX_SEQ, dtype=np.int32)
    bad = np.array([1, VOCAB, 2], np.int32)
    prompt = _ids(0, 5)
    with Engine(_cfg()) as a:
        _setup(a)
        assert L.llmi_engine_edit(a._h, 0, one.ctypes.data, 1) == -1  # no prompt set
        assert b"set_prompt" in L.llmi_last_error()
        a.set_prompt(prompt)
        a.decode(20)
        before = (a.tokens().copy(), _bits(a.logits()).copy(), a.position())
        assert L.llmi_engine_edit(a._h, 21, one.ctypes.data, 1) == -1  # keep > P
        assert L.llmi_engine_edit(a._h, -1, one.ctypes.data, 1) == -1  # keep < 0
        assert L.llmi_engine_edit(a._h, 10, None, 0) == -1  # n == 0 below P
        assert L.llmi_engine_edit(a._h, 20, many.ctypes.data, MAX_SEQ - 19) == -1  # keep + n > max_seq
        assert b"max_seq" in L.llmi_last_error()
        assert L.llmi_engine_edit(a._h, 10, bad.ctypes.data, 3) == -1  # an id equal to vocab
        assert L.llmi_engine_edit(a._h, 10, one.ctypes.data, -1) == -1
        after = (a.tokens().copy(), _bits(a.logits()).copy(), a.position())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
        a.decode(10)
        got = _state(a, 31)
    _same(got, _fresh(prompt, (("decode", 30),)))
    with Engine(preset("llama2-7b", layers=2, max_seq=64)) as e:  # (the ring layer needs hidden 4096)
        e.set_prompt(prompt)
        e.set_decode_mode(1)
        assert L.llmi_engine_edit(e._h, 0, one.ctypes.data, 1) == -2
        assert b"ring" in L.llmi_last_error()
        assert e.position() == (0, 5)


def test_a_speculating_engine_can_be_edited():
    from llmi.engine import Engine
    over = dict(vocab=64)  # a small vocabulary, so that the lookup proposes something
    from llmi.engine import synth_prompt
    forced = synth_prompt(1051, 3, 64)
    with Engine(_cfg(**over)) as a:
        _setup(a)
        a.set_speculation(4)
        a.set_prompt(synth_prompt(1000, 5, 64))
        a.decode(50)
        toks = a.tokens(51)
        a.edit(30, forced)
        a.decode(3)
        st = a.generate_lookup(40, 4)
        assert a.position() == (73, 33)
        assert st.verify_steps + st.accepted == 40
        got = _state(a, 74, (0, 29, 30, 63, 64, 72))
    _same(got, _fresh(np.concatenate([toks[:30], forced]), (("decode", 73),), (0, 29, 30, 63, 64, 72), **over))


def test_batch_edit_touches_one_slot():
    from llmi import _lib
    from llmi.engine import Batch, Engine
    L = _lib.lib()
    prompts = [_ids(0, 5), _ids(1, 7), _ids(2, 4)]
    with Engine(_cfg()) as e:  # slot 1's sequence in an engine of its own, edited the same way
        _setup(e)
        e.set_prompt(prompts[1])
        e.decode(40)
        e.edit(25, R)
        e.decode(30)
        want1 = (e.tokens(56).copy(), _bits(e.logits()).copy())
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(SEED)
        for i, p in enumerate(prompts):
            b.set_prompt(i, p)
        b.decode(40)
        assert L.llmi_batch_edit(b._h, 3, 25, R.ctypes.data, 3) == -1  # no such slot
        assert L.llmi_batch_edit(b._h, 1, 41, R.ctypes.data, 3) == -1  # keep > P
        b.edit(1, 25, R)
        b.decode(30)
        assert np.array_equal(b.tokens(1, 56), want1[0])
        assert np.array_equal(_bits(b.logits(1)), want1[1])
        for i in (0, 2):
            ref = _fresh(prompts[i], (("decode", 70),))
            assert np.array_equal(b.tokens(i, 71), ref[0])
            assert np.array_equal(_bits(b.logits(i)), ref[1])
