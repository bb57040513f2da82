"""Draft-model speculative decoding (llmi_engine_generate_draft, engine_spec.hip): a second engine
proposes, the target verifies, and WHATEVER the draft proposes the target's tokens, final logits,
hidden state and cache are BITWISE those of plain greedy decode. The reference throughout is a
plain Engine with the same seed running generate(prompt, 136). No tolerance anywhere.

The `tiny` preset with max_seq 192: positions 0 .. 139 are stepped, across the attention split
boundaries at 64 and 128. Every engine lives in a `with` block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
MAX_SEQ = 192
PROMPT_N = 5
N_NEW = 136
TOTAL = PROMPT_N + N_NEW
KV_AT = (0, 63, 64, TOTAL - 2)  # (the last position stepped)


def _cfg(**over):
    from llmi.engine import preset
    over.setdefault("max_seq", MAX_SEQ)
    return preset("tiny", **over)


def _prompt():
    from llmi.engine import synth_prompt
    return synth_prompt(1000, PROMPT_N, 32000)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _state(e):
    kv = [_bits(e.kv_slot(l, p, v)).copy() for l in (0, 1) for v in (False, True) for p in KV_AT]
    return (e.tokens(TOTAL).copy(), _bits(e.logits()).copy(), _bits(e.hidden()).copy(), kv)


_REF = {}


def _plain(**over):
    from llmi.engine import Engine
    key = tuple(sorted(over.items()))
    if key not in _REF:
        with Engine(_cfg(**over)) as e:
            e.load_synthetic(SEED)
            e.generate(_prompt(), N_NEW)
            _REF[key] = _state(e)
    return _REF[key]


def _same_as_plain(e, **over):
    got, want = _state(e), _plain(**over)
    assert np.array_equal(got[0], want[0]), "tokens differ from plain decode's"
    assert np.array_equal(got[1], want[1]), "final logits differ from plain decode's"
    assert np.array_equal(got[2], want[2]), "final hidden state differs from plain decode's"
    for g, w in zip(got[3], want[3]):
        assert np.array_equal(g, w), "a KV cache slot differs from plain decode's"


def _run(k, use_graph=True, prefill=False, draft_seed=SEED, draft_over=None, target_over=None, plain_steps=0,
         calls=None):
    """Target: prompt, PROMPT_N + plain_steps decode steps, then generate_draft calls covering the
    rest (calls: their n_steps; default one call). Returns the summed counts."""
    from llmi.engine import Engine
    target_over = target_over or {}
    left = N_NEW - 1 - plain_steps
    calls = calls or [left]
    assert sum(calls) == left
    with Engine(_cfg(**target_over)) as t, Engine(_cfg(**(draft_over or {}))) as d:
        t.load_synthetic(SEED)
        d.load_synthetic(draft_seed)
        t.set_speculation(k)
        t.set_prompt(_prompt())
        t.decode(PROMPT_N + plain_steps, use_graph)
        tot = [0, 0, 0]
        for n in calls:
            s = t.generate_draft(d, n, k, prefill=prefill, use_graph=use_graph)
            assert s.verify_steps + s.accepted == n
            assert 0 <= s.accepted <= s.drafted
            tot = [tot[0] + s.verify_steps, tot[1] + s.drafted, tot[2] + s.accepted]
        assert t.position() == (TOTAL - 1, PROMPT_N)
        _same_as_plain(t, **target_over)
        # the draft is left aligned with the target: it holds the target's ids up to its position
        dp = d.position()[0]
        assert dp <= TOTAL - 1 and np.array_equal(d.tokens(dp)[:dp], _plain(**target_over)[0][:dp])
    return tot


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_a_twin_draft_is_always_accepted(k, use_graph):
    """Same configuration and seed: every proposal is the target's own token, so every cycle takes
    the all-accepted resync (the two-id edit)."""
    steps, drafted, accepted = _run(k, use_graph)
    assert accepted == drafted > 0
    assert steps == -(-(N_NEW - 1) // (k + 1))


def test_a_draft_with_another_seed():
    """Other weights: acceptance is about zero, every cycle takes the one-id edit."""
    steps, drafted, accepted = _run(4, draft_seed=SEED + 1)
    print(f"[draft] other seed: verify_steps {steps} drafted {drafted} accepted {accepted}")
    assert drafted > 0 and 0 <= accepted <= drafted


def test_a_draft_of_another_kind():
    from llmi import _lib
    steps, drafted, accepted = _run(4, draft_over=dict(layers=1, weight_dtype=_lib.I4, kv_dtype=_lib.I8))
    print(f"[draft] 1 layer, int4 weights, int8 KV: verify_steps {steps} drafted {drafted} accepted {accepted}")


def test_int8_target_with_f32_kv():
    from llmi import _lib
    _run(4, target_over=dict(weight_dtype=_lib.I8, kv_dtype=_lib.F32))


@pytest.mark.parametrize("prefill", [True, False], ids=["prefill", "steps"])
def test_late_start(prefill):
    """The target is 30 plain steps past its prompt when a draft without a prompt joins: the draft
    catches up from position 0, through its prefill or as decode steps."""
    _run(4, prefill=prefill, plain_steps=30)


def test_two_calls_in_a_row():
    """The second call's catch-up finds the draft already in step."""
    steps, drafted, accepted = _run(4, calls=[60, 75])
    assert accepted == drafted > 0


def test_refusals():
    from llmi import _lib
    from llmi.engine import Engine
    import ctypes as C
    L = _lib.lib()
    st = _lib.SpecStats()

    def rc(t, d, k=3):
        return L.llmi_engine_generate_draft(t._h, d._h, 10, k, 0, 1, C.byref(st))

    with Engine(_cfg()) as t, Engine(_cfg()) as d:
        t.load_synthetic(SEED)
        d.load_synthetic(SEED)
        t.set_prompt(_prompt())
        t.decode(PROMPT_N)
        assert rc(t, d) == -1 and b"max_draft" in L.llmi_last_error()  # no set_speculation
        t.set_speculation(2)
        assert rc(t, d, 3) == -1 and b"max_draft" in L.llmi_last_error()  # above set_speculation's
        t.set_speculation(4)
        assert rc(t, t) == -1 and b"itself" in L.llmi_last_error()
        with Engine(_cfg(vocab=64)) as o:
            assert rc(t, o) == -1 and b"vocab" in L.llmi_last_error()
        with Engine(_cfg(max_seq=128)) as o:
            assert rc(t, o) == -1 and b"max_seq" in L.llmi_last_error()
        t.set_speculation(0)
        t.set_sampling(4, 1)
        assert rc(t, d) == -2 and b"sampler" in L.llmi_last_error()
        t.set_sampling(0)
        t.set_speculation(4)
        assert t.position() == (PROMPT_N, PROMPT_N) and d.position() == (0, 0)
        # both engines are usable afterwards
        s = t.generate_draft(d, N_NEW - 1, 4)
        assert s.accepted == s.drafted > 0
        _same_as_plain(t)


def test_generate_with_a_draft_engine():
    from llmi.engine import Engine
    with Engine(_cfg()) as t, Engine(_cfg()) as d:
        t.load_synthetic(SEED)
        d.load_synthetic(SEED + 1)
        toks = t.generate(_prompt(), N_NEW, speculate=4, draft=d)
        assert np.array_equal(toks, _plain()[0][PROMPT_N:])
        _same_as_plain(t)
        s = t.spec_stats
        assert s.verify_steps + s.accepted == N_NEW - 1 and s.drafted > 0
