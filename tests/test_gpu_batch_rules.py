"""Logit rules per Batch slot (llmi_batch_set_logit_rules / _set_allowed): three slots with prompts
of different lengths -- no rules, bias + ban + penalties, a mask only -- each bitwise the lone
Engine with the same prompt and rules, eager and replayed, after a slot prefill too; changing one
slot's allowed set between replayed steps changes only that slot.

Run this file in its own pytest process: its exit status is part of the result."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = 12
A, V = 1234, 32000
MASK = [4321, 77, 31999, 15000]


def _fixture():
    return np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)


PROMPT = _fixture()["prompt"]
GOLDEN = [int(t) for t in _fixture()["tokens"]]
RULES = dict(bias={A: 64.0, GOLDEN[0]: -np.inf}, presence_penalty=0.5, frequency_penalty=40.0)
# prompts of 8, 5 and 11 ids
PROMPTS = [PROMPT, PROMPT[:5], np.concatenate([PROMPT, PROMPT[:3]])]
SETUP = [None, ("set_logit_rules", RULES), ("set_allowed", dict(ids=MASK))]


def _cfg():
    import llmi
    from llmi.engine import preset
    cfg = preset("tiny")
    cfg.kv_dtype = llmi.F32
    return cfg


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_LONE = {}


def _lone(slot, prefill=False):
    """The lone Engine of slot's prompt and rules -> (tokens [N_NEW], processed row of the last step or None)."""
    if (slot, prefill) not in _LONE:
        from llmi.engine import Engine
        with Engine(_cfg()) as e:
            e.load_synthetic(int(_fixture()["seed"]))
            if SETUP[slot]:
                getattr(e, SETUP[slot][0])(**SETUP[slot][1])
            toks = [int(t) for t in e.generate(PROMPTS[slot], N_NEW, use_graph=False, prefill=prefill)]
            _LONE[(slot, prefill)] = (toks, e.processed_logits() if SETUP[slot] else None)
    return _LONE[(slot, prefill)]


def _batch():
    from llmi.engine import Batch
    b = Batch(_cfg(), 3)
    b.load_synthetic(int(_fixture()["seed"]))
    for s in range(3):
        if SETUP[s]:
            getattr(b, SETUP[s][0])(s, **SETUP[s][1])
    return b


def _run(b, use_graph, prefill=False, ruled=(1, 2)):
    """Every slot to N_NEW tokens, stepping all active slots together; a finished slot's processed
    row (slots `ruled`: those with rules on) is read before it goes idle."""
    for s in range(3):
        b.set_prompt(s, PROMPTS[s])
        if prefill:
            b.prefill(s)
    left = {s: (0 if prefill else len(PROMPTS[s])) + N_NEW - 1 for s in range(3)}
    toks, rows = {}, {}
    while left:
        n = min(left.values())
        b.decode(n, use_graph)
        for s in list(left):
            left[s] -= n
            if left[s] == 0:
                toks[s] = [int(t) for t in b.tokens(s, len(PROMPTS[s]) + N_NEW)[len(PROMPTS[s]):]]
                rows[s] = b.processed_logits(s) if s in ruled else None
                b.reset(s)
                del left[s]
    return toks, rows


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("prefill", [False, True], ids=["decode", "prefill"])
def test_each_slot_is_the_lone_engine_with_its_rules(use_graph, prefill):
    with _batch() as b:
        toks, rows = _run(b, use_graph, prefill)
        again, _ = _run(b, use_graph, prefill)  # the slots' rules outlive a reset and a new prompt
    for s in range(3):
        want, want_row = _lone(s, prefill)
        assert toks[s] == want and again[s] == want, s
        if SETUP[s]:
            assert np.array_equal(_bits(rows[s]), _bits(want_row)), s
    assert _lone(0)[0] == GOLDEN[:N_NEW]
    assert _lone(1)[0][:2] == [A, A] and set(_lone(2)[0]) <= set(MASK)


def test_a_slots_rules_are_its_own():
    from llmi._lib import LlmiError
    with _batch() as b:
        with pytest.raises(LlmiError, match="logit rules are off"):
            b.processed_logits(0)
        with pytest.raises(LlmiError, match="seq out of range"):
            b.set_allowed(3, [1])
        with pytest.raises(LlmiError, match="token ids"):
            b.set_allowed(2, [V])
        b.clear_logit_rules(1)
        b.set_allowed(2, None)
        toks, _ = _run(b, True, ruled=())
        assert toks[0] == GOLDEN[:N_NEW]
        # slot 1 and 2 run their prompts greedily now: the lone greedy engine's tokens
        from llmi.engine import Engine
        with Engine(_cfg()) as e:
            e.load_synthetic(int(_fixture()["seed"]))
            for s in (1, 2):
                assert toks[s] == [int(t) for t in e.generate(PROMPTS[s], N_NEW)]


def test_changing_one_slots_allowed_set_between_replayed_steps():
    """All three slots share one prompt, so a slot differs from slot 0 only through its own mask."""
    from llmi.engine import Batch
    n = len(PROMPT)
    with Batch(_cfg(), 3) as b:
        b.load_synthetic(int(_fixture()["seed"]))
        b.set_allowed(1, [GOLDEN[0]])  # the greedy token itself: slot 1 stays on the greedy path
        for s in range(3):
            b.set_prompt(s, PROMPT)
        b.decode(n, True)
        sets = [[GOLDEN[1]], [555], [GOLDEN[3], 556], [557]]  # slot 1's set before each further step
        for ids in sets:
            b.set_allowed(1, ids)  # contents only: the captured step is replayed
            b.decode(1, True)
        got = [[int(t) for t in b.tokens(s, n + 1 + len(sets))[n:]] for s in range(3)]
    assert got[0] == GOLDEN[:5] and got[2] == GOLDEN[:5]
    assert got[1][:2] == GOLDEN[:2] and got[1][2] == 555 and got[1][3] in (GOLDEN[3], 556) and got[1][4] == 557
