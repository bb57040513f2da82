"""The captured-step caches of Batch and of the verify step (GraphCache in engine.h): a bounded
cache that fills up is dropped whole and rebuilt, and a slot's setter drops the batch's captured
steps. Nothing of that may show in what is computed: every comparison here is BITWISE
(np.array_equal on ids and on the logits' raw bits), graph replay against eager launches of the
same calls, or a batch against a fresh batch configured that way from the start.

The `tiny` preset widths (hidden 512, 4 heads, 2 layers) with a max_seq long enough to pass 64
distinct step keys."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
CACHE_BOUND = 64  # Batch::kMaxGraphs and Engine::kMaxSpecGraphs
CHUNK = 64        # positions one captured step is valid for (kAttnChunk)


def _cfg(**over):
    from llmi.engine import preset
    return preset("tiny", **over)


def _prompt(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(1000 + i, n, 32000)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. Batch cache overflow
B_LEAD = 32                 # slot 1 starts this many steps after slot 0
B_STEPS = 66 * 32           # steps of the two slots together, in one decode call
B_MORE = 40                 # ... and a second call after the overflow
B_MAX_SEQ = 2240


def _batch_keys():
    """The distinct step keys (active slots and their split counts) of the run below."""
    keys = {((0, p // CHUNK + 1),) for p in range(B_LEAD)}
    for i in range(B_STEPS + B_MORE):
        keys.add(((0, (B_LEAD + i) // CHUNK + 1), (1, i // CHUNK + 1)))
    return keys


def _batch_run(use_graph):
    from llmi.engine import Batch
    with Batch(_cfg(max_seq=B_MAX_SEQ), 2) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, _prompt(0, 5))
        b.decode(B_LEAD, use_graph)
        b.set_prompt(1, _prompt(1, 3))
        b.decode(B_STEPS, use_graph)  # one run through more keys than the cache holds
        mid = [(b.tokens(i).copy(), _bits(b.logits(i)).copy()) for i in range(2)]
        b.decode(B_MORE, use_graph)   # continued after the overflow
        end = [(b.tokens(i).copy(), _bits(b.logits(i)).copy()) for i in range(2)]
    return mid, end


def test_batch_cache_overflow_is_invisible():
    assert len(_batch_keys()) > CACHE_BOUND + 1
    eager_mid, eager_end = _batch_run(False)
    graph_mid, graph_end = _batch_run(True)
    assert len(eager_mid[0][0]) == B_LEAD + B_STEPS + 1 and len(eager_mid[1][0]) == B_STEPS + 1
    assert len(eager_end[0][0]) == B_LEAD + B_STEPS + B_MORE + 1
    for what, got, want in (("first run", graph_mid, eager_mid), ("continued run", graph_end, eager_end)):
        for i in range(2):
            assert np.array_equal(got[i][0], want[i][0]), f"{what}: slot {i}'s tokens differ from the eager run's"
            assert np.array_equal(got[i][1], want[i][1]), f"{what}: slot {i}'s logits differ from the eager run's"
    assert not np.array_equal(eager_end[0][0][5:40], eager_end[1][0][3:38])  # two sequences, not one twice


# ----------------------------------------------------------------- 2. verify cache overflow
V_MAX_SEQ = 704
V_BLOCKS = V_MAX_SEQ // CHUNK  # 11 split counts x draft lengths 1..7 = 77 keys
V_PROMPT = 5


def _verify_truth():
    from llmi.engine import Engine
    prompt = _prompt(2, V_PROMPT)
    with Engine(_cfg(max_seq=V_MAX_SEQ)) as e:
        e.load_synthetic(SEED)
        e.generate(prompt, V_MAX_SEQ - V_PROMPT)
        return prompt, e.tokens(V_MAX_SEQ).copy()


def _verify_run(prompt, true, use_graph):
    """Every block of 64 positions: verify steps with drafts of 1..7 ids (the true continuation;
    odd lengths with a wrong last id), then plain decode steps to the next block's start."""
    from llmi.engine import Engine
    keys, accepted, want = set(), [], []
    with Engine(_cfg(max_seq=V_MAX_SEQ)) as e:
        e.load_synthetic(SEED)
        e.set_speculation(7)
        e.set_prompt(prompt)
        e.decode(V_PROMPT, use_graph)
        p = V_PROMPT
        for blk in range(V_BLOCKS):
            for k in range(1, 8):
                draft = true[p + 1:p + 1 + k].copy()
                if k % 2:
                    draft[k - 1] = (draft[k - 1] + 1) % 32000
                assert (p + k) // CHUNK == blk
                keys.add((k + 1, (p + k) // CHUNK + 1))
                accepted.append(e.verify(draft, use_graph))
                want.append(k - k % 2)
                p += accepted[-1] + 1
            if blk + 1 < V_BLOCKS:
                e.decode(CHUNK * (blk + 1) - p, use_graph)
                p = CHUNK * (blk + 1)
        e.decode(4, use_graph)
        p += 4
        return keys, accepted, want, e.tokens(p + 1).copy(), _bits(e.logits()).copy()


def test_verify_cache_overflow_is_invisible():
    prompt, true = _verify_truth()
    keys, acc_e, want, toks_e, logits_e = _verify_run(prompt, true, False)
    _, acc_g, _, toks_g, logits_g = _verify_run(prompt, true, True)
    assert len(keys) > CACHE_BOUND + 7  # the cache overflows, and whole blocks follow the overflow
    assert acc_e == want, "eager verify steps: accepted counts"
    assert acc_g == acc_e, "graph verify steps accept other counts than eager ones"
    assert np.array_equal(toks_e, true[:len(toks_e)]), "eager verify steps leave plain decode's tokens"
    assert np.array_equal(toks_g, toks_e)
    assert np.array_equal(logits_g, logits_e), "final logits differ between graph and eager verify steps"


# ------------------------------------------------- 3. a slot's setters and the batch's steps
S_MAX_SEQ = 128
S_LEAD = 3   # steps before the first setter call: the two-slot step is captured and replayed
S_N = 6      # steps after every setter call (slot 0 restarts its prompt, slot 1 runs on)
S_BIAS = {1234: 64.0}
S_RULES = dict(bias=S_BIAS, presence_penalty=0.5, frequency_penalty=2.0)
S_MASK1 = [11, 222, 3333, 4444]
S_MASK2 = [7, 88, 999, 10101, 20202]
S_SAMPLING = dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, seed=4242)

# (what is called on slot 0, the slot's whole configuration after the call)
S_STAGES = [
    ("set_logit_rules", lambda b: b.set_logit_rules(0, **S_RULES), dict(rules=S_RULES)),
    ("set_allowed: first mask", lambda b: b.set_allowed(0, S_MASK1), dict(rules=S_RULES, allowed=S_MASK1)),
    ("set_allowed: replaced mask", lambda b: b.set_allowed(0, S_MASK2), dict(rules=S_RULES, allowed=S_MASK2)),
    ("set_allowed: removed mask, rules stay", lambda b: b.set_allowed(0, None), dict(rules=S_RULES)),
    ("clear_logit_rules", lambda b: b.clear_logit_rules(0), dict()),
    ("set_allowed: first mask turns the rules on", lambda b: b.set_allowed(0, S_MASK1), dict(allowed=S_MASK1)),
    ("set_allowed: replaced mask alone", lambda b: b.set_allowed(0, S_MASK2), dict(allowed=S_MASK2)),
    ("set_allowed: removed mask turns the rules off", lambda b: b.set_allowed(0, None), dict()),
    ("set_logprobs", lambda b: b.set_logprobs(0, 2), dict(logprobs=2)),
    ("set_sampling_params", lambda b: b.set_sampling_params(0, **S_SAMPLING), dict(logprobs=2, sampling=S_SAMPLING)),
]


def _slot0_outputs(b, conf):
    out = dict(tokens=b.tokens(0).copy(), logits=_bits(b.logits(0)).copy())
    if "rules" in conf or "allowed" in conf:
        out["processed"] = _bits(b.processed_logits(0)).copy()
    if "logprobs" in conf:
        lp, ids, tlp = b.logprobs(0)
        out.update(tok_lp=_bits(lp).copy(), top_ids=ids.copy(), top_lp=_bits(tlp).copy())
    return out


def _fresh_slot0(conf, p0, p1):
    """Slot 0's outputs in a new batch that has this configuration from the start."""
    from llmi.engine import Batch
    with Batch(_cfg(max_seq=S_MAX_SEQ), 2) as b:
        b.load_synthetic(SEED)
        if "rules" in conf:
            b.set_logit_rules(0, **conf["rules"])
        if "allowed" in conf:
            b.set_allowed(0, conf["allowed"])
        if "logprobs" in conf:
            b.set_logprobs(0, conf["logprobs"])
        if "sampling" in conf:
            b.set_sampling_params(0, **conf["sampling"])
        b.set_prompt(0, p0)
        b.set_prompt(1, p1)
        b.decode(S_N)
        return _slot0_outputs(b, conf)


def test_slot_setters_invalidate_the_batch():
    from llmi.engine import Batch
    p0, p1 = _prompt(3, 2), _prompt(4, 4)
    total = S_LEAD + S_N * len(S_STAGES)
    assert total < CHUNK  # slot 1 stays in one split count: every stage meets the same step key
    got = {}
    with Batch(_cfg(max_seq=S_MAX_SEQ), 2) as b:
        b.load_synthetic(SEED)
        b.set_prompt(0, p0)
        b.set_prompt(1, p1)
        b.decode(S_LEAD)  # captured, and replayed twice
        for name, call, conf in S_STAGES:
            call(b)
            b.set_prompt(0, p0)
            b.decode(S_N)
            got[name] = _slot0_outputs(b, conf)
        other = (b.tokens(1).copy(), _bits(b.logits(1)).copy())
    for name, _, conf in S_STAGES:
        want = _fresh_slot0(conf, p0, p1)
        assert sorted(got[name]) == sorted(want)
        for k in want:
            assert np.array_equal(got[name][k], want[k]), f"after {name}: slot 0's {k} differ from a fresh batch's"
    # the captured step follows a replaced mask: what was generated lies in the new set
    n0 = len(p0)
    for name in ("set_allowed: replaced mask", "set_allowed: replaced mask alone"):
        assert set(got[name]["tokens"][n0:].tolist()) <= set(S_MASK2), name
    for name in ("set_allowed: first mask", "set_allowed: first mask turns the rules on"):
        assert set(got[name]["tokens"][n0:].tolist()) <= set(S_MASK1), name
    assert not np.array_equal(got["set_logit_rules"]["tokens"], got["clear_logit_rules"]["tokens"])
    # the other slot ran on through all of it as if alone
    with Batch(_cfg(max_seq=S_MAX_SEQ), 2) as b:
        b.load_synthetic(SEED)
        b.set_prompt(1, p1)
        b.decode(total)
        assert np.array_equal(b.tokens(1), other[0]), "slot 1's tokens changed with slot 0's setters"
        assert np.array_equal(_bits(b.logits(1)), other[1]), "slot 1's logits changed with slot 0's setters"
