"""Batch option "prefix_attn" (csrc/attn_prefix.hip behind Batch::record_step): the `tiny` preset at
max_seq 192 with 4 and 2 kv heads, fp16 and int8 cache. Slot 0 prefills a 130-id prompt and is forked
into slots 1, 2 and -- by a second fork, which joins the group -- 3; every slot's tokens and final logits
against the numpy oracle's greedy continuation of that slot's own sequence, under the bars of
tests/test_gpu_engine_gqa.py. Then the group's upkeep (edit, set_prompt), a fork after capture, the
fp32-cache fallback and the option's errors. The oracle runs the prompt once per case and branches."""
import numpy as np
import pytest

import kv8_ref

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

SEED, MAX_SEQ, PLEN, STEPS, LOGIT_TOL = 20240607, 192, 130, 40, 1e-3
CASES = pytest.mark.parametrize("kvh,kv", [(4, "F16"), (4, "I8"), (2, "F16"), (2, "I8")])
A, B, E = [11], [22], [33, 44]  # forced ids of the two forks and of the edit


def _ids(i, n):
    from llmi.engine import synth_prompt
    return synth_prompt(5000 + i, n, 32000)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _batch(kvh, kv, n=4):
    import llmi
    from llmi.engine import Batch, preset
    b = Batch(preset("tiny", kv_heads=kvh, max_seq=MAX_SEQ, kv_dtype=getattr(llmi, kv)), n)
    b.load_synthetic(SEED)
    return b


class Oracles:
    """The fp-cache oracle and, for an int8 cache, the quantising one beside it, stepped together:
    want(keep, ids, n) = (tokens, logits, bar) of prompt[:keep] + ids continued greedily for n tokens."""

    def __init__(self, kvh, kv, prompt):
        cfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=kvh, inter=1024, layers=2, max_seq=MAX_SEQ)
        w = R.make_model_weights(cfg, SEED, False)
        self.o = [R.LlamaOracle(cfg, kv_dtype=np.float32 if kv == "I8" else np.float16, weights=w)]
        if kv == "I8":
            self.o.append(kv8_ref.Kv8Oracle(cfg, weights=w))
        for o in self.o:
            o.prefill(prompt)  # (the slot's prompt is one prefill pass too)

    def want(self, keep, ids, n):
        res = []
        for o in self.o:  # rows below keep are the prompt's in every branch; the rest is rewritten
            o.pos = keep
            res.append(o.greedy(np.asarray(ids), n))
        if len(res) == 1:
            return res[0] + (LOGIT_TOL,)
        # (an engine that kept its rows unquantised would sit at d8 from the quantising oracle)
        return res[1] + (min(LOGIT_TOL, _rel(res[1][1], res[0][1]) / 4),)


def _check(b, seq, n_prompt, want, what):
    toks, logits, bar = want
    got = b.tokens(seq, n_prompt + len(toks))[n_prompt:]
    r = _rel(b.logits(seq), logits)
    print(f"{what}: slot {seq} logits rel-L2 to the oracle {r:.3e} (bar {bar:.3e})")
    np.testing.assert_array_equal(got, toks, err_msg=what)
    assert r < bar, what


def _forked(b, prompt, use_graph):
    """The main scenario up to its decode: (slot, its sequence's prompt length, keep, forced ids)."""
    b.set_prompt(0, prompt)
    b.prefill(0)
    b.fork(0, [1, 2], keep=PLEN, ids=A)
    b.fork(0, [3], keep=PLEN, ids=B)  # slot 0 is in a group that shares 130 rows: slot 3 joins it
    b.set_option("prefix_attn", 1)
    b.decode(STEPS, use_graph)


@CASES
def test_forked_slots_follow_the_oracle_eager_and_captured(kvh, kv):
    prompt, other = _ids(0, PLEN), _ids(1, 9)
    orc = Oracles(kvh, kv, prompt)
    # slot 0 goes on from its pending token: the oracle's greedy of the prompt's last id at row 129.
    # (A branch rewrites the oracle's rows from its keep on: the ones that keep fewer rows come last.)
    wa = orc.want(PLEN, A, STEPS)
    wants = [orc.want(PLEN - 1, prompt[-1:], STEPS + 1), wa, wa, orc.want(PLEN, B, STEPS)]
    edited, fresh = orc.want(70, E, 11), orc.want(0, other, 4)
    with _batch(kvh, kv) as b:
        _forked(b, prompt, False)
        for s, w in enumerate(wants):
            _check(b, s, PLEN if s == 0 else PLEN + 1, w, f"kv_heads {kvh} {kv} eager")
        eager = [(b.tokens(s).copy(), _bits(b.logits(s)).copy()) for s in range(4)]
        # upkeep: slot 2 rewinds to 70 (its shared rows fall to 70, the group's P to 64); slot 1
        # leaves the group with a prompt of its own
        b.edit(2, 70, E)
        b.set_prompt(1, other)
        b.decode(12, False)
        _check(b, 2, 72, edited, "after edit")
        _check(b, 1, 9, fresh, "after set_prompt")
    with _batch(kvh, kv) as b:
        _forked(b, prompt, True)
        for s, (t, l) in enumerate(eager):
            np.testing.assert_array_equal(b.tokens(s), t)
            np.testing.assert_array_equal(_bits(b.logits(s)), l)


@pytest.mark.parametrize("kv", ["F16", "I8"])
def test_fork_after_capture_gets_a_plan_of_its_own(kv):
    """Captured steps survive a fork, so the plan must be part of their key. Steps are captured with
    slot 1 in slot 0's group; slot 1 is then forked anew from slot 2, an unrelated prompt of the same
    length -- same slots, same split counts, and a replay of the old steps would read slot 0's rows."""
    prompt, other = _ids(0, PLEN), _ids(2, PLEN)
    want = Oracles(2, kv, other).want(PLEN, B, 10)
    with _batch(2, kv, 3) as b:
        b.set_option("prefix_attn", 1)
        for s, p in ((0, prompt), (2, other)):
            b.set_prompt(s, p)
            b.prefill(s)
        b.fork(0, [1], keep=PLEN, ids=A)
        b.decode(2, True)
        b.fork(2, [1], keep=PLEN, ids=B)
        b.decode(10, True)
        _check(b, 1, PLEN + 1, want, f"{kv} forked after capture")


def test_fp32_cache_runs_as_without_the_option():
    out = []
    for on in (1, 0):
        with _batch(4, "F32", 3) as b:
            b.set_option("prefix_attn", on)
            b.set_prompt(0, _ids(0, 70))
            b.prefill(0)
            b.fork(0, [1, 2], keep=70, ids=A)
            b.decode(8, False)
            out.append([(b.tokens(s).copy(), _bits(b.logits(s)).copy()) for s in range(3)])
    for (t1, l1), (t0, l0) in zip(*out):
        np.testing.assert_array_equal(t1, t0)
        np.testing.assert_array_equal(l1, l0)


def test_bad_value_and_unknown_name_raise():
    from llmi import _lib
    with _batch(4, "F16", 2) as b:
        with pytest.raises(_lib.LlmiError, match="prefix_attn"):
            b.set_option("prefix_attn", 2)
        with pytest.raises(_lib.LlmiError, match="unknown option"):
            b.set_option("prefix_atn", 1)
        b.set_option("prefix_attn", 1)
        assert all(len(t) == 3 for t in b.generate([_ids(0, 4), _ids(1, 7)], 3))
