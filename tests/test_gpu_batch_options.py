"""The four options of Batch::record_step -- rows_mfma, gqa_attn, batch_attn, prefix_attn -- switched on
together (csrc/engine_batch.hip): the `tiny` preset at max_seq 192, seed 20240607. Every case id spells
the options as m<rows_mfma>g<gqa_attn>b<batch_attn>p<prefix_attn>.

1. The bitwise relations the code promises, under every setting of the other options: tokens, final
   logits and the cache rows {0, 63, 64, last} of layers 0 and 1, eager and captured. One GPU run per
   (shape, options, scenario, eager / captured), kept for every relation that needs it.
2. The combinations that are bitwise nothing (prefix_attn with gqa_attn and rows_mfma, batch_attn set
   beside it): six slots in one launch -- a served group (0, 2, 4), an unserved one that shares 17 rows
   (1, 3) and a slot of no group (5), so the grouped-query compaction takes slots 1, 3 and 5 out of the
   middle -- against the numpy oracle's continuation of each slot's own sequence. rows_mfma 0: tokens
   and logits under the bars of tests/test_gpu_batch_prefix.py. rows_mfma 1: teacher-forced (24 forced
   ids a slot, which is above engine_fork.hip's kForkByValue = 8: the ids travel by the copy path),
   final logits within LOGIT_TOL = 1e-3 of the matching oracle. The baseline -- rows_mfma 1 with every
   attention option off, same scenario, same oracle -- is a case of its own; its worst slot measured
   9.583e-06 on an MI355X (kv_heads 2, int8 cache; the combinations' worst slot is the same 9.583e-06):
   it meets 1e-3, so the bar of the combinations is 1e-3.
3. The fork groups' upkeep when the leader (the lowest-numbered member, whose rows all members read)
   goes idle, is re-prompted, rewound, becomes a fork's destination, forks to fewer rows; a reload; and
   eight slots in kAttnPrefixGroups = 4 groups. Against the oracle under the bars of 2 (rows_mfma 0).

The oracle is built once per (kv heads, cache type, seed) and every continuation it computes is kept."""
import functools
import hashlib

import numpy as np
import pytest

import kv8_ref
from test_gpu_batch_prefix import LOGIT_TOL, MAX_SEQ, PLEN, SEED, _bits, _ids, _rel

pytestmark = pytest.mark.gpu

from oracle import llama_ref as R  # noqa: E402

STEPS, FORCED, SEED2 = 40, 24, 20240608
F1, F2, F3, E = [11], [22], [33], [33, 44]  # forced ids of the forks and of the edit
NAMES = ("rows_mfma", "gqa_attn", "batch_attn", "prefix_attn")
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
KV = pytest.mark.parametrize("kv", ["F16", "I8"])
KVH = pytest.mark.parametrize("kvh", [4, 2, 1], ids=lambda k: f"kvh{k}")
KVH_GQA = pytest.mark.parametrize("kvh", [2, 1], ids=lambda k: f"kvh{k}")
G = pytest.mark.parametrize("g", [0, 1], ids=["g0", "g1"])
M = pytest.mark.parametrize("m", [0, 1], ids=["m0", "m1"])


def _tag(o):
    return "m%dg%db%dp%d" % tuple(o)


def _cat(*a):
    return np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in a])


def _batch(kvh, kv, n, opts=(0, 0, 0, 0), wdt="F16", seed=SEED):
    import llmi
    from llmi.engine import Batch, preset
    b = Batch(preset("tiny", kv_heads=kvh, max_seq=MAX_SEQ, kv_dtype=getattr(llmi, kv),
                     weight_dtype=getattr(llmi, wdt)), n)
    b.load_synthetic(seed)
    for name, v in zip(NAMES, opts):
        b.set_option(name, v)
    return b


# ------------------------------------------------------------------------------------------ the oracle
class Ref:
    """The fp-cache oracle and, for an int8 cache, the quantising one beside it. A prompt that a slot
    prefills is prefilled here once and its cache rows kept; want() puts them back and branches."""

    def __init__(self, kvh, kv, seed):
        cfg = R.LlamaConfig(hidden=512, heads=4, kv_heads=kvh, inter=1024, layers=2, max_seq=MAX_SEQ)
        w = R.make_model_weights(cfg, seed, False)
        self.o = [R.LlamaOracle(cfg, kv_dtype=np.float32 if kv == "I8" else np.float16, weights=w)]
        if kv == "I8":
            self.o.append(kv8_ref.Kv8Oracle(cfg, weights=w))
        self.kvh, self.kv, self.rows, self.memo = kvh, kv, {}, {}

    def _restore(self, pre):
        key = pre.tobytes()
        if key not in self.rows:
            snap = []
            for o in self.o:
                o.pos = 0
                o.prefill(pre)
                snap.append((o.k_cache[:, :, :len(pre)].copy(), o.v_cache[:, :, :len(pre)].copy()))
            self.rows[key] = snap
        for o, (k, v) in zip(self.o, self.rows[key]):
            o.k_cache[:, :, :len(pre)] = k
            o.v_cache[:, :, :len(pre)] = v

    def want(self, pre, keep, ids, n):
        """(tokens, logits, bar) of pre[:keep] + ids continued greedily for n tokens; pre: the rows a
        slot took by prefill (or by a fork of them), ids: what it consumed as decode steps."""
        pre, ids = _cat(pre), _cat(ids)
        key = (pre.tobytes(), keep, ids.tobytes(), n)
        if key in self.memo:
            return self.memo[key]
        if keep:
            self._restore(pre)
        res = []
        for o in self.o:
            o.pos = keep
            for t in ids[:-1]:  # (a forced id's logits are not needed: forward_token without the head)
                x = o.embed[int(t)].astype(np.float32)
                for l in range(o.cfg.layers):
                    x = o.layer_forward(l, x, o.pos)
                o.pos += 1
            res.append(o.greedy(ids[-1:], n))
        if len(res) == 1:
            out = res[0] + (LOGIT_TOL,)
        else:  # (an engine that kept its rows unquantised would sit at d8 from the quantising oracle)
            out = res[1] + (min(LOGIT_TOL, _rel(res[1][1], res[0][1]) / 4),)
        self.memo[key] = out
        return out


@functools.lru_cache(maxsize=None)
def _ref(kvh, kv, seed=SEED):
    return Ref(kvh, kv, seed)


def _check(b, seq, n_prompt, want, what, tokens=True, bar=None):
    toks, logits, wbar = want
    bar = wbar if bar is None else bar
    r = _rel(b.logits(seq), logits)
    print(f"{what}: slot {seq} logits rel-L2 to the oracle {r:.3e} (bar {bar:.3e})")
    if tokens:
        np.testing.assert_array_equal(b.tokens(seq, n_prompt + len(toks))[n_prompt:], toks, err_msg=f"{what} slot {seq}")
    assert r < bar, f"{what} slot {seq}"
    return r


# --------------------------------------------------------------------- 1. what a run leaves, bit for bit
def _digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).digest(), np.uint8)


def _collect(x, kv, last, slot=None):
    """x: a Batch (slot given) or an Engine. Tokens, the logits' bits (as a digest: hundreds of runs are
    kept) and the cache rows {0, 63, 64, last} of both layers as stored."""
    sel = () if slot is None else (slot,)
    out = {"tokens": x.tokens(*sel), "logits": _digest(_bits(x.logits(*sel)))}
    for layer in (0, 1):
        for pos in sorted({p for p in (0, 63, 64, last) if p <= last}):
            for v in (False, True):
                name = f"L{layer}.{'v' if v else 'k'}[{pos}]"
                if kv == "I8":
                    out[name + ".q"], out[name + ".s"] = x.kv_slot_q8(*sel, layer, pos, v)
                else:
                    out[name] = _bits(x.kv_slot(*sel, layer, pos, v))
    return out


def _collect_all(b, kv, last):
    return {f"slot{s}.{k}": v for s, n in enumerate(last) if n is not None for k, v in _collect(b, kv, n, s).items()}


@functools.lru_cache(maxsize=None)
def _prompts():
    """p: the 130-id prompt of every group's leader; q: the 17-id one; the rest by length."""
    return dict(p=_ids(0, PLEN), q=_ids(1, 17), n5=_ids(2, 5), n60=_ids(3, 60), n9=_ids(4, 9),
                t=[_ids(10 + i, FORCED) for i in range(6)], pair=[_ids(20 + i, 70) for i in range(4)],
                fresh=[_ids(30, 70), _ids(31, 70), _ids(32, 9), _ids(33, 5)])


def _fork4(b, use_graph):
    """Slot 0 prefills 130 ids, slots 1 and 2 are forked from it, slot 3 holds 17 ids of its own."""
    pr = _prompts()
    b.set_prompt(0, pr["p"])
    b.prefill(0)
    b.fork(0, [1], keep=PLEN, ids=F1)
    b.fork(0, [2], keep=PLEN, ids=F2)
    b.set_prompt(3, pr["q"])
    b.decode(STEPS, use_graph)
    return [PLEN + STEPS - 1] * 3 + [STEPS - 1]


def _nogroup4(b, use_graph):
    """Four unrelated prompts of 5, 60, 17 and 130 ids; the two long ones by prefill, so that slot 1
    crosses the split boundary at 64 on its way while slot 3 reads three splits."""
    pr = _prompts()
    for s, ids in enumerate((pr["n5"], pr["n60"], pr["q"], pr["p"])):
        b.set_prompt(s, ids)
        if len(ids) >= 60:
            b.prefill(s)
    b.decode(STEPS, use_graph)
    return [STEPS - 1, 60 + STEPS - 1, STEPS - 1, PLEN + STEPS - 1]


def _three(b, use_graph):
    pr = _prompts()
    for s, ids in enumerate((pr["n5"], pr["n60"], pr["q"])):
        b.set_prompt(s, ids)
    b.decode(STEPS, use_graph)
    return [STEPS - 1] * 3


def _one(b, use_graph):
    b.set_prompt(1, _prompts()["q"])
    b.decode(STEPS, use_graph)
    return [None, STEPS - 1, None]


def _six(b, use_graph, forced):
    """Served group (0, 2, 4) on 130 rows, unserved group (1, 3) on 17 rows, slot 5 in no group on 60
    rows of its own (it crosses 64). forced: every slot consumes 24 given ids and nothing it sampled."""
    pr = _prompts()
    t = pr["t"] if forced else [(), (), F1, F2, F3, ()]
    for s, pre in ((0, pr["p"]), (1, pr["q"]), (5, pr["n60"])):
        b.set_prompt(s, _cat(pre, t[s]))
        b.prefill(s, len(pre))
    b.fork(0, [2], keep=PLEN, ids=t[2])
    b.fork(1, [3], keep=17, ids=t[3])
    b.fork(0, [4], keep=PLEN, ids=t[4])
    n = FORCED if forced else STEPS
    b.decode(n, use_graph)
    return [PLEN + n - 1, 17 + n - 1, PLEN + n - 1, 17 + n - 1, PLEN + n - 1, 60 + n - 1]


def _six_wants(ref, forced):
    """The oracle's side of _six, slot by slot: (prompt length of the slot's sequence, want)."""
    pr = _prompts()
    pre = [pr["p"], pr["q"], pr["p"], pr["q"], pr["p"], pr["n60"]]
    if forced:
        return [(len(p) + FORCED, ref.want(p, len(p), t, 1)) for p, t in zip(pre, pr["t"])]
    out = []
    for s, p in enumerate(pre):
        if s in (0, 1, 5):  # goes on from its pending token: the prompt's last id at its last row
            out.append((len(p), ref.want(p, len(p) - 1, p[-1:], STEPS + 1)))
        else:
            out.append((len(p) + 1, ref.want(p, len(p), (F1, F2, F3)[s - 2], STEPS)))
    return out


SCENARIOS = dict(fork=(_fork4, 4), nogroup=(_nogroup4, 4), three=(_three, 3), one=(_one, 3),
                 six=(functools.partial(_six, forced=False), 6), forced=(functools.partial(_six, forced=True), 6))


@functools.lru_cache(maxsize=None)
def _run(kvh, kv, opts, scen, use_graph, wdt="F16"):
    fn, n = SCENARIOS[scen]
    with _batch(kvh, kv, n, opts, wdt) as b:
        return _collect_all(b, kv, fn(b, use_graph))


def _same(x, y, what):
    assert x.keys() == y.keys()
    bad = [k for k in x if not np.array_equal(x[k], y[k])]
    assert not bad, f"{what}: differ in {bad}"


@KVH
@KV
@G
@M
@GRAPH
def test_batch_attn_on_is_bitwise_off(kvh, kv, g, m, use_graph):
    _same(_run(kvh, kv, (m, g, 1, 0), "fork", use_graph), _run(kvh, kv, (m, g, 0, 0), "fork", use_graph),
          f"batch_attn 1 / 0 under {_tag((m, g, 0, 0))}")


@pytest.mark.parametrize("scen", ["fork", "nogroup"])
@KVH
@KV
@G
@M
@GRAPH
def test_prefix_attn_ignores_batch_attn(scen, kvh, kv, g, m, use_graph):
    _same(_run(kvh, kv, (m, g, 1, 1), scen, use_graph), _run(kvh, kv, (m, g, 0, 1), scen, use_graph),
          f"batch_attn 1 / 0 under {_tag((m, g, 0, 1))}, {scen}")


@KVH
@KV
@G
@M
@GRAPH
def test_prefix_attn_without_a_group_is_batch_attn_is_neither(kvh, kv, g, m, use_graph):
    """(gqa_attn 1: the per-slot grouped-query launches with the batched o_proj behind them.)"""
    off = _run(kvh, kv, (m, g, 0, 0), "nogroup", use_graph)
    _same(_run(kvh, kv, (m, g, 0, 1), "nogroup", use_graph), off, f"{_tag((m, g, 0, 1))} / {_tag((m, g, 0, 0))}")
    _same(_run(kvh, kv, (m, g, 1, 0), "nogroup", use_graph), off, f"{_tag((m, g, 1, 0))} / {_tag((m, g, 0, 0))}")


@pytest.mark.parametrize("b,p", [(1, 0), (0, 1)], ids=["b1p0", "b0p1"])
@KV
@M
@GRAPH
def test_gqa_attn_changes_nothing_at_4_kv_heads(b, p, kv, m, use_graph):
    """One query head a kv head: the grouped-query kernel refuses, every slot stays in the launch."""
    _same(_run(4, kv, (m, 1, b, p), "fork", use_graph), _run(4, kv, (m, 0, b, p), "fork", use_graph),
          f"gqa_attn 1 / 0 under {_tag((m, 0, b, p))}")


@pytest.mark.parametrize("scen", ["three", "one"])
@pytest.mark.parametrize("b", [0, 1], ids=["b0", "b1"])
@GRAPH
def test_rows_mfma_falls_back_on_fp32_weights(scen, b, use_graph):
    """The matrix-core GEMV refuses fp32 weights: three slots take the multi-row GEMV, one slot the
    single-row GEMV with the engine's own arguments -- which is an Engine alone, bit for bit."""
    on, off = (_run(4, "F16", (m, 0, b, 0), scen, use_graph, "F32") for m in (1, 0))
    _same(on, off, f"rows_mfma 1 / 0 with fp32 weights under b{b}, {scen}")
    if scen == "one":
        import llmi
        from llmi.engine import Engine, preset
        with Engine(preset("tiny", kv_heads=4, max_seq=MAX_SEQ, kv_dtype=llmi.F16, weight_dtype=llmi.F32)) as e:
            e.load_synthetic(SEED)
            e.set_prompt(_prompts()["q"])
            e.decode(STEPS, use_graph)
            alone = {f"slot1.{k}": v for k, v in _collect(e, "F16", STEPS - 1).items()}
        _same(on, alone, "rows_mfma 1, one slot / an Engine alone")


@KVH_GQA
@KV
@G
@M
def test_six_slots_eager_is_captured(kvh, kv, g, m):
    scen = "forced" if m else "six"
    _same(_run(kvh, kv, (m, g, 1, 1), scen, True), _run(kvh, kv, (m, g, 1, 1), scen, False),
          f"captured / eager under {_tag((m, g, 1, 1))}")


# ------------------------------------------------------------------------ 2. six slots against the oracle
def _six_against_the_oracle(kvh, kv, opts, use_graph):
    forced = bool(opts[0])
    wants = _six_wants(_ref(kvh, kv), forced)  # (before the batch exists: off the GPU path's clock)
    fn, n = SCENARIOS["forced" if forced else "six"]
    what = f"kv_heads {kvh} {kv} {_tag(opts)} {'graph' if use_graph else 'eager'}"
    with _batch(kvh, kv, n, opts) as b:
        fn(b, use_graph)
        # rows_mfma 1: the forced ids' final logits under LOGIT_TOL; sampled tokens are not compared
        return max(_check(b, s, plen, w, what, tokens=not forced, bar=LOGIT_TOL if forced else None)
                   for s, (plen, w) in enumerate(wants))


@KVH_GQA
@KV
@G
@M
@GRAPH
def test_six_slots_follow_the_oracle(kvh, kv, g, m, use_graph):
    _six_against_the_oracle(kvh, kv, (m, g, 1, 1), use_graph)


@KVH_GQA
@KV
def test_rows_mfma_alone_meets_the_bar(kvh, kv):
    """The baseline of the rows_mfma 1 cases above: the same forced scenario and oracle with every
    attention option off. It has to meet LOGIT_TOL for LOGIT_TOL to be the combinations' bar."""
    worst = _six_against_the_oracle(kvh, kv, (1, 0, 0, 0), False)
    print(f"kv_heads {kvh} {kv}: rows_mfma 1 alone, worst slot {worst:.3e}")


# --------------------------------------------------------------------- 3. the groups' upkeep, leader first
def _start(b, n_forks=3):
    """Slots 1 .. n_forks forked off slot 0's 130-id prompt, each with a forced id of its own."""
    b.set_prompt(0, _prompts()["p"])
    b.prefill(0)
    for s, f in zip(range(1, n_forks + 1), (F1, F2, F3)):
        b.fork(0, [s], keep=PLEN, ids=f)


def _member(ref, s, steps):
    return PLEN + 1, ref.want(_prompts()["p"], PLEN, (F1, F2, F3)[s - 1], steps)


def _leader(ref, steps, p=None):
    p = _prompts()["p"] if p is None else p
    return len(p), ref.want(p, len(p) - 1, p[-1:], steps + 1)


def _leader_reset(b, ref, pr):
    """The leader goes idle, slot 1 is the one read; later it comes back with a prompt of its own."""
    b.decode(6, True)
    b.reset(0)
    b.decode(8, False)
    b.decode(4, True)
    b.set_prompt(0, pr["n9"])
    b.decode(12, True)
    return [(9, ref.want((), 0, pr["n9"], 4))] + [_member(ref, s, 30) for s in (1, 2, 3)]


def _leader_reprompted(b, ref, pr):
    b.decode(6, True)
    b.set_prompt(0, pr["n9"])
    b.decode(12, False)
    b.decode(6, True)
    return [(9, ref.want((), 0, pr["n9"], 10))] + [_member(ref, s, 24) for s in (1, 2, 3)]


def _leader_edited(keep, b, ref, pr):
    """keep 70: the group's shared rows fall to 64; keep 40: below a split, the group is unserved."""
    b.decode(6, True)
    b.edit(0, keep, E)
    b.decode(8, False)
    b.decode(4, True)
    return [(keep + 2, ref.want(pr["p"], keep, E, 11))] + [_member(ref, s, 18) for s in (1, 2, 3)]


def _leader_becomes_destination(b, ref, pr):
    """Slot 2 into slot 0 as it stands: those two are a new group on 141 rows and bitwise each other
    from there on; slots 1 and 3 stay a served group of the old id, slot 1 leading."""
    b.decode(10, True)
    b.fork(2, [0])
    b.decode(8, False)
    b.decode(4, True)
    np.testing.assert_array_equal(b.tokens(0), b.tokens(2))
    np.testing.assert_array_equal(_bits(b.logits(0)), _bits(b.logits(2)))
    return [_member(ref, 2, 22)] + [_member(ref, s, 22) for s in (1, 2, 3)]


def _fork_to_fewer_rows(b, ref, pr):
    """Slots 0 to 2 share 130 rows; slot 3 joins on 64 and the whole group reads one split together."""
    b.decode(6, True)
    b.fork(0, [3], keep=64, ids=E)
    b.decode(8, False)
    b.decode(4, True)
    return [_leader(ref, 18), _member(ref, 1, 18), _member(ref, 2, 18), (66, ref.want(pr["p"], 64, E, 11))]


def _reloaded(b, ref, pr):
    """Other weights under a batch that holds a group: no slot may read another's rows afterwards."""
    b.decode(6, True)
    b.load_synthetic(SEED2)
    for s, ids in enumerate(pr["fresh"]):
        b.set_prompt(s, ids)
        if len(ids) >= 64:
            b.prefill(s)
    b.decode(10, True)
    b.decode(6, False)
    new = _ref(ref.kvh, ref.kv, SEED2)
    return [_leader(new, 16, ids) if len(ids) >= 64 else (len(ids), new.want((), 0, ids, 16 - len(ids) + 1))
            for ids in pr["fresh"]]


def _eight_slots(b, ref, pr):
    """Four pairs on 70 rows each, all served; then slot 7 is forked anew on 63 rows of its pair's
    leader: three served pairs and two slots whose group shares less than a split. At last slot 1
    goes idle, which leaves slot 0 alone in its group: with gqa_attn 1 an odd number of slots is then
    taken out in front of the served pairs, so that a group or row count picked at the index before
    the compaction would pair slots 3 and 4, of different prompts."""
    for i, ids in enumerate(pr["pair"]):
        b.set_prompt(2 * i, ids)
        b.prefill(2 * i)
        b.fork(2 * i, [2 * i + 1], keep=70, ids=[100 + i])
    b.decode(6, True)
    b.fork(6, [7], keep=63, ids=E)
    b.decode(8, False)
    _check(b, 1, 71, ref.want(pr["pair"][0], 70, [100], 14), "eight_slots, slot 1 before it goes idle")
    b.reset(1)
    b.decode(4, True)
    out = []
    for i, ids in enumerate(pr["pair"]):
        out += [_leader(ref, 18, ids), (71, ref.want(ids, 70, [100 + i], 18))]
    out[1] = None
    out[7] = (65, ref.want(pr["pair"][3], 63, E, 11))
    return out


UPKEEP = {
    "leader_reset": (_leader_reset, 4, 3), "leader_reprompted": (_leader_reprompted, 4, 3),
    "leader_edit70": (functools.partial(_leader_edited, 70), 4, 3),
    "leader_edit40": (functools.partial(_leader_edited, 40), 4, 3),
    "leader_becomes_destination": (_leader_becomes_destination, 4, 3),
    "fork_to_fewer_rows": (_fork_to_fewer_rows, 4, 2), "reloaded": (_reloaded, 4, 3),
    "eight_slots": (_eight_slots, 8, 0),
}


@pytest.mark.parametrize("case", list(UPKEEP))
@KV
@G
def test_fork_group_upkeep(case, kv, g):
    fn, n, forks = UPKEEP[case]
    ref, pr = _ref(2, kv), _prompts()
    with _batch(2, kv, n, (0, g, 0, 1)) as b:
        if forks:
            _start(b, forks)
        wants = fn(b, ref, pr)
        for s, w in enumerate(wants):
            if w is not None:  # (None: the slot is idle by now and was checked before it left)
                _check(b, s, *w, f"{case} {kv} {_tag((0, g, 0, 1))}")
