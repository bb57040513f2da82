"""csrc/attn_prefix.hip through llmi_debug_attn_oproj_batch with prefix_group set: the slots of a fork
group read their shared leading rows once, from the lowest-numbered member. Buffers as in
tests/test_gpu_attn_batch.py (max_seq 192: three splits, W_o [256, heads * 128] fp16, 0xFF workspaces,
an xacc pattern, NaN rows / NaN scales at and behind a position). The members of a group get bitwise
equal rows [0, prefix_rows), and in every member but the leader the rows of the served prefix are
then NaN (int8: NaN scales) on the device: a finite, correct result proves they were read from the
leader only. Per slot: xacc against float64 over the member's logical cache (rel-L2 < 4e-6, the bar
of tests/test_gpu_attn_batch.py and tests/test_gpu_attn_gqa.py); tail partials, the written cache row,
scales and the error word bitwise those of the same call with every prefix_group 0 on un-poisoned
caches; no other cache byte changes."""
import numpy as np
import pytest

import kv8_ref
from test_gpu_attn_batch import BAR, FX, collect, prepare, reference, slot, weights

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# per slot (position, group, prefix_rows, P / 64 the launch must serve: 0 = the slot runs ungrouped)
LAYOUTS = {
    "p128-one-tail": [(130, 1, 128, 2), (191, 1, 128, 2)],
    "p64-current-row-alone": [(64, 1, 64, 1), (64, 1, 64, 1)],
    "rounds-down-to-64": [(100, 1, 100, 1), (129, 1, 127, 1)],
    "rows-below-64-unserved": [(70, 1, 63, 0), (80, 1, 63, 0)],
    "two-groups-two-loners": list(zip((130, 150, 191, 64, 65, 0, 129, 140), (1, 1, 1, 2, 2, 0, 0, 1),
                                      (128, 128, 128, 64, 64, 0, 0, 64), (1, 1, 1, 1, 1, 0, 0, 1))),
    "eight-members": [(130 + 7 * i, 1, 128, 2) for i in range(8)],  # at (4, 1): 32 query rows, four passes
}
CASES = [(c, hk, name) for c in ("f16", "i8") for hk in ((4, 4), (4, 2), (4, 1)) for name in list(LAYOUTS)[:5]] + \
    [(c, (4, 1), "eight-members") for c in ("f16", "i8")]


@pytest.mark.parametrize("cache,hk,name", CASES)
def test_members_against_float64_and_the_ungrouped_call(cache, hk, name):
    from llmi import ops
    heads, kvh = hk
    layout = LAYOUTS[name]
    rng = np.random.default_rng(CASES.index((cache, hk, name)))
    w_kw, w64 = weights(rng, heads, "f16")
    slots = [slot(rng, heads, kvh, cache, lay[0]) for lay in layout]
    first = {}  # group -> (its first member, that member's rows): two members share the smaller count
    for s, (_, g, rows, _) in zip(slots, layout):
        if g and g in first:
            n = min(rows, first[g][1])
            for mine, theirs in zip(s["cache"], first[g][0]["cache"]):
                mine[:, :n] = theirs[:, :n]
        first.setdefault(g, (s, rows))
    kws0, outs0 = prepare(slots, heads, kvh, cache, w_kw)
    ops.debug_attn_oproj_batch(kws0)
    plain = collect(outs0, heads)

    kws, outs = prepare(slots, heads, kvh, cache, w_kw)
    poisoned = (1, 3) if cache == "i8" else (0, 2)  # the scales / the rows themselves
    leaders = {}
    for i, (kw, (_, g, rows, skip), out) in enumerate(zip(kws, layout, outs)):
        kw.update(prefix_group=g, prefix_rows=rows)
        if skip and leaders.setdefault(g, i) != i:  # what the kernel must not read
            for j in poisoned:
                out[3][j][:, :64 * skip] = kv8_ref.NAN_BITS
    ops.debug_attn_oproj_batch(kws)
    worst = 0.0
    for i, (s, got, want) in enumerate(zip(slots, collect(outs, heads), plain)):
        (xacc, err, ml, o, after), (xacc0, err0, ml0, o0, after0) = got, want
        pos, nact, skip = s["pos"], s["pos"] // 64 + 1, layout[i][3]
        tag = f"{name} slot {i} pos={pos} skip={skip} heads={heads}/{kvh} cache={cache}"
        assert err == 0 and err0 == 0, tag
        assert np.array_equal(ml[:, skip:nact], ml0[:, skip:nact]) and np.array_equal(o[:, skip:nact], o0[:, skip:nact]), \
            (tag, "tail partials differ from the ungrouped call")
        if skip == 0:
            assert np.array_equal(xacc, xacc0), (tag, "a slot outside a served group is not bitwise the ungrouped call")
        for j, (nm, b, a, a0) in enumerate(zip(("k", "k scale", "v", "v scale"), s["cache"], after, after0)):
            exp = b.copy()
            if skip and leaders[layout[i][1]] != i and j in poisoned:
                exp[:, :64 * skip] = kv8_ref.NAN_BITS
            exp[:, pos] = a0[:, pos]
            assert np.array_equal(a, exp), (tag, nm, "the written row differs, or another byte changed")
        if cache == "i8":
            kc = kv8_ref.dequant(after0[0].view(np.int8), after0[1].view(np.uint16))
            vc = kv8_ref.dequant(after0[2].view(np.int8), after0[3].view(np.uint16))
        else:
            kc, vc = after0[0].view(np.float16), after0[2].view(np.float16)
        ref = reference(s["qkv"][:heads * 128].reshape(heads, 128), kc, vc, pos, w64)
        r = float(np.linalg.norm((xacc - s["seed"]).astype(np.float64) / FX - ref) / np.linalg.norm(ref))
        worst = max(worst, r)
        assert r < BAR, (tag, r)  # (NaN fails too: a poisoned row that was read)
    print(f"[rel-L2] prefix attn+o_proj: {name} heads={heads}/{kvh} cache={cache}: worst {worst:.3e}")
