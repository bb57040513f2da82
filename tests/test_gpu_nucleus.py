"""llmi_sample_nucleus (csrc/nucleus.hip) against the numpy restatement tests/nucleus_ref.py
over the shared input recipe: the id is equal on every decided case (both slacks >= 1e-6:
two correct fp32 expf differ by ~2 ulp = 2.4e-7 relative per weight and so per sum), the
kept count wherever the cut is decided; plus the argmax identity, non-finite rows, graph
capture and the argument checks."""
import numpy as np
import pytest

import nucleus_ref as N

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _run(z, h, prm, step, **kw):
    torch = _torch()
    from llmi import ops
    r, T, k, p = prm
    zd = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    hd = None if h is None else torch.from_numpy(np.ascontiguousarray(h)).cuda()
    ids, kept = ops.sample_nucleus(zd, step, top_k=k, top_p=p, temperature=T, repetition_penalty=r, history=hd, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(zd.cpu().numpy().view(np.uint32), np.ascontiguousarray(z).view(np.uint32)), "logits were modified"
    return ids.cpu().numpy(), kept.cpu().numpy()


def test_recipe_matches_restatement():
    want = N.recipe_expected()
    got = {}
    for ci, (ii, z, h, prm, step, rows) in enumerate(N.recipe_calls()):
        ids, kept = _run(z, h, prm, step)
        for b in range(rows):
            got[(ci, b)] = (int(ids[b]), int(kept[b]))
    undecided, bad = 0, []
    for ci, b, tok, kept, cs, ds, w in want:
        g_id, g_kept = got[(ci, b)]
        assert 0 <= g_id < len(w) and w[g_id] > 0, (ci, b, g_id)
        if cs >= N.DECIDED and g_kept != kept:
            bad.append(("kept", ci, b, g_kept, kept, cs))
        if cs >= N.DECIDED and ds >= N.DECIDED:
            if g_id != tok:
                bad.append(("id", ci, b, g_id, tok, cs, ds))
        else:
            undecided += 1
    print(f"undecided {undecided} of {len(want)}; mismatches {len(bad)}")
    assert not bad, bad[:10]
    assert undecided <= 0.05 * len(want)


def test_top_k_1_is_argmax_with_ties():
    torch = _torch()
    from llmi import ops
    rng = np.random.default_rng(5)
    for V in (7, 1027, 32000, 40003):
        z = rng.standard_normal((2, V)).astype(np.float32)
        z[1, [V // 3, V // 2, V - 1]] = z[1].max() + 1  # tied maxima: the lowest id wins
        ids, kept = _run(z, None, (1.0, 1.0, 1, 1.0), 9)
        for b in range(2):
            want = int(ops.argmax(torch.from_numpy(z[b]).cuda()).cpu()[0])
            assert ids[b] == want == int(np.argmax(z[b])) and kept[b] == 1


def test_minus_inf_nan_and_plus_inf_rows():
    rng = np.random.default_rng(6)
    V = 1027
    z = rng.standard_normal((3, V)).astype(np.float32)
    z[0, ::2] = -np.inf          # -inf: weight 0, never drawn
    z[1, 5::7] = np.nan          # NaN counts as -inf
    z[2, [11, 500, 1026]] = np.inf  # +inf: the draw is shared by the +inf ids alone
    seen2 = set()
    for step in range(1, 13):
        ids, kept = _run(z, None, (1.0, 0.9, 0, 1.0), step)
        for b in range(3):
            want = N.sample(z[b], [], 1.0, 0.9, 0, 1.0, step, b)
            if want[3] >= N.DECIDED:
                assert ids[b] == want[0], (b, step)
            assert kept[b] == V
        assert ids[0] % 2 == 1 and (ids[1] - 5) % 7 != 0
        seen2.add(int(ids[2]))
    assert seen2 <= {11, 500, 1026} and len(seen2) >= 2
    # a row of nothing but -inf / NaN: uniform over all ids, in range
    z = np.full((1, 9), -np.inf, np.float32)
    z[0, 3] = np.nan
    ids, kept = _run(z, None, (1.0, 1.0, 0, 1.0), 4)
    assert 0 <= ids[0] < 9 and kept[0] == 9
    assert ids[0] == N.sample(z[0], [], 1.0, 1.0, 0, 1.0, 4)[0]


def test_graph_replay_equals_eager():
    torch = _torch()
    from llmi import ops
    rng = np.random.default_rng(7)
    z = torch.from_numpy((rng.standard_normal((3, 32000)) * 3).astype(np.float32)).cuda()
    h = torch.from_numpy(rng.integers(0, 32000, (3, 24)).astype(np.int32)).cuda()
    hl = torch.full((3,), 24, device="cuda", dtype=torch.int32)
    kw = dict(top_k=50, top_p=0.95, temperature=0.8, repetition_penalty=1.2, history=h, history_len=hl)
    eager = [t.clone() for t in ops.sample_nucleus(z, 21, **kw)]  # also places the jump table before the capture
    out_id = torch.full((3,), -1, device="cuda", dtype=torch.int32)
    out_kept = torch.full((3,), -1, device="cuda", dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.sample_nucleus(z, 21, out_id=out_id, out_kept=out_kept, **kw)
    out_id.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_id, eager[0]) and torch.equal(out_kept, eager[1])
    # the replay reads its inputs again: other logits, the eager result for them
    z.copy_(torch.from_numpy((rng.standard_normal((3, 32000)) * 3).astype(np.float32)))
    g.replay()
    torch.cuda.synchronize()
    again = ops.sample_nucleus(z, 21, **kw)
    assert torch.equal(out_id, again[0]) and torch.equal(out_kept, again[1])


def test_argument_checks():
    torch = _torch()
    from llmi import ops
    from llmi._lib import LlmiError, call
    z = torch.zeros(2, 100, device="cuda")
    out = torch.zeros(2, device="cuda", dtype=torch.int32)
    with pytest.raises(LlmiError, match=r"temperature must be > 0 \(greedy decoding is top_k = 1\)"):
        ops.sample_nucleus(z, 1, temperature=0.0)
    with pytest.raises(LlmiError, match="temperature must be > 0"):
        ops.sample_nucleus(z, 1, temperature=-1.0)
    for p in (0.0, 1.5, -0.1):
        with pytest.raises(LlmiError, match=r"top_p must be in \(0, 1\]"):
            ops.sample_nucleus(z, 1, top_p=p)
    with pytest.raises(LlmiError, match="repetition_penalty must be > 0"):
        ops.sample_nucleus(z, 1, repetition_penalty=0.0)
    with pytest.raises(LlmiError, match="top_k must be >= 0"):
        ops.sample_nucleus(z, 1, top_k=-1)
    for bad in (100, -1):
        h = torch.tensor([[1, 2, 3], [4, bad, 6]], device="cuda", dtype=torch.int32)
        with pytest.raises(LlmiError, match=r"history ids must be in \[0, vocab\)"):
            ops.sample_nucleus(z, 1, repetition_penalty=1.1, history=h)
    with pytest.raises(LlmiError, match="null logits or out_id"):
        call("llmi_sample_nucleus", None, 2, 100, None, 0, None, 1.0, 1.0, 0, 1.0, 1, out.data_ptr(), None, None)
    with pytest.raises(LlmiError, match="null logits or out_id"):
        call("llmi_sample_nucleus", z.data_ptr(), 2, 100, None, 0, None, 1.0, 1.0, 0, 1.0, 1, None, None, None)
    with pytest.raises(LlmiError, match="history_len without a history"):
        call("llmi_sample_nucleus", z.data_ptr(), 2, 100, None, 0, out.data_ptr(), 1.0, 1.0, 0, 1.0, 1,
             out.data_ptr(), None, None)
    with pytest.raises(LlmiError, match="vocab above 131072"):
        call("llmi_sample_nucleus", z.data_ptr(), 1, 131073, None, 0, None, 1.0, 1.0, 0, 1.0, 1, out.data_ptr(),
             None, None)
    with pytest.raises(LlmiError, match="at most 65536 rows"):
        call("llmi_sample_nucleus", z.data_ptr(), 65537, 1, None, 0, None, 1.0, 1.0, 0, 1.0, 1, out.data_ptr(),
             None, None)
    # out_kept is optional
    call("llmi_sample_nucleus", z.data_ptr(), 2, 100, None, 0, None, 1.0, 1.0, 0, 1.0, 1, out.data_ptr(), None, None)
    torch.cuda.synchronize()


def test_large_vocab_rereads_the_row():
    """vocab > 32768: keys are recomputed from the row in every pass; the bound is 131072."""
    rng = np.random.default_rng(8)
    V = 131072
    z = (rng.standard_normal((2, V)) * 2).astype(np.float32)
    h = rng.integers(0, V, (2, 24)).astype(np.int32)
    for prm, step in (((1.1, 0.6, 0, 0.9), 3), ((1.2, 0.8, 50, 0.95), 4)):
        ids, kept = _run(z, h, prm, step)
        for b in range(2):
            tok, k, cs, ds = N.sample(z[b], h[b], *prm, step, b)
            if cs >= N.DECIDED:
                assert kept[b] == k
                if ds >= N.DECIDED:
                    assert ids[b] == tok
