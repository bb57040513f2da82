"""llmi_process_logits (csrc/logit_rules.hip) against the numpy restatement
tests/logit_rules_ref.py: processed rows and ids are compared BITWISE -- every operation of the
rule is one correctly rounded fp32 operation and every count an integer, so there is no
tolerance and no undecided case. Shapes cover both counter passes (vocab > 65536), rows whose
start is not 16-byte aligned (odd vocab, rows 1 and 2) and a misaligned output."""
import numpy as np
import pytest

import logit_rules_ref as L

pytestmark = pytest.mark.gpu

VOCABS = (7, 1027, 32000, 40003, 70001)


def _torch():
    import torch
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _logits(rng, rows, V):
    """Rows with NaN, +-inf, +-0 and tied maxima (the lowest id must win)."""
    z = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    z[:, 1 % V] = np.nan
    z[:, 2 % V] = -np.inf
    z[:, 3 % V] = -0.0
    z[:, 4 % V] = 0.0
    for b in range(rows):
        top = np.float32(z[b][np.isfinite(z[b])].max() + 1)
        z[b, [V // 3, V // 2, V - 1]] = top
    if rows > 1:
        z[1, V - 2] = np.inf
    return z


def _hist_ids(V):
    """5 distinct ids, in both counter halves where the vocabulary has two, among them a tied maximum."""
    return np.unique(np.array([0, V // 3, V // 2, V - 1, (V * 5) // 7], np.int64) % V)


def _history(rng, rows, V, lens):
    ids = _hist_ids(V)
    h = rng.choice(ids, size=(rows, 300)).astype(np.int32)
    return h, np.array(lens[:rows], np.int32)


def _bias(rng, V):
    b = np.zeros(V, np.float32)
    n = max(1, V // 5)
    idx = rng.choice(V, size=n, replace=False)
    b[idx] = rng.standard_normal(n).astype(np.float32)
    b[idx[: max(1, n // 4)]] = -np.inf
    b[idx[-1]] = -0.0
    b[3 % V] = 0.5   # -0.0 + 0.5
    b[V // 3] = -np.inf  # ban one of the tied maxima
    return b


def _bitmaps(rng, rows, V):
    W = (V + 31) // 32
    ones = np.full(W, 0xFFFFFFFF, np.uint32)
    single = L.words_of(V, [V // 2])
    alt = np.full(W, 0xAAAAAAAA, np.uint32)
    stray = L.words_of(V, [V - 1, 0])
    if V % 32:
        stray[-1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)  # bits at or above vocab
    per_row = np.stack([ones, alt, stray][:rows]) if rows > 1 else None
    return {"ones": ones, "single": single, "alt": alt, "stray": stray, "per_row": per_row}


def _run(z, bias=None, allowed=None, history=None, hlen=None, presence=0.0, frequency=0.0, out=None):
    torch = _torch()
    from llmi import ops
    zd = _dev(z)
    o, ids = ops.process_logits(zd, bias=_dev(bias), allowed=_dev(allowed), history=_dev(history),
                                history_len=_dev(hlen), presence_penalty=presence, frequency_penalty=frequency,
                                out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(zd.cpu().numpy()), _bits(z)), "the input row was modified"
    return o.cpu().numpy(), ids.cpu().numpy()


def _want(z, bias, allowed, history, hlen, presence, frequency):
    rows = z.shape[0]
    vs, ids = [], []
    for b in range(rows):
        a = None if allowed is None else (allowed[b] if allowed.ndim == 2 else allowed)
        h = [] if history is None else history[b, : hlen[b]]
        v, i = L.process(z[b], bias, a, h, presence, frequency)
        vs.append(v)
        ids.append(i)
    return np.stack(vs), np.array(ids, np.int32)


def _check(z, **kw):
    got_v, got_i = _run(z, **kw)
    want_v, want_i = _want(z, kw.get("bias"), kw.get("allowed"), kw.get("history"), kw.get("hlen"),
                           kw.get("presence", 0.0), kw.get("frequency", 0.0))
    bad = np.flatnonzero(_bits(got_v).ravel() != _bits(want_v).ravel())
    assert bad.size == 0, (bad[:8], got_v.ravel()[bad[:8]], want_v.ravel()[bad[:8]])
    assert np.array_equal(got_i, want_i), (got_i, want_i)
    return got_v, got_i


@pytest.mark.parametrize("V", VOCABS)
def test_rows_and_ids_are_the_restatement_bitwise(V):
    rng = np.random.default_rng(100 + V)
    for rows, lens in ((1, [300]), (2, [1, 300]), (3, [300, 1, 0])):
        z = _logits(rng, rows, V)
        h, hl = _history(rng, rows, V, lens)
        bias = _bias(rng, V)
        maps = _bitmaps(rng, rows, V)
        # empty rules: the identity, NaN aside, and the plain argmax
        v, i = _check(z)
        keep = ~np.isnan(z)
        assert np.array_equal(_bits(v)[keep], _bits(z)[keep]) and (v[np.isnan(z)] == -np.inf).all()
        # each rule alone
        _check(z, bias=bias)
        _check(z, history=h, hlen=hl, presence=0.4, frequency=0.0)
        _check(z, history=h, hlen=hl, presence=0.0, frequency=0.07)
        for name in ("ones", "single", "alt", "stray"):
            _check(z, allowed=maps[name])
        if rows > 1:
            _check(z, allowed=maps["per_row"])
        # zero penalties with a history: nothing is counted, nothing changes
        v0, _ = _check(z, history=h, hlen=hl)
        assert np.array_equal(_bits(v0), _bits(v))
        # all of them together (counts reach 60: 300 ids over 5)
        v, i = _check(z, bias=bias, allowed=maps["alt"], history=h, hlen=hl, presence=0.3, frequency=0.11)
        _check(z, bias=bias, allowed=maps["per_row"] if rows > 1 else maps["stray"], history=h, hlen=hl,
               presence=-0.2, frequency=0.05)
    assert L.counts(V, h[0]).max() >= 60


def test_ties_bans_and_an_empty_allowed_set():
    V = 1027
    z = np.zeros((1, V), np.float32)
    z[0, [100, 200, 300]] = 5.0
    assert _check(z)[1][0] == 100                      # tied maxima: the lowest id
    b = np.zeros(V, np.float32)
    b[100] = -np.inf
    assert _check(z, bias=b)[1][0] == 200              # the banned one is out
    assert _check(z, allowed=L.words_of(V, [300, 7]))[1][0] == 300
    v, i = _check(z, allowed=np.zeros((V + 31) // 32, np.uint32))
    assert i[0] == 0 and (v == -np.inf).all()          # nothing allowed: all -inf, id 0
    z[0, 100] = np.inf
    v, i = _check(z, bias=b)                           # +inf meeting a ban: -inf, not NaN
    assert v[0, 100] == -np.inf and i[0] == 200


def test_misaligned_output_rows():
    torch = _torch()
    rng = np.random.default_rng(7)
    V, rows = 1027, 2
    z = _logits(rng, rows, V)
    h, hl = _history(rng, rows, V, [300, 300])
    big = torch.zeros(rows * V + 3, device="cuda")
    for off in (1, 2, 3):
        out = big[off:off + rows * V]
        got, ids = _run(z, bias=_bias(np.random.default_rng(8), V), history=h, hlen=hl, presence=0.3, frequency=0.1,
                        out=out)
        want_v, want_i = _want(z, _bias(np.random.default_rng(8), V), None, h, hl, 0.3, 0.1)
        assert np.array_equal(_bits(got), _bits(want_v)) and np.array_equal(ids, want_i)
        assert np.array_equal(_bits(out.cpu().numpy().reshape(rows, V)), _bits(want_v))


def test_graph_replay_equals_eager():
    torch = _torch()
    from llmi import ops
    rng = np.random.default_rng(9)
    V, rows = 32000, 3
    z = _dev(_logits(rng, rows, V))
    h, hl = _history(rng, rows, V, [300, 1, 0])
    kw = dict(bias=_dev(_bias(rng, V)), allowed=_dev(_bitmaps(rng, rows, V)["alt"]), history=_dev(h),
              history_len=_dev(hl), presence_penalty=0.3, frequency_penalty=0.11)
    eager = [t.clone() for t in ops.process_logits(z, **kw)]
    out = torch.zeros(rows, V, device="cuda")
    out_ids = torch.full((rows,), -1, device="cuda", dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.process_logits(z, out=out, out_ids=out_ids, **kw)
    out.zero_()
    out_ids.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager[0].view(torch.int32)) and torch.equal(out_ids, eager[1])
    # the replay reads its inputs again: other logits, the eager result for them
    z.copy_(_dev(_logits(rng, rows, V)))
    g.replay()
    torch.cuda.synchronize()
    again = ops.process_logits(z, **kw)
    assert torch.equal(out.view(torch.int32), again[0].view(torch.int32)) and torch.equal(out_ids, again[1])


def test_argument_checks_return_minus_one_and_launch_nothing():
    torch = _torch()
    from llmi import _lib
    lib = _lib.lib()
    V, W = 100, 4
    z = torch.zeros(2, V, device="cuda")
    out = torch.full((2, V), 7.0, device="cuda")
    ids = torch.full((2,), -5, device="cuda", dtype=torch.int32)
    hist = torch.tensor([[1, 2, 3], [4, 5, 6]], device="cuda", dtype=torch.int32)
    hlen = torch.tensor([3, 3], device="cuda", dtype=torch.int32)
    bias = torch.zeros(V, device="cuda")
    allowed = torch.full((W,), -1, device="cuda", dtype=torch.int32)
    P = lambda t: None if t is None else t.data_ptr()

    def rc(logits=z, rows=2, vocab=V, b=None, a=None, a_stride=0, h=None, h_stride=0, hl=None, pres=0.0, freq=0.0,
           o=out, oi=ids):
        r = lib.llmi_process_logits(P(logits), rows, vocab, P(b), P(a), a_stride, P(h), h_stride, P(hl), pres, freq,
                                    P(o), P(oi), None)
        torch.cuda.synchronize()
        return r, lib.llmi_last_error().decode()

    bad_hist = torch.tensor([[1, 2, 3], [4, V, 6]], device="cuda", dtype=torch.int32)
    neg_hist = torch.tensor([[1, -1, 3], [4, 5, 6]], device="cuda", dtype=torch.int32)
    long_len = torch.tensor([3, 4], device="cuda", dtype=torch.int32)
    nan_bias, inf_bias = bias.clone(), bias.clone()
    nan_bias[5] = float("nan")
    inf_bias[6] = float("inf")
    cases = [
        (dict(logits=None), "null logits, out or out_ids"),
        (dict(o=None), "null logits, out or out_ids"),
        (dict(oi=None), "null logits, out or out_ids"),
        (dict(o=z), "out must not be the logits"),
        (dict(rows=0), "rows must be in"),
        (dict(rows=65537), "rows must be in"),
        (dict(vocab=0), "vocab must be positive"),
        (dict(pres=float("nan")), "penalties must be finite"),
        (dict(freq=float("inf")), "penalties must be finite"),
        (dict(a=allowed, a_stride=W - 1), "allowed_stride"),
        (dict(a=None, a_stride=W), "allowed_stride"),
        (dict(hl=hlen), "history_len without a history"),
        (dict(h=hist, h_stride=-1, hl=hlen), "history_len without a history"),
        (dict(h=hist, h_stride=3, hl=long_len, pres=0.5), "history_len must be in"),
        (dict(h=bad_hist, h_stride=3, hl=hlen, pres=0.5), "history ids must be in"),
        (dict(h=neg_hist, h_stride=3, hl=hlen, pres=0.5), "history ids must be in"),
        (dict(b=nan_bias), "bias values must be finite or -inf"),
        (dict(b=inf_bias), "bias values must be finite or -inf"),
    ]
    for kw, msg in cases:
        r, err = rc(**kw)
        assert r == -1 and msg in err, (kw.keys(), r, err)
        assert (out == 7.0).all() and (ids == -5).all(), "a refused call launched"
    # the two "not built" sizes say so (LLMI_EUNSUPPORTED), and launch nothing either
    r, err = rc(rows=1, vocab=131073)
    assert r == -2 and "vocab above 131072" in err
    r, err = rc(h=hist, h_stride=65536, hl=hlen, pres=0.5)
    assert r == -2 and "65535" in err
    assert (out == 7.0).all() and (ids == -5).all()
    # and a good call with everything optional absent works
    r, err = rc()
    assert r == 0 and (out == 0.0).all() and (ids == 0).all()
