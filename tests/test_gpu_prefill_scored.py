"""llmi_engine_prefill_scored: the prefill that also fills the log-probability records of the
rows it consumes (final norm + lm_head GEMM over each chunk's rows into a logits slab, then the
row-record form of the logprob launch).

The logprob launch is isolated from the GEMM's numerics as tests/test_gpu_engine_logprobs.py
does it for the token step: the float64 restatement (tests/logprob_ref.py) runs on the run's
OWN slab rows (llmi_engine_scored_logits), within logprob_ref.tolerance, top-n ids exact.
Everything the unscored prefill leaves is compared bitwise. Against the decode path the slab
rows are held to the rel-L2 bar tests/test_gpu_prefill.py holds prefill-versus-decode logits
to, and the records to a bound derived from the two logit rows of each position."""
import numpy as np
import pytest

import logprob_ref as L

pytestmark = pytest.mark.gpu

SEED = 20240611
LOGIT_TOL = 1e-3  # tests/test_gpu_prefill.py's bar for prefill-versus-decode logits


def _engine(name="tiny", n_top=3, weight_dtype=None, kv_dtype=None, **over):
    from llmi.engine import Engine, preset
    cfg = preset(name, **over)
    if weight_dtype is not None:
        cfg.weight_dtype = weight_dtype
    if kv_dtype is not None:
        cfg.kv_dtype = kv_dtype
    e = Engine(cfg)
    e.load_synthetic(SEED)
    if n_top >= 0:
        e.set_logprobs(n_top)
    return e


def _prompt(n, vocab=32000, seed=7):
    from llmi.engine import synth_prompt
    return synth_prompt(seed, n, vocab)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _check_records(e, prompt, qs, n_top, rows=None, what=""):
    """Check 1: records q in qs against the restatement on slab row q - 1 (rows[q - 1] if the
    caller read the slab earlier, else read now)."""
    lp, tids, tlp = e.logprobs()
    vocab = e.cfg.vocab
    for q in qs:
        z = rows[q - 1] if rows is not None else e.scored_logits(q - 1)
        assert np.isfinite(z).all()
        want, _ = L.logprobs(z)
        tok = int(prompt[q])
        assert np.isfinite(lp[q]), (what, q)
        L.assert_close(lp[q:q + 1], want[tok:tok + 1], vocab, f"{what} record {q} token {tok}")
        if n_top:
            wi, wl = L.top_n(z, n_top)
            np.testing.assert_array_equal(tids[q], wi)
            assert np.isfinite(tlp[q]).all(), (what, q)
            L.assert_close(tlp[q], wl, vocab, f"{what} record {q} top")


@pytest.mark.parametrize("exact", [0, 1, 2])
@pytest.mark.parametrize("n_top", [0, 3, 8])
def test_records_are_the_restatement_on_the_runs_own_logits(n_top, exact):
    prompt = _prompt(40)
    with _engine(n_top=n_top, max_seq=64) as e:
        e.set_prompt(prompt)
        e.prefill(40, exact=exact, score=True)
        lp, tids, tlp = e.logprobs()
        assert len(lp) == 41 and tids.shape == tlp.shape == (41, n_top)
        assert np.isnan(lp[0]) and not np.isnan(lp[1:]).any() and not np.isnan(tlp[1:]).any()
        assert (tids[1:] >= 0).all()
        _check_records(e, prompt, range(1, 40), n_top, what=f"exact {exact} n_top {n_top}")


@pytest.mark.parametrize("exact", [0, 1, 2])
def test_nothing_else_moves(exact):
    prompt = _prompt(40)
    got = []
    for score in (False, True):
        with _engine(max_seq=64) as e:
            e.set_prompt(prompt)
            e.prefill(40, exact=exact, score=score)
            lp, tids, tlp = e.logprobs()
            got.append((e.tokens(41), e.logits(), e.kv_slot(0, 0), e.kv_slot(1, 39, True),
                        (lp[40:], tids[40:], tlp[40:]), lp))
    plain, scored = got
    np.testing.assert_array_equal(plain[0], scored[0])
    assert len(plain[0]) == 41
    for i in (1, 2, 3):
        assert np.array_equal(_bits(plain[i]), _bits(scored[i])), i
    assert _same(plain[4], scored[4]) and np.isfinite(scored[4][0]).all()
    # the plain call leaves its rows "not computed", the scored one none of them
    assert np.isnan(plain[5][:40]).all() and np.isfinite(scored[5][1:]).all()


_DECODE = {}


def _decode_path(key, make, ids):
    """The text stepped eagerly: per-position logits, the records, and score(ids) (bitwise the
    eager records). Computed once per configuration."""
    if key not in _DECODE:
        rows = []
        with make() as e:
            e.set_prompt(ids)
            for _ in range(len(ids) - 1):
                e.decode(1, use_graph=False)
                rows.append(e.logits())
            lp = e.logprobs(len(ids))[0][1:].copy()
            stepped = e.score(ids)
        assert np.array_equal(_bits(stepped), _bits(lp))
        _DECODE[key] = (rows, stepped)
    return _DECODE[key]


@pytest.mark.parametrize("name,over,n", [("tiny", dict(max_seq=576), 530),
                                        ("llama2-7b", dict(layers=1, max_seq=160), 130)])
def test_against_the_decode_path(name, over, n):
    """Two chunks at `tiny` (512 + 17 rows: row 511, the last of the first chunk, is scored);
    one chunk of 129 rows at the 7B width (the gemm2 / gemm3 tile counts)."""
    def make():
        return _engine(name, n_top=0, **over)
    ids = _prompt(n, seed=11)
    dec_rows, dec_lp = _decode_path((name, n), make, ids)
    with make() as e:
        got = e.score(ids, prefill=True)
        one_call = e.logprobs(n)
        # the slab rows, chunk by chunk (a scored call leaves its last chunk's rows readable)
        e.set_prompt(ids)
        rows, p = [], 0
        while p < n - 1:
            m = min(512, n - 1 - p)
            e.prefill(m, score=True)
            rows += [e.scored_logits(q) for q in range(p, p + m)]
            p += m
        by_chunk = e.logprobs(n)
        # a row scored by both runs has the same record; the chunk calls' last rows (their
        # records are the token step's head) are the one call's scored rows: check 1 on those
        ends = [q for q in range(512, n - 1, 512)]
        keep = np.ones(n, bool)
        keep[ends] = False
        assert np.array_equal(_bits(one_call[0][keep]), _bits(by_chunk[0][keep]))
        e.score(ids, prefill=True)
        _check_records(e, ids, ends, 0, rows=rows, what=f"{name} chunk end")
    assert got.shape == (n - 1,) and np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(one_call[0][1:]))
    worst_l2 = worst = 0.0
    for p in range(n - 1):
        zs, zd = rows[p].astype(np.float64), dec_rows[p].astype(np.float64)
        r = rel(zs, zd)
        worst_l2 = max(worst_l2, r)
        assert r < LOGIT_TOL, (p, r)
        # lp = z_t - logsumexp(z): each term moves by at most max |dz|; plus both kernels' own error
        bound = 2.0 * np.abs(zs - zd).max() + L.tolerance(len(zs), got[p]) + L.tolerance(len(zs), dec_lp[p])
        d = abs(float(got[p]) - float(dec_lp[p]))
        worst = max(worst, d / bound)
        assert d <= bound, (p, d, bound)
    print(f"{name}: worst logits rel-L2 {worst_l2:.3e}, worst |dlp| / bound {worst:.3f}")


def test_history_before_the_prefill():
    prompt = _prompt(100, seed=5)
    with _engine(max_seq=128) as e:
        stepped = e.score(prompt)
    with _engine(max_seq=128) as e:
        e.set_prompt(prompt)
        e.decode(37)
        e.prefill(63, score=True)
        lp, tids, tlp = e.logprobs()
        assert len(lp) == 101 and np.isfinite(lp[1:]).all() and np.isfinite(tlp[1:]).all() and (tids[1:] >= 0).all()
        assert np.array_equal(_bits(lp[1:38]), _bits(stepped[:37]))
        _check_records(e, prompt, range(38, 100), 3, what="after 37 steps")


@pytest.mark.parametrize("exact", [0, 1])
def test_int8_engine_scores_through_the_fused_norm_gemm(exact):
    """The older GEMM (gemm.hip) with its fp16 lm_head, at the shape
    tests/test_gpu_prefill.py::test_prefill_then_decode_matches_reference runs it."""
    import llmi
    with _engine("llama2-13b", weight_dtype=llmi.I8, kv_dtype=llmi.F32, layers=1, max_seq=32) as e:
        prompt = _prompt(24, seed=3)
        e.set_prompt(prompt)
        e.prefill(24, exact=exact, score=True)
        lp = e.logprobs()[0]
        assert len(lp) == 25 and np.isfinite(lp[1:]).all()
        _check_records(e, prompt, range(1, 24), 3, what=f"int8 exact {exact}")


def test_fp32_weights_fall_back_to_decode_steps():
    import llmi
    prompt = _prompt(20, seed=9)
    with _engine(weight_dtype=llmi.F32, kv_dtype=llmi.F32) as e:
        e.set_prompt(prompt)
        e.decode(20)
        want = e.logprobs()
        toks = e.tokens(21)
        e.set_prompt(prompt)
        e.prefill(20, score=True)
        assert _same(e.logprobs(), want) and np.isfinite(want[0][1:]).all()
        np.testing.assert_array_equal(e.tokens(21), toks)
        got = e.score(prompt, prefill=True)
        assert np.array_equal(_bits(got), _bits(e.score(prompt)))


def test_errors_leave_tokens_and_records_alone():
    from llmi._lib import LlmiError
    prompt = _prompt(40)
    with _engine(max_seq=64) as e:
        e.set_prompt(prompt)
        e.prefill(20, score=True)
        toks, rec = e.tokens(), e.logprobs()
        assert len(toks) == 20 and len(rec[0]) == 21

        def unchanged():
            np.testing.assert_array_equal(e.tokens(), toks)
            assert _same(e.logprobs(), rec)

        with pytest.raises(LlmiError, match=r"failed \(-1\).*rows must lie inside the prompt"):
            e.prefill(21, score=True)
        unchanged()
        for pos in (-1, 20, 39):  # the chunk holds rows 0 .. 19
            with pytest.raises(LlmiError, match=r"failed \(-1\).*no scored chunk holds this position"):
                e.scored_logits(pos)
        unchanged()
        e.set_logprobs(-1)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*set_logprobs first"):
            e.prefill(5, score=True)
        np.testing.assert_array_equal(e.tokens(), toks)
        e.set_logprobs(3)  # the same n_top: the records are kept
        unchanged()
        e.prefill(20, score=True)  # and the engine goes on
        assert np.isfinite(e.logprobs()[0][1:]).all() and len(e.tokens()) == 41
        e.set_prompt(prompt)  # a new prompt forgets the chunk
        with pytest.raises(LlmiError, match="no scored chunk holds this position"):
            e.scored_logits(0)
    with _engine(n_top=-1, max_seq=64) as e:  # never turned on
        e.set_prompt(prompt)
        with pytest.raises(LlmiError, match=r"failed \(-1\).*set_logprobs first"):
            e.prefill(40, score=True)
        e.prefill(40)
        assert len(e.tokens()) == 41
