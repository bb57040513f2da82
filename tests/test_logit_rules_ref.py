"""The numpy restatement of the logit rules (tests/logit_rules_ref.py) against hand-worked
cases, and its trie walk for constrained choice."""
import numpy as np
import pytest

import logit_rules_ref as L


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_empty_rules_are_the_identity_bit_for_bit():
    rng = np.random.default_rng(1)
    z = rng.standard_normal(1027).astype(np.float32)
    z[[3, 40, 77, 500]] = [0.0, -0.0, np.inf, -np.inf]
    v, i = L.process(z)
    assert np.array_equal(_bits(v), _bits(z)) and i == 77
    # zero penalties with a history, an all-zero bias and an all-ones mask change nothing either
    v2, i2 = L.process(z, bias=np.zeros(1027, np.float32), allowed=np.full(33, 0xFFFFFFFF, np.uint32),
                       history=[3, 3, 40], presence=0.0, frequency=0.0)
    assert np.array_equal(_bits(v2), _bits(z)) and i2 == 77
    # NaN is the one exception: it becomes -inf
    z[5] = np.nan
    v3, _ = L.process(z)
    assert v3[5] == -np.inf and np.array_equal(_bits(np.delete(v3, 5)), _bits(np.delete(z, 5)))


def test_minus_zero_guard():
    z = np.array([-0.0, -0.0, 0.0, -1.0], np.float32)
    for b0 in (0.0, -0.0):
        v, i = L.process(z, bias=np.array([b0, b0, b0, b0], np.float32))
        assert np.array_equal(_bits(v), _bits(z))  # -0.0 + 0.0 would have been +0.0
        assert i == 2                              # argmax_key orders -0.0 below +0.0
    assert np.float32(-0.0) + np.float32(0.0) == 0 and not np.signbit(np.float32(-0.0) + np.float32(0.0))
    k = L.argmax_key(np.array([-0.0, 0.0], np.float32), [0, 1])
    assert k[1] > k[0]


def test_ban_and_mask_give_minus_inf():
    z = np.array([1.0, 5.0, 3.0, 4.0, 2.0], np.float32)
    b = np.array([0.0, -np.inf, 0.5, 0.0, 0.0], np.float32)
    v, i = L.process(z, bias=b)
    assert v[1] == -np.inf and v[2] == np.float32(3.5) and i == 3
    v, i = L.process(z, bias=b, allowed=L.words_of(5, [0, 1, 4]))
    assert list(v) == [1.0, -np.inf, -np.inf, -np.inf, 2.0] and i == 4
    # stray bits at or above the vocabulary are ignored
    w = L.words_of(5, [0, 4]) | np.uint32(0xFFFFFFE0)
    assert L.process(z, allowed=w)[1] == 4
    # +inf meeting a ban is -inf, not NaN
    z2 = np.array([np.inf, 0.0], np.float32)
    v, i = L.process(z2, bias=np.array([-np.inf, 0.0], np.float32))
    assert v[0] == -np.inf and i == 1


def test_counts_with_repeats_and_the_order_of_the_operations():
    z = np.array([2.0, 2.0, 2.0, 2.0], np.float32)
    h = [1, 3, 3, 3, 1, 3]
    assert list(L.counts(4, h)) == [0, 2, 0, 4]
    pres, freq = np.float32(0.3), np.float32(0.1)
    v, i = L.process(z, history=h, presence=pres, frequency=freq)
    want1 = np.float32(2.0) - np.float32(pres + np.float32(freq * np.float32(2)))
    want3 = np.float32(2.0) - np.float32(pres + np.float32(freq * np.float32(4)))
    assert np.array_equal(_bits(v), _bits([2.0, want1, 2.0, want3])) and i == 0
    # presence alone, frequency alone, a negative penalty (a reward)
    assert L.process(z, history=h, presence=1.0)[0].tolist() == [2.0, 1.0, 2.0, 1.0]
    assert L.process(z, history=h, frequency=0.5)[0].tolist() == [2.0, 1.0, 2.0, 0.0]
    assert L.process(z, history=h, frequency=-0.5)[1] == 3
    # an empty history: nothing is penalised
    assert np.array_equal(_bits(L.process(z, history=[], presence=1.0, frequency=1.0)[0]), _bits(z))
    # bias first, then the penalty
    v, _ = L.process(z, bias=np.array([0, 1e-7, 0, 0], np.float32), history=[1], presence=0.25)
    assert v[1] == np.float32(np.float32(np.float32(2.0) + np.float32(1e-7)) - np.float32(0.25))


def test_all_minus_inf_gives_id_0_and_ties_go_to_the_lowest_id():
    z = np.full(9, -np.inf, np.float32)
    z[4] = np.nan
    assert L.process(z)[1] == 0
    assert L.process(np.array([1.0, 2.0], np.float32), allowed=np.zeros(1, np.uint32))[1] == 0
    z = np.array([0.0, 7.0, 3.0, 7.0, 7.0], np.float32)
    assert L.process(z)[1] == 1 and L.argmax(z) == 1
    assert L.process(z, allowed=L.words_of(5, [0, 3, 4]))[1] == 3


def test_bitmap_words():
    for V in (7, 32, 33, 1027, 32000):
        w = L.words_of(V, [0, V - 1])
        assert w.dtype == np.uint32 and len(w) == (V + 31) // 32
        assert (int(w[0]) & 1) and (int(w[(V - 1) >> 5]) >> ((V - 1) & 31)) & 1
        assert sum(bin(int(x)).count("1") for x in w) == (1 if V == 1 else 2)


def test_trie_walk_and_rejections():
    choices = [[5, 6, 7], [5, 6, 8], [5, 9], [2]]
    nodes = L.build_trie(choices)
    assert sorted(nodes[0]["next"]) == [2, 5] and nodes[nodes[0]["next"][2]]["leaf"] == 3
    assert L.walk(choices, lambda kids, step: kids[-1]) == (2, [5, 9])
    assert L.walk(choices, lambda kids, step: kids[0]) == (3, [2])
    assert L.walk(choices, lambda kids, step: {0: 5, 1: 6, 2: 8}[step]) == (1, [5, 6, 8])
    for bad in ([], [[1, 2], [1, 2]], [[1, 2], [1]], [[1], [1, 2]], [[1], []]):
        with pytest.raises(ValueError):
            L.build_trie(bad)


def test_the_symbol_exists():
    from llmi import _lib
    name = "llmi_process_logits"
    assert name in _lib._SIGS and name in _lib.header_functions() and hasattr(_lib.lib(), name)
