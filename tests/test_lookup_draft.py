"""Prompt-lookup drafting on the host (llmi_lookup_draft, include/llmi.h): the worked cases of the
rule, a seeded sweep of short sequences over a 4-symbol alphabet against a numpy restatement of
the rule, and the argument errors. No GPU."""
import ctypes as C

import numpy as np
import pytest

import llmi
from llmi import _lib


def rule(ids, ngram_max, ngram_min, max_draft):
    """The rule, restated: g from ngram_max down to ngram_min with g <= n - 1; among the starts
    0 <= s <= n - g - 1 whose g ids equal the suffix, the largest; ids[s + g : s + g + max_draft]."""
    ids = list(ids)
    n = len(ids)
    for g in range(ngram_max, ngram_min - 1, -1):
        if g > n - 1:
            continue
        suffix = ids[n - g:]
        starts = [s for s in range(0, n - g) if ids[s:s + g] == suffix]
        if starts:
            s = max(starts)
            return ids[s + g:min(n, s + g + max_draft)]
    return []


@pytest.mark.parametrize("ids,ngram,want", [
    ([1, 2, 3, 4, 1, 2, 3], (3, 1), [4, 1, 2, 3]),
    ([5, 6, 7, 5, 6, 8, 5, 6], (2, 2), [8, 5, 6]),
    ([1, 2, 3, 9, 2, 3], (3, 1), [9, 2, 3]),      # g = 3 has no match, g = 2 matches at s = 1
    ([1, 2, 3], (3, 1), []),
])
def test_worked_cases(ids, ngram, want):
    got = llmi.lookup_draft(ids, ngram[0], ngram[1], 4)
    assert got.dtype == np.int32 and got.tolist() == want
    assert rule(ids, ngram[0], ngram[1], 4) == want


def test_random_sequences_against_the_rule():
    rng = np.random.default_rng(20241020)
    seen_hit = seen_miss = 0
    for _ in range(400):
        n = int(rng.integers(0, 25))
        ids = rng.integers(0, 4, n).astype(np.int32)
        gmin = int(rng.integers(1, 4))
        gmax = gmin + int(rng.integers(0, 3))
        k = int(rng.integers(0, 8))
        want = rule(ids, gmax, gmin, k)
        got = llmi.lookup_draft(ids, gmax, gmin, k).tolist()
        assert got == want, (ids.tolist(), gmax, gmin, k)
        seen_hit += bool(want)
        seen_miss += not want
    assert seen_hit > 50 and seen_miss > 20  # the sweep saw both outcomes


def test_bad_arguments():
    L = _lib.lib()
    ids = np.array([1, 2, 1, 2], np.int32)
    out = np.zeros(8, np.int32)
    n = C.c_int(-1)

    def rc(idp, cnt, gmax, gmin, k, outp, np_):
        return L.llmi_lookup_draft(idp, cnt, gmax, gmin, k, outp, np_)

    ok = (ids.ctypes.data, 4, 3, 1, 4, out.ctypes.data, C.byref(n))
    assert rc(*ok) == 0 and n.value == 2 and out[:2].tolist() == [1, 2]
    bad = [
        (None,) + ok[1:],                                   # null ids
        ok[:5] + (None, ok[6]),                             # null out
        ok[:6] + (None,),                                   # null n_out
        ok[:3] + (0,) + ok[4:],                             # ngram_min < 1
        ok[:2] + (1, 2) + ok[4:],                           # ngram_max < ngram_min
        ok[:4] + (8,) + ok[5:],                             # max_draft > 7
        ok[:4] + (-1,) + ok[5:],                            # max_draft < 0
        (ok[0], -1) + ok[2:],                               # n < 0
    ]
    for args in bad:
        assert rc(*args) == -1, args
        assert b"[llmi][ERROR]" in L.llmi_last_error()
    with pytest.raises(_lib.LlmiError):
        llmi.lookup_draft(ids, 1, 2, 4)
