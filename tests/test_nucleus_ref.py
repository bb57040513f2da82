"""The numpy restatement of the nucleus sampler (tests/nucleus_ref.py) against hand-worked
rows, its own properties, and the share of the shared input recipe it leaves undecided."""
import math

import numpy as np

import nucleus_ref as N

ONE = float(N.ONE)
LN = math.log


def _hand_row():
    # weights 1, 1/2, 1/4, 0, 1 (times 2^32); order 0, 4, 1, 2, 3
    return np.array([0.0, LN(0.5), LN(0.25), -np.inf, 0.0], np.float32)


def test_hand_worked_weights_and_order():
    z = _hand_row()
    w = N.weights(N.scaled(z, [], 1, 1))
    assert w[0] == N.ONE and w[4] == N.ONE and w[3] == 0
    np.testing.assert_allclose(w[[1, 2]] / ONE, [0.5, 0.25], rtol=1e-6)
    p = N.Prepared(z, [], 1, 1, 0, 1.0)
    assert p.kept == 5 and p.cut_slack == 1.0 and list(p.ids) == [0, 1, 2, 3, 4]


def test_hand_worked_top_p_and_top_k():
    z = _hand_row()
    # S = 2.75; P = 0.7 * 2.75 = 1.925: rank prefix 1, 2 -> K = {0, 4}
    p = N.Prepared(z, [], 1, 1, 0, 0.7)
    assert p.kept == 2 and list(p.ids) == [0, 4]
    assert abs(p.cut_slack - (2 - 1.925) / 2.75) < 1e-6
    # top_k 3: C = {0, 4, 1}, S_C = 2.5; P = 0.9 * 2.5 = 2.25: prefix 1, 2, 2.5 -> all three
    p = N.Prepared(z, [], 1, 1, 3, 0.9)
    assert p.kept == 3 and list(p.ids) == [0, 1, 4]
    # top_k 3, top_p 1: K = C
    assert N.Prepared(z, [], 1, 1, 3, 1.0).kept == 3
    # top_k 2 cuts inside the tie-free part: {0, 4}
    assert list(N.Prepared(z, [], 1, 1, 2, 1.0).ids) == [0, 4]


def test_hand_worked_draw_walks_ids_in_ascending_order():
    z = _hand_row()
    p = N.Prepared(z, [], 1, 1, 3, 1.0)  # ids 0, 1, 4 with weights 1, .5, 1: prefix 1, 1.5, 2.5
    for u, want in ((0.01, 0), (0.39, 0), (0.41, 1), (0.59, 1), (0.61, 4), (0.99, 4)):
        tok, slack = p.draw(np.float32(u))
        assert tok == want and slack > 1e-3, (u, tok, slack)
    tok, slack = p.draw(np.float32(0.4))  # R = ceil(0.4f * 2.5 * 2^32): on the boundary up to fp32(0.4)
    assert slack < 1e-6


def test_top_k_1_is_lowest_id_argmax():
    z = np.array([0.5, 3.0, -1.0, 3.0, 3.0], np.float32)
    for step in range(1, 20):
        tok, kept, cs, ds = N.sample(z, [], 1, 1, 1, 1.0, step)
        assert (tok, kept, cs) == (1, 1, 1.0)


def test_tiny_top_p_is_argmax():
    rng = np.random.default_rng(3)
    z = rng.standard_normal(1000).astype(np.float32)
    for step in (1, 2, 3):
        tok, kept, _, _ = N.sample(z, [], 1, 0.7, 0, 1e-6, step)
        assert tok == int(np.argmax(z)) and kept == 1


def test_penalty_sign_rule_duplicates_and_empty_history():
    z = np.array([2.0, -2.0, 1.0, 0.0], np.float32)
    np.testing.assert_array_equal(N.scaled(z, [0, 1, 3], 2.0, 1.0), np.array([1.0, -4.0, 1.0, 0.0], np.float32))
    np.testing.assert_array_equal(N.scaled(z, [0, 1, 1, 0, 0], 2.0, 1.0), N.scaled(z, [1, 0], 2.0, 1.0))
    np.testing.assert_array_equal(N.scaled(z, [], 2.0, 1.0), z)
    np.testing.assert_array_equal(N.scaled(z, [0, 1], 1.0, 0.5), z * 2)
    # penalty before temperature, both correctly rounded fp32
    np.testing.assert_array_equal(N.scaled(z, [0], 1.1, 0.6)[0], np.float32(np.float32(2.0) / np.float32(1.1)) / np.float32(0.6))


def test_non_finite_rules():
    z = np.array([1.0, np.nan, -np.inf, 2.0], np.float32)
    p = N.Prepared(z, [], 1, 1, 0, 1.0)
    assert p.w[1] == 0 and p.w[2] == 0 and p.w[3] == N.ONE and 0 < p.w[0] < N.ONE
    z = np.array([1.0, np.inf, 5.0, np.inf], np.float32)
    p = N.Prepared(z, [], 1, 1, 0, 1.0)
    assert list(p.w) == [0, N.ONE, 0, N.ONE]
    assert {N.sample(z, [], 1, 1, 0, 1.0, s)[0] for s in range(1, 40)} == {1, 3}
    z = np.full(6, -np.inf, np.float32)
    assert list(N.Prepared(z, [], 1, 1, 0, 1.0).w) == [N.ONE] * 6


def test_draw_frequencies_match_softmax():
    z = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.9, -2.5], np.float32)
    p = N.Prepared(z, [], 1, 1, 0, 1.0)
    n = 4000
    from oracle import xorwow
    got = np.bincount([p.draw(xorwow.curand_uniform(s, 0))[0] for s in range(1, n + 1)], minlength=8)
    q = np.exp(z.astype(np.float64))
    q /= q.sum()
    sigma = np.sqrt(n * q * (1 - q))
    assert (np.abs(got - n * q) <= 4 * sigma).all(), (got, n * q, sigma)


def test_recipe_undecided_share():
    cases = N.recipe_expected()
    assert len(cases) == len(N.VOCABS) * len(N.SCALES) * len(N.PARAMS) * (2 * N.ROWS + 2)
    undecided = sum(1 for _, _, _, _, cs, ds, _ in cases if cs < N.DECIDED or ds < N.DECIDED)
    print(f"undecided {undecided} of {len(cases)}")
    assert undecided <= 0.05 * len(cases)
    for _, _, tok, kept, _, _, w in cases:
        assert 0 <= tok < len(w) and w[tok] > 0 and 1 <= kept <= len(w)
