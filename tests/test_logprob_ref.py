"""tests/logprob_ref.py, the float64 restatement the logprob kernel is held against: it is
torch.log_softmax in float64 on finite rows, and gives the stated values on rows with +inf,
-inf and NaN entries. CPU only."""
import numpy as np
import torch

import logprob_ref as L


def test_finite_rows_are_log_softmax():
    rng = np.random.default_rng(0)
    for vocab, sigma in ((1, 1.0), (7, 4.0), (1000, 4.0), (32000, 4.0), (1000, 1e-3)):
        z = (rng.standard_normal(vocab) * sigma).astype(np.float32)
        lp, lse = L.logprobs(z)
        want = torch.log_softmax(torch.from_numpy(z.astype(np.float64)), dim=0).numpy()
        np.testing.assert_allclose(lp, want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(lse, torch.logsumexp(torch.from_numpy(z.astype(np.float64)), 0).item(), atol=1e-12)
        assert abs(np.exp(lp).sum() - 1.0) < 1e-12


def test_a_dominant_logit_keeps_the_others_finite():
    z = np.zeros(100, np.float32)
    z[17] = 1e4
    lp, _ = L.logprobs(z)
    assert lp[17] == 0.0
    assert np.all(lp[np.arange(100) != 17] == -1e4)


def test_non_finite_rows():
    z = np.array([0.5, np.nan, -np.inf, 1.5, np.nan], np.float32)
    lp, _ = L.logprobs(z)
    want = torch.log_softmax(torch.tensor([0.5, 1.5], dtype=torch.float64), 0).numpy()
    np.testing.assert_allclose(lp[[0, 3]], want, atol=1e-15)
    assert np.all(np.isneginf(lp[[1, 2, 4]]))
    # +inf entries share the mass, everything else has none
    lp, lse = L.logprobs(np.array([1.0, np.inf, -2.0, np.inf, np.nan], np.float32))
    np.testing.assert_array_equal(lp, [-np.inf, -np.log(2.0), -np.inf, -np.log(2.0), -np.inf])
    assert lse == np.inf
    # nothing finite: uniform
    for row in ([-np.inf] * 6, [np.nan, -np.inf, np.nan]):
        lp, lse = L.logprobs(np.array(row, np.float32))
        np.testing.assert_array_equal(lp, np.full(len(row), -np.log(len(row))))
        assert lse == -np.inf


def test_top_n_order_and_padding():
    z = np.array([1.0, 3.0, 3.0, -np.inf, np.nan, 2.0], np.float32)
    ids, lp = L.top_n(z, 8)
    np.testing.assert_array_equal(ids, [1, 2, 5, 0, 3, 4, -1, -1])  # ties to the lower id; NaN is -inf
    full, _ = L.logprobs(z)
    np.testing.assert_array_equal(lp[:6], full[ids[:6]])
    assert np.all(np.isneginf(lp[6:]))
    ids, _ = L.top_n(np.full(9, 0.25, np.float32), 4)
    np.testing.assert_array_equal(ids, [0, 1, 2, 3])
    ids, lp = L.top_n(z, 0)
    assert ids.shape == (0,) and lp.shape == (0,)


def test_tolerance_terms():
    t = L.tolerance(32768, np.array([0.0, -8.0, -np.inf]))
    np.testing.assert_allclose(t, [2.0 ** -18 + 2.0 ** -17, 2.0 ** -18 + 2.0 ** -17 + 2.0 ** -20, 2.0 ** -18 + 2.0 ** -17])
