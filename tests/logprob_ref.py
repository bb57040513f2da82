"""numpy float64 restatement of llmi_logprobs (include/llmi.h, DESIGN.md "Log-probabilities"):
logprob = z - logsumexp(z) over the RAW logits, with the operator's non-finite conventions:
NaN counts as -inf; if the maximum is +inf the +inf entries get -log(their count) and every
other id -inf; a row of only -inf / NaN gets -log(vocab) everywhere. The top-n order is
(value descending, id ascending), padded with id -1 / logprob -inf past the vocabulary.
The kernel's integer weights are not restated: this is the mathematical value the kernel is
held against, within tolerance()."""
import numpy as np


def logprobs(z):
    """z [vocab] -> (lp float64 [vocab], logsumexp float64)."""
    z = np.asarray(z, np.float64).copy()
    z[np.isnan(z)] = -np.inf
    m = z.max()
    at_max = z == m
    if not np.isfinite(m):  # +inf entries, or nothing finite at all
        lse = m + np.log(at_max.sum()) if m > 0 else -np.inf
        return np.where(at_max, -np.log(at_max.sum()), -np.inf), lse
    with np.errstate(under="ignore"):
        d = z - m
        s = np.exp(d).sum()
    return d - np.log(s), m + np.log(s)


def top_n(z, n):
    """-> (ids int32 [n], lp float64 [n]) by (value descending, id ascending)."""
    z = np.asarray(z, np.float64).copy()
    z[np.isnan(z)] = -np.inf
    lp, _ = logprobs(z)
    order = np.lexsort((np.arange(len(z)), -z))[:n]
    ids = np.full(n, -1, np.int32)
    out = np.full(n, -np.inf)
    ids[:len(order)] = order
    out[:len(order)] = lp[order]
    return ids, out


def tolerance(vocab, lp):
    """Per-entry bound on |kernel - restatement|, derived, not measured:
    vocab * 2^-33: every weight is rounded to an integer of scale 2^32 (error <= 1/2 each)
    and S >= 2^32, so the relative error of S, hence the absolute error of log S, is at most
    vocab * 2^-33; 2^-17: a few float ulp of expf and of its float argument z - m over the
    terms that matter (each weight is relatively off by ~2^-22, and so is their sum, with room);
    |lp| * 2^-23: the final rounding of the logprob to float."""
    lp = np.asarray(lp, np.float64)
    with np.errstate(invalid="ignore"):
        return vocab * 2.0 ** -33 + 2.0 ** -17 + np.where(np.isfinite(lp), np.abs(lp), 0.0) * 2.0 ** -23


def assert_close(got, want, vocab, what=""):
    """got float32, want float64: equal where the restatement is not finite, else within
    tolerance(). Prints the worst ratio before asserting."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), (what, got[~fin][:8], want[~fin][:8])
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        tol = tolerance(vocab, want[fin])
        print(f"{what}: max err {err.max():.3e}, worst err / tol {(err / tol).max():.3f}")
        assert np.isfinite(got[fin]).all(), what
        assert (err <= tol).all(), (what, float(err.max()), float((err / tol).max()))
