"""TEST INFRASTRUCTURE ONLY. Numpy restatement of the nucleus sampler (llmi_sample_nucleus,
llmi_engine_set_sampling_params; DESIGN.md "Nucleus sampler"), for tests/test_nucleus_ref.py
and the GPU tests.

Per row: logits z[V] fp32, history ids, repetition penalty r, temperature T, top_k (0: no
limit), top_p in (0, 1], u = the first curand_uniform of curand_init(step, row, 0).

  1. penalty (r != 1): for every distinct history id, z = z > 0 ? z / r : z * r   (fp32)
  2. temperature (T != 1): z = z / T                                               (fp32)
     NaN -> -inf (the documented rule for NaN)
  3. order: value descending, ties to the lower id -- the argmax key's order
  4. m = max z;  w = uint64(rint(float64(expf(z - m)) * 2^32)); z == m has 2^32 exactly
     (which also defines a +inf maximum: the +inf ids share the draw, all others weigh 0)
  5. C = the first top_k of the order
  6. P = ceil(float64(top_p) * S_C); K = the shortest rank prefix of C with weight >= P
  7. R = ceil(float64(u) * S_K); the id = the first id of K, ascending, whose running
     weight reaches R

The slacks say how far a case is from a boundary that a 2-ulp difference between two
correct fp32 expf implementations could move: a case is decided when both are >= 1e-6.
"""
import math

import numpy as np

from oracle import xorwow

ONE = 1 << 32
DECIDED = 1e-6


def key_of(z):
    """The ordered 32-bit key of fp32 values (the high half of csrc/common.h argmax_key)."""
    b = np.asarray(z, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def scaled(z, history, r, T):
    """Steps 1-2: the penalised, tempered, NaN-free fp32 row."""
    z = np.array(z, np.float32, copy=True)
    r, T = np.float32(r), np.float32(T)
    ids = np.unique(np.asarray(history, np.int64)) if len(history) else np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        if r != np.float32(1) and len(ids):
            v = z[ids]
            z[ids] = np.where(v > 0, v / r, v * r).astype(np.float32)
        if T != np.float32(1):
            z = (z / T).astype(np.float32)
    z[np.isnan(z)] = -np.inf
    return z


def weights(z):
    """Step 4: integer weights (int64; the maximum's is 2^32) of a scaled row."""
    key = key_of(z)
    m = z[np.argmax(key)]
    with np.errstate(all="ignore"):
        e = np.exp((z - m).astype(np.float32)).astype(np.float32)
    e[np.isnan(e)] = 0
    w = np.rint(e.astype(np.float64) * 4294967296.0).astype(np.int64)
    w[key == key.max()] = ONE
    return w


class Prepared:
    """Steps 1-6 of one row: everything but the draw."""

    def __init__(self, z, history, r, T, top_k, top_p):
        z = scaled(z, history, r, T)
        V = len(z)
        self.w = weights(z)
        order = np.argsort(-key_of(z).astype(np.int64), kind="stable")  # stable: ties keep the lower id first
        C = order if top_k == 0 or top_k >= V else order[:top_k]
        cum = np.cumsum(self.w[C])
        S_C = int(cum[-1])
        n, self.cut_slack = len(C), 1.0
        if np.float32(top_p) < np.float32(1):
            x = float(np.float64(np.float32(top_p)) * np.float64(S_C))
            P = min(max(int(math.ceil(x)), 1), S_C)
            n = int(np.searchsorted(cum, P, side="left")) + 1
            below = float(cum[n - 2]) if n >= 2 else 0.0
            self.cut_slack = min(abs(x - below), abs(float(cum[n - 1]) - x)) / S_C
        self.kept = n
        self.ids = np.sort(C[:n])
        self.cum = np.cumsum(self.w[self.ids])
        self.S_K = int(self.cum[-1])

    def draw(self, u):
        """Step 7 -> (id, draw_slack)."""
        y = float(np.float64(np.float32(u)) * np.float64(self.S_K))
        R = min(max(int(math.ceil(y)), 1), self.S_K)
        j = int(np.searchsorted(self.cum, R, side="left"))
        below = float(self.cum[j - 1]) if j >= 1 else 0.0
        return int(self.ids[j]), min(abs(y - below), abs(float(self.cum[j]) - y)) / self.S_K


def sample(z, history, r, T, top_k, top_p, step, row=0, u=None):
    """-> (id, kept, cut_slack, draw_slack); u overrides the XORWOW draw."""
    p = Prepared(z, history, r, T, top_k, top_p)
    if u is None:
        u = xorwow.curand_uniform(int(step), int(row))
    tok, draw_slack = p.draw(u)
    return tok, p.kept, p.cut_slack, draw_slack


# ---------------------------------------------------------------- the shared input recipe
VOCABS = (1, 5, 1027, 32000, 40003)
SCALES = (1.0, 4.0)
PARAMS = ((1.0, 1.0, 0, 0.9), (1.1, 0.6, 0, 0.9), (1.2, 0.8, 50, 0.95), (1.0, 1.5, 0, 1.0), (1.3, 0.7, 40, 0.5))
STEPS = (1, 2, 77, 1000003)  # steps 1 and 77 are sampled as 3 rows, the others as row 0 alone
ROWS = 3
N_HISTORY = 24


def recipe_inputs():
    """[(V, scale, logits [ROWS, V] fp32, history [ROWS, N_HISTORY] int32)] from a fixed seed."""
    rng = np.random.default_rng(20240607)
    out = []
    for V in VOCABS:
        for s in SCALES:
            z = (rng.standard_normal((ROWS, V)) * s).astype(np.float32)
            h = rng.integers(0, V, size=(ROWS, N_HISTORY)).astype(np.int32)
            out.append((V, s, z, h))
    return out


def recipe_calls():
    """Every call of the recipe: (input index, logits, history, (r, T, k, p), step, rows)."""
    for ii, (V, s, z, h) in enumerate(recipe_inputs()):
        for prm in PARAMS:
            for i, step in enumerate(STEPS):
                rows = ROWS if i % 2 == 0 else 1
                yield ii, z[:rows], h[:rows], prm, step, rows


_EXPECTED = None


def recipe_expected():
    """[(call index, row, id, kept, cut_slack, draw_slack, weights)] for every case, computed once."""
    global _EXPECTED
    if _EXPECTED is None:
        prepared, out = {}, []
        for ci, (ii, z, h, prm, step, rows) in enumerate(recipe_calls()):
            for b in range(rows):
                if (ii, prm, b) not in prepared:
                    prepared[(ii, prm, b)] = Prepared(z[b], h[b], *prm)
                p = prepared[(ii, prm, b)]
                tok, ds = p.draw(xorwow.curand_uniform(step, b))
                out.append((ci, b, tok, p.kept, p.cut_slack, ds, p.w))
        _EXPECTED = out
    return _EXPECTED
