"""Numpy restatement of the logit rules (csrc/logit_rules.hip, DESIGN.md "Logit rules") and of
the trie walk of constrained choice (the host side of the per-step allowed set).

For a raw row z (fp32) and id i, in this order, every step ONE np.float32 operation (IEEE
round-to-nearest, which is what the kernel's mul_rn / add_rn / sub_rn are: never an fma):
  1. v = z[i]; NaN -> -inf;
  2. bias b (None: none): if b[i] != 0, v = v + b[i]   (a zero of either sign leaves the bits);
  3. c = occurrences of i in the history; if c > 0 and a penalty is non-zero:
     t = frequency * float32(c); t = presence + t; v = v - t;
     a NaN that steps 2 and 3 produce (+inf meeting -inf) -> -inf, as in step 1;
  4. allowed bitmap (None: none): bit i & 31 of word i >> 5 clear -> v = -inf.
The id is the maximum of argmax_key(v[i], i): value descending (-0.0 below +0.0), ties to the
lower id; a row of only -inf gives id 0. Nothing here has a tolerance: the kernel's row and id
are these bits.
"""
import numpy as np

NEG_INF = np.float32(-np.inf)


def argmax_key(v, idx):
    """csrc/common.h argmax_key, over arrays: uint64 keys, larger = earlier in the order."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    neg = (b & np.uint64(0x80000000)) != 0
    b = np.where(neg, ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    return (b << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx, np.uint64))


def argmax(v) -> int:
    k = argmax_key(v, np.arange(len(v), dtype=np.uint64))
    return int(np.uint64(0xFFFFFFFF) - (k.max() & np.uint64(0xFFFFFFFF)))


def words_of(vocab: int, ids) -> np.ndarray:
    """The allowed bitmap of a list of ids, uint32 [(vocab + 31) // 32]."""
    w = np.zeros((vocab + 31) // 32, np.uint32)
    for i in ids:
        w[int(i) >> 5] |= np.uint32(1) << np.uint32(int(i) & 31)
    return w


def counts(vocab: int, history) -> np.ndarray:
    h = np.asarray(history, np.int64).reshape(-1)
    return np.bincount(h, minlength=vocab).astype(np.int64)


def process(z, bias=None, allowed=None, history=(), presence=0.0, frequency=0.0):
    """(processed row fp32 [vocab], argmax id)."""
    z = np.ascontiguousarray(z, np.float32)
    V = len(z)
    presence, frequency = np.float32(presence), np.float32(frequency)
    with np.errstate(invalid="ignore", over="ignore"):
        v = z.copy()
        v[np.isnan(v)] = NEG_INF
        if bias is not None:
            b = np.ascontiguousarray(bias, np.float32)
            m = b != 0
            v[m] = (v[m] + b[m]).astype(np.float32)
        if (presence != 0 or frequency != 0) and len(history):
            c = counts(V, history)
            m = c > 0
            t = (frequency * c[m].astype(np.float32)).astype(np.float32)
            t = (presence + t).astype(np.float32)
            v[m] = (v[m] - t).astype(np.float32)
        v[np.isnan(v)] = NEG_INF
        if allowed is not None:
            w = np.ascontiguousarray(allowed, np.uint32)
            i = np.arange(V)
            bit = (w[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)
            v[bit == 0] = NEG_INF
    return v, argmax(v)


# ------------------------------------------------------------------ the trie walk
def build_trie(choices) -> list:
    """Nodes {"next": {id: node}, "leaf": choice index or -1}, node 0 the root. ValueError for
    no choice, an empty choice, duplicates, and a choice that is a prefix of another."""
    if len(choices) == 0:
        raise ValueError("no choices")
    nodes = [{"next": {}, "leaf": -1}]
    for k, ch in enumerate(choices):
        ch = [int(t) for t in ch]
        if not ch:
            raise ValueError("an empty choice")
        at = 0
        for t in ch:
            if nodes[at]["leaf"] >= 0:
                raise ValueError("a choice is a prefix of another")
            if t not in nodes[at]["next"]:
                nodes[at]["next"][t] = len(nodes)
                nodes.append({"next": {}, "leaf": -1})
            at = nodes[at]["next"][t]
        if nodes[at]["leaf"] >= 0:
            raise ValueError("duplicate choices")
        if nodes[at]["next"]:
            raise ValueError("a choice is a prefix of another")
        nodes[at]["leaf"] = k
    return nodes


def walk(choices, pick):
    """The constrained-choice walk: from the root, pick(allowed ids, step) -> one of
    them, until a leaf. Returns (choice index, ids)."""
    nodes = build_trie(choices)
    at, ids = 0, []
    while nodes[at]["leaf"] < 0:
        kids = sorted(nodes[at]["next"])
        tok = int(pick(kids, len(ids)))
        assert tok in nodes[at]["next"], (tok, kids)
        ids.append(tok)
        at = nodes[at]["next"][tok]
    return nodes[at]["leaf"], ids
