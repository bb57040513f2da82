"""Python handle on the native decode engine (llmi_engine_* in include/llmi.h).

Mirrors the reference's model-level API (src/models/basemodel.h:14-42,
src/utils/model_utils.h:63-70): build a Llama with dummy (here: synthetic
PRNG) weights, feed a prompt, greedy-decode. All compute runs in
libllmi.so on the GPU; this class only moves ids/logits across the boundary.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import F16, F32, I8, Config, call


def preset(name: str, **overrides) -> Config:
    cfg = Config()
    call("llmi_config_preset", name.encode(), C.byref(cfg))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def tp_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    call("llmi_tp_unique_id", buf)
    return buf.raw


def synth_prompt(seed: int, n: int, vocab: int) -> np.ndarray:
    out = np.zeros(n, np.int32)
    call("llmi_synth_prompt", seed, n, vocab, out.ctypes.data)
    return out


def lookup_draft(ids, ngram_max: int = 3, ngram_min: int = 1, max_draft: int = 7) -> np.ndarray:
    """Prompt-lookup draft (llmi_lookup_draft, on the host): the ids that followed the most
    recent earlier occurrence of the sequence's longest matching suffix (ngram_max down to
    ngram_min ids), at most max_draft of them; empty when nothing matches."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    out = np.zeros(8, np.int32)
    n = C.c_int()
    call("llmi_lookup_draft", ids.ctypes.data, len(ids), int(ngram_max), int(ngram_min), int(max_draft),
         out.ctypes.data, C.byref(n))
    return out[:n.value].copy()


def _read_logprobs(fn: str, handle: tuple, n: int):
    """The records of llmi_engine_logprobs / llmi_batch_logprobs as numpy arrays."""
    valid, top = C.c_int(), C.c_int()
    call(fn, *handle, None, None, None, 0, C.byref(valid), C.byref(top))
    n, k = min(n, valid.value), top.value
    lp = np.zeros(n, np.float32)
    ids = np.zeros((n, k), np.int32)
    tlp = np.zeros((n, k), np.float32)
    call(fn, *handle, lp.ctypes.data, ids.ctypes.data if k else None, tlp.ctypes.data if k else None, n,
         C.byref(valid), C.byref(top))
    return lp, ids, tlp


def _bias_pairs(bias):
    """(ids int32 [n], values fp32 [n]) of a logit bias given as a dict {id: value} or as a dense
    array (its non-zero entries; a NaN entry is kept, for the library to refuse)."""
    if bias is None:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    if isinstance(bias, dict):
        ids = np.array([int(k) for k in bias], np.int32).reshape(-1)
        vals = np.array([float(bias[k]) for k in bias], np.float32).reshape(-1)
        return ids, vals
    dense = np.ascontiguousarray(bias, np.float32)
    if dense.ndim != 1:
        raise ValueError("bias: a dict {id: value} or a one-dimensional array")
    ids = np.flatnonzero(dense != 0).astype(np.int32)
    return ids, np.ascontiguousarray(dense[ids])


def _set_rules(fn: str, handle: tuple, bias, presence_penalty, frequency_penalty, count_prompt):
    ids, vals = _bias_pairs(bias)
    call(fn, *handle, ids.ctypes.data if len(ids) else None, vals.ctypes.data if len(ids) else None, len(ids),
         float(presence_penalty), float(frequency_penalty), 1 if count_prompt else 0)


def _set_allowed(fn: str, handle: tuple, ids):
    """Returns the set as the wrapper remembers it (None: no mask)."""
    if ids is None:
        call(fn, *handle, None, 0)
        return None
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    if len(ids) == 0:
        raise ValueError("set_allowed: an empty allowed set (None removes the mask)")
    call(fn, *handle, ids.ctypes.data, len(ids))
    return ids.copy()


def choice_trie(choices) -> list:
    """The trie of constrained choice over token-id sequences: nodes {"next": {id: node},
    "leaf": choice index or -1}, node 0 the root. ValueError for no choice, an empty choice,
    duplicates, and a choice that is a prefix of another (the walk could not tell them apart)."""
    if len(choices) == 0:
        raise ValueError("choose: no choices")
    nodes = [{"next": {}, "leaf": -1}]
    for k, ch in enumerate(choices):
        ch = [int(t) for t in ch]
        if not ch:
            raise ValueError("choose: an empty choice")
        at = 0
        for t in ch:
            if nodes[at]["leaf"] >= 0:
                raise ValueError("choose: a choice is a prefix of another")
            if t not in nodes[at]["next"]:
                nodes[at]["next"][t] = len(nodes)
                nodes.append({"next": {}, "leaf": -1})
            at = nodes[at]["next"][t]
        if nodes[at]["leaf"] >= 0:
            raise ValueError("choose: duplicate choices")
        if nodes[at]["next"]:
            raise ValueError("choose: a choice is a prefix of another")
        nodes[at]["leaf"] = k
    return nodes


class Engine:
    def __init__(self, cfg: Config, device: int = 0, tp_id: Optional[bytes] = None):
        self.cfg = cfg
        h = C.c_void_p()
        idbuf = C.create_string_buffer(tp_id, 128) if tp_id else None
        call("llmi_engine_create", C.byref(cfg), device, idbuf, C.byref(h))
        self._h = h
        self._lp_top = -1
        self._allowed = None  # the allowed set as last given to set_allowed (None: no mask)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().llmi_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ api
    def load_synthetic(self, seed: int):
        call("llmi_engine_load_synthetic", self._h, seed)

    def set_sampling(self, k: int, seed: int = 0):
        """Top-k stochastic sampling in the decode step (k = 0: greedy, the default)."""
        call("llmi_engine_set_sampling", self._h, int(k), int(seed))

    def set_sampling_params(self, top_k: int = 0, top_p: float = 1.0, temperature: float = 1.0,
                            repetition_penalty: float = 1.0, seed: int = 0):
        """Temperature / top-k / top-p / repetition-penalty sampling in the token step
        (llmi_engine_set_sampling_params; top_k = 0: no limit). Replaces set_sampling's
        sampler; set_sampling (any k) replaces this one."""
        p = _lib.SamplingParams(int(top_k), float(top_p), float(temperature), float(repetition_penalty), int(seed))
        call("llmi_engine_set_sampling_params", self._h, C.byref(p))

    def set_logprobs(self, n_top: int):
        """Per-token log-probabilities in the token step (llmi_engine_set_logprobs): -1 off (the
        default), 0 the chosen token's logprob, 1..8 also that many alternatives. They are those
        of the raw logits (no penalty, no temperature), whatever sampler is set."""
        call("llmi_engine_set_logprobs", self._h, int(n_top))
        self._lp_top = int(n_top)

    def logprobs(self, n: Optional[int] = None):
        """(tok_lp [n], top_ids [n, n_top], top_lp [n, n_top]) of the first n records (None: all
        that exist). Record p holds the logprob of the sequence's token at position p under the
        forward at p - 1; NaN / id -1 = not computed (record 0, and prompt rows a batched prefill
        consumed)."""
        return _read_logprobs("llmi_engine_logprobs", (self._h,), self.cfg.max_seq + 1 if n is None else int(n))

    def set_logit_rules(self, bias=None, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                        count_prompt: bool = False):
        """Logit rules in the token step (llmi_engine_set_logit_rules), applied to every row before
        the sampler (or the greedy argmax) reads it: bias, a dict {id: value} or a dense array
        (value -inf bans the id); presence / frequency penalties over the ids generated so far
        (count_prompt: the prompt's too). Replaces the bias and penalties set before and leaves
        the allowed set alone; all defaults = none of the three."""
        _set_rules("llmi_engine_set_logit_rules", (self._h,), bias, presence_penalty, frequency_penalty, count_prompt)

    def set_allowed(self, ids):
        """Only these ids may be chosen (llmi_engine_set_allowed); None removes the mask. Cheap
        to change between steps: a replayed graph keeps working."""
        self._allowed = _set_allowed("llmi_engine_set_allowed", (self._h,), ids)

    def clear_logit_rules(self):
        """Remove bias, penalties and the allowed set (llmi_engine_clear_logit_rules)."""
        call("llmi_engine_clear_logit_rules", self._h)
        self._allowed = None

    def processed_logits(self) -> np.ndarray:
        """The row the last step chose from, after the rules (llmi_engine_processed_logits)."""
        out = np.zeros(self.cfg.vocab, np.float32)
        call("llmi_engine_processed_logits", self._h, out.ctypes.data, self.cfg.vocab)
        return out

    def choose(self, prompt, choices, use_graph: bool = True):
        """Constrained choice: after `prompt`, generate exactly one of `choices` (token-id
        sequences), each token picked by the engine (its rules and sampler included) among the
        ids that keep a choice reachable. Returns (index of the choice, its ids). Walks the trie
        of the choices: set_allowed(children) before the step that picks the next token, one
        decode step, read the token. The allowed set in force before the call is restored."""
        nodes = choice_trie(choices)
        prompt = np.ascontiguousarray(prompt, dtype=np.int32).reshape(-1)
        before = self._allowed
        try:
            self.set_prompt(prompt)
            if len(prompt) > 1:
                self.decode(len(prompt) - 1, use_graph)  # (their picks are the prompt's: no mask needed)
            at, ids = 0, []
            while nodes[at]["leaf"] < 0:
                self.set_allowed(sorted(nodes[at]["next"]))
                self.decode(1, use_graph)
                p = len(prompt) + len(ids)
                tok = int(self.tokens(p + 1)[p])
                if tok not in nodes[at]["next"]:
                    raise _lib.LlmiError(f"choose: the engine picked id {tok} outside the allowed set")
                ids.append(tok)
                at = nodes[at]["next"][tok]
            return nodes[at]["leaf"], ids
        finally:
            self.set_allowed(before)

    def score(self, ids, use_graph: bool = True, prefill: bool = False, exact=True) -> np.ndarray:
        """Log-likelihood of a given text: logprob of ids[p] given ids[:p] for p = 1 .. len - 1
        (fp32 [len - 1]; their negated mean is the log-perplexity). Steps the text through
        len - 1 decode steps, or -- prefill=True -- runs it as one scored prefill of len - 1
        rows (no token step; `exact` as in prefill); turns logprobs on (n_top 0) for the call
        if they are off."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        was = self._lp_top
        if was < 0:
            self.set_logprobs(0)
        try:
            self.set_prompt(ids)
            if prefill:
                if len(ids) > 1:
                    self.prefill(len(ids) - 1, exact, score=True)
            else:
                self.decode(len(ids) - 1, use_graph)
            return self.logprobs(len(ids))[0][1:]
        finally:
            if was < 0:
                self.set_logprobs(-1)

    def load_bin(self, weight_path: str, quantize: bool = False):
        """Llama<T>::loadWeights(weight_path): weight_path + "<name>.bin" raw fp32 files
        (llmi/convert.py writes them); the path is used as a prefix, like the reference's.
        quantize (int8 engines, which take the files no other way): the linear weights are
        quantised to W8A16 on the device (llmi_engine_load_bin_quantized)."""
        call("llmi_engine_load_bin_quantized" if quantize else "llmi_engine_load_bin", self._h,
             weight_path.encode())

    def load_tensor(self, name: str, values: np.ndarray, quantize: bool = False):
        v = np.ascontiguousarray(values, dtype=np.float32)
        call("llmi_engine_load_tensor_quantized" if quantize else "llmi_engine_load_tensor", self._h,
             name.encode(), v.ctypes.data, v.size)

    def set_prompt(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        call("llmi_engine_set_prompt", self._h, ids.ctypes.data, len(ids))

    def decode(self, n_steps: int, use_graph: bool = True):
        call("llmi_engine_decode", self._h, n_steps, 1 if use_graph else 0)

    def prefill(self, n_tokens: int, exact=True, score: bool = False):
        """exact: True / 1 fp32-faithful (two fp16 planes), 2 fp16 hi + e4m3 lo planes on
        the fp8 MFMA (~1e-4), False / 0 fp16 activations (llmi_engine_prefill). score: also
        fill the logprob records of the rows consumed (llmi_engine_prefill_scored; needs
        set_logprobs); everything else is bitwise the unscored call's."""
        mode = int(exact)
        if mode not in (0, 1, 2):
            raise ValueError("prefill: exact must be False/0, True/1 or 2")
        call("llmi_engine_prefill_scored" if score else "llmi_engine_prefill", self._h, n_tokens, mode)

    def scored_logits(self, pos: int) -> np.ndarray:
        """Test / debug: the fp32 logits row of prompt position pos as the last scored prefill
        chunk's lm_head GEMM left it (llmi_engine_scored_logits)."""
        out = np.zeros(self.cfg.vocab, np.float32)
        call("llmi_engine_scored_logits", self._h, int(pos), out.ctypes.data, self.cfg.vocab)
        return out

    def sync(self):
        call("llmi_engine_sync", self._h)

    def tokens(self, n: Optional[int] = None) -> np.ndarray:
        n = self.cfg.max_seq + 1 if n is None else n
        out = np.zeros(n, np.int32)
        valid = C.c_int()
        call("llmi_engine_tokens", self._h, out.ctypes.data, n, C.byref(valid))
        return out[:min(n, valid.value)]

    def logits(self) -> np.ndarray:
        n = self.cfg.vocab // self.cfg.tp_world
        out = np.zeros(n, np.float32)
        call("llmi_engine_logits", self._h, out.ctypes.data, n)
        return out

    def hidden(self) -> np.ndarray:
        out = np.zeros(self.cfg.hidden, np.float32)
        call("llmi_engine_hidden", self._h, out.ctypes.data, self.cfg.hidden)
        return out

    def kv_slot(self, layer: int, pos: int, which_v: bool = False) -> np.ndarray:
        kvl = self.cfg.kv_heads // self.cfg.tp_world
        out = np.zeros((kvl, self.cfg.head_dim), np.float32)
        call("llmi_engine_kv_slot", self._h, layer, pos, 1 if which_v else 0, out.ctypes.data)
        return out

    def kv_slot_q8(self, layer: int, pos: int, which_v: bool = False):
        """An int8 cache's slot as stored: (q [kv_heads, head_dim] int8, scale bits [kv_heads] uint16)."""
        kvl = self.cfg.kv_heads // self.cfg.tp_world
        q = np.zeros((kvl, self.cfg.head_dim), np.int8)
        s = np.zeros(kvl, np.uint16)
        call("llmi_engine_kv_slot_q8", self._h, layer, pos, 1 if which_v else 0, q.ctypes.data, s.ctypes.data)
        return q, s

    def bytes_per_token(self):
        w, kv = C.c_uint64(), C.c_uint64()
        call("llmi_engine_bytes", self._h, C.byref(w), C.byref(kv))
        return w.value, kv.value

    def debug_set_next_pos(self, next_pos: int):
        """Test hook: move the device decode state's next position only (not the host's)."""
        call("llmi_engine_debug_set_next_pos", self._h, int(next_pos))

    def stream(self) -> int:
        return _lib.lib().llmi_engine_stream(self._h) or 0

    # allreduce / allreduce_graph: one residual all-reduce of the TP exchange (needs a tp_id),
    # launched eagerly / replayed from a captured graph of `iters` calls
    KERNELS = {"qkv": 0, "attn": 1, "o": 2, "gate_up": 3, "down": 4, "lm_head": 5, "allreduce": 6,
               "allreduce_graph": 7, "xchg": 8, "xchg_graph": 9, "ring": 10, "qkv_attn": 11}

    # one-shot peer exchange (tensor parallel without RCCL in the token graph)
    def xchg_handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        call("llmi_engine_xchg_handle", self._h, buf)
        return buf.raw

    def xchg_open(self, handles):
        """handles: every rank's 64-byte inbox handle, in rank order."""
        blob = b"".join(bytes(h) for h in handles)
        assert len(blob) == 64 * self.cfg.tp_world
        buf = C.create_string_buffer(blob, len(blob))
        call("llmi_engine_xchg_open", self._h, buf)

    def set_option(self, name: str, value: int):
        """llmi_engine_set_option: tuning switches for same-process A/B ("kpar": 0 / 1)."""
        call("llmi_engine_set_option", self._h, name.encode(), int(value))

    def xchg_loopback(self):
        """Price ONE tensor-parallel rank on one GPU (llmi_engine_xchg_loopback): every peer
        inbox is this rank's own; the timing and launch structure are a rank's, the tokens
        are not the TP model's. Then set_exchange(0 | 1 | 2)."""
        call("llmi_engine_xchg_loopback", self._h)

    def set_exchange(self, mode: int):
        """0: RCCL all-reduces (needs a tp_id at create); 1: the one-shot peer exchange;
        2: the same exchange fused into the producing launches (o_proj / down / lm_head)."""
        call("llmi_engine_set_exchange", self._h, int(mode))

    def set_decode_mode(self, mode: int):
        """0: five launches per layer; 1: the persistent ring layer (ring.hip: attention +
        one launch per layer). Raises LlmiError where mode 1 is unsupported."""
        call("llmi_engine_set_decode_mode", self._h, int(mode))

    def time_kernel(self, which: str, iters: int = 50):
        us, b = C.c_float(), C.c_uint64()
        call("llmi_engine_time_kernel", self._h, self.KERNELS[which], iters, C.byref(us), C.byref(b))
        return us.value, b.value

    def set_speculation(self, max_draft: int):
        """Speculative decoding (llmi_engine_set_speculation): allocate lanes for up to max_draft
        (0..7) proposed tokens per verify step; 0 turns it off. Raises LlmiError where the
        configuration has no verify step (TP, int4 weights, an int8 KV cache, the ring mode, a
        sampler, logprobs)."""
        call("llmi_engine_set_speculation", self._h, int(max_draft))

    def verify(self, draft, use_graph: bool = True) -> int:
        """One verify step (llmi_engine_verify): the pending token and the proposed continuation
        `draft` run through the model in one pass; returns how many draft ids were accepted (a).
        The engine is then exactly where a + 1 decode steps would have left it."""
        d = np.ascontiguousarray(draft, dtype=np.int32)
        a = C.c_int()
        call("llmi_engine_verify", self._h, d.ctypes.data if len(d) else None, len(d), 1 if use_graph else 0,
             C.byref(a))
        return a.value

    def generate_lookup(self, n_steps: int, max_draft: int, ngram=(3, 1), use_graph: bool = True):
        """llmi_engine_generate_lookup: advance exactly n_steps positions with prompt-lookup drafts
        (ngram = (max, min) suffix lengths); returns the counts (llmi_spec_stats: verify_steps,
        drafted, accepted)."""
        st = _lib.SpecStats()
        call("llmi_engine_generate_lookup", self._h, int(n_steps), int(max_draft), int(ngram[0]), int(ngram[1]),
             1 if use_graph else 0, C.byref(st))
        return st

    def generate_draft(self, draft: "Engine", n_steps: int, max_draft: int, prefill: bool = False,
                       use_graph: bool = True):
        """llmi_engine_generate_draft: advance exactly n_steps positions with the engine `draft`
        proposing up to max_draft ids a verify step (prefill: the draft catches up on the sequence
        so far through its prefill where it has one); the tokens are plain greedy decode's bit for
        bit whatever the draft proposes. Returns the counts (llmi_spec_stats)."""
        st = _lib.SpecStats()
        call("llmi_engine_generate_draft", self._h, draft._h, int(n_steps), int(max_draft), 1 if prefill else 0,
             1 if use_graph else 0, C.byref(st))
        return st

    def edit(self, keep: int, ids):
        """llmi_engine_edit: keep positions 0 .. keep - 1, forget the pending token and everything
        after them, and force `ids` on the positions that follow (as a prompt would)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        call("llmi_engine_edit", self._h, int(keep), ids.ctypes.data if len(ids) else None, len(ids))

    def position(self):
        """(next position, prompt length) as the host tracks them (llmi_engine_position; no sync)."""
        p, n = C.c_int(), C.c_int()
        call("llmi_engine_position", self._h, C.byref(p), C.byref(n))
        return p.value, n.value

    def extend(self, ids):
        """Append `ids` after the whole text so far (the pending token included): a new turn
        without feeding the history again. edit(P, [pending] + ids); needs the prompt consumed."""
        p, n = self.position()
        if n == 0 or p < n:
            raise _lib.LlmiError("extend: the prompt is not consumed yet (decode or prefill it first)")
        pending = self.tokens(p + 1)[p:]
        self.edit(p, np.concatenate([pending, np.asarray(ids, np.int32).reshape(-1)]))

    def generate(self, prompt, n_new: int, use_graph: bool = True, prefill: bool = False,
                 exact: bool = True, speculate: int = 0, ngram=(3, 1), draft: Optional["Engine"] = None) -> np.ndarray:
        """Greedy: feed the prompt, produce n_new tokens (Llama<T>::Response).
        prefill=True runs the prompt as one batched pass (firstTokenGen). speculate=k (1..7):
        after the prompt, the n_new - 1 steps run as verify steps over prompt-lookup drafts of
        up to k ids, or -- draft=another Engine -- over that engine's proposals (the same
        tokens, bit for bit); the counts are left in self.spec_stats."""
        prompt = np.asarray(prompt, np.int32)
        self.set_prompt(prompt)
        if speculate:
            self.set_speculation(speculate)
            if prefill:
                self.prefill(len(prompt), exact)
            else:
                self.decode(len(prompt), use_graph)
            if draft is not None:
                self.spec_stats = self.generate_draft(draft, n_new - 1, speculate, prefill, use_graph)
            else:
                self.spec_stats = self.generate_lookup(n_new - 1, speculate, ngram, use_graph)
            return self.tokens(len(prompt) + n_new)[len(prompt):]
        if prefill:
            self.prefill(len(prompt), exact)
            self.decode(n_new - 1, use_graph)
        else:
            self.decode(len(prompt) + n_new - 1, use_graph)
        toks = self.tokens(len(prompt) + n_new)
        return toks[len(prompt):]


class TPGroup:
    """In-process tensor-parallel group (llmi_group_* in include/llmi.h): `world`
    rank engines on one device, stepped together, reductions by a kernel in
    place of RCCL. The single-GPU parity harness for the sharded decode path."""

    def __init__(self, cfg: Config, world: int, device: int = 0):
        self.cfg, self.world = cfg, world
        h = C.c_void_p()
        call("llmi_group_create", C.byref(cfg), world, device, C.byref(h))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().llmi_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_synthetic(self, seed: int):
        call("llmi_group_load_synthetic", self._h, seed)

    def load_bin(self, weight_path: str, quantize: bool = False):
        call("llmi_group_load_bin_quantized" if quantize else "llmi_group_load_bin", self._h,
             weight_path.encode())

    def tokens(self, rank: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.cfg.max_seq + 1 if n is None else n
        out = np.zeros(n, np.int32)
        valid = C.c_int()
        call("llmi_group_tokens", self._h, rank, out.ctypes.data, n, C.byref(valid))
        return out[:min(n, valid.value)]

    def logits(self) -> np.ndarray:
        out = np.zeros(self.cfg.vocab, np.float32)
        call("llmi_group_logits", self._h, out.ctypes.data, self.cfg.vocab)
        return out

    def hidden(self, rank: int = 0) -> np.ndarray:
        out = np.zeros(self.cfg.hidden, np.float32)
        call("llmi_group_hidden", self._h, rank, out.ctypes.data, self.cfg.hidden)
        return out

    def set_exchange(self, mode: int):
        """0: in-place reduction kernel; 1: the one-shot peer exchange kernels; 2: the push
        fused into every rank's producing launches, then the reduce kernels."""
        call("llmi_group_set_exchange", self._h, int(mode))

    def generate(self, prompt, n_new: int, use_graph: bool = True) -> np.ndarray:
        prompt = np.ascontiguousarray(prompt, np.int32)
        call("llmi_group_set_prompt", self._h, prompt.ctypes.data, len(prompt))
        call("llmi_group_decode", self._h, len(prompt) + n_new - 1, 1 if use_graph else 0)
        return self.tokens(0, len(prompt) + n_new)[len(prompt):]


class Batch:
    """Batched decode (llmi_batch_* in include/llmi.h): up to 8 sequence slots over one copy
    of the weights, stepped together -- every weight but W_o is streamed once per step for all
    active slots. A slot's tokens and logits are bitwise those of an Engine decoding the same
    sequence alone. Admission and eviction are the caller's (set_prompt / reset)."""

    def __init__(self, cfg: Config, n_seq: int, device: int = 0):
        self.cfg, self.n_seq = cfg, n_seq
        h = C.c_void_p()
        call("llmi_batch_create", C.byref(cfg), n_seq, device, C.byref(h))
        self._h = h
        self._lp_top = [-1] * n_seq
        self._plen = [0] * n_seq  # each slot's prompt length (0: idle) and next position
        self._pos = [0] * n_seq

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().llmi_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_synthetic(self, seed: int):
        call("llmi_batch_load_synthetic", self._h, seed)

    def load_bin(self, weight_path: str, quantize: bool = False):
        call("llmi_batch_load_bin_quantized" if quantize else "llmi_batch_load_bin", self._h,
             weight_path.encode())

    def set_prompt(self, seq: int, ids):
        """(Re)start slot seq with this prompt; the other slots are left where they are."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        call("llmi_batch_set_prompt", self._h, int(seq), ids.ctypes.data, len(ids))
        self._plen[int(seq)], self._pos[int(seq)] = len(ids), 0

    def reset(self, seq: int):
        """Make slot seq idle (its buffers keep their contents)."""
        call("llmi_batch_reset", self._h, int(seq))
        self._plen[int(seq)], self._pos[int(seq)] = 0, 0

    def edit(self, seq: int, keep: int, ids):
        """Engine.edit for one slot (llmi_batch_edit); the other slots are left where they are."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        call("llmi_batch_edit", self._h, int(seq), int(keep), ids.ctypes.data if len(ids) else None, len(ids))
        if len(ids):
            self._plen[int(seq)], self._pos[int(seq)] = int(keep) + len(ids), int(keep)

    def fork(self, src: int, dst, keep: Optional[int] = None, ids=()):
        """Copy slot src's sequence into the slot(s) dst (an int or up to 7 ints) on the device, in
        stream order (llmi_batch_fork): the cache rows, the ids and the decode state. With ids,
        every destination becomes what src would be after edit(src, keep, ids) -- the first keep
        positions kept (None: all consumed ones), the pending token forgotten, ids forced next.
        Without ids (keep None or src's position) it becomes src as it stands, pending token
        included. A destination keeps its own sampler, seed, logit rules and logprob setting;
        src is left as it is."""
        src = int(src)
        dst = [int(dst)] if isinstance(dst, (int, np.integer)) else [int(d) for d in dst]
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        to = (C.c_int * max(len(dst), 1))(*dst)
        call("llmi_batch_fork", self._h, src, to, len(dst), -1 if keep is None else int(keep),
             ids.ctypes.data if len(ids) else None, len(ids))
        pos = self._pos[src] if keep is None else int(keep)
        for d in dst:
            self._plen[d] = pos + len(ids) if len(ids) else self._plen[src]
            self._pos[d] = pos

    def sample(self, prompt, n: int, n_new: int, seeds=None, prefill: bool = True, use_graph: bool = True,
               **sampling_params):
        """n <= n_seq continuations of n_new tokens of one prompt for one prompt pass: every slot
        is reset, slot i gets set_sampling_params(seed=seeds[i], **sampling_params) (seeds default
        to the `seed` keyword + 0 .. n - 1), slot 0 consumes all but the last prompt row (one
        prefill, or decode steps with prefill=False) and is forked into slots 1 .. n - 1, and the
        n slots decode together from the last prompt position, so each continuation is bitwise
        that of an Engine alone with that seed. Returns the n id arrays; where the n slots have
        logprobs on, (ids, sums) with each continuation's summed token logprob (fp64 sum of the
        fp32 records) for a best-of-n pick. The samplers stay set and the slots active."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32).reshape(-1)
        n, n_new, plen = int(n), int(n_new), len(prompt)
        if not 1 <= n <= self.n_seq:
            raise ValueError("sample: n must be in [1, n_seq]")
        if plen < 1 or n_new < 1:
            raise ValueError("sample: an empty prompt, or n_new < 1")
        seed = int(sampling_params.pop("seed", 0))
        seeds = [seed + i for i in range(n)] if seeds is None else [int(s) for s in seeds]
        if len(seeds) != n:
            raise ValueError("sample: one seed per continuation")
        for i in range(self.n_seq):
            self.reset(i)
        for i in range(n):
            self.set_sampling_params(i, seed=seeds[i], **sampling_params)
        self.set_prompt(0, prompt)
        if plen > 1 and prefill:
            self.prefill(0, plen - 1)
        elif plen > 1:
            self.decode(plen - 1, use_graph)
        if n > 1:
            self.fork(0, range(1, n), keep=plen - 1, ids=prompt[-1:])
        self.decode(n_new, use_graph)
        out = [self.tokens(i, plen + n_new)[plen:] for i in range(n)]
        if any(self._lp_top[i] < 0 for i in range(n)):
            return out
        sums = np.array([np.sum(self.logprobs(i, plen + n_new)[0][plen:], dtype=np.float64) for i in range(n)])
        return out, sums

    def prefill(self, seq: int, n: Optional[int] = None, exact=True, score: bool = False):
        """Engine.prefill for one slot (llmi_batch_prefill): its next n prompt rows (None: the
        rest of its prompt) in one batched pass on the batch's stream; the other slots are
        untouched, and the next decode steps the slot with them. score: Engine.prefill's."""
        seq, mode = int(seq), int(exact)
        if mode not in (0, 1, 2):
            raise ValueError("prefill: exact must be False/0, True/1 or 2")
        if n is None and 0 <= seq < self.n_seq:
            n = self._plen[seq] - self._pos[seq]
        call("llmi_batch_prefill", self._h, seq, int(n or 0), mode, 1 if score else 0)
        self._pos[seq] += int(n)

    def set_sampling_params(self, seq: int, top_k: int = 0, top_p: float = 1.0, temperature: float = 1.0,
                            repetition_penalty: float = 1.0, seed: int = 0):
        p = _lib.SamplingParams(int(top_k), float(top_p), float(temperature), float(repetition_penalty), int(seed))
        call("llmi_batch_set_sampling_params", self._h, int(seq), C.byref(p))

    def set_logit_rules(self, seq: int, bias=None, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                        count_prompt: bool = False):
        """Engine.set_logit_rules for one slot (the rules and the processed row are the slot's own)."""
        _set_rules("llmi_batch_set_logit_rules", (self._h, int(seq)), bias, presence_penalty, frequency_penalty,
                   count_prompt)

    def set_allowed(self, seq: int, ids):
        """Engine.set_allowed for one slot; replacing a set's contents keeps the captured steps."""
        _set_allowed("llmi_batch_set_allowed", (self._h, int(seq)), ids)

    def clear_logit_rules(self, seq: int):
        call("llmi_batch_clear_logit_rules", self._h, int(seq))

    def processed_logits(self, seq: int) -> np.ndarray:
        out = np.zeros(self.cfg.vocab, np.float32)
        call("llmi_batch_processed_logits", self._h, int(seq), out.ctypes.data, self.cfg.vocab)
        return out

    def set_logprobs(self, seq: int, n_top: int):
        """Engine.set_logprobs for one slot (the setting and the records are the slot's own)."""
        call("llmi_batch_set_logprobs", self._h, int(seq), int(n_top))
        self._lp_top[int(seq)] = int(n_top)

    def logprobs(self, seq: int, n: Optional[int] = None):
        """Engine.logprobs for one slot (before the slot is reset: an idle slot has no records)."""
        return _read_logprobs("llmi_batch_logprobs", (self._h, int(seq)),
                              self.cfg.max_seq + 1 if n is None else int(n))

    def score(self, texts, use_graph: bool = True, prefill: bool = False) -> list:
        """Engine.score over up to n_seq texts of different lengths at once: slot i steps
        texts[i] (None: idle) and goes idle when its text ends; prefill=True: one scored slot
        prefill per text instead (bitwise Engine.score(t, prefill=True)). Returns one fp32
        [len - 1] array per text. Slots with logprobs off have them on (n_top 0) for the call."""
        if len(texts) > self.n_seq:
            raise ValueError("score: more texts than slots")
        was = list(self._lp_top)
        left, out = {}, [None] * len(texts)
        try:
            for i in range(self.n_seq):
                self.reset(i)
            for i, t in enumerate(texts):
                if t is None:
                    continue
                t = np.ascontiguousarray(t, np.int32)
                if was[i] < 0:
                    self.set_logprobs(i, 0)
                self.set_prompt(i, t)
                if prefill:
                    if len(t) > 1:
                        self.prefill(i, len(t) - 1, score=True)
                    out[i] = self.logprobs(i, len(t))[0][1:]
                    self.reset(i)
                    continue
                left[i] = len(t) - 1
            while left:
                n = min(left.values())
                self.decode(n, use_graph)
                for i in list(left):
                    left[i] -= n
                    if left[i] == 0:
                        out[i] = self.logprobs(i, len(texts[i]))[0][1:]
                        self.reset(i)
                        del left[i]
        finally:
            for i in range(len(texts)):
                if was[i] < 0 and self._lp_top[i] >= 0:
                    self.set_logprobs(i, -1)
        return out

    def decode(self, n_steps: int, use_graph: bool = True):
        """Every active slot advances n_steps tokens."""
        call("llmi_batch_decode", self._h, int(n_steps), 1 if use_graph else 0)
        for i in range(self.n_seq):
            if self._plen[i] > 0:
                self._pos[i] += int(n_steps)

    def sync(self):
        call("llmi_batch_sync", self._h)

    def tokens(self, seq: int, n: Optional[int] = None) -> np.ndarray:
        n = self.cfg.max_seq + 1 if n is None else n
        out = np.zeros(n, np.int32)
        valid = C.c_int()
        call("llmi_batch_tokens", self._h, int(seq), out.ctypes.data, n, C.byref(valid))
        return out[:min(n, valid.value)]

    def logits(self, seq: int) -> np.ndarray:
        out = np.zeros(self.cfg.vocab, np.float32)
        call("llmi_batch_logits", self._h, int(seq), out.ctypes.data, self.cfg.vocab)
        return out

    def bytes_per_step(self):
        """(weight bytes one step over the active slots streams, KV bytes per position and slot)."""
        w, kv = C.c_uint64(), C.c_uint64()
        call("llmi_batch_bytes", self._h, C.byref(w), C.byref(kv))
        return w.value, kv.value

    def generate(self, prompts, n_new: int, use_graph: bool = True, prefill: bool = False) -> list:
        """Greedy (or each slot's sampler): slot i takes prompts[i] (None: idle) and produces
        n_new tokens; prompts are consumed by decode steps, or -- prefill=True -- by one slot
        prefill each. A slot that has its n_new tokens goes idle while longer prompts finish.
        Returns one id array per slot (None: idle)."""
        if len(prompts) > self.n_seq:
            raise ValueError("generate: more prompts than slots")
        left, out = {}, [None] * len(prompts)
        for i in range(self.n_seq):
            self.reset(i)
        for i, p in enumerate(prompts):
            if p is None:
                continue
            p = np.ascontiguousarray(p, np.int32)
            self.set_prompt(i, p)
            if prefill:
                self.prefill(i)
            left[i] = (0 if prefill else len(p)) + n_new - 1
        plen = {i: len(prompts[i]) for i in left}
        while left:
            n = min(left.values())
            self.decode(n, use_graph)
            for i in list(left):
                left[i] -= n
                if left[i] == 0:
                    out[i] = self.tokens(i, plen[i] + n_new)[plen[i]:]
                    self.reset(i)
                    del left[i]
        return out
