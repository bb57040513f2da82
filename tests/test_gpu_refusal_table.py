"""Which engine mode refuses which (the table behind Engine::refuse in engine.hip): for every
refused (mode that is on, setter called) pair the return code, the pinned part of the message, and
that the refused call changed nothing -- the engine decodes on bitwise like a twin that never
made the call.

The pairs held in full by other tests are not repeated here: the logit rules against
speculation, the ring mode and tensor-parallel ranks, both ways round (test_gpu_engine_rules.py);
set_sampling_params and set_logprobs on a tensor-parallel rank (test_gpu_engine_nucleus.py,
test_gpu_engine_logprobs.py); int4 weights against a batch, a group and the ring mode
(test_gpu_engine_i4.py); a tensor-parallel batch (test_gpu_batch.py). test_gpu_spec_verify.py
checks the return codes of the speculation pairs; their messages and what they leave are here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607
EINVAL, EUNSUPPORTED = -1, -2


def _tiny(**over):
    from llmi.engine import preset
    return preset("tiny", **over)


def _ring_width():
    from llmi.engine import preset
    return preset("llama2-7b", layers=2, max_seq=64)  # the smallest engine the ring layer runs on


def _i4():
    from llmi import _lib
    return _tiny(weight_dtype=_lib.I4)


def _kv8():
    from llmi import _lib
    return _tiny(kv_dtype=_lib.I8)


def _tp_rank():
    return _tiny(tp_rank=0, tp_world=2)


def _loopback(e):
    e.xchg_loopback()  # one rank alone can decode (every peer inbox its own)


def _spec_on(e):
    e.set_speculation(3)


def _nucleus(L, e):
    from llmi import _lib
    p = _lib.SamplingParams(0, 0.9, 0.8, 1.0, 0)
    return L.llmi_engine_set_sampling_params(e._h, C.byref(p))


def _speculation(L, e):
    return L.llmi_engine_set_speculation(e._h, 3)


# (id, config, what turns the refusing mode on, the refused call, its code, the message)
CASES = [
    ("tp_rank-set_sampling", _tp_rank, _loopback, lambda L, e: L.llmi_engine_set_sampling(e._h, 4, 1), EINVAL,
     "set_sampling: sampling needs the full logits (tp_world 1)"),
    ("speculation-set_sampling", _tiny, _spec_on, lambda L, e: L.llmi_engine_set_sampling(e._h, 4, 1), EUNSUPPORTED,
     "set_sampling: speculation is on (greedy only; set_speculation 0 first)"),
    ("speculation-set_sampling_params", _tiny, _spec_on, _nucleus, EUNSUPPORTED,
     "set_sampling_params: speculation is on (greedy only; set_speculation 0 first)"),
    ("speculation-set_logprobs", _tiny, _spec_on, lambda L, e: L.llmi_engine_set_logprobs(e._h, 0), EUNSUPPORTED,
     "set_logprobs: speculation is on (the verify step records none; set_speculation 0 first)"),
    ("speculation-set_decode_mode", _tiny, _spec_on, lambda L, e: L.llmi_engine_set_decode_mode(e._h, 1),
     EUNSUPPORTED, "set_decode_mode: speculation is on (the ring layer has no verify step)"),
    ("tp_rank-set_speculation", _tp_rank, _loopback, _speculation, EUNSUPPORTED,
     "set_speculation: tensor-parallel ranks and group ranks are not built (tp_world must be 1)"),
    ("int4-set_speculation", _i4, None, _speculation, EUNSUPPORTED,
     "set_speculation: int4 weights are not built into the multi-row GEMV"),
    ("kv8-set_speculation", _kv8, None, _speculation, EUNSUPPORTED,
     "set_speculation: an int8 KV cache is not built into the multi-row attention"),
    ("ring-set_speculation", _ring_width, lambda e: e.set_decode_mode(1), _speculation, EUNSUPPORTED,
     "set_speculation: the ring decode mode has no verify step (set_decode_mode 0)"),
    ("top_k-set_speculation", _tiny, lambda e: e.set_sampling(4, 1), _speculation, EUNSUPPORTED,
     "set_speculation: a sampler is active (speculative sampling is not built; greedy only)"),
    ("nucleus-set_speculation", _tiny, lambda e: e.set_sampling_params(top_p=0.9, temperature=0.8), _speculation,
     EUNSUPPORTED, "set_speculation: a sampler is active (speculative sampling is not built; greedy only)"),
    ("logprobs-set_speculation", _tiny, lambda e: e.set_logprobs(2), _speculation, EUNSUPPORTED,
     "set_speculation: logprobs are on (the verify step records none)"),
]


def _run(cfg, turn_on, refused=None):
    """(tokens, logits bits) of 3 + 5 decode steps, with the refused call (if any) in between."""
    from llmi import _lib
    from llmi.engine import Engine, synth_prompt
    L = _lib.lib()
    prompt = synth_prompt(1000, 3, cfg.vocab)
    with Engine(cfg) as e:
        e.load_synthetic(SEED)
        if turn_on:
            turn_on(e)
        e.set_prompt(prompt)
        e.decode(3)
        rc, msg = (refused(L, e), L.llmi_last_error().decode()) if refused else (None, "")
        e.decode(5)
        return e.tokens(9).copy(), np.ascontiguousarray(e.logits(), np.float32).view(np.uint32).copy(), rc, msg


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refused_call_reports_and_changes_nothing(case):
    _, make_cfg, turn_on, refused, code, text = case
    toks, logits, rc, msg = _run(make_cfg(), turn_on, refused)
    assert rc == code, (rc, msg)
    assert msg.startswith("[llmi][ERROR] " + text), msg
    twin_toks, twin_logits, _, _ = _run(make_cfg(), turn_on)
    assert len(toks) == 9 and np.array_equal(toks, twin_toks), "the refused call changed the tokens that follow"
    assert np.array_equal(logits, twin_logits), "the refused call changed the logits that follow"
