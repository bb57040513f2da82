"""Llama<T>::setLogprobs(n_top, score_prompt) / lastPromptLogprobs (include/llmi/model.h): with
score_prompt the model's one-pass prompt prefill is the scored form, so the prompt's own
records are finite, and they are the Python engine's scored prefill's bit for bit (as are the
generated ids and their records); without it the prompt's records stay "not computed"."""
import json
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "llm-inference_amd", "lib")
VOCAB = os.path.join(REPO, "tests", "golden", "llama2-7b-tokenizer.bin")
SRC = os.path.join(REPO, "tests", "cpp", "test_prompt_logprobs.cpp")


def _build(src, out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include"), src, "-L", LIBDIR, "-lllmi",
           f"-Wl,-rpath,{LIBDIR}", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_prompt_logprobs_compiles_and_links(tmp_path):
    exe = _build(SRC, str(tmp_path / "test_prompt_logprobs"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # no arguments: no device work
    assert r.returncode == 0, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_cpp_prompt_records_are_the_python_engines_scored_prefill(tmp_path):
    import llmi
    from llmi.engine import Engine, preset
    n_new, n_top = 6, 2
    exe = _build(SRC, str(tmp_path / "test_prompt_logprobs"))
    r = subprocess.run([exe, VOCAB, str(n_new), str(n_top)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    got = next(l for l in lines if "tokens" in l)
    prompt = np.array(got["prompt"], np.int32)
    n = len(prompt)
    assert got["n_top"] == n_top and n == 13 and len(got["tokens"]) == n_new
    # Llama<half_t> at the tiny geometry: fp16 weights and cache, dummy seed 0
    cfg = preset("tiny")
    cfg.weight_dtype, cfg.kv_dtype = llmi.F16, llmi.F16
    with Engine(cfg) as e:
        e.load_synthetic(0)
        e.set_logprobs(n_top)
        e.set_prompt(prompt)
        e.prefill(n, exact=1, score=True)
        e.decode(n_new - 1)
        toks = e.tokens(n + n_new)
        lp, tids, tlp = e.logprobs()
    assert len(lp) == n + n_new and np.isfinite(lp[1:]).all() and (tids[1:] >= 0).all()
    np.testing.assert_array_equal(got["tokens"], toks[n:])

    def bits(a):
        return np.ascontiguousarray(a).view(np.uint32)

    for key, lo, hi in (("prompt_", 1, n), ("", n, n + n_new)):
        glp = np.array(got[key + "logprob_bits"], np.uint32)
        assert np.isfinite(glp.view(np.float32)).all()
        np.testing.assert_array_equal(glp, bits(lp[lo:hi]))
        np.testing.assert_array_equal(np.array(got[key + "top_ids"], np.int32).reshape(hi - lo, n_top), tids[lo:hi])
        np.testing.assert_array_equal(np.array(got[key + "top_logprob_bits"], np.uint32).reshape(hi - lo, n_top),
                                      bits(tlp[lo:hi]))
    assert next(l for l in lines if "plain_same_tokens" in l) == {"plain_prompt_not_computed": True,
                                                                  "plain_same_tokens": True}
