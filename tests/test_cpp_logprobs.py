"""LlamaModel::setLogprobs / lastLogprobs (include/llmi/model.h): the C++ model API's Response
gives the generated ids and log-probabilities the Python engine gives, bit for bit; the headers
compile and link with the new entry points in both model classes."""
import json
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "llm-inference_amd", "lib")


def _build(src, out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include"), src, "-L", LIBDIR, "-lllmi",
           f"-Wl,-rpath,{LIBDIR}", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_logprobs_compiles_and_links(tmp_path):
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_logprobs.cpp"), str(tmp_path / "test_logprobs"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # no arguments: no device work
    assert r.returncode == 0, (r.stdout, r.stderr)


@pytest.mark.gpu
def test_cpp_response_gives_the_python_engines_logprobs(tmp_path):
    import llmi
    from llmi.engine import Engine, preset
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"))
    n_new, n_top, n = 12, 2, len(f["prompt"])
    cfg = preset("tiny")
    cfg.weight_dtype, cfg.kv_dtype = llmi.F16, llmi.F32
    with Engine(cfg) as e:
        e.load_synthetic(int(f["seed"]))
        e.set_logprobs(n_top)
        want = e.generate(f["prompt"], n_new)
        lp, tids, tlp = e.logprobs()
    assert np.isfinite(lp[n:]).all() and len(lp) == n + n_new
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_logprobs.cpp"), str(tmp_path / "test_logprobs"))
    args = [exe, str(int(f["seed"])), str(n_new), str(n_top)] + [str(int(t)) for t in f["prompt"]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    got = next(l for l in lines if "tokens" in l)
    assert got["n_top"] == n_top
    np.testing.assert_array_equal(got["tokens"], want)
    np.testing.assert_array_equal(np.array(got["logprob_bits"], np.uint32), lp[n:].view(np.uint32))
    np.testing.assert_array_equal(np.array(got["top_ids"], np.int32).reshape(n_new, n_top), tids[n:])
    np.testing.assert_array_equal(np.array(got["top_logprob_bits"], np.uint32).reshape(n_new, n_top),
                                  np.ascontiguousarray(tlp[n:]).view(np.uint32))
    assert next(l for l in lines if "off_same_tokens" in l) == {"off_same_tokens": True, "off_refused": True}
