"""LlamaModel::setSamplingParams (include/llmi/model.h): the C++ model API's Response samples
the tokens the Python engine samples for the same parameters; the headers and the two
example programs compile and link with the new entry points."""
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


def test_cpp_sampling_params_compiles_and_links(tmp_path):
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_sampling_params.cpp"), str(tmp_path / "test_sampling_params"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # no arguments: no device work
    assert r.returncode == 0, (r.stdout, r.stderr)
    _build(os.path.join(REPO, "examples", "user_entry.cpp"), str(tmp_path / "user_entry"))
    _build(os.path.join(REPO, "examples", "chat_ids.cpp"), str(tmp_path / "chat_ids"))


@pytest.mark.gpu
def test_cpp_response_samples_the_python_engines_tokens(tmp_path):
    import llmi
    from llmi.engine import Engine, preset
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"))
    n_new, prm = 12, dict(top_k=40, top_p=0.9, temperature=0.6, repetition_penalty=1.1, seed=77)
    cfg = preset("tiny")
    cfg.weight_dtype, cfg.kv_dtype = llmi.F16, llmi.F32
    with Engine(cfg) as e:
        e.load_synthetic(int(f["seed"]))
        e.set_sampling_params(**prm)
        want = e.generate(f["prompt"], n_new)
    assert (want != f["tokens"][:n_new]).any()
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_sampling_params.cpp"), str(tmp_path / "test_sampling_params"))
    args = [exe, str(int(f["seed"])), str(n_new), str(prm["top_k"]), repr(prm["top_p"]), repr(prm["temperature"]),
            repr(prm["repetition_penalty"]), str(prm["seed"])] + [str(int(t)) for t in f["prompt"]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    np.testing.assert_array_equal(next(l["tokens"] for l in lines if "tokens" in l), want)
    np.testing.assert_array_equal(next(l["greedy"] for l in lines if "greedy" in l), f["tokens"][:n_new])
