"""LlamaModel::setLogitRules / setAllowedTokens / clearLogitRules (include/llmi/model.h): the C++
model API's Response emits the tokens the Python engine emits for the same settings; the headers
and the two example programs compile and link with the new entry points."""
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


def test_cpp_logit_rules_compiles_and_links(tmp_path):
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_logit_rules.cpp"), str(tmp_path / "test_logit_rules"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)  # no arguments: no device work
    assert r.returncode == 0, (r.stdout, r.stderr)
    _build(os.path.join(REPO, "examples", "user_entry.cpp"), str(tmp_path / "user_entry"))
    _build(os.path.join(REPO, "examples", "chat_ids.cpp"), str(tmp_path / "chat_ids"))


@pytest.mark.gpu
def test_cpp_response_applies_the_python_engines_rules(tmp_path):
    import llmi
    from llmi.engine import Engine, preset
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"))
    golden = [int(t) for t in f["tokens"]]
    n_new = 12
    banned = golden[0]
    a = next(i for i in range(100, 200) if i not in golden)  # an id greedy decoding does not produce
    only = a + 1
    cfg = preset("tiny")
    cfg.weight_dtype, cfg.kv_dtype = llmi.F16, llmi.F32
    with Engine(cfg) as e:
        e.load_synthetic(int(f["seed"]))
        e.set_logit_rules({a: 64.0, banned: -np.inf}, presence_penalty=0.5, frequency_penalty=40.0)
        want = e.generate(f["prompt"], n_new)
        e.set_allowed([only])
        masked = e.generate(f["prompt"], n_new)
    assert (want != f["tokens"][:n_new]).any() and a in want and want[0] != banned
    np.testing.assert_array_equal(masked, [only] * n_new)
    exe = _build(os.path.join(REPO, "tests", "cpp", "test_logit_rules.cpp"), str(tmp_path / "test_logit_rules"))
    args = [exe, str(int(f["seed"])), str(n_new), str(a), "64.0", str(banned), "0.5", "40.0", str(only),
            str(len(f["prompt"]))] + [str(int(t)) for t in f["prompt"]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    got = {k: v for l in lines for k, v in l.items()}
    np.testing.assert_array_equal(got["rules"], want)
    np.testing.assert_array_equal(got["masked"], masked)
    np.testing.assert_array_equal(got["unmasked"], want)
    np.testing.assert_array_equal(got["greedy"], f["tokens"][:n_new])
