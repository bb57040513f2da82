"""LlamaModel("tiny", LLMI_F16, LLMI_I8) (include/llmi/model.h) with synthetic weights generates
the tokens of the Python engine with the int8 KV cache, and llmi_engine_kv_slot_q8 is reachable
from C++ (tests/cpp/test_kv8.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "llm-inference_amd", "lib")
N_NEW = 8


def test_cpp_llama_model_int8_kv(tmp_path):
    import llmi
    from llmi.engine import Engine, preset
    f = np.load(os.path.join(REPO, "tests", "golden", "tiny.npz"), allow_pickle=False)
    seed, prompt = int(f["seed"]), np.asarray(f["prompt"], np.int32)
    with Engine(preset("tiny", kv_dtype=llmi.I8)) as e:
        e.load_synthetic(seed)
        want = e.generate(prompt, N_NEW)
    exe = str(tmp_path / "test_kv8")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "test_kv8.cpp"), "-L", LIBDIR, "-lllmi",
           f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [exe, str(seed), str(N_NEW)] + [str(int(t)) for t in prompt]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = next(json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))
    np.testing.assert_array_equal(out["tokens"], want)
    assert out["slot_ok"] is True
