"""LlamaModel("tiny", LLMI_I4).loadWeightsQuantized (include/llmi/model.h) gives the tokens of the
oracle on the numpy-quantised weights (the fixture of tests/test_gpu_engine_i4.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_engine_i4 import N_NEW, tiny  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(REPO, "llm-inference_amd", "lib")


def test_cpp_load_weights_quantized_i4(tiny, tmp_path):  # noqa: F811
    exe = str(tmp_path / "test_i4_load")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "cpp", "test_i4_load.cpp"), "-L", LIBDIR, "-lllmi",
           f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [exe, tiny["prefix"], str(N_NEW)] + [str(int(t)) for t in tiny["prompt"]]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = next(json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))
    np.testing.assert_array_equal(out["tokens"], tiny["tokens"])
    assert out["plain_refused"] is True and len(out["factory_tokens"]) == N_NEW
