"""The host logic of the engine's logit rules (csrc/rules_host.h: sparse bias pairs to a dense
row, an id list to bitmap words, the size and value checks) under the address and
undefined-behaviour sanitizers: tests/cpp/test_rules_host.cpp is a stand-alone program with its
own main (the sanitizer runtimes linked into it), so it needs no preload and no GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rules_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_rules_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(REPO, "llm-inference_amd", "csrc"),
           os.path.join(REPO, "tests", "cpp", "test_rules_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "all checks passed" in r.stdout
