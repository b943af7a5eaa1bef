"""The host side of the stepped device loops (g4s_amd/csrc/step_batch.hpp: the batch constants, the grid sized from the frontier the host saw, the cap
above which a step asks for a larger grid, the doubling batch) on the host, without a GPU: tests/cpp/step_batch_test.cpp is built with AddressSanitizer
and UBSan and run. It pins the clamp at both ends and in between, the cap of a sized grid and of the largest one, a largest grid below the smallest
clipped to it as betweenness.hip needs, and the batch sequence 16, 32, 64, 64."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_batch_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_batch_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "g4s_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "step_batch_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "step_batch_test: ok" in r.stdout


def test_the_step_batch_header_is_plain_cxx():
    with open(os.path.join(ROOT, "g4s_amd", "csrc", "step_batch.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "#include \"" not in text
