"""The ledger behind the small device-to-host reads (g4s_amd/csrc/read_ledger.hpp) on the host, without a GPU: tests/cpp/read_ledger_test.cpp is built
with AddressSanitizer and UBSan and run. It asserts that a wait hands out the notes of its stream only, that a dropped owner's notes are never written
(the destination is freed before the next delivery: the sanitizer would see the write), that an event delivery stops at the mark, that slots are not
handed out twice and a full block refuses, and that a nested wait delivers the outer owner's notes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_ledger_under_sanitizers(tmp_path):
    exe = str(tmp_path / "read_ledger_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "g4s_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "read_ledger_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read_ledger_test: ok" in r.stdout


def test_the_ledger_header_is_plain_cxx():
    with open(os.path.join(ROOT, "g4s_amd", "csrc", "read_ledger.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "#include \"" not in text
