"""The host side of the level-scheduled calls (g4s_amd/csrc/level_schedule.hpp: the launch list of a solve and of a factorisation, the two rules that
spread a level's rows over its threads, and the walk that turns the list into launches) on the host, without a GPU: tests/cpp/level_schedule_test.cpp is
built with AddressSanitizer and UBSan and run. It pins the chaining rule at no level, at one, at runs around G4S_TRSV_CHAIN_LEVELS and at widths around
G4S_TRSV_CHAIN_WIDTH, both stride rules at every doubling, and the walk's calls, grids and row coverage on a small schedule."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_schedule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "level_schedule_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "g4s_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "level_schedule_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "level_schedule_test: ok" in r.stdout


def test_the_level_schedule_header_is_plain_cxx():
    with open(os.path.join(ROOT, "g4s_amd", "csrc", "level_schedule.hpp")) as f:
        text = f.read()
    assert "#include <hip" not in text and "#include \"" not in text
