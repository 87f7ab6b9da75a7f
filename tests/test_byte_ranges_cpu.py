"""The alias predicate of the C-ABI entries (cuda-flow2d_amd/csrc/byte_ranges.hpp) against a brute-force intersection of byte
sets: tests/c/byte_ranges_check.cpp, a program of its own that includes nothing but that header, built by the host compiler with
its address and undefined-behaviour sanitizers and run as it is (no device, no HIP, nothing loaded into this process)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_predicate_is_the_intersection_of_the_byte_sets(tmp_path):
    exe = tmp_path / "byte_ranges_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cuda-flow2d_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "byte_ranges_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 wrong" in out.stdout and "comparisons" in out.stdout, out.stdout


def test_the_header_needs_no_hip():
    """It is included by the host-only check above and by every kernel file through common.hpp: no HIP include of its own."""
    text = open(os.path.join(ROOT, "cuda-flow2d_amd", "csrc", "byte_ranges.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"]
