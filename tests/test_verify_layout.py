"""The tree verifier's host-side index arithmetic (sheep_amd/csrc/verify_layout.h): sort items,
children runs, Euler-tour successors, list ranking and the report assembly, checked against a
recursive DFS on forests of up to 64 ranks (tests/cpp/verify_layout.cpp).  A stand-alone program
built with the address and undefined-behaviour sanitizers; host code only, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_verify_layout(tmp_path):
    exe = tmp_path / "verify_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sheep_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "verify_layout.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
