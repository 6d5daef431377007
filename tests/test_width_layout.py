"""The exact tree widths' host-side index arithmetic (sheep_amd/csrc/width_layout.h): the
range-minimum structure over the Euler tour's depths, the arc -> LCA rule, the sort keys and the
weight construction, checked on forests of up to 64 ranks against linear scans, parent walks and
bags unioned up the tree (tests/cpp/width_layout.cpp).  A stand-alone program built with the
address and undefined-behaviour sanitizers; host code only, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_width_layout(tmp_path):
    exe = tmp_path / "width_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sheep_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "width_layout.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
