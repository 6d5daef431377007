"""The degree passes' and the radix sort's scratch layouts (sheep_amd/csrc/front_layout.h):
every table inside its buffer, none overlapping, u64 and 16-byte alignment, the room behind the u16 entry arrays, and
every offset and total equal to the size formulas and launcher pointer arithmetic the layouts
replaced (frozen in tests/cpp/front_layout.cpp).  Host code only (g++), no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_front_layouts(tmp_path):
    exe = tmp_path / "front_layout"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I",
                    os.path.join(ROOT, "sheep_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "front_layout.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
