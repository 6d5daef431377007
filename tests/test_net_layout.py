"""The .net ingest's host-side arithmetic (sheep_amd/csrc/net_layout.h): byte classes, token-start
masks, the one-token parse, the chunk loop with its carry, the window guard, the stop pair and
the host tail, run as the whole chunked pipeline at chunk sizes 16, 32, 48 and 4096 and compared
with SNAPReader (sheep_amd/lib/readerwriter.h) on the same bytes: the case table of irregular
tokens, 200 seeded random texts, the empty file, whitespace only, one token, no trailing newline
(tests/cpp/net_layout.cpp).  A stand-alone program built with the address and
undefined-behaviour sanitizers; host code only, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_net_layout(tmp_path):
    exe = tmp_path / "net_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sheep_amd", "csrc"), "-I",
                    os.path.join(ROOT, "sheep_amd", "lib"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "net_layout.cpp")], check=True)
    out = subprocess.run([str(exe), str(tmp_path / "text.net")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
