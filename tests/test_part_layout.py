"""The host half of sheep_partition_dev (sheep_amd/csrc/part_layout.h): the walk over the heavy
ranks, the reference's sort and first-fit packing of a cut rank's kids, the kids orders kept from
one k to the next, the roots and the push-down's deltas, checked on heap-ordered forests of up to
64 ranks against a restatement of lib/partition.h's loop on one table
(tests/cpp/part_layout.cpp).  A stand-alone program built with the address and
undefined-behaviour sanitizers; host code only, no GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_part_layout(tmp_path):
    exe = tmp_path / "part_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sheep_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "part_layout.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
