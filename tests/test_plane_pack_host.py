"""csrc/kta_plane_pack.h on the CPU: tests/native/plane_pack_check.cpp — a program of its own, built with
AddressSanitizer + UBSan — fills one front slot of the plane form to exactly the bound of one plane interval (8192 records
for 1, 2 and 4 replicas, fewer for 8 and 64) with the longest lengths (254, 65534), both markers (0xFF, 0xFFFF), (0, 0) and
random mixes, record by record and as uniform quads, through the header's pack, unpack and interval functions, and compares
the unpacked fields and the corrected sums with plain 64-bit sums; it shows that replicas must be unpacked one by one and
that one record beyond the bound leaves the value field.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_pack_check(tmp_path):
    exe = str(tmp_path / "plane_pack_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "plane_pack_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plane_pack_check OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
