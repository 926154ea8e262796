"""csrc/kta_tile.h's size extrema on the CPU: tests/native/tile_size_check.cpp — a program of its own, built
with AddressSanitizer + UBSan — checks that tile_plane_host writes a marked tile's two words (the least and the largest
key + value size of its valued records, a None key as 0, 0xFFFFFFFF / 0 without a valued record), leaves them alone for
a tile it does not mark, and writes the same plane whether the words are asked for or not; and the address rule of the
words behind the marks.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_size_check(tmp_path):
    exe = str(tmp_path / "tile_size_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_size_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tile_size_check OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
