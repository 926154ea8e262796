"""csrc/kta_tile.h's scan plane on the CPU (include/kta_hip.h): tests/native/tile_plane_check.cpp — a program of
its own, built with AddressSanitizer + UBSan — checks the fit rule at its edges (partition -1, 0, 255, 256; key -1, 0,
254, 255; value -1, 0, 65534, 65535), pack and unpack of every fitting triple it draws, the mark of a whole tile, of a
tile with one record that does not fit, of a partial and of a raw tile, and that tile_pack_host's images next to
tile_plane_host's are what tile_pack_host alone writes outside bytes [4096, 8192) of the ts image.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_plane_check(tmp_path):
    exe = str(tmp_path / "tile_plane_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_plane_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tile_plane_check OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
