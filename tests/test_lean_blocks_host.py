"""csrc/kta_lean_blocks.h on the CPU: tests/native/lean_blocks_check.cpp — a program of its own, built with
AddressSanitizer + UBSan — drives the lean kernel's block rule (64 steps at a time, from a plane and a lean ballot) over
per-tile classes and compares the taken plane and lean steps, the list words, the handover and the end with a step-by-step
restatement of the rule: exhaustive patterns of others around steps 62-66 and 126-130 behind 0 to 6 earlier others, random
patterns of 1 to 300 steps, an end inside a block and at a block's last and first step, a workgroup whose first tile lies
past the end, and the last block of 2^31 - 1 steps.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lean_blocks_check(tmp_path):
    exe = str(tmp_path / "lean_blocks_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "lean_blocks_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lean_blocks_check OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
