"""csrc/kta_fold_groups.h on the CPU: tests/native/fold_groups_check.cpp — a program of its own, built with
AddressSanitizer + UBSan — walks the group rule of the fold for 1 to 4096 rows: every row in exactly one group, the
groups' sizes summing to the rows and the last group's size.  Once for
every candidate group size (the header's kFoldGroupRows is a build switch) and once for the size the header ships.
No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = (8, 16, 32, 64, 128, 256)


def _shipped():
    src = open(os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc", "kta_fold_groups.h")).read()
    return int(re.search(r"#define KTA_FOLD_GROUP_ROWS (\d+)", src).group(1))


def test_the_shipped_group_size_is_a_candidate():
    assert _shipped() in CANDIDATES


@pytest.mark.parametrize("group_rows", [None, *CANDIDATES])
def test_fold_groups_check(tmp_path, group_rows):
    exe = str(tmp_path / "fold_groups_check")
    switch = [] if group_rows is None else ["-DKTA_FOLD_GROUP_ROWS=%d" % group_rows]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        *switch, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "fold_groups_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    want = "fold_groups_check OK (group rows %d)" % (group_rows or _shipped())
    assert r.returncode == 0 and want in r.stdout, (r.stdout + r.stderr)[-2000:]
