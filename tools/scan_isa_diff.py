"""Compare the gfx950 assembly of every kernel of csrc/kta_kernels.hip and csrc/kta_alive.hip between two trees (no GPU
needed): each tree's files are compiled with `hipcc --cuda-device-only -S` and the build's flags, labels are renumbered,
comments dropped, and the scan instantiations of the base tree are matched to this tree's with an empty `Extra` pack (the
timeline's kernel argument).  Prints one line per kernel and exits non-zero when any kernel differs.

    python tools/scan_isa_diff.py <base tree> [<tree, default: this one>]"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
OLD, NEW = "EEEvNS_11ScanColumnsEmjjPmj", "EJEEEvNS_11ScanColumnsEmjjPmjDpT3_"


SOURCES = ("kta_kernels.hip", "kta_alive.hip")


def assemble(tree, src, out):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-I", os.path.join(tree, "include"),
                    "-I", os.path.join(tree, "kafka_topic_analyzer_amd", "csrc"),
                    os.path.join(tree, "kafka_topic_analyzer_amd", "csrc", src), "-o", out],
                   check=True, capture_output=True)


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1).replace(NEW, OLD)
            out[cur] = []
            continue
        if cur:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            s = line.split(";")[0].rstrip()
            if s:
                s = re.sub(r"\.LBB\d+_", ".LBB_", s)
                out[cur].append(re.sub(r"\.Ltmp\d+", ".Ltmp", s).replace(NEW, OLD))
    return out


def main():
    base = sys.argv[1]
    tree = sys.argv[2] if len(sys.argv) > 2 else HERE
    ka, kb = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for src in SOURCES:
            a, b = os.path.join(d, "base_" + src + ".s"), os.path.join(d, "tree_" + src + ".s")
            assemble(base, src, a)
            assemble(tree, src, b)
            ka.update(kernels(a))
            kb.update(kernels(b))
    bad = 0
    for k in sorted(ka):
        same = ka[k] == kb.get(k)
        bad += not same
        print("%-9s %5d instructions  %s" % ("identical" if same else "DIFFERENT", len(ka[k]), k))
    print("new in this tree: %d kernel(s): %s" % (len(set(kb) - set(ka)), " ".join(sorted(set(kb) - set(ka)))))
    print("kernels of the base tree: %d, different: %d" % (len(ka), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
