"""Compare the gfx950 assembly of every kernel of the five sources that hold kernels (SOURCES; kta_api.hip and kta_comm.hip
hold none) between two trees (no GPU needed): each tree's files are compiled with `hipcc --cuda-device-only -S` and the build's flags, labels are renumbered,
comments dropped, and the scan instantiations of the base tree are matched to this tree's with an empty `Extra` pack (the
timeline's kernel argument).  Prints one line per kernel and exits non-zero when any kernel differs, or
when a name that follows an `.amdhsa_kernel` directive in either tree's assembly is not among the labels compared (so
that no kernel is skipped silently).

    python tools/scan_isa_diff.py <base tree> [<tree, default: this one>]"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
OLD, NEW = "EEEvNS_11ScanColumnsEmjjPmj", "EJEEEvNS_11ScanColumnsEmjjPmjDpT3_"


SOURCES = ("kta_kernels.hip", "kta_alive.hip", "kta_sketch.hip", "kta_kafka.hip", "kta_synth.hip")


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


def directives(path):
    """The kernel names of the assembly's `.amdhsa_kernel` directives."""
    return {m.group(1).replace(NEW, OLD) for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M)}


def main():
    base = sys.argv[1]
    tree = sys.argv[2] if len(sys.argv) > 2 else HERE
    ka, kb, da, db = {}, {}, set(), set()
    with tempfile.TemporaryDirectory() as d:
        for src in SOURCES:
            a, b = os.path.join(d, "base_" + src + ".s"), os.path.join(d, "tree_" + src + ".s")
            assemble(base, src, a)
            assemble(tree, src, b)
            ka.update(kernels(a))
            kb.update(kernels(b))
            da |= directives(a)
            db |= directives(b)
    bad = 0
    for k in sorted(ka):
        same = ka[k] == kb.get(k)
        bad += not same
        print("%-9s %5d instructions  %s" % ("identical" if same else "DIFFERENT", len(ka[k]), k))
    print("new in this tree: %d kernel(s): %s" % (len(set(kb) - set(ka)), " ".join(sorted(set(kb) - set(ka)))))
    print("kernels of the base tree: %d, different: %d" % (len(ka), bad))
    missed = sorted((da | db) - set(ka))   # the loop above compares the labels of the base tree
    print(".amdhsa_kernel directives: base %d, this tree %d; not compared: %d %s" % (len(da), len(db), len(missed), " ".join(missed)))
    return 1 if bad or missed else 0


if __name__ == "__main__":
    sys.exit(main())
