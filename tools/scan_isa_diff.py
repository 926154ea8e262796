"""Compare the gfx950 assembly of every kernel of the sources that hold kernels (SOURCES; kta_api.hip and kta_comm.hip
hold none) between two trees (no GPU needed): each tree's files are compiled with `hipcc --cuda-device-only -S` and the build's flags, labels are renumbered,
comments dropped, and the scan instantiations of the base tree are matched to this tree's with an empty `Extra` pack (the
timeline's kernel argument).  Prints one line per kernel: identical or not, the instruction lines of the
base tree and of this one, and base -> this tree of the kernel descriptor's registers and memory (RESOURCES: vector and
scalar registers, scratch bytes, static LDS bytes).  Exits non-zero when a kernel whose text differs takes more vector
registers or more scratch than the base tree's, another amount of LDS, or changes its instruction lines by more than
MAX_COUNT_CHANGE; or when a name that follows an `.amdhsa_kernel` directive in either tree's assembly is not among the
labels compared or listed as new in this tree (so that no kernel is skipped silently).  Only assembler directives are read and lines counted.

    python tools/scan_isa_diff.py <base tree> [<tree, default: this one>]"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
OLD, NEW = "EEEvNS_11ScanColumnsEmjjPmj", "EJEEEvNS_11ScanColumnsEmjjPmjDpT3_"


SOURCES = ("kta_kernels.hip", "kta_alive_table.hip", "kta_alive.hip", "kta_sketch.hip", "kta_hot.hip", "kta_kafka.hip",
           "kta_synth.hip", "kta_ts_order.hip", "kta_partitioner.hip", "kta_filter.hip", "kta_compaction.hip",
           "kta_size_quantiles.hip", "kta_segments.hip", "kta_record_batches.hip", "kta_payload.hip", "kta_header_names.hip",
           "kta_value_bytes.hip", "kta_lz4_model.hip")
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
# The bound on a changed kernel's instruction lines, as a fraction of the base tree's: the largest change that
# profiles/r14_scan_isa_diff.txt shows among the kernels that only had the tile codec's functions moved (the TILED scan
# instantiations at most 2 of 925, kta_tiles_to_raw none, synth_fill_tiles 1595 -> 1582), plus 1 % for the moves that a
# different inlining order reshuffles.
MAX_COUNT_CHANGE = 13 / 1595 + 0.01


def assemble(tree, src, out):
    if not os.path.exists(os.path.join(tree, "kafka_topic_analyzer_amd", "csrc", src)):
        open(out, "w").close()   # a source this tree does not have (yet, or any more) holds no kernel
        return
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


def resources(path):
    """Per kernel name, the RESOURCES values of its `.amdhsa_kernel` block."""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)^\s*\.end_amdhsa_kernel", open(path).read(), re.M | re.S):
        out[m.group(1).replace(NEW, OLD)] = tuple(int(re.search(r"\.amdhsa_%s\s+(\d+)" % r, m.group(2)).group(1)) for r in RESOURCES)
    return out


def main():
    base = sys.argv[1]
    tree = sys.argv[2] if len(sys.argv) > 2 else HERE
    ka, kb, da, db, ra, rb = {}, {}, set(), set(), {}, {}
    with tempfile.TemporaryDirectory() as d:
        for src in SOURCES:
            a, b = os.path.join(d, "base_" + src + ".s"), os.path.join(d, "tree_" + src + ".s")
            assemble(base, src, a)
            assemble(tree, src, b)
            ka.update(kernels(a))
            kb.update(kernels(b))
            da |= directives(a)
            db |= directives(b)
            ra.update(resources(a))
            rb.update(resources(b))
    bad = worse = 0
    print("          instructions   vgpr     sgpr     scratch  lds            (base -> this tree)")
    for k in sorted(ka):
        same = ka[k] == kb.get(k)
        bad += not same
        na, nb = len(ka[k]), len(kb.get(k, ()))
        va, vb = ra.get(k), rb.get(k)
        res = "  ".join("%3d->%-3d" % p if i < 2 else "%d->%d" % p for i, p in enumerate(zip(va, vb))) if va and vb else "(no descriptor)"
        verdict = "identical" if same else "DIFFERENT"
        if not same and (not va or not vb or vb[0] > va[0] or vb[2] > va[2] or vb[3] != va[3] or abs(nb - na) > MAX_COUNT_CHANGE * na):
            verdict = "WORSE"
            worse += 1
        print("%-9s %5d->%-5d  %s  %s" % (verdict, na, nb, res, k))
    print("new in this tree: %d kernel(s): %s" % (len(set(kb) - set(ka)), " ".join(sorted(set(kb) - set(ka)))))
    print("kernels of the base tree: %d, different: %d, of them over a bound (WORSE): %d" % (len(ka), bad, worse))
    missed = sorted((da | db) - set(ka) - set(kb))   # the loop above compares the labels of the base tree; this tree's other labels are listed as new
    print(".amdhsa_kernel directives: base %d, this tree %d; not compared: %d %s" % (len(da), len(db), len(missed), " ".join(missed)))
    return 1 if worse or missed else 0


if __name__ == "__main__":
    sys.exit(main())
