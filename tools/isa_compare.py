#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel, without a GPU: every csrc/*.hip of both trees is compiled to gfx950
assembly with the Makefile's flags plus `--cuda-device-only -S` (same relative file names), and each function is listed as
identical, different or removed (in the parent only; one that only this tree has is an error) -- for a different one the count of changed lines (also with the register numbers masked, which
leaves the changes that are not a renaming) and its row of the build's resource report
(aligner_amd/lib/obj/*.resources.txt: both trees must have been built) before and after.

    python tools/isa_compare.py [--brief] [--rename=REGEX=REPL] /path/to/parent/checkout [/path/to/this/tree] > profiles/NAME_isa.txt

A kernel that lost or gained a template parameter has another mangled name: `--rename` rewrites the parent's names
(`re.sub` on its assembly and its resource rows) so that it is compared with its successor.

The one line a compiler changes for any edit of a file or of a header it includes, the hash in the `__hip_cuid_` symbol,
is masked, and so is the function's number in its local labels (`.LBB57_12`).  `--brief` names only the functions that are
not identical."""
import difflib
import functools
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import parse  # noqa: E402

# a function's local labels carry its number in the file (.LBB57_12, .LJTI57_0), which changes when an instantiation before
# it comes or goes, and the long-branch labels count through the file (.Lpost_getpc122): masked, a block's own number stays;
# so is the padding between a label and its comment, which follows the label's width
LOCAL_LABEL = re.compile(r"(\.L|\b)(BB|JTI|CPI|post_getpc)\d+")          # (the loop comments name blocks without the .L)
LABEL_PAD = re.compile(r":\s+;")
# an inline-asm statement's own labels end in its number in the file (`%=`: .Lwr63_153): renumbered by first appearance in the function
ASM_LABEL = re.compile(r"(\.L(?!BB|JTI|CPI)[A-Za-z]+\d*_)(\d+)\b")
ROW = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = var["CXXFLAGS"]
    while "$(" in flags:
        flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    return var["HIPCC"], flags.split()


def assembly(tree, out):
    csrc = os.path.join(tree, "aligner_amd", "csrc")
    hipcc, flags = makefile_flags(csrc)
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(src):
        subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-x", "hip", src, "-o", os.path.join(out, src + ".s")],
                       cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(one, srcs))
    return srcs


def functions(path, renames=()):
    """{name: lines} of every function of an assembly file, and the lines outside them."""
    funcs, rest, name, declared = {}, [], None, set()
    for line in open(path):
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
        line = LABEL_PAD.sub(": ;", LOCAL_LABEL.sub(r"\1\2", line))
        for old, new in renames:
            line = re.sub(old, new, line)
        m = re.match(r"\s*\.type\s+(\w+),@function", line)
        if m:
            declared.add(m.group(1))
        if name is None and line.split(":")[0] in declared and re.match(r"^\w+:\s*(;.*)?$", line):
            name = line.split(":")[0]
            funcs[name], ids = [], {}
        elif name is not None and line.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            funcs[name].append(ASM_LABEL.sub(lambda m: m.group(1) + str(ids.setdefault(m.group(2), len(ids))), line))
        else:
            rest.append(line)
    return funcs, rest


def changed(a, b):
    return sum(1 for ln in difflib.unified_diff(a, b, n=0) if ln[0] in "+-" and ln[:3] not in ("+++", "---"))


def masked(lines):
    """The lines with every register number replaced: what is left of a difference is not a renaming."""
    return [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1N", ln) for ln in lines]


def resources(tree, src):
    path = os.path.join(tree, "aligner_amd", "lib", "obj", src + ".resources.txt")
    if not os.path.isfile(path):
        raise SystemExit("%s is missing: build the tree first (make -C %s/aligner_amd/csrc)" % (path, tree))
    return {k: " ".join("%s %d" % (f.split(" [")[0], v.get(f, 0)) for f in ROW) for k, v in parse(path)}


@functools.lru_cache(maxsize=4)
def text(path):
    return open(path).read()


def row(res, name, path):
    """A kernel's resource row; a device function that is not a kernel has none in either build."""
    if name not in res and ("amdhsa_kernel " + name) in text(path):
        raise SystemExit("no resource row for kernel %s of %s" % (name, os.path.basename(path)))
    return res.get(name, "(not a kernel: no resource row)")


def main():
    renames = [a[len("--rename="):].split("=", 1) for a in sys.argv[1:] if a.startswith("--rename=")]
    brief = "--brief" in sys.argv[1:]
    paths = [a for a in sys.argv[1:] if not a.startswith("--rename=") and a != "--brief"]
    if any(len(r) != 2 for r in renames) or not paths:
        raise SystemExit("usage: isa_compare.py [--brief] [--rename=REGEX=REPL ...] PARENT_TREE [THIS_TREE]")
    parent = os.path.abspath(paths[0])
    this = os.path.abspath(paths[1]) if len(paths) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        srcs = assembly(parent, a)
        assert srcs == assembly(this, b), "the two trees have different kernel files"
        same = diff = gone = 0
        for src in srcs:
            (fa, ra), (fb, rb) = functions(os.path.join(a, src + ".s"), renames), functions(os.path.join(b, src + ".s"))
            assert not set(fb) - set(fa), src + ": functions that the parent does not have: %s" % sorted(set(fb) - set(fa))
            # (outside the functions: the kernel descriptors and the metadata, which repeat a different function's sizes)
            lone = ra != rb and fa == fb
            print("%s: %d functions%s" % (src, len(fa), "; DIFFERENT outside the functions only" if lone else ""))
            for name in sorted(set(fa) - set(fb)):          # an instantiation that nothing asks for any more
                gone += 1
                print("  removed    %s" % name)
                del fa[name]
            res_a, res_b = resources(parent, src), resources(this, src)
            for old, new in renames:
                res_a = {re.sub(old, new, k): v for k, v in res_a.items()}
            for name in fa:
                rows = row(res_a, name, os.path.join(a, src + ".s")), row(res_b, name, os.path.join(b, src + ".s"))
                if fa[name] == fb[name] and rows[0] == rows[1]:
                    same += 1
                    if not brief:
                        print("  identical  %s" % name)
                    continue
                diff += 1
                print("  DIFFERENT  %s: %d changed lines (of %d), %d with the register numbers masked"
                      % (name, changed(fa[name], fb[name]), len(fa[name]), changed(masked(fa[name]), masked(fb[name]))))
                print("      before %s\n      after  %s%s" % (*rows, "" if rows[0] == rows[1] else "   <-- resources changed"))
            if brief:
                print("  identical  every other function")
        print("%d functions identical, %d different, %d removed" % (same, diff, gone))


if __name__ == "__main__":
    main()
