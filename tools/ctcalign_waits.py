#!/usr/bin/env python3
"""What the whole-tile loop of every ctcalign_kernel instantiation waits for (tools/pausepath_waits.py
is the same listing for the pause kernel).

    make -C aligner_amd/csrc asm SRC=ctcalign.hip && python tools/ctcalign_waits.py

Reads the ISA the build keeps (aligner_amd/lib/asm), finds in each instantiation the basic block that holds the 32
per-frame barriers of a whole tile and prints its loads (L), barriers (|) and the count of every `s_waitcnt vmcnt(N)` in
program order.  With one row group a frame issues two loads (its token column and the blank column): a frame that waits
for the blank loaded 16 frames earlier shows vmcnt(30) to (32); a vmcnt(0), or a count below the loads issued in the
last frame or two, would be a frame waiting for memory."""
import os
import re
import sys

ASM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aligner_amd", "lib", "asm",
                   "ctcalign-hip-amdgcn-amd-amdhsa-gfx950.s")


def main():
    if not os.path.isfile(ASM):
        sys.exit(f"{ASM} not found: make -C aligner_amd/csrc asm SRC=ctcalign.hip")
    s = open(ASM).read()
    names = re.findall(r"^(_ZN\S*ctcalign_kernelILi(\d)ELi(\d)E\S*):\s", s, re.M)
    vt = {"0": "fp32", "1": "bf16", "2": "fp16"}
    worst = None
    for name, R, VT in names:
        i = s.index("\n" + name + ":")
        body = s[i:s.index("s_endpgm", i)]
        blocks = re.split(r"\n(?=\.LBB\d+_\d+:|; %bb)", body)
        for b in [b for b in blocks if b.count("s_barrier") >= 32]:
            seq = []
            for line in b.split("\n"):
                if "vmcnt" in line:
                    seq.append(re.search(r"vmcnt\((\d+)\)", line).group(1))
                elif "global_load" in line or "global_store" in line or "flat_" in line:
                    seq.append("L")
                elif "s_barrier" in line:
                    seq.append("|")
            vm = [int(x) for x in seq if x.isdigit()]
            worst = min(vm + ([worst] if worst is not None else []))
            print(f"row groups {R}, {vt[VT]}: {len(vm)} waits, vmcnt {min(vm)} .. {max(vm)}")
            print("    " + " ".join(seq))
    print(f"{len(names)} instantiations, lowest count in a whole-tile loop: vmcnt({worst})")


if __name__ == "__main__":
    main()
