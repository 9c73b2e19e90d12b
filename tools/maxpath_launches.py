#!/usr/bin/env python3
"""What the alignment search launches: a fixed matrix of small calls through the C ABI with the debug option
`maxpath_log_launch` set, which reaches every branch of the host side's plan (aligner_amd/csrc/maxpath.hip, plan_search).
Prints, per call, the library's launch lines (kernel with its template arguments, grid, block, LDS; of MaxpathParams what
is not 0 / set) and a hash of each output (path, token index, durations, status word), and asserts that the search kernels seen are exactly the
ones that are built (the rows of aligner_amd/lib/obj/maxpath.hip.resources.txt), each at least once.

    python tools/maxpath_launches.py > profiles/NAME_launches.txt
    ALIGNER_AMD_LIB=/path/to/other/libaligner_amd.so python tools/maxpath_launches.py > other.txt      # and diff the two

(another build needs the option too: tools/experiments/maxpath_launch_log_parent.patch adds it to the tree before the plan.)"""
import ctypes
import hashlib
import os
import re
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aligner_amd import _lib  # noqa: E402

DT = {"f32": (torch.float32, _lib.DT_F32), "bf16": (torch.bfloat16, _lib.DT_BF16), "f16": (torch.float16, _lib.DT_F16),
      "i32": (torch.int32, _lib.DT_I32), "u8": (torch.uint8, _lib.DT_U8), "i64": (torch.int64, _lib.DT_I64),
      "f64": (torch.float64, _lib.DT_F64)}
VT = {"f32": "VT_F32", "bf16": "VT_BF16", "f16": "VT_F16"}
STRICT, GENERIC, NO_PREV, WRITE_Q, STREAM, ONE_CU, TWO_CUS, PREZEROED, SEPARATE = (
    _lib.F_STRICT_MASK, _lib.F_FORCE_GENERIC, _lib.F_NO_PREV_TABLE, _lib.F_WRITE_Q, _lib.F_STREAM_PATH, _lib.F_ONE_CU,
    _lib.F_TWO_CUS, _lib.F_PATH_PREZEROED, _lib.F_SEPARATE_EXPAND)
FLAG_NAMES = {STRICT: "STRICT_MASK", GENERIC: "FORCE_GENERIC", NO_PREV: "NO_PREV_TABLE", WRITE_Q: "WRITE_Q", STREAM: "STREAM_PATH",
              ONE_CU: "ONE_CU", TWO_CUS: "TWO_CUS", PREZEROED: "PATH_PREZEROED", SEPARATE: "SEPARATE_EXPAND"}


def matrix():
    """(B, Tx, Ty, score dtype, keywords of run())"""
    calls = []

    def add(B, Tx, Ty, dt="f32", **kw):
        calls.append((B, Tx, Ty, dt, kw))
    # wave tiers x loaders, fp32 (16-byte loaders at Ty % 4 == 0; Ty odd): no mask; a strict mask verified in front (no path:
    # MASKMODE 2); one with a 0.5 in it beside a path (optimistic + redo); eight waves multiply, at depth 1
    for Tx, Tys in ((40, (64, 61)), (100, (128, 125)), (200, (256, 253)), (400, (448, 445))):
        for Ty in Tys:
            add(3, Tx, Ty)
            add(3, Tx, Ty, mask="prefix", flags=STRICT, path=None)
            add(3, Tx, Ty, mask="half", flags=STRICT)
    # the strict mask's other settings
    add(3, 100, 128, mask="prefix", flags=STRICT)
    add(3, 100, 128, mask="half", flags=STRICT, path=None)
    for mask in ("prefix", "half"):
        add(3, 100, 128, mask=mask, flags=STRICT, options={"maxpath_no_mask_verify": 1})
        add(3, 100, 128, mask=mask, flags=STRICT, options={"maxpath_no_optimistic_mask": 1})
    # 16-bit scores: four and eight waves at Ty % 8 == 0, the generic kernel otherwise
    for dt in ("bf16", "f16"):
        add(3, 40, 64, dt)
        add(3, 40, 64, dt, mask="prefix", flags=STRICT, path=None)
        add(3, 40, 64, dt, mask="half", flags=STRICT)
        add(3, 400, 448, dt)
        add(3, 400, 448, dt, mask="half", flags=STRICT)
        add(3, 100, 124, dt)
    # decision words: in LDS without the P table; more than 64 tiles (windowed backtrack)
    add(2, 40, 256, flags=NO_PREV)
    add(2, 40, 2080)
    # the generic kernel
    for dt in ("f32", "bf16", "f16"):
        for Tx, Ty in ((100, 128), (300, 320), (600, 608), (1100, 1104)):
            add(1 if Tx > 600 else 2, Tx, Ty, dt, flags=GENERIC)
            add(1 if Tx > 600 else 2, Tx, Ty, dt, flags=GENERIC | STRICT, mask="half")
    add(2, 100, 128, flags=WRITE_Q)
    # the dense path
    add(3, 100, 128, flags=STREAM)
    add(3, 100, 128, path="misaligned")
    add(3, 100, 128, flags=SEPARATE)
    add(3, 100, 125, flags=SEPARATE | STREAM, path_dtype="u8")
    add(3, 100, 128, flags=PREZEROED, path="prezeroed", path_dtype="bf16")
    add(3, 100, 128, path=None)
    # lengths from the mask: a mask that only supplies them, and a strict one
    add(3, 100, 128, mask="prefix", lengths=False)
    add(3, 100, 128, mask="prefix", mask_dtype="u8", lengths=False)
    add(3, 100, 128, mask="half", flags=STRICT, lengths=False, path=None)
    # two workgroups per utterance
    for dt in ("f32", "bf16", "f16"):
        add(2, 260, 288, dt, flags=TWO_CUS)
        add(2, 260, 288, dt, flags=TWO_CUS | STRICT, mask="half")
    add(2, 260, 1792, flags=STREAM)
    add(2, 260, 1792, flags=ONE_CU)
    add(2, 260, 1792, ld=1824)
    add(2, 260, 1792, options={"maxpath_no_split_walk": 1})
    add(1, 260, 6016)
    add(2, 260, 288, flags=TWO_CUS, options={"maxpath_zero_blocks": 40})
    # a row pitch of whole 128-byte lines
    add(3, 100, 100, ld=128)
    add(3, 100, 104, "bf16", ld=128)
    return calls


def run(lib, dev, n, B, Tx, Ty, dt, mask=None, mask_dtype=None, lengths=True, path="aligned", path_dtype="i32", flags=0, ld=None,
        options=None):
    rng = np.random.default_rng(1000 + n)
    tdt, cdt = DT[dt]
    ldv = ld or Ty
    v = torch.from_numpy(rng.standard_normal((B, Tx, ldv)).astype(np.float32)).to(dev).to(tdt)
    ty = np.array([Ty] + [int(rng.integers(Tx, Ty + 1)) for _ in range(B - 1)], np.int32)        # ragged, utterance 0 full
    tx = np.array([Tx] + [int(rng.integers(1, Tx + 1)) for _ in range(B - 1)], np.int32)
    t_x, t_y = torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)
    m, mdt = None, 0
    if mask:
        m = ((torch.arange(Tx, device=dev)[None, :, None] < t_x[:, None, None]) &
             (torch.arange(Ty, device=dev)[None, None, :] < t_y[:, None, None]))
        mtd, mdt = DT[mask_dtype or dt]
        m = m.to(mtd)
        if mask == "half":
            m[B - 1, 0, int(ty[B - 1]) // 2] = 0.5               # inside the last utterance's rectangle
    nbytes = B * Tx * Ty * DT[path_dtype][0].itemsize if path else 0
    pbuf = torch.full((nbytes + 16,), 0 if path == "prezeroed" else 0x7F, dtype=torch.uint8, device=dev)
    off = 4 if path == "misaligned" else 0
    p = pbuf[off:off + nbytes] if path else None
    tok = torch.full((B, Ty), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    dur = torch.full((B, Tx), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    ws = torch.zeros(lib.aligner_maxpath_workspace_bytes(B, Tx, Ty), dtype=torch.uint8, device=dev)
    for k, val in (options or {}).items():
        assert lib.aligner_debug_set_option(k.encode(), val) == 0, k
    torch.cuda.synchronize()
    names = "|".join(name for bit, name in FLAG_NAMES.items() if flags & bit) or "0"
    os.write(2, ("== call %d: [%d,%d,%d] %s flags=%s mask=%s%s lengths=%s path=%s/%s%s%s\n" % (
        n, B, Tx, Ty, dt, names, mask, "/" + mask_dtype if mask_dtype else "", "given" if lengths else "from the mask", path,
        path_dtype, " ld=%d" % ld if ld else "", "".join(" %s=%d" % kv for kv in (options or {}).items()))).encode())
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    if ld:
        rc = lib.aligner_maxpath_ld(v.data_ptr(), cdt, ld, ptr(t_x), ptr(t_y), ptr(p), DT[path_dtype][1], tok.data_ptr(), dur.data_ptr(),
                                    ws.data_ptr(), ws.numel(), B, Tx, Ty, -1e9, flags, None)
    else:
        rc = lib.aligner_maxpath(v.data_ptr(), cdt, ptr(m), mdt, ptr(t_x) if lengths else None, ptr(t_y) if lengths else None, ptr(p),
                                 DT[path_dtype][1], tok.data_ptr(), dur.data_ptr(), ws.data_ptr(), ws.numel(), B, Tx, Ty, -1e9, flags, None)
    torch.cuda.synchronize()
    for k in (options or {}):
        lib.aligner_debug_set_option(k.encode(), 0)
    status = ctypes.c_int32(-1)
    _lib.check(lib.aligner_maxpath_read_status(ws.data_ptr(), ctypes.addressof(status), None))
    digest = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] if t is not None else "-"      # noqa: E731
    os.write(2, ("   rc=%d%s status=%d path=%s tok=%s dur=%s\n" % (
        rc, " (%s)" % lib.aligner_last_error().decode() if rc else "", status.value, digest(p), digest(tok), digest(dur))).encode())
    return rc


def built_search_kernels():
    """The search kernels of the in-tree build, named as the launch log names them."""
    rows = open(os.path.join(ROOT, "aligner_amd", "lib", "obj", "maxpath.hip.resources.txt")).read()
    vt = ["VT_F32", "VT_BF16", "VT_F16"]
    out = set()
    for a in re.findall(r"maxpath_pipelined_kernelILi(\d)ELi(\d)ELb(\d)ELi(\d)ELi(\d)ELb(\d)EE", rows):
        out.add("maxpath_pipelined_kernel<%s,%s,%s,%s,%s,%s>" % (a[0], a[1], a[2], a[3], vt[int(a[4])], a[5]))
    for a in re.findall(r"maxpath_generic_kernelILi(\d)ELi(\d)ELi(\d)EE", rows):
        out.add("maxpath_generic_kernel<%s,%s,%s>" % (a[0], a[1], vt[int(a[2])]))
    return out


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    assert lib.aligner_debug_set_option(b"maxpath_log_launch", 1) == 0, "this library has no maxpath_log_launch"
    sys.stderr.flush()
    saved = os.dup(2)
    log = tempfile.TemporaryFile()
    os.dup2(log.fileno(), 2)                       # the library writes its lines to the C stderr
    try:
        rcs = [run(lib, dev, n, *c[:4], **c[4]) for n, c in enumerate(matrix())]
        # the one refusal that comes behind a HIP call (the device's LDS limit): aligner_maxpath_scatter_path's path dtype
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        rc = lib.aligner_maxpath_scatter_path(buf.data_ptr(), buf.data_ptr(), 99, 1, 4, 8, None)
        os.write(2, ("== aligner_maxpath_scatter_path, path dtype 99: rc=%d (%s)\n" % (rc, lib.aligner_last_error().decode())).encode())
    finally:
        lib.aligner_debug_set_option(b"maxpath_log_launch", 0)
        os.dup2(saved, 2)
        log.seek(0)
        text = log.read().decode()
        print("(of MaxpathParams a scalar that is 0 and a pointer that is set are left out; the library's line has them all:\n"
              " B Tx Ty ldv NT ROWS WT bits_in_lds lds_bits_off lds_prev_off split_walk lds_total force_exact neg flags verify redo\n"
              " path1_es path1_one zero_blocks zero_nt zero_n16 | value mask t_xs t_ys starts tok dur bits status mflag qout xring\n"
              " xflag xwalk stamps dump path1 zsync)")
        for line in text.splitlines():
            head, bar, params = line.partition(" | ")
            print(head + bar + " ".join(f for f in params.split(" ") if not re.fullmatch(r"\w+=(0|0x0|set)", f)))
    assert not any(rcs), "a call of the matrix was refused"
    seen = set(re.findall(r"maxpath launch: (maxpath_(?:pipelined|generic)_kernel<[^>]*>)", text))
    built = built_search_kernels()
    print("search kernels seen: %d, built: %d" % (len(seen), len(built)))
    assert seen == built, "never launched: %s; launched but not in the table: %s" % (sorted(built - seen), sorted(seen - built))


if __name__ == "__main__":
    main()
