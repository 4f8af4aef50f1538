#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.  Needs no GPU.

    scripts/compare_device_code.py BEFORE_DIR AFTER_DIR

Each directory holds device-only objects of the translation units to compare, one per .hip file, compiled with the
Makefile's flags plus `--cuda-device-only -c`, e.g. in elfi_amd/csrc:

    for f in distance mahalanobis multiw adaptive summaries reject; do
      hipcc $CXXFLAGS --cuda-device-only -c $f.hip -o DIR/$f.o
    done

Every object is unbundled (clang-offload-bundler), disassembled (llvm-objdump -d) and its code-object metadata read
(llvm-readelf --notes).  A kernel may move from one translation unit to another: the comparison is over the union of
each side's objects.  For every kernel symbol it checks
  * that the symbol exists on both sides (none added, none lost);
  * that the instruction stream is the same once addresses are dropped: the address comments, the raw offset of a branch
    (its target stays, as symbol + offset inside the kernel) and the pc-relative constants behind s_getpc_b64.  Device
    functions that were not inlined are compared as a set of code bodies (a lambda's name depends on its number in the
    translation unit);
  * that the metadata is the same: VGPR, AGPR and SGPR counts, spills, scratch, static LDS, kernarg size and arguments.
Exit status 0 when all of that holds, 1 otherwise; the last line is a one-line summary.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size", ".kernarg_segment_align",
        ".max_flat_workgroup_size", ".uses_dynamic_stack", ".wavefront_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def normalise(line, pcrel):
    """One instruction without anything that depends on where the code was placed."""
    target = re.search(r"<([^>]+)>\s*$", line)
    text = line.split("//")[0].strip()
    op = text.split()[0] if text else ""
    if op.startswith("s_cbranch") or op == "s_branch" or op == "s_call_b64":
        text = op + " " + (target.group(1) if target else "?")
    elif pcrel and op in ("s_add_u32", "s_addc_u32"):
        text = re.sub(r",\s*[^,]+$", ", <pcrel>", text)
    return text


def load(directory):
    """{symbol: instructions} for every function and {kernel: metadata} of the directory's objects."""
    code, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(directory)):
            if not name.endswith(".o"):
                continue
            co = os.path.join(tmp, name + ".co")
            run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                "--input=" + os.path.join(directory, name), "--output=" + co)
            sym, pcrel = None, 0
            for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).split("\n"):
                head = re.match(r"^<(.+)>:$", line)
                if head:
                    sym = head.group(1)
                    code[sym] = []
                elif sym and line.startswith("\t"):
                    text = normalise(line, pcrel > 0)
                    pcrel = 2 if text.startswith("s_getpc_b64") else pcrel - 1
                    code[sym].append(text)
            for lines in code.values():   # the padding behind a function's last instruction is not its code
                while lines and lines[-1].split()[0] in ("s_nop", "s_code_end", "..."):   # ("...": zeros up to the section's end)
                    lines.pop()
            cur = None
            for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).split("\n"):
                kv = re.match(r"^(\s+(?:- )?)(\.\w+):\s+(.*)$", line)
                if not kv:
                    continue
                indent, key, val = len(kv.group(1)), kv.group(2), kv.group(3)
                if kv.group(1) == "  - ":   # a kernel's first key
                    cur = {"args": []}
                if cur is None:
                    continue
                if indent == 4 and key == ".name":
                    meta[val] = cur
                elif indent == 4 and key in META:
                    cur[key] = val
                elif indent > 4 and key in (".offset", ".size", ".value_kind"):
                    cur["args"].append(key + "=" + val)
    return code, meta


def body(sym, code):
    return [text.replace(sym, "<self>") for text in code[sym]]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (code_a, meta_a), (code_b, meta_b) = load(sys.argv[1]), load(sys.argv[2])
    lost, added = sorted(set(meta_a) - set(meta_b)), sorted(set(meta_b) - set(meta_a))
    for k in lost:
        print("LOST   ", k)
    for k in added:
        print("ADDED  ", k)
    code_diff, meta_diff = [], []
    for k in sorted(set(meta_a) & set(meta_b)):
        if body(k, code_a) != body(k, code_b):
            code_diff.append(k)
            print("CODE   ", k, "(%d -> %d instructions)" % (len(code_a[k]), len(code_b[k])))
        if meta_a[k] != meta_b[k]:
            meta_diff.append(k)
            changed = {f: (meta_a[k].get(f), meta_b[k].get(f)) for f in set(meta_a[k]) | set(meta_b[k]) if meta_a[k].get(f) != meta_b[k].get(f)}
            print("META   ", k, changed)
    # device functions that were not inlined: lambdas are numbered per translation unit, so by code, not by name
    fn_a, fn_b = (sorted(hashlib.sha256("\n".join(body(f, c)).encode()).hexdigest() for f in c if f not in m)
                  for c, m in ((code_a, meta_a), (code_b, meta_b)))
    if fn_a != fn_b:
        print("FUNCS   the non-kernel device functions differ: %d before, %d after" % (len(fn_a), len(fn_b)))
    lines_a, lines_b = (sum(len(v) for v in c.values()) for c in (code_a, code_b))
    print("kernels: %d before, %d after; lost %d, added %d; code differs in %d, metadata differs in %d; "
          "instructions compared: %d before, %d after"
          % (len(meta_a), len(meta_b), len(lost), len(added), len(code_diff), len(meta_diff), lines_a, lines_b))
    return 1 if (lost or added or code_diff or meta_diff or fn_a != fn_b) else 0


if __name__ == "__main__":
    sys.exit(main())
