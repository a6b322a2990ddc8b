#!/usr/bin/env python
"""Do kernels of two builds of librerevst_hip.so compile to the same gfx950 instructions?
    python tools/isa_diff.py OLD.so NEW.so [--match conv_first_k]
Unbundles the gfx950 code object of each library (clang-offload-bundler), disassembles it (llvm-objdump -d) and compares, kernel by
kernel, the instruction text without addresses and encodings.  Prints one line per kernel of OLD whose name contains --match:
same / DIFFERENT (with the first differing instructions) / missing, then the kernels only NEW has; exit status 1 if any differs.
A pc-relative literal (the s_add_u32 behind s_getpc_b64 that addresses a constant table) moves with the code object's layout and
shows as a one-operand difference in kernels whose source did not change."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co]).decode()
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"//.*", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", line)).strip())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(a.old, tmp, "old"), kernels(a.new, tmp, "new")
    bad = 0
    for name, ins in old.items():
        if a.match not in name:
            continue
        if name not in new:
            print("missing  ", name)
            bad += 1
        elif new[name] == ins:
            print("same      %s (%d instructions)" % (name, len(ins)))
        else:
            diff = [(x, y) for x, y in zip(ins, new[name]) if x != y]
            print("DIFFERENT %s (%d -> %d instructions, %d differ in place)" % (name, len(ins), len(new[name]), len(diff)))
            for x, y in diff[:4]:
                print("            %s | %s" % (x, y))
            bad += 1
    for name in new:
        if a.match in name and name not in old:
            print("new       %s (%d instructions)" % (name, len(new[name])))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
