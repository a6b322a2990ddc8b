#!/usr/bin/env python
"""Where does a built librerevst_hip.so spill?  Per kernel: the code object's sgpr_spill_count / vgpr_spill_count, and per basic
block the vector instructions that only move spilled values, next to the block's MFMA count.
    python tools/isa_ledger.py LIB.so [--match conv_f43_k] [--blocks]
Unbundles and disassembles the gfx950 code object as tools/isa_diff.py does.  Counted per block:
  lane : v_readlane_b32 / v_writelane_b32 — scalar registers spilled into lanes of a vector register.  On gfx950 they issue on the
         vector port, between the MFMAs (profiles/r03_mfma_filler_cost.txt: ~13 clocks for a single one, ~4 when batched);
  agpr : v_accvgpr_write_b32, and v_accvgpr_read_b32 of an AGPR that some v_accvgpr_write_b32 of the kernel fills and no MFMA writes
         — vector registers parked in the accumulator file (reads of MFMA results are the kernel's own work and are not counted);
  scratch : scratch_load / scratch_store / buffer accesses through the scratch descriptor are reported as vgpr_spill_count only.
A basic block ends behind a branch / s_endpgm and in front of every branch target.  One summary line per kernel:
    <kernel>  sgpr_spill N  vgpr_spill N  code BYTES  lane ops: TOTAL (IN MFMA BLOCKS)  agpr moves: TOTAL (IN MFMA BLOCKS)
and with --blocks one line per block that has lane ops or agpr moves.  ledger() returns the same as a dict for tests."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import LLVM      # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
_REG = re.compile(r"\ba(\d+)\b|\ba\[(\d+):(\d+)\]")


def _agprs(operand):
    m = _REG.search(operand)
    if not m:
        return set()
    if m.group(1) is not None:
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def unbundle(lib, tmp, tag="lib"):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=" + TARGET,
                           "--input=" + fat, "--output=" + co])
    return co


def metadata(co):
    """{kernel: {sgpr_spill_count, vgpr_spill_count, ...}} from the code object's AMDGPU metadata note.  A kernel's record is a list
    item whose keys are sorted: it starts at "- .agpr_count" (or "- .args") and holds .symbol = <kernel>.kd somewhere in the middle."""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(2), m.group(3).strip().strip("'\"")
        if m.group(1) and k in ("agpr_count", "args"):
            cur = {}
        if cur is None:
            continue
        if k == "symbol":
            out[v[:-3] if v.endswith(".kd") else v] = cur
        elif k in ("sgpr_spill_count", "vgpr_spill_count", "sgpr_count", "vgpr_count", "agpr_count", "private_segment_fixed_size"):
            cur[k] = int(v)
    return out


def disassemble(co):
    """{kernel: [(address, text, branch target or None)]}: llvm-objdump prints the address, and behind a branch its target as
    <kernel+0xOFFSET>, in the comment of each line"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co]).decode()
    out, cur, base = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.+)>:", line)
        if m:
            cur, base = out.setdefault(m.group(2), []), int(m.group(1), 16)
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line) if cur is not None else None
        if m:
            tgt = re.search(r"<[^>+]+(?:\+0x([0-9a-f]+))?>\s*$", m.group(3))
            cur.append((int(m.group(2), 16), m.group(1), (base + int(tgt.group(1) or "0", 16)) if tgt else None))
    return out


def _is_branch(op):
    return op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64")


def blocks(ins):
    """[(first address, [instruction text])]: split behind branches and in front of branch targets."""
    leaders = set()
    for i, (a, t, tgt) in enumerate(ins):
        if _is_branch(t.split()[0]):
            if i + 1 < len(ins):
                leaders.add(ins[i + 1][0])
            if tgt is not None:
                leaders.add(tgt)
    out = []
    for a, t, _ in ins:
        if a in leaders or not out:
            out.append((a, []))
        out[-1][1].append(t)
    return out


def ledger(lib, match=""):
    """{kernel: {"sgpr_spill", "vgpr_spill", "code_bytes", "lane", "lane_mfma", "agpr", "agpr_mfma",
                 "blocks": [(address, instructions, mfma, lane, agpr)]}} for kernels whose name contains `match`."""
    with tempfile.TemporaryDirectory() as tmp:
        co = unbundle(lib, tmp)
        meta, dis = metadata(co), disassemble(co)
    res = {}
    for name, ins in dis.items():
        if match not in name or name not in meta:
            continue
        filled, mfma_dst = set(), set()
        for _, t, _ in ins:
            f = t.replace(",", " ").split()
            if f[0] == "v_accvgpr_write_b32":
                filled |= _agprs(f[1])
            elif f[0].startswith("v_mfma") or f[0].startswith("v_smfmac"):
                mfma_dst |= _agprs(f[1])
        parked = filled - mfma_dst
        rows = []
        for addr, body in blocks(ins):
            mf = lane = ag = 0
            for t in body:
                f = t.replace(",", " ").split()
                if f[0].startswith("v_mfma") or f[0].startswith("v_smfmac"):
                    mf += 1
                elif f[0] in ("v_readlane_b32", "v_writelane_b32"):
                    lane += 1
                elif f[0] == "v_accvgpr_write_b32" and (_agprs(f[1]) & parked):
                    ag += 1
                elif f[0] == "v_accvgpr_read_b32" and (_agprs(f[2]) & parked):
                    ag += 1
            rows.append((addr, len(body), mf, lane, ag))
        m = meta[name]
        res[name] = {"sgpr_spill": m.get("sgpr_spill_count", 0), "vgpr_spill": m.get("vgpr_spill_count", 0),
                     "code_bytes": (ins[-1][0] + 4 - ins[0][0]) if ins else 0,
                     "lane": sum(r[3] for r in rows), "lane_mfma": sum(r[3] for r in rows if r[2]),
                     "agpr": sum(r[4] for r in rows), "agpr_mfma": sum(r[4] for r in rows if r[2]), "blocks": rows}
    return res


def demangle(names):
    try:
        out = subprocess.check_output([os.path.join(LLVM, "llvm-cxxfilt")] + list(names)).decode().splitlines()
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--match", default="")
    ap.add_argument("--blocks", action="store_true", help="one line per basic block with lane ops or AGPR spill moves")
    a = ap.parse_args()
    res = ledger(a.lib, a.match)
    pretty = demangle(list(res))
    for name, r in res.items():
        print("%s\n    sgpr_spill %d  vgpr_spill %d  code %d B  lane ops: %d (%d in MFMA blocks)  agpr moves: %d (%d in MFMA blocks)"
              % (re.sub(r"^void ", "", pretty[name]).replace("(ConvP)", ""), r["sgpr_spill"], r["vgpr_spill"], r["code_bytes"],
                 r["lane"], r["lane_mfma"], r["agpr"], r["agpr_mfma"]))
        if a.blocks:
            for addr, n, mf, lane, ag in r["blocks"]:
                if lane or ag:
                    print("      block +0x%x: %d instructions, %d MFMA, %d lane ops, %d agpr moves" % (addr - r["blocks"][0][0], n, mf, lane, ag))


if __name__ == "__main__":
    main()
