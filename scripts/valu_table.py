#!/usr/bin/env python3
"""Static instruction counts of the kernels of one .hip file, from the gfx950 assembly the compiler writes: vector-ALU instructions
(mnemonics v_*), how many of them are v_bitop3_b32, and the registers, scratch and occupancy of the kernel's resource comments.
Cross-compiles, no GPU needed.
usage: python3 scripts/valu_table.py [file.hip] [name filter]      (default: floxer_amd/csrc/flx_device.hip, kernels named ed_*)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "floxer_amd", "csrc")


def assembly(path):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           path, "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=CSRC).stdout


def table(asm):
    rows, cur = [], None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = {"name": m.group(1), "valu": 0, "bitop3": 0}
            rows.append(cur)
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith("v_"):
            cur["valu"] += 1
            cur["bitop3"] += t.startswith("v_bitop3_b32")
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")):
            m = re.match(pat, t)
            if m:
                cur[key] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for r, n in zip(rows, names):
        r["name"] = re.sub(r"\(.*", "", n).replace("void ", "").replace("flx::", "")
    return [r for r in rows if "occ" in r]


def main():
    path = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(CSRC, "flx_device.hip")
    flt = sys.argv[2] if len(sys.argv) > 2 else "ed_"
    print(f"{'kernel':40s} {'VALU':>6s} {'bitop3':>6s} {'VGPR':>5s} {'scratch B/lane':>14s} {'waves/SIMD':>10s}")
    for r in table(assembly(path)):
        if flt in r["name"]:
            print(f"{r['name'][:40]:40s} {r['valu']:6d} {r['bitop3']:6d} {r.get('vgpr', 0):5d} {r.get('scratch', 0):14d} {r.get('occ', 0):10d}")


if __name__ == "__main__":
    main()
