#!/usr/bin/env python3
"""Compare the gfx950 machine code of a kernel family between two builds (no GPU needed).

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --cuda-device-only -S conv_halo.hip -o new.s
    python tools/halo_asm_compare.py [halo] old.s new.s
    python tools/halo_asm_compare.py pointwise old_pointwise.s new_pointwise.s new_conv1x1_lds.s

A family (FAMILIES) is a pattern for the kernels' mangled names and the function that turns a demangled name into a pairing key; the
kernels of every file after the first are looked up in the first.  Kernels are paired by what they are, because the mangled names
change with a template's parameter list:
  halo       conv3x3_halo_kernel: (dtype, patch rows, packed images, persistent, fused first layer, chain, chained blocks) out of
             thirteen parameters, of which CT = 64 is kept, or those seven;
  pointwise  every kernel that pointwise.hip held before the LDS-resident 1x1 GEMM moved to conv1x1_lds.hip: shortcut1x1s2_lds_kernel
             by (CIN, STAGE, SPLIT, CONVT) out of <CIN, NW, PREFETCH, STAGE, SPLIT, CONVT>, of which NW = 8, PREFETCH = true are kept,
             or those four; every other kernel by its demangled name.
A pair is identical when the instruction streams match line by line after stripping `;` comments and the function index
in local labels, and the .amdhsa_ fields (registers, LDS, scratch) and the occupancy the compiler reports match as well.
Prints one markdown table row per kernel of the second file; exit status 1 if any pair differs or is missing."""
from __future__ import annotations

import re
import subprocess
import sys

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(n.replace("DF16_", "Dh") for n in names),   # _Float16 as __fp16: older demanglers lack the former
                          capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def template_args(demangled):
    return [x.strip() for x in demangled[demangled.index("<") + 1:demangled.index(">(")].split(",")]


def halo_key(demangled):
    a = template_args(demangled)
    a[0] = a[0].replace("cv::", "").replace("_t", "").replace("__fp16", "half")
    if len(a) == 13:                                    # T, CT, TH, WGC, NW, TPS, NSW, IMG, PERSIST, DBH, FUSE0, CHAIN, CNB
        return None if a[1] != "64" else (a[0], a[2], a[7], a[8], a[10], a[11], a[12])
    assert len(a) == 7, demangled                       # T, TH, IMG, PERSIST, FUSE0, CHAIN, CNB
    return tuple(a)


def pointwise_key(demangled):
    name = demangled.split("(")[0].replace("void ", "").replace("cv::", "").replace("__fp16", "half")
    if not name.startswith("shortcut1x1s2_lds_kernel<"):
        return (name,)
    a = template_args(demangled)
    if len(a) == 6:                                     # CIN, NW, PREFETCH, STAGE, SPLIT, CONVT
        return None if (a[1], a[2]) != ("8", "true") else ("shortcut1x1s2_lds_kernel", a[0], *a[3:])
    assert len(a) == 4, demangled                       # CIN, STAGE, SPLIT, CONVT
    return ("shortcut1x1s2_lds_kernel", *a)


FAMILIES = {"halo": (r"_ZN2cv19conv3x3_halo_kernel\w+", halo_key, "T, TH, IMG, PERSIST, FUSE0, CHAIN, CNB"),
            "pointwise": (r"_ZN2cv\w+", pointwise_key, "kernel (shortcut1x1s2_lds_kernel: CIN, STAGE, SPLIT, CONVT)")}


def kernels(path, pattern):
    """{mangled name: (instruction lines, {resource field: value})}"""
    label = re.compile(r"^(" + pattern + r"):\s*(;.*)?$")
    found, name, body, res = {}, None, None, None
    for line in open(path):
        m = label.match(line)
        if m:
            name, body, res = m.group(1), [], {}
            continue
        if name is None:
            continue
        if line.startswith(("; NumVgprs:", "; NumAgprs:", "; TotalNumSgprs:", "; ScratchSize:", "; Occupancy:")):
            res[line[2:].split(":")[0]] = line.split(":")[1].strip()
        if line.startswith("; Occupancy:"):              # last line of interest of a function's trailer
            if ".amdhsa_next_free_vgpr" in res:         # a kernel, not a device function
                found[name] = (body, res)
            name = None
            continue
        code = LABEL.sub(lambda l: "." + l.group(1), line.split(";")[0]).strip()
        if code.startswith(".amdhsa_") and not code.startswith(".amdhsa_kernel"):
            field, value = code.split(None, 1)
            res[field] = value
        elif code and not code.startswith((".size", ".set", ".section", ".p2align", ".end_amdhsa_kernel", ".amdhsa_kernel", ".text")):
            body.append(code)
    return found


def main() -> int:
    args = sys.argv[1:]
    pattern, key_of, what = FAMILIES[args.pop(0) if args[0] in FAMILIES else "halo"]
    old, new = kernels(args[0], pattern), {}
    for path in args[1:]:
        new.update(kernels(path, pattern))
    names = demangle(list(old) + list(new))
    old_by_key = {key_of(names[n]): n for n in old if key_of(names[n])}
    print(f"{len(old)} kernels in {args[0]}, {len(new)} in {', '.join(args[1:])}\n")
    print(f"| {what} | lines | VGPR / AGPR / SGPR | scratch | static LDS | occupancy | identical |")
    print("|---|---|---|---|---|---|---|")
    bad = 0
    for n in sorted(new, key=lambda n: key_of(names[n])):
        key = key_of(names[n])
        body, res = new[n]
        o = old.get(old_by_key.get(key))
        same = o is not None and o[0] == body and o[1] == res
        bad += not same
        print(f"| {', '.join(key)} | {len(body)} | {res['NumVgprs']} / {res['NumAgprs']} / {res['TotalNumSgprs']} | "
              f"{res['ScratchSize']} | {res['.amdhsa_group_segment_fixed_size']} | {res['Occupancy']} | {'yes' if same else 'NO'} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
