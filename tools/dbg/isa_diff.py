#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds of youtokentome_amd/csrc kernel by kernel (needs no GPU).

  make -C youtokentome_amd/csrc            # in a checkout of each commit
  tools/dbg/isa_diff.py OLD/youtokentome_amd/csrc/build NEW/youtokentome_amd/csrc/build [--rename OLD_SYMBOL=NEW_SYMBOL ...]

For every object file of both builds the gfx950 code object is taken out (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle), disassembled (llvm-objdump -d) and cut
at the kernel symbols; a kernel is "identical" when its instruction stream is, text for text (addresses stripped, the kernel's own name
in branch targets replaced, pc-relative addresses of constants taken as section + offset).  The code-object metadata (llvm-readelf --notes: VGPRs, SGPRs, LDS, scratch, kernarg size) is compared too.
Exit status 1 if any kernel differs or exists on one side only."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def code_object(obj, tmp):
    fat, out = os.path.join(tmp, os.path.basename(obj) + ".fatbin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    r = subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None  # (host-only translation unit)
    subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle", "--input=" + fat, "--output=" + out],
                   check=True, capture_output=True)
    return out if os.path.getsize(out) else None


def kernels(build):
    """{symbol: (instruction lines, {metadata key: value})} over every object file of a build directory"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(build)):
            if not f.endswith(".o"):
                continue
            co = code_object(os.path.join(build, f), tmp)
            if not co:
                continue
            notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for blk in re.split(r"\n  - (?=\.agpr_count:)", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name:
                    meta[name.group(1)] = {k: (re.search(re.escape(k) + r":\s+(\S+)", blk) or [None, "-"])[1] for k in META}
            dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
            sections = [(int(m.group(2), 16), int(m.group(3), 16), m.group(1)) for m in re.finditer(
                r"\]\s+(\.\S+)\s+\S+\s+([0-9a-f]{16})\s+[0-9a-f]+\s+([0-9a-f]+)", subprocess.run([LLVM + "/llvm-readelf", "-S", co], check=True, capture_output=True, text=True).stdout)]
            cur, getpc = None, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
                if m:
                    cur = m.group(1)
                    res[cur] = ([], meta.get(cur))
                elif cur and line.strip() == "...":
                    continue  # (objdump's mark for the zero padding between two functions: present behind a kernel once another follows it)
                elif cur and line.strip():
                    text = re.sub(r"\s*//.*$", "", line).strip().replace(cur, "SELF")
                    at = re.search(r"//\s*([0-9A-Fa-f]+):", line)
                    # `s_getpc_b64` + `s_add_u32 lo, lo, literal`: the address of a constant, relative to the code -- it moves when a section in
                    # front of .text changes size (a longer symbol name does that): compared as section + offset
                    lit = re.match(r"s_add_u32 (\S+) \1 0x([0-9a-f]{8})$", text.replace(",", ""))
                    if lit and getpc is not None:
                        target = (getpc + int(lit.group(2), 16)) & 0xffffffff
                        sec = next(((n, target - a0) for a0, sz, n in sections if a0 <= target < a0 + sz), None)
                        if sec:
                            text = "s_add_u32 %s, %s, <%s+0x%x - pc>" % (lit.group(1), lit.group(1), sec[0], sec[1])
                    getpc = int(at.group(1), 16) + 4 if text.startswith("s_getpc_b64") and at else None
                    res[cur][0].append(text)
    return {k: v for k, v in res.items() if v[1] is not None}  # kernels only (device functions are inlined or have no metadata entry)


def main():
    it = iter(sys.argv[1:])
    args, rename = [], {}
    for a in it:
        if a == "--rename":
            o, n = next(it).split("=", 1)
            rename[o] = n
        else:
            args.append(a)
    old, new = kernels(args[0]), kernels(args[1])
    old = {rename.get(k, k): v for k, v in old.items()}
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("%-10s %s" % ("only old" if k in old else "only new", k))
            bad += 1
            continue
        same_isa, same_meta = old[k][0] == new[k][0], old[k][1] == new[k][1]
        print("%-10s %6d instructions  vgpr %s sgpr %s lds %s scratch %s kernarg %s  %s" % (
            "identical" if same_isa and same_meta else "DIFFERS", len(new[k][0]), new[k][1][".vgpr_count"], new[k][1][".sgpr_count"],
            new[k][1][".group_segment_fixed_size"], new[k][1][".private_segment_fixed_size"], new[k][1][".kernarg_segment_size"], k))
        if not same_meta:
            print("           metadata: old %s\n                     new %s" % (old[k][1], new[k][1]))
        if not same_isa:
            bad += 1
            n = next((i for i, (a, b) in enumerate(zip(old[k][0], new[k][0])) if a != b), min(len(old[k][0]), len(new[k][0])))
            print("           first difference at instruction %d: old `%s` new `%s` (old %d, new %d instructions)" % (
                n, old[k][0][n] if n < len(old[k][0]) else "-", new[k][0][n] if n < len(new[k][0]) else "-", len(old[k][0]), len(new[k][0])))
        elif not same_meta:
            bad += 1
    print("%d kernels, %d not identical" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
