#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel: a refactor that must not change the code that runs.
    python tools/isa_compare.py OLD_BUILD_DIR NEW_BUILD_DIR        (directories of `make`'s build/*.o)

For every object present in both: the gfx950 code object out of the .hip_fatbin section, its disassembly split per kernel (addresses and
encodings dropped) and the per-kernel metadata of its notes (register counts, spills, LDS / scratch / kernarg sizes, block size).  Prints the
kernels compared, those present in one build only and the code-object sizes; the exit status is 1 when a kernel present in both differs or
one appears only in the new build."""
import os, re, subprocess, sys, tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """path of the object's gfx950 code object, None when it has no device code"""
    if ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-readelf"), "-S", obj):
        return None
    tag = os.path.join(tmp, os.path.basename(obj))
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + tag + ".fatbin", obj, tag + ".tmp")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + tag + ".fatbin",
        "--output=" + tag + ".co")
    return tag + ".co"


def kernels(co):
    """{symbol: (instruction lines, metadata dict)}"""
    code, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^(\S+) <(.+)>:$", line) or re.match(r"^<(.+)>:$", line)
        if m:
            cur = m.group(m.lastindex)
            code[cur] = []
        elif cur is not None and line.strip():
            code[cur].append(re.sub(r"\s*//.*$", "", line).rstrip())
    meta, item = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)
        if m:
            item = {}
        m = m or re.match(r"^    (\.\w+):\s*(.*)$", line)
        if m and item is not None:
            item[m.group(1)] = m.group(2).strip()
            if m.group(1) == ".name":
                meta[item[".name"]] = item
    out = {}
    for name, it in meta.items():
        out[name] = (code.get(name, []), {k: it.get(k) for k in META})
    return out


def main(old_dir, new_dir):
    bad = 0
    tot = {"compared": 0, "removed": 0, "old_bytes": 0, "new_bytes": 0}
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "old")); os.mkdir(os.path.join(tmp, "new"))
        for f in sorted(os.listdir(old_dir)):
            if not f.endswith(".o") or not os.path.exists(os.path.join(new_dir, f)):
                continue
            co_old, co_new = code_object(os.path.join(old_dir, f), os.path.join(tmp, "old")), code_object(os.path.join(new_dir, f), os.path.join(tmp, "new"))
            if co_old is None and co_new is None:
                continue
            a, b = kernels(co_old) if co_old else {}, kernels(co_new) if co_new else {}
            sa, sb = (os.path.getsize(c) if c else 0 for c in (co_old, co_new))
            tot["old_bytes"] += sa; tot["new_bytes"] += sb
            same = [k for k in a if k in b and a[k] == b[k]]
            diff = [k for k in a if k in b and a[k] != b[k]]
            gone = [k for k in a if k not in b]
            new = [k for k in b if k not in a]
            tot["compared"] += len(same) + len(diff); tot["removed"] += len(gone)
            print(f"{f}: {len(same) + len(diff)} kernels compared, {len(same)} identical, {len(diff)} differ, {len(gone)} removed, {len(new)} new; "
                  f"code object {sa} -> {sb} bytes")
            for k in diff:
                what = "metadata " + str({m: (a[k][1][m], b[k][1][m]) for m in META if a[k][1][m] != b[k][1][m]}) if a[k][0] == b[k][0] else \
                    f"instructions ({len(a[k][0])} -> {len(b[k][0])} lines)"
                print(f"  DIFFERS {k}: {what}")
            for k in gone:
                print(f"  removed {k}")
            for k in new:
                print(f"  NEW {k}")
            bad += len(diff) + len(new)
    print(f"total: {tot['compared']} kernels compared, {tot['removed']} removed, code objects {tot['old_bytes']} -> {tot['new_bytes']} bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
