#!/usr/bin/env python3
"""Compare the gfx950 code of two builds kernel by kernel: a refactor that must not change the code that runs.
    python tools/isa_compare.py OLD_BUILD_DIR NEW_BUILD_DIR        (directories of `make`'s build/*.o)

For every object: the gfx950 code object out of the .hip_fatbin section, its disassembly split per kernel (addresses and encodings
dropped) and the per-kernel metadata of its notes (register counts, spills, LDS / scratch / kernarg sizes, block size).  Kernels are paired
BY NAME over all objects of a build, so one that moved to another translation unit is compared like any other; the same name in two
objects of one build is an error.  Prints kernel counts and code-object sizes per object, the kernels that changed object, those that
differ and those present in one build only; the exit status is 1 when a kernel present in both differs or one appears only in the new build.
--rename NEW=OLD (any number, after the directories): the substring NEW of a mangled name in the new build is read as OLD before pairing - for a change
that renames an argument TYPE (the type is part of the symbol) and must leave the code alone."""
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
        lines = code.get(name, [])
        # Padding between a kernel and whatever follows it in the section (it depends on the neighbour, so a kernel that moved or became the
        # last of its object would differ by it): dropped only where it follows the instruction that ends the code - nothing falls through there.
        end = len(lines)
        while end and lines[end - 1].strip() in ("s_nop 0", "s_code_end", "..."):
            end -= 1
        if end and lines[end - 1].split()[0] in ("s_endpgm", "s_branch", "s_setpc_b64"):
            lines = lines[:end]
        out[name] = (lines, {k: it.get(k) for k in META})
    return out


def build(build_dir, tmp):
    """every kernel of a build: ({symbol: (instruction lines, metadata dict, object)}, {object: code-object bytes})"""
    os.mkdir(tmp)
    found, sizes = {}, {}
    for f in sorted(os.listdir(build_dir)):
        co = code_object(os.path.join(build_dir, f), tmp) if f.endswith(".o") else None
        if co is None:
            continue
        sizes[f] = os.path.getsize(co)
        for k, (code, meta) in kernels(co).items():
            if k in found:
                sys.exit(f"{build_dir}: kernel {k} is in {found[k][2]} and in {f}")
            found[k] = (code, meta, f)
    return found, sizes


def main(old_dir, new_dir, renames=()):
    with tempfile.TemporaryDirectory() as tmp:
        (a, sa), (b, sb) = build(old_dir, os.path.join(tmp, "old")), build(new_dir, os.path.join(tmp, "new"))
    real = {k: k for k in b}                        # paired name -> the symbol as the new build has it (what is printed for a kernel only it has)
    for new_part, old_part in renames:
        real = {k.replace(new_part, old_part): v for k, v in real.items()}
    b = {k: b[v] for k, v in real.items()}
    for f in sorted(set(sa) | set(sb)):
        print(f"{f}: {sum(v[2] == f for v in a.values())} -> {sum(v[2] == f for v in b.values())} kernels; code object {sa.get(f, 0)} -> {sb.get(f, 0)} bytes")
    both = [k for k in a if k in b]
    diff = [k for k in both if a[k][:2] != b[k][:2]]
    moved = [k for k in both if a[k][2] != b[k][2]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    for k in moved:
        print(f"  moved {k}: {a[k][2]} -> {b[k][2]}")
    for k in diff:
        what = "metadata " + str({m: (a[k][1][m], b[k][1][m]) for m in META if a[k][1][m] != b[k][1][m]}) if a[k][0] == b[k][0] else \
            f"instructions ({len(a[k][0])} -> {len(b[k][0])} lines)"
        print(f"  DIFFERS {k} ({b[k][2]}): {what}")
    for k in gone:
        print(f"  removed {k} ({a[k][2]})")
    for k in new:
        print(f"  NEW {real[k]} ({b[k][2]})")
    print(f"total: {len(both)} kernels compared, {len(both) - len(diff)} identical, {len(diff)} differ, {len(moved)} changed object, {len(gone)} removed, {len(new)} new; "
          f"code objects {sum(sa.values())} -> {sum(sb.values())} bytes")
    return 1 if diff or new else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    renames = []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    if len(args) != 2 or any(len(r) != 2 for r in renames):
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], renames))
