#!/usr/bin/env python3
"""tools/kernel_diff.py <build dir A> <build dir B> [name-filter]: compares the gfx950 code of every kernel symbol present
in the object files of both build directories (sprintz_amd/csrc/build of two trees), paired by symbol over all the objects of
a directory -- a kernel that moved to another unit is still the same kernel; one that two objects of a directory hold is
reported ("twice"), and compared as the first holds it: identical / differing only in the
offsets of kernel-argument loads (a DecodeArgs field appended or moved) / differing only in the order of the two sources
of a commutative VALU instruction (same opcode, same registers) / differing otherwise.  Prints the counts and the names of
the last three classes.  Needs no GPU."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj, tmp):
    """{symbol: [instruction text, ...]} of the gfx950 code object bundled in `obj`"""
    u = os.path.join(tmp, os.path.basename(obj))
    subprocess.check_call(["cp", obj, u])
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", os.path.basename(u)], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = glob.glob(u + ".*gfx950*")
    if not co:
        return {}
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co[0]], capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":      # ("...": the zero padding between two symbols, which depends on what follows)
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    return out


def strip_karg(ins):
    """kernel-argument loads with their offset blanked"""
    return [re.sub(r"^(s_load_dword\w*\s+\S+\s+s\[\d+:\d+\],)\s*\S+", r"\1 OFF", i) for i in ins]


def commute(ins):
    """the two sources of v_or / v_and / v_xor / v_add_u32 / v_max / v_min (e32) in sorted order"""
    out = []
    for i in ins:
        m = re.match(r"^(v_(?:or|and|xor)_b32_e32|v_add_u32_e32|v_(?:max|min)_[iu]32_e32)\s+(\S+),\s*(\S+),\s*(\S+)$", i)
        out.append(f"{m.group(1)} {m.group(2)} " + " ".join(sorted((m.group(3), m.group(4)))) if m else i)
    return out


def directory(d, filt):
    """{symbol: instructions} over every object file of `d` (a symbol may change its unit between two builds), and the
    symbols that more than one object of `d` holds, with those objects"""
    out, where = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(d, "*.o"))):
            for k, ins in kernels(obj, tmp).items():
                if filt.search(k):
                    where.setdefault(k, []).append(os.path.basename(obj))
                    out.setdefault(k, ins)
    return out, {k: w for k, w in where.items() if len(w) > 1}


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    filt = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    (ka, twice_a), (kb, twice_b) = directory(a_dir, filt), directory(b_dir, filt)
    same, karg, comm, other = 0, [], [], []
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for k in sorted(set(ka) & set(kb)):
        if ka[k] == kb[k]:
            same += 1
        elif strip_karg(ka[k]) == strip_karg(kb[k]):
            karg.append(k)
        elif commute(strip_karg(ka[k])) == commute(strip_karg(kb[k])):
            comm.append(k)
        else:
            other.append(k)
    print(f"symbols in both: {same + len(karg) + len(comm) + len(other)}; identical: {same}; kernel-argument offsets only: {len(karg)}; "
          f"commuted sources only: {len(comm)}; differ otherwise: {len(other)}; only in A: {len(only_a)}; only in B: {len(only_b)}; "
          f"twice in A: {len(twice_a)}; twice in B: {len(twice_b)}")
    for tag, names in (("karg ", karg), ("comm ", comm), ("OTHER", other), ("only A", only_a), ("only B", only_b)):
        for k in names:
            print(f"  {tag}", k)
    for tag, twice in (("twice A", twice_a), ("twice B", twice_b)):
        for k, w in sorted(twice.items()):
            print(f"  {tag}", k, "in", ", ".join(w))


if __name__ == "__main__":
    main()
