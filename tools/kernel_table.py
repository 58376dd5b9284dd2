#!/usr/bin/env python3
"""The device kernels of a built library, one line each: unit, size, registers, scratch, LDS, kernarg bytes, a hash of the
kernel's bytes, demangled name.  Reads the objects `make` leaves in a build directory; inspects no instructions.

    tools/kernel_table.py pde_multigrid_amd/csrc/build > branch.txt
    tools/kernel_table.py --diff parent.txt branch.txt     # kernels added / removed / changed / held by more units
"""
import collections, glob, hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def table(build):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(build, "mgx_*.o"))):
            fb, co, text = (os.path.join(tmp, n) for n in ("fb", "co", "text"))
            run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb)
            run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}")
            run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, text)
            code = open(text, "rb").read()
            base = int(re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-SW", co)).group(1), 16)
            notes, seen = {}, set()  # a kernel is in .dynsym and in .symtab: listed once
            for entry in run(f"{LLVM}/llvm-readelf", "--notes", co).split("\n  - ")[1:]:
                name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
                if name: notes[name.group(1)] = [re.search(rf"^    \{k}:\s+(\d+)", entry, re.M).group(1) for k in KEYS]
            for ln in run(f"{LLVM}/llvm-readelf", "-sW", co).splitlines():
                f = ln.split()
                if len(f) == 8 and f[3] == "FUNC" and f[7] in notes and f[7] not in seen:
                    seen.add(f[7])
                    off, size = int(f[1], 16) - base, int(f[2])
                    rows.append([os.path.basename(obj)[:-2], str(size)] + notes[f[7]] + [hashlib.sha1(code[off : off + size]).hexdigest()[:12], f[7]])
    names = subprocess.run(["c++filt"], input="\n".join(r[-1] for r in rows), check=True, capture_output=True, text=True).stdout.splitlines()
    return ["\t".join(r[:-1] + [n]) for r, n in zip(rows, names)]


def diff(a, b):
    def load(path):
        d = collections.defaultdict(list)  # name -> [(unit, facts)]
        for ln in open(path):
            f = ln.rstrip("\n").split("\t")
            if len(f) == 9 and f[1].isdigit():
                d[f[8]].append((f[0], f[1:8]))
        return d
    A, B = load(a), load(b)
    for n in sorted(set(A) - set(B)): print("removed\t" + n)
    for n in sorted(set(B) - set(A)): print("added\t" + n)
    same = 0
    for n in sorted(set(A) & set(B)):
        if len(B[n]) > len(A[n]): print(f"held by {len(B[n])} units (was {len(A[n])})\t{n}")
        if {tuple(f) for _, f in A[n]} != {tuple(f) for _, f in B[n]}:
            print("changed\t" + n + "\t" + "; ".join(u + ": " + " ".join(f) for u, f in A[n]) + " -> " + "; ".join(u + ": " + " ".join(f) for u, f in B[n]))
        else: same += 1
    print(f"{len(A)} kernels before, {len(B)} after, {same} with the same size, registers, scratch, LDS, kernarg bytes and code bytes")
    for n in sorted(B):
        for u, f in B[n]:
            if f[3] != "0": print(f"scratch after: {f[3]} bytes in {u}\t{n}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff": diff(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 2: print("unit\tbytes\tvgpr\tsgpr\tscratch\tlds\tkernarg\tsha1\tkernel\n" + "\n".join(table(sys.argv[1])))
    else: sys.exit(__doc__)
