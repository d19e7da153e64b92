#!/usr/bin/env python3
"""Compare the gfx950 kernels that one csrc/*.hip file compiles to in two source trees (host only, no GPU).

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE gemm_glds.hip [more.hip ...]

Each file is compiled with build_library's flags plus --cuda-device-only -S.  Per kernel two texts are compared for equality: the
instructions between the kernel's label and its .Lfunc_end (comments, local labels, the kernel's own symbol and the zero block's
symbol masked) and the .amdhsa_kernel ... .end_amdhsa_kernel block.  Prints the kernels that are gone, new and different; a gone and
a new kernel with equal texts (a template parameter list that changed) are reported as one renamed kernel.  Exit status 1 when a
surviving kernel differs or a kernel is new.
"""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-fno-slp-vectorize", "-fno-vectorize"]


def kernels(tree, name):
    """-> {symbol: (instruction text, descriptor text)}, total codeLenInByte"""
    src = os.path.join(tree, "seq2seq_vc_amd", "csrc", name)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(["hipcc"] + FLAGS + ["--cuda-device-only", "-S", src, "-o", out], check=True)
        asm = open(out).read()
    desc = {m.group(1): m.group(0) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", asm, re.S)}
    res = {}
    for sym in desc:
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), asm, re.S | re.M).group(0)
        texts = []
        for text in (body, desc[sym]):
            text = re.sub(r";.*", "", text).replace(sym, "<self>")
            text = re.sub(r"\.L\w+", ".L", text)
            text = re.sub(r"_ZN\d+_GLOBAL__N_1\d+g_zero16\w*E", "<zero>", text)
            texts.append("\n".join(line.strip() for line in text.splitlines() if line.strip()))
        res[sym] = tuple(texts)
    return res, sum(int(n) for n in re.findall(r"; codeLenInByte = (\d+)", asm))


def demangle(syms):
    if not syms:
        return []
    return subprocess.run(["c++filt"] + list(syms), check=True, capture_output=True, text=True).stdout.split("\n")[:len(syms)]


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = False
    for name in files:
        (old, old_bytes), (new, new_bytes) = kernels(old_tree, name), kernels(new_tree, name)
        gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        renamed = []
        for a in list(added):
            twin = next((g for g in gone if old[g] == new[a]), None)
            if twin:
                renamed.append((twin, a))
                gone.remove(twin)
                added.remove(a)
        differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
        print(f"{name}: {len(old)} kernels / {old_bytes} code bytes -> {len(new)} kernels / {new_bytes} code bytes; "
              f"{len(gone)} gone, {len(added)} new, {len(renamed)} renamed (same text), {len(differ)} different")
        for title, syms in (("gone", gone), ("new", added), ("different", differ)):
            for d in demangle(syms):
                print(f"  {title}: {d}")
        for (a, b), da, db in zip(renamed, demangle([a for a, _ in renamed]), demangle([b for _, b in renamed])):
            print(f"  renamed: {da} -> {db}")
        bad = bad or bool(added or differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
